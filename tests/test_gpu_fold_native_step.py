"""GPU: one train step with the folded layer's weight products on the grouped native launches
(fused.FOLD_NATIVE, csrc/fold.hip) against the same step on the bgnn GEMM chain they replace: the
loss, every gradient and every BatchNorm buffer bit-identical, and the native entry points really
taken (once per direction)."""
import pytest
import torch

import bgnn
from bgnn import _lib, fused
from bgnn import synthetic as S

pytestmark = pytest.mark.gpu


def step(dev, model_name, native, monkeypatch):
    b = S.make_batch(24, 4)          # N >= 1024: the fused encoder path, so layer 0 is folded
    assert b.num_nodes >= 1024
    torch.manual_seed(0)
    m = bgnn.BuckGNN(16, 5, hidden_channels=64, num_layers=6, dropout_rate=0.0, model_name=model_name)
    m = m.to(dev).train()
    calls = []
    real = _lib.call

    def counting(name, *args):
        if name.startswith("bgnn_fold_weights_"):
            calls.append(name)
        return real(name, *args)

    monkeypatch.setattr(_lib, "call", counting)
    monkeypatch.setattr(fused, "FOLD_NATIVE", native)
    bd = b.to(dev)
    pred, _ = m(bd.x, bd.edge_index, bd.edge_attr, bd.batch)
    loss = bgnn.RelativeErrorLoss()(pred, bd.y)
    loss.backward()
    torch.cuda.synchronize()
    out = {"loss": loss.detach().clone(), "pred": pred.detach().clone()}
    out.update({"grad " + k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})
    out.update({"buffer " + k: v.detach().clone() for k, v in m.named_buffers()})
    return out, calls


@pytest.mark.parametrize("model_name", ["GraphSage_addAggr", "GraphSage_meanAggr", "GraphSage_addAggr_Shared"])
def test_train_step_is_bit_identical_with_native_fold(dev, model_name, monkeypatch):
    got, calls = step(dev, model_name, True, monkeypatch)
    assert calls == ["bgnn_fold_weights_fwd", "bgnn_fold_weights_bwd"]
    ref, calls = step(dev, model_name, False, monkeypatch)
    assert calls == []
    assert set(got) == set(ref) and any(k.startswith("grad ") for k in got)
    for k in ref:
        a, r = got[k], ref[k]
        if a.is_floating_point():
            assert torch.equal(a.view(torch.int32), r.view(torch.int32)), k
        else:
            assert torch.equal(a, r), k
