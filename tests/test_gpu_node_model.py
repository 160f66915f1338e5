"""GPU: bgnn.BuckGNN with the node-level prediction types (static_disp, static_stress, mode_shape)
and bgnn.train_step on them, on >= 1,024-node synthetic batches (where the fused encoder, layer loop
and the decoder tail kernel bgnn_head2 run), against the fp64 oracle: oracle.buckgnn_ref.forward(...,
return_nodes=True) followed by oracle.buckgnn_ref._mlp(sd, "decoder", nodes).

Bounds, from tests/test_gpu_model.py: predictions and loss rtol = atol = 1e-4 (:70-72); gradients
by their checksums [sum, sum |g|, projection], |d| <= 2e-3 |ref| + 2e-4 + 1e-4 sum |g| (:86-97, the
form that file uses on its >= 1,024-node fixtures)."""
import copy

import numpy as np
import pytest
import torch

import bgnn
from recipe import grad_checksum

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
C_OUT = {"static_disp": 2, "static_stress": 3, "mode_shape": 3}
# model_name, hidden, prediction_type, super nodes + pooling
VARIANTS = [
    ("GraphSage_addAggr", 64, "static_disp", False, "mean"),
    ("GraphSage_addAggr", 512, "static_stress", False, "mean"),
    ("GraphSage_addAggr_Shared", 128, "mode_shape", False, "mean"),
    ("GraphSage_addAggr", 64, "static_stress", True, "supernode_only"),
]
IDS = ["add_h64_disp", "add_h512_stress", "shared_h128_mode", "add_h64_stress_super"]
LAYERS = 3


def _batch(super_node, ptype, dev, seed=0):
    """Three 19 x 19 meshes (1,083 nodes; 1,086 with super nodes) with a node-level y: one row per
    real node, in graph order."""
    from bgnn import synthetic
    b = synthetic.make_batch(19, 3, super_node=super_node, seed0=seed)
    g = torch.Generator().manual_seed(seed + 77)
    n_real = int((b.x[:, -1] == 0).sum()) if super_node else b.x.size(0)
    y = torch.rand(n_real, C_OUT[ptype], generator=g) * 1.5 + 0.5
    y = y * torch.where(torch.rand(y.shape, generator=g) < 0.5, -1.0, 1.0)
    b.y = y
    assert b.x.size(0) >= 1024
    return b.to(dev)


def _model(name, h, ptype, pooling, dev, seed=0):
    torch.manual_seed(seed)
    m = bgnn.BuckGNN(16, 5, hidden_channels=h, num_layers=LAYERS, pooling_layer=pooling, prediction_type=ptype,
                     dropout_rate=0.0, model_name=name)
    return m.to(dev)


def _sd64(model, grad=False):
    sd = {}
    for k, v in model.state_dict().items():
        t = v.detach().cpu()
        t = t.double() if t.is_floating_point() else t.clone()
        sd[k] = t.requires_grad_(grad and t.is_floating_point() and "running" not in k)
    return sd


def _oracle_nodes(sd, name, b, training, pooling, super_node):
    """fp64 node-level prediction and the returned batch vector (Models/BuckGNN.py:519-526)."""
    from oracle import buckgnn_ref as R
    x = b.x.detach().cpu()
    batch = b.batch.cpu()
    _, nodes = R.forward(sd, name, x.double(), b.edge_index.cpu(), batch, training, pooling, 0.0, num_layers=LAYERS,
                         return_nodes=True)
    if super_node:
        real = x[:, -1] == 0
        return R._mlp(sd, "decoder", nodes[real]), batch[real]
    return R._mlp(sd, "decoder", nodes), batch


def _spy(monkeypatch):
    from bgnn import _lib
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    return calls


@pytest.mark.parametrize("name,h,ptype,super_node,pooling", VARIANTS, ids=IDS)
def test_eval_prediction_matches_fp64_oracle(dev, monkeypatch, name, h, ptype, super_node, pooling):
    b = _batch(super_node, ptype, dev)
    model = _model(name, h, ptype, pooling, dev).eval()
    calls = _spy(monkeypatch)
    with torch.no_grad():
        pred, out_batch = model(b.x, b.edge_index, b.edge_attr, b.batch)
    assert calls.count("bgnn_head2_fwd") == 1
    ref, ref_batch = _oracle_nodes(_sd64(model), name, b, False, pooling, super_node)
    assert pred.shape == ref.shape == b.y.shape
    assert torch.equal(out_batch.cpu(), ref_batch)
    np.testing.assert_allclose(pred.cpu().numpy(), ref.numpy(), **TOL)
    # the torch decoder on the same features gives the same rows (and the same filter)
    from bgnn import fused
    monkeypatch.setattr(fused, "FUSED_NODE_HEAD", False)
    with torch.no_grad():
        pred_t, batch_t = model(b.x, b.edge_index, b.edge_attr, b.batch)
    assert calls.count("bgnn_head2_fwd") == 1 and torch.equal(batch_t, out_batch)
    np.testing.assert_allclose(pred_t.cpu().numpy(), ref.numpy(), **TOL)


def test_ea_model_takes_the_head(dev, monkeypatch):
    """EA_GNN goes through the same forward tail: one smoke case."""
    b = _batch(False, "static_disp", dev)
    model = _model("EA_GNN", 64, "static_disp", "mean", dev).eval()
    calls = _spy(monkeypatch)
    with torch.no_grad():
        pred, _ = model(b.x, b.edge_index, b.edge_attr, b.batch)
        assert calls.count("bgnn_head2_fwd") == 1
        model.use_fused = False
        ref, _ = model(b.x, b.edge_index, b.edge_attr, b.batch)
    assert pred.shape == (b.x.size(0), 2)
    np.testing.assert_allclose(pred.cpu().numpy(), ref.cpu().numpy(), **TOL)


def _loss64(pred, y, batch, scaler, eps=0.1):
    """GraphRelativeError (bgnn/losses.py) on ColumnScaler-denormalised values, in fp64."""
    s, c = scaler.scale.double(), scaler.center.double()
    p, t = pred * s + c, y.double() * s + c
    rel = (p - t).abs() / (t.abs() + eps)
    B = int(batch.max()) + 1
    cnt = torch.bincount(batch, minlength=B).double() * rel.size(1)
    return (torch.zeros(B, dtype=torch.float64).index_add_(0, batch, rel.sum(1)) / cnt).mean() * 10000


def _step(model, b, scaler, criterion=None):
    """One train_step with a zero learning rate (the gradients stay on the parameters)."""
    model.zero_grad(set_to_none=True)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    loss = bgnn.train_step(model, b, opt, criterion or bgnn.GraphRelativeError(), scaler)
    return loss, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


def _check_grads(grads, ref):
    assert set(grads) == set(ref)
    for k, g in grads.items():
        want = grad_checksum(ref[k].numpy())
        got = grad_checksum(g.double().cpu().numpy())
        bound = 2e-3 * np.abs(want) + 2e-4 + 1e-4 * float(want[1])
        assert (np.abs(got - want) <= bound).all(), (k, got, want)


@pytest.mark.parametrize("name,h,ptype,super_node,pooling", VARIANTS, ids=IDS)
def test_train_step_matches_fp64_autograd(dev, monkeypatch, name, h, ptype, super_node, pooling):
    from bgnn import fused, losses
    b = _batch(super_node, ptype, dev, seed=3)
    C = C_OUT[ptype]
    scaler = bgnn.ColumnScaler(center=[0.1 * (c + 1) for c in range(C)], scale=[0.8 + 0.3 * c for c in range(C)])
    model = _model(name, h, ptype, pooling, dev, seed=1).train()
    state = copy.deepcopy(model.state_dict())
    sd = _sd64(model, grad=True)
    calls = _spy(monkeypatch)
    loss, grads = _step(model, b, scaler)
    for k in ("bgnn_head2_fwd", "bgnn_head2_bwd", "bgnn_graph_loss"):
        assert calls.count(k) == 1, k
    # fp64 autograd through the restatement (train mode: BatchNorm on batch statistics)
    pred64, batch64 = _oracle_nodes(sd, name, b, True, pooling, super_node)
    loss64 = _loss64(pred64, b.y.cpu(), batch64, scaler)
    loss64.backward()
    ref = {k: v.grad for k, v in sd.items() if v.grad is not None}
    print(f"{name} h={h} {ptype}: loss {loss.item():.8g} fp64 {loss64.item():.10g}")
    np.testing.assert_allclose(loss.item(), loss64.item(), **TOL)
    _check_grads(grads, ref)
    # a second fused step from the same state: the same bits
    model.load_state_dict(state)
    loss2, grads2 = _step(model, b, scaler)
    assert torch.equal(loss, loss2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
    # both switches off: the torch decoder and the torch loss, within the same bounds
    model.load_state_dict(state)
    monkeypatch.setattr(fused, "FUSED_NODE_HEAD", False)
    monkeypatch.setattr(losses, "FUSED_GRAPH_LOSS", False)
    n = len(calls)
    loss3, grads3 = _step(model, b, scaler)
    assert not {"bgnn_head2_fwd", "bgnn_head2_bwd", "bgnn_graph_loss"} & set(calls[n:])
    np.testing.assert_allclose(loss3.item(), loss64.item(), **TOL)
    _check_grads(grads3, ref)


def test_train_step_other_routes(dev, monkeypatch):
    """A reference-style normalizer object (denormalize_displacement / denormalize_gp_stresses, chosen
    by prediction type), a criterion that is not a bgnn.losses class (it receives the reference's
    filtered_x), no normalizer, and sync_metrics."""
    b = _batch(True, "static_stress", dev, seed=5)
    model = _model("GraphSage_addAggr", 64, "static_stress", "supernode_only", dev, seed=2).train()
    state = copy.deepcopy(model.state_dict())
    scaler = bgnn.ColumnScaler(center=[0.1, 0.2, 0.3], scale=[0.8, 1.1, 1.4])
    want, _ = _step(model, b, scaler)

    class RefNormalizer:   # the reference's interface (Normalizer.py:298-312)
        used = []

        def denormalize_displacement(self, v):
            raise AssertionError("static_stress denormalises stresses")

        def denormalize_gp_stresses(self, v):
            self.used.append(v.shape)
            return scaler.denormalize(v)

    model.load_state_dict(state)
    got, _ = _step(model, b, RefNormalizer())
    assert len(RefNormalizer.used) == 2
    np.testing.assert_allclose(got.item(), want.item(), rtol=1e-5)

    seen = {}

    def criterion(pred, target, batch, x):
        seen["x"] = x
        return bgnn.GraphRelativeError()(pred, target, batch, x)

    model.load_state_dict(state)
    got, _ = _step(model, b, scaler, criterion)
    assert torch.equal(seen["x"], b.x[b.x[:, -1] == 0])
    np.testing.assert_allclose(got.item(), want.item(), rtol=1e-5)

    model.load_state_dict(state)
    plain, _ = _step(model, b, None)
    with torch.no_grad():
        model.load_state_dict(state)
        model.train()
        pred, ob = model(b.x, b.edge_index, b.edge_attr, b.batch)
    monkeypatch.setattr(bgnn.losses, "FUSED_GRAPH_LOSS", False)
    np.testing.assert_allclose(plain.item(), bgnn.GraphRelativeError()(pred, b.y, ob, None).item(), rtol=1e-5)
    model.load_state_dict(state)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    lv, mape = bgnn.train_step(model, b, opt, bgnn.GraphMAELoss(), scaler, sync_metrics=True)
    assert isinstance(lv, float) and isinstance(mape, float)
    assert mape == pytest.approx(bgnn.losses.mape_error(pred, b.y, "static_stress").item(), rel=1e-4)


def test_buckling_train_step_unchanged(dev):
    """train_step on a buckling model computes what its buckling branch computed before the
    node-level branch was added (a copy of that branch, inlined here): the same bits."""
    from bgnn import synthetic
    from bgnn.graph import prepare
    from bgnn.train import _fused_loss
    b = synthetic.make_batch(19, 3).to(dev)
    torch.manual_seed(4)
    model = bgnn.BuckGNN(16, 5, hidden_channels=64, num_layers=LAYERS, dropout_rate=0.0,
                         model_name="GraphSage_addAggr").to(dev).train()
    state = copy.deepcopy(model.state_dict())
    crit, norm = bgnn.RelativeErrorLoss(), bgnn.EigenvalueScaler(0.3, 1.7)

    def before(model, batch, optimizer, criterion, normalizer):
        prepare(batch.edge_index, batch.x.size(0), batch.batch, getattr(batch, "num_graphs", None) or None)
        pred, _ = model(batch.x, batch.edge_index, batch.edge_attr, batch.batch)
        loss = _fused_loss(criterion, normalizer, pred, batch.y)
        if loss is None:
            if normalizer is not None:
                loss = criterion(normalizer.denormalize_eigenvalue(pred), normalizer.denormalize_eigenvalue(batch.y))
            else:
                loss = criterion(pred, batch.y)
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        return loss.detach()

    out = []
    for fn in (before, bgnn.train_step):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        opt = torch.optim.SGD(model.parameters(), lr=0.01)
        loss = fn(model, b, opt, crit, norm)
        out.append((loss, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                    copy.deepcopy(model.state_dict())))
    assert torch.equal(out[0][0], out[1][0])
    assert set(out[0][1]) == set(out[1][1])
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k
    for k in out[0][2]:
        assert torch.equal(out[0][2][k], out[1][2][k]), k
