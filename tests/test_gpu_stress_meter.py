"""bgnn.losses.StressErrorMeter, bgnn.train_step(..., metrics=) and bgnn.evaluate_nodes on the GPU.

The meter adds each batch's sums over graphs of the bgnn_graph_metrics table on the device; a
stress_errors call reads the same sums back. Both add the same doubles in the same order, so the
meter equals the key-wise sum of the calls to a relative 1e-12 (NaNs matching). train_step with a
meter must leave the loss, the gradients and the parameters bit-identical to train_step without one."""
import copy
import glob
import os

import numpy as np
import pytest
import torch

import bgnn
from bgnn import losses
from recipe import make_weights, meta_from_array

pytestmark = pytest.mark.gpu
HEADS = os.path.join(os.path.dirname(__file__), "golden", "heads")
FILES = sorted(glob.glob(os.path.join(HEADS, "node_*.npz")))
C_OUT = {"static_disp": 2, "static_stress": 3}


def _same(d, ref, rel, tag=None):
    assert sorted(d) == sorted(ref), tag
    for k, v in ref.items():
        if np.isnan(v):
            assert np.isnan(d[k]), (tag, k, d[k])
        else:
            assert d[k] == pytest.approx(v, rel=rel, abs=1e-6 if rel > 1e-9 else 0.0), (tag, k, d[k], v)


def _ragged(seed, sizes, C, thr, dev):
    g = torch.Generator().manual_seed(seed)
    N = sum(sizes)
    t = torch.randn(N, C, generator=g) * torch.pow(10.0, torch.rand(N, 1, generator=g) * 2 - 1.0) * thr * 3
    p = t * (1 - (torch.rand(N, C, generator=g) * 0.3 + 0.01))
    b = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    return p.to(dev), t.to(dev), b.to(dev)


@pytest.mark.parametrize("kind,C", [("static_stress", 3), ("static_disp", 2)])
def test_meter_equals_the_sum_of_calls(dev, monkeypatch, kind, C):
    thr = losses.DEFAULT_THRESHOLD[kind]
    batches = [_ragged(1, [40, 3, 17, 120], C, thr, dev), _ragged(2, [9, 64], C, thr, dev),
               _ragged(3, [1, 5, 1, 33, 8], C, thr, dev)]
    from bgnn import _lib
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    meter = losses.StressErrorMeter(kind)
    total = {k: 0.0 for k in losses.METRIC_KEYS[kind]}
    for p, t, b in batches:
        meter.update(p, t, b)
        for k, v in losses.stress_errors(p, t, b, kind, thr).items():
            total[k] += v
    assert calls.count("bgnn_graph_metrics") == 6
    assert meter.counts == (11, 3) and meter.state().shape == (30,) and meter.state().is_cuda
    _same(meter.compute("graph"), {k: v / 11 for k, v in total.items()}, 1e-12)
    _same(meter.compute("batch"), {k: v / 3 for k, v in total.items()}, 1e-12)
    # an input the kernel declines (doubles) goes through the torch code, with a ColumnScaler's affine
    p, t, b = batches[1]
    scale = torch.tensor([0.5 + 0.37 * c for c in range(C)], device=dev)
    center = torch.tensor([0.05 * thr * (c + 1) for c in range(C)], device=dev)
    meter.reset()
    assert meter.counts == (0, 0)
    n = calls.count("bgnn_graph_metrics")
    meter.update(p.double(), t.double(), b, scale.double(), center.double())
    assert calls.count("bgnn_graph_metrics") == n and meter.counts == (2, 1)
    want = losses.stress_errors(p.double() * scale + center, t.double() * scale + center, b, kind, thr)
    _same(meter.compute("batch"), want, 1e-12)
    # and the kernel with the affine folded in agrees with it (float32 against double inputs)
    meter.reset()
    meter.update(p, t, b, scale, center)
    assert calls.count("bgnn_graph_metrics") == n + 1
    _same(meter.compute("batch"), want, 5e-5)


def _golden_model(path, dev):
    z = np.load(path)
    meta = meta_from_array(z["meta"])
    m = bgnn.BuckGNN(16, 5, hidden_channels=meta["hidden"], num_layers=meta["num_layers"],
                     pooling_layer=meta["pooling"], prediction_type=meta["prediction_type"], dropout_rate=0.0,
                     model_name=meta["model_name"])
    sd = m.state_dict()
    w = make_weights({k: tuple(v.shape) for k, v in sd.items()}, meta["weight_seed"])
    m.load_state_dict({k: torch.from_numpy(w[k]) if k in w else sd[k] for k in sd})
    b = bgnn.Data(**{k: torch.from_numpy(z[k]) for k in ("x", "edge_index", "edge_attr", "y")})
    b.batch = torch.from_numpy(z["batch"])
    return m.to(dev), b.to(dev), meta


@pytest.mark.parametrize("path", FILES, ids=os.path.basename)
@pytest.mark.parametrize("with_scaler", [True, False], ids=["scaled", "plain"])
def test_train_step_with_a_meter_changes_nothing(dev, path, with_scaler):
    model, b, meta = _golden_model(path, dev)
    kind = meta["prediction_type"]
    assert kind in C_OUT and meta["hidden"] == 64
    C = C_OUT[kind]
    scaler = bgnn.ColumnScaler(center=[0.1 * (c + 1) for c in range(C)],
                               scale=[0.8 + 0.3 * c for c in range(C)]) if with_scaler else None
    state = copy.deepcopy(model.state_dict())
    out = []
    seen = []

    class Recording(losses.StressErrorMeter):
        def update(self, pred, target, batch, scale=None, center=None):
            seen.append((pred.clone(), target, batch, scale, center, pred.requires_grad))
            super().update(pred, target, batch, scale, center)

    meter = Recording(kind)
    for m in (None, meter):
        model.load_state_dict(state)
        model.train()
        model.zero_grad(set_to_none=True)
        torch.manual_seed(7)
        opt = torch.optim.SGD(model.parameters(), lr=0.01)
        loss = bgnn.train_step(model, b, opt, bgnn.GraphRelativeError(), scaler, metrics=m)
        out.append((loss, {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None},
                    copy.deepcopy(model.state_dict())))
    assert torch.equal(out[0][0], out[1][0])
    assert set(out[0][1]) == set(out[1][1]) and out[0][1]
    for k in out[0][1]:
        assert torch.equal(out[0][1][k], out[1][1][k]), k
    for k in out[0][2]:
        assert torch.equal(out[0][2][k], out[1][2][k]), k
    # the meter holds stress_errors of the step's detached prediction on the denormalised values,
    # and that prediction is the train-mode forward from the state before the step
    assert len(seen) == 1
    pred, y, out_batch, scale, center, had_grad = seen[0]
    assert not had_grad and (scale is None) == (scaler is None) == (center is None)
    model.load_state_dict(state)
    model.train()
    with torch.no_grad():
        again, again_batch = model(b.x, b.edge_index, b.edge_attr, b.batch)
    assert torch.equal(again_batch, out_batch) and torch.equal(y, b.y)
    np.testing.assert_allclose(pred.cpu().numpy(), again.cpu().numpy(), rtol=1e-4, atol=1e-4)
    if scaler is not None:
        pred, y = scaler.denormalize(pred), scaler.denormalize(y)
    want = losses.stress_errors(pred, y, out_batch, kind, losses.DEFAULT_THRESHOLD[kind])
    assert meter.counts == (int(out_batch.max()) + 1, 1)
    _same(meter.compute("batch"), want, 1e-12)


def test_a_meter_needs_a_static_head(dev):
    from bgnn import synthetic
    b = synthetic.make_batch(8, 2).to(dev)
    torch.manual_seed(0)
    model = bgnn.BuckGNN(16, 5, hidden_channels=64, num_layers=2, dropout_rate=0.0,
                         model_name="GraphSage_addAggr").to(dev).train()
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    with pytest.raises(ValueError):
        bgnn.train_step(model, b, opt, bgnn.RelativeErrorLoss(), metrics=losses.StressErrorMeter("static_disp"))
    shape = bgnn.BuckGNN(16, 5, hidden_channels=64, num_layers=2, dropout_rate=0.0, prediction_type="mode_shape",
                         model_name="GraphSage_addAggr").to(dev).train()
    b.y = torch.randn(b.x.size(0), 3, device=dev)
    with pytest.raises(ValueError):
        bgnn.train_step(shape, b, torch.optim.SGD(shape.parameters(), lr=0.0), bgnn.GraphRelativeError(),
                        metrics=losses.StressErrorMeter("static_stress"))
    with pytest.raises(ValueError):
        bgnn.evaluate_nodes(model, [b])


@pytest.mark.parametrize("kind,super_node,pooling", [("static_disp", False, "mean"),
                                                     ("static_stress", True, "supernode_only")])
def test_evaluate_nodes(dev, kind, super_node, pooling):
    from bgnn import synthetic as S
    from bgnn.data import Batch
    C = C_OUT[kind]
    thr = losses.DEFAULT_THRESHOLD[kind]
    gs = []
    for s in range(5):
        d = S.make_mesh_graph(6 + s, seed=20 + s, super_node=super_node)
        g = torch.Generator().manual_seed(s)
        n_real = d.x.size(0) - (1 if super_node else 0)
        d.y = torch.randn(n_real, C, generator=g)
        gs.append(d)
    torch.manual_seed(1)
    model = bgnn.BuckGNN(16, 5, hidden_channels=64, num_layers=3, pooling_layer=pooling, prediction_type=kind,
                         dropout_rate=0.0, model_name="GraphSage_addAggr").to(dev)
    # denormalised targets on both sides of the threshold
    scaler = bgnn.ColumnScaler(center=[0.1 * thr * (c + 1) for c in range(C)],
                               scale=[3 * thr * (0.8 + 0.3 * c) for c in range(C)])
    crit = bgnn.GraphMAELoss()
    host = [Batch.from_data_list(gs[i:i + 2]) for i in range(0, 5, 2)]
    r1 = bgnn.evaluate_nodes(model, host, scaler, crit, device=dev)
    assert not model.training
    store = bgnn.GraphStore(gs, dev)
    r2 = bgnn.evaluate_nodes(model, store.loader(2), scaler, crit)
    assert r1["graphs"] == r2["graphs"] == 5 and r1["batches"] == r2["batches"] == 3
    # (the two loaders group aggregation rows differently: predictions agree to fp32 rounding)
    for key in ("metrics_per_graph", "metrics_per_batch"):
        assert set(r1[key]) == set(losses.METRIC_KEYS[kind])
        _same(r2[key], r1[key], 5e-5, key)
    assert r2["loss"] == pytest.approx(r1["loss"], rel=1e-5)
    # a hand-written loop: model calls plus stress_errors on the denormalised values
    total = {k: 0.0 for k in losses.METRIC_KEYS[kind]}
    loss = 0.0
    with torch.no_grad():
        for hb in host:
            hb = hb.to(dev)
            pred, ob = model(hb.x, hb.edge_index, hb.edge_attr, hb.batch)
            p, t = scaler.denormalize(pred), scaler.denormalize(hb.y)
            for k, v in losses.stress_errors(p, t, ob, kind, thr).items():
                total[k] += v
            loss += crit(p, t, ob, None).item()
    _same(r1["metrics_per_batch"], {k: v / 3 for k, v in total.items()}, 5e-5, "loop")
    _same(r1["metrics_per_graph"], {k: v / 5 for k, v in total.items()}, 5e-5, "loop")
    assert r1["loss"] == pytest.approx(loss / 3, rel=1e-5)
    assert bgnn.evaluate_nodes(model, host, scaler, device=dev)["loss"] is None
