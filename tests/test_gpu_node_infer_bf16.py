"""GPU: bf16 inference of the node-level heads with the decoder on bf16 rows
(BuckGNN.infer_bf16_decoder; evaluate_nodes(bf16=..., return_predictions=...)).

Model level: 6-layer models (skip layers exist) with non-trivial running statistics on three
19 x 19 meshes (N >= 1024) against the fp64 oracle, with a torch restatement of this path's
rounding points as the yardstick: r_ours <= 1.5 r_torch + 1e-4 in relative L2 over all [n, C]
entries (the margin tests/test_gpu_sage_infer.py and tests/test_gpu_sage_infer_max.py use for the
layer loop). Route: a spy on _lib.call sees bgnn_head2_fwd_bf16 once and bgnn_head2_fwd not at all;
under infer_bf16 alone it sees bgnn_head2_fwd once (that route's bits cannot be recorded from the
code before this path existed without a GPU run of it, so the route is what is asserted).
Fall-backs: every case outside the path is bit-identical to the flag being off."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bgnn
from bgnn import _lib, losses
from bgnn import synthetic as S

pytestmark = pytest.mark.gpu
C_OUT = {"static_disp": 2, "static_stress": 3, "mode_shape": 3}
L = 6
# model_name, hidden, prediction_type, infer_bf16, super nodes, pooling
CASES = [
    ("GraphSage_addAggr", 64, "static_disp", True, False, "mean"),
    ("GraphSage_meanAggr", 512, "static_stress", True, False, "mean"),
    ("GraphSage_addAggr_Shared", 128, "mode_shape", True, False, "mean"),
    ("GraphSage_maxAggr", 512, "static_stress", "all", False, "mean"),
    ("GraphSage_addAggr", 64, "static_stress", True, True, "supernode_only"),
]
IDS = ["add_h64_disp", "mean_h512_stress", "shared_h128_mode", "max_h512_stress_all", "add_h64_stress_super"]


@functools.lru_cache(maxsize=None)
def host_batch(super_node, ptype, seed=0, n=19):
    """Three n x n meshes (n = 19: 1,083 nodes; 1,086 with super nodes) with a node-level y."""
    b = S.make_batch(n, 3, super_node=super_node, seed0=seed)
    g = torch.Generator().manual_seed(seed + 77)
    n_real = int((b.x[:, -1] == 0).sum()) if super_node else b.x.size(0)
    y = torch.rand(n_real, C_OUT.get(ptype, 1), generator=g) * 1.5 + 0.5
    b.y = y * torch.where(torch.rand(y.shape, generator=g) < 0.5, -1.0, 1.0)
    return b


def make_model(name, h, ptype, pooling, dev, seed=77, **kw):
    from recipe import make_weights
    torch.manual_seed(0)
    model = bgnn.BuckGNN(16, 5, hidden_channels=h, num_layers=L, pooling_layer=pooling, prediction_type=ptype,
                         dropout_rate=kw.pop("dropout_rate", 0.0), model_name=name, **kw)
    sd = model.state_dict()
    w = make_weights({k: tuple(v.shape) for k, v in sd.items()}, seed)   # non-trivial running statistics
    sd = {k: torch.from_numpy(w[k]) if k in w else sd[k] for k in sd}
    model.load_state_dict(sd)
    return model.to(dev).eval(), sd


@pytest.fixture
def spy(monkeypatch):
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    return calls


def run(model, b, infer, dec):
    model.infer_bf16, model.infer_bf16_decoder = infer, dec
    try:
        with torch.no_grad():
            return model(b.x, b.edge_index, b.edge_attr, b.batch)
    finally:
        model.infer_bf16, model.infer_bf16_decoder = False, False


def torch_rows_bf16(sd, name, x, ei):
    """The layer loop's rounding points in torch, the last layer rounded to bf16 too: the sum /
    mean / Shared loop as torch_bf16_forward of tests/test_gpu_sage_infer.py (f32 encoder, per layer
    bf16 x and weights, F.linear with a bf16 output, f32 aggregation and tail, one bf16 round), the
    max loop as torch_bf16_max_forward of tests/test_gpu_sage_infer_max.py (an exact bf16 max, one
    F.linear over [agg | x])."""
    from oracle import buckgnn_ref as R
    attr, aggr, use_bn = R.SAGE[name]
    x = R._mlp(sd, "node_encoder", x)
    n, H = x.shape
    src, dst = ei
    deg = torch.bincount(dst, minlength=n).clamp_min(1).float().unsqueeze(1)
    idx = dst.view(-1, 1).expand(-1, H)
    for i in range(L):
        pre = attr if name.endswith("_Shared") else f"{attr}.{i}"
        xb = x.bfloat16()
        if aggr == "max":
            agg = torch.zeros(n, H, dtype=torch.bfloat16, device=x.device).scatter_reduce(
                0, idx, xb[src], "amax", include_self=False)
            w = torch.cat([sd[pre + ".lin_l.weight"], sd[pre + ".lin_r.weight"]], 1).bfloat16()
            pre_norm = F.linear(torch.cat([agg, xb], 1), w).float()
        else:
            zl = F.linear(xb, sd[pre + ".lin_l.weight"].bfloat16())
            zr = F.linear(xb, sd[pre + ".lin_r.weight"].bfloat16())
            agg = torch.zeros(n, H, device=x.device).index_add_(0, dst, zl.float()[src])
            if aggr == "mean":
                agg = agg / deg
            pre_norm = agg + zr.float()
        o = F.normalize(pre_norm + sd[pre + ".lin_l.bias"], p=2.0, dim=-1)
        if use_bn:
            b = f"batch_norms.{i}"
            o = F.batch_norm(o, sd[b + ".running_mean"], sd[b + ".running_var"], sd[b + ".weight"], sd[b + ".bias"],
                             False, 0.1, 1e-5)
        y = torch.relu(o)
        if 0 < i < L - 1:
            y = y + xb.float()
        x = y.bfloat16().float()
    return x.bfloat16()


def torch_decoder_bf16(sd, rows):
    """The decoder on bf16 rows as this path rounds: at h >= 256 the front Linear as autocast's bf16
    F.linear (bf16 rows, weight and bias; bf16 output) with its ReLU; the last two Linears in f32
    on the widened rows."""
    idx = sorted({int(k.split(".")[1]) for k in sd if k.startswith("decoder.")})
    x = rows
    if len(idx) == 3:
        i = idx[0]
        x = torch.relu(F.linear(x, sd[f"decoder.{i}.weight"].bfloat16(), sd[f"decoder.{i}.bias"].bfloat16()))
        idx = idx[1:]
    x = x.float()
    x = torch.relu(F.linear(x, sd[f"decoder.{idx[0]}.weight"], sd[f"decoder.{idx[0]}.bias"]))
    return F.linear(x, sd[f"decoder.{idx[1]}.weight"], sd[f"decoder.{idx[1]}.bias"])


def rel(a, r):
    return float((a.double().cpu() - r).norm() / r.norm())


@pytest.mark.parametrize("name,h,ptype,flag,super_node,pooling", CASES, ids=IDS)
def test_bf16_decoder_path(dev, spy, name, h, ptype, flag, super_node, pooling):
    from oracle import buckgnn_ref as R
    hb = host_batch(super_node, ptype)
    assert hb.x.size(0) >= 1024
    b = hb.to(dev)
    model, sd = make_model(name, h, ptype, pooling, dev)
    f32, f32_batch = run(model, b, False, False)
    assert "bgnn_head2_fwd_bf16" not in spy and spy.count("bgnn_head2_fwd") == 1
    # infer_bf16 alone keeps its route: the bf16 loop, the f32 hand-over, the f32 tail
    del spy[:]
    old, old_batch = run(model, b, flag, False)
    assert spy.count("bgnn_head2_fwd") == 1 and "bgnn_head2_fwd_bf16" not in spy
    loop = "bgnn_sage_tail_bf16" if "max" in name else "bgnn_sage_infer_bf16"
    assert spy.count(loop) == L
    # the new path really ran
    del spy[:]
    ours, ours_batch = run(model, b, flag, True)
    assert spy.count("bgnn_head2_fwd_bf16") == 1 and "bgnn_head2_fwd" not in spy
    assert spy.count(loop) == L
    # the returned batch vector and the shape are the f32 path's, super nodes filtered
    assert ours.dtype == torch.float32 and ours.shape == f32.shape == old.shape == hb.y.shape
    assert torch.equal(ours_batch, f32_batch) and torch.equal(old_batch, f32_batch)
    # accuracy against the fp64 oracle, torch's restatement of the same rounding points as yardstick
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    _, nodes = R.forward(sd64, name, hb.x.double(), hb.edge_index, hb.batch, False, pooling, 0.0, num_layers=L,
                         return_nodes=True)
    real = hb.x[:, -1] == 0 if super_node else torch.ones(hb.x.size(0), dtype=torch.bool)
    ref = R._mlp(sd64, "decoder", nodes[real])
    assert torch.equal(f32_batch.cpu(), hb.batch[real])
    sdd = {k: v.to(dev) for k, v in sd.items()}
    with torch.no_grad():
        tor = torch_decoder_bf16(sdd, torch_rows_bf16(sdd, name, b.x, b.edge_index))[real.to(dev)]
    r_ours, r_torch, r_f32, r_old = rel(ours, ref), rel(tor, ref), rel(f32, ref), rel(old, ref)
    print(f"{name} h={h} {ptype}: rel L2 vs the fp64 oracle: bf16 decoder path {r_ours:.3e}, torch restatement "
          f"{r_torch:.3e}, f32 path {r_f32:.3e} (infer_bf16 alone {r_old:.3e})")
    assert r_ours <= 1.5 * r_torch + 1e-4, (r_ours, r_torch)
    # deterministic
    assert torch.equal(run(model, b, flag, True)[0], ours)


def _same(d, ref, rel_tol, tag=None):
    assert sorted(d) == sorted(ref), tag
    for k, v in ref.items():
        if np.isnan(v):
            assert np.isnan(d[k]), (tag, k, d[k])
        else:
            assert d[k] == pytest.approx(v, rel=rel_tol, abs=1e-6), (tag, k, d[k], v)


@pytest.mark.parametrize("name,h,flag", [("GraphSage_addAggr", 64, True), ("GraphSage_maxAggr", 512, "all")],
                         ids=["add_h64", "max_h512_all"])
def test_evaluate_nodes_bf16_and_predictions(dev, spy, name, h, flag):
    kind = "static_stress"
    thr = losses.DEFAULT_THRESHOLD[kind]
    hosts = [host_batch(False, kind, seed=0), host_batch(False, kind, seed=5)]
    model, _ = make_model(name, h, kind, "mean", dev)
    scaler = bgnn.ColumnScaler(center=[0.1 * thr * (c + 1) for c in range(3)],
                               scale=[3 * thr * (0.8 + 0.3 * c) for c in range(3)])
    direct = [run(model, hb.to(dev), flag, True) for hb in hosts]
    assert spy.count("bgnn_head2_fwd_bf16") == 2
    del spy[:]
    # attributes pre-existing: both are as before the call
    model.infer_bf16, model.infer_bf16_decoder = False, False
    r = bgnn.evaluate_nodes(model, hosts, scaler, device=dev, bf16=flag, return_predictions=True)
    assert model.infer_bf16 is False and model.infer_bf16_decoder is False
    assert spy.count("bgnn_head2_fwd_bf16") == 2 and "bgnn_head2_fwd" not in spy
    assert r["graphs"] == 6 and r["batches"] == 2 and len(r["predictions"]) == 2
    meter = losses.StressErrorMeter(kind)
    for (p, ob), (dp, dob), hb in zip(r["predictions"], direct, hosts):
        assert torch.equal(p, scaler.denormalize(dp)) and torch.equal(ob, dob)   # bit for bit
        meter.update(p, scaler.denormalize(hb.y.to(dev)), ob)
    # (the driver folds the scaler into the metric kernel: tests/test_gpu_stress_meter.py's 5e-5)
    _same(r["metrics_per_graph"], meter.compute("graph"), 5e-5, "graph")
    total = {k: 0.0 for k in losses.METRIC_KEYS[kind]}
    for (p, ob), hb in zip(r["predictions"], hosts):
        for k, v in losses.stress_errors(p, scaler.denormalize(hb.y.to(dev)), ob, kind, thr).items():
            total[k] += v
    _same(r["metrics_per_graph"], {k: v / 6 for k, v in total.items()}, 5e-5, "stress_errors")
    # without return_predictions the dict is the one it was
    r0 = bgnn.evaluate_nodes(model, hosts, scaler, device=dev, bf16=flag)
    assert set(r0) == {"metrics_per_graph", "metrics_per_batch", "graphs", "batches", "loss"}
    _same(r0["metrics_per_graph"], r["metrics_per_graph"], 1e-12, "no predictions")
    # attributes absent (a model object from before the flags): absent again afterwards
    del model.infer_bf16, model.infer_bf16_decoder
    bgnn.evaluate_nodes(model, hosts[:1], scaler, device=dev, bf16=flag)
    assert "infer_bf16" not in vars(model) and "infer_bf16_decoder" not in vars(model)
    # bf16=False on a flagged model: neither bf16 kernel
    model.infer_bf16, model.infer_bf16_decoder = flag, True
    del spy[:]
    rf = bgnn.evaluate_nodes(model, hosts[:1], scaler, device=dev, bf16=False, return_predictions=True)
    assert model.infer_bf16 == flag and model.infer_bf16_decoder is True
    assert not {"bgnn_head2_fwd_bf16", "bgnn_sage_infer_bf16", "bgnn_sage_tail_bf16", "bgnn_spmm_max_bf16"} & set(spy)
    assert spy.count("bgnn_head2_fwd") == 1
    f32 = run(model, hosts[0].to(dev), False, False)[0]
    assert torch.equal(rf["predictions"][0][0], scaler.denormalize(f32))
    # bf16=None follows the model
    model.infer_bf16, model.infer_bf16_decoder = flag, True
    del spy[:]
    rn = bgnn.evaluate_nodes(model, hosts[:1], scaler, device=dev, return_predictions=True)
    assert model.infer_bf16 == flag and model.infer_bf16_decoder is True
    assert spy.count("bgnn_head2_fwd_bf16") == 1 and "bgnn_head2_fwd" not in spy
    assert torch.equal(rn["predictions"][0][0], r["predictions"][0][0])
    model.infer_bf16, model.infer_bf16_decoder = False, False
    del spy[:]
    bgnn.evaluate_nodes(model, hosts[:1], scaler, device=dev)
    assert "bgnn_head2_fwd_bf16" not in spy and spy.count("bgnn_head2_fwd") == 1


# ----------------------------------------------------------------------------- fall-backs
FALLBACKS = ["train", "grad", "buckling", "sag", "ea", "h68", "hooked", "small_n", "bn_no_running_stats",
             "infer_bf16_off", "max_under_true"]


def _fallback(case, dev):
    """(model, batch, infer_bf16) of a case outside the path; the same weights on every call."""
    name, h, ptype, infer, n = "GraphSage_addAggr", 64, "static_disp", True, 19
    if case == "max_under_true":
        name = "GraphSage_maxAggr"
    elif case == "sag":
        name = "GraphSAGE_SAG"
    elif case == "ea":
        name = "EA_GNN"
    elif case == "h68":
        h = 68
    elif case == "buckling":
        ptype = "buckling"
    elif case == "small_n":
        n = 10
    elif case == "infer_bf16_off":
        infer = False
    torch.manual_seed(3)
    model = bgnn.BuckGNN(16, 5, hidden_channels=h, num_layers=L, prediction_type=ptype,
                         dropout_rate=0.1 if case == "train" else 0.0, model_name=name).to(dev)
    if case == "bn_no_running_stats":
        model.batch_norms[2] = torch.nn.BatchNorm1d(h, track_running_stats=False).to(dev)
    if case == "hooked":
        model.decoder.register_forward_hook(lambda m, i, o: None)
    model = model.train() if case == "train" else model.eval()
    b = host_batch(False, ptype, n=n).to(dev)
    assert (b.x.size(0) >= 1024) == (case != "small_n")
    return model, b, infer


@pytest.mark.parametrize("case", FALLBACKS)
def test_fallbacks_are_bit_identical(dev, spy, case):
    preds = []
    for dec in (False, True):
        model, b, infer = _fallback(case, dev)
        model.infer_bf16, model.infer_bf16_decoder = infer, dec
        torch.manual_seed(11)   # the train-mode dropout seeds
        with torch.set_grad_enabled(case in ("train", "grad")):
            pred, ob = model(b.x, b.edge_index, b.edge_attr, b.batch)
        preds.append((pred.detach(), ob))
    assert "bgnn_head2_fwd_bf16" not in spy
    assert torch.equal(preds[0][0], preds[1][0])
    assert (preds[0][1] is None and preds[1][1] is None) or torch.equal(preds[0][1], preds[1][1])
