"""GPU: the bf16 inference path of GraphSage_maxAggr (BuckGNN.infer_bf16 = "all").

Kernel level: bgnn_sage_tail_bf16 against the formula of include/bgnn.h evaluated in fp64 on the
same bf16 inputs, with and without BatchNorm coefficients, a skip input and a strided output. Model
level: the 6-layer max model against the fp64 oracle, with a torch restatement of the same bf16
arithmetic as the yardstick. Switches: True keeps its meaning, "all" adds only the max model, and
every case outside the path is bit-identical to the flag being off."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bgnn
from bgnn import _lib, fused
from bgnn import synthetic as S
from bgnn.data import Batch
from bgnn.graph import _stream

pytestmark = pytest.mark.gpu

# the tolerance of the bgnn_sage_infer_bf16-against-fp64 test (tests/test_gpu_sage_infer.py)
RTOL, ATOL = 1e-4, 1e-4
N_ROWS = 1003   # no multiple of the 8 rows a block takes per trip


# ----------------------------------------------------------------------------- tail kernel
@functools.lru_cache(maxsize=None)
def inputs(n, H):
    g = torch.Generator().manual_seed(1000 + H + n)
    y = torch.randn(n, H, generator=g).bfloat16()
    xp = torch.randn(n, H, generator=g).bfloat16()
    bias = 0.1 * torch.randn(H, generator=g)
    sign = torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0)
    scale = H ** 0.5 * (0.5 + torch.rand(H, generator=g)) * sign
    shift = 0.5 * torch.randn(H, generator=g)
    return y, xp, bias, scale, shift


@functools.lru_cache(maxsize=None)
def reference(n, H, bn, skip):
    """fp64, from the same bf16 inputs (computed once per case, shared by the output forms)."""
    y, xp, bias, scale, shift = inputs(n, H)
    h = y.double() + bias.double()
    o = h / h.norm(dim=1, keepdim=True).clamp_min(1e-12)
    v = torch.relu(o * scale.double() + shift.double()) if bn else torch.relu(o)
    return v + xp.double() if skip else v


def run_tail(n, H, bn, skip, out_f32, strided, dev):
    """The tail's output on the host. strided: out is plane 1 of a [n, 2H] buffer whose plane 0
    must come back untouched (the model path's layout)."""
    y, xp, bias, scale, shift = (t.to(dev) for t in inputs(n, H))
    dt = torch.float32 if out_f32 else torch.bfloat16
    if strided:
        buf = torch.full((n, 2 * H), float("nan"), dtype=dt, device=dev)
        buf[:, :H] = 3.0
        out = buf[:, H:]
    else:
        out = torch.full((n, H), float("nan"), dtype=dt, device=dev)
    _lib.call("bgnn_sage_tail_bf16", y.data_ptr(), y.stride(0), bias.data_ptr(), scale.data_ptr() if bn else None,
              shift.data_ptr() if bn else None, xp.data_ptr() if skip else None, xp.stride(0) if skip else 0, n, H,
              out.data_ptr(), out.stride(0), int(out_f32), _stream())
    torch.cuda.synchronize()
    if strided:
        assert bool((buf[:, :H] == 3.0).all())
    return out.contiguous().cpu()


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("H", [64, 200, 512])
def test_tail_matches_fp64(dev, H, bn, skip, strided):
    n = N_ROWS
    ref = reference(n, H, bn, skip)
    if bn and not skip:   # the inputs do what the test wants: about half the ReLUs fire
        assert 0.3 < float((ref > 0).double().mean()) < 0.7
    o32 = run_tail(n, H, bn, skip, True, strided, dev)
    o16 = run_tail(n, H, bn, skip, False, strided, dev)
    e32 = (o32.double() - ref).abs()
    e16 = (o16.double() - ref).abs()
    print(f"tail H={H} bn={bn} skip={skip} strided={strided}: max f32 err {float(e32.max()):.3e}, "
          f"max bf16 err / bound {float((e16 / (2.0 ** -8 * ref.abs() + ATOL)).max()):.3f}")
    # every element, none excluded
    assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(o16.float()).all())
    assert bool((e32 <= ATOL + RTOL * ref.abs()).all()), float((e32 - RTOL * ref.abs()).max())
    assert bool((e16 <= 2.0 ** -8 * ref.abs() + ATOL).all())
    # the bf16 store is the f32 result rounded once: elements that differ from torch's rounding of
    # the f32 output are counted, split by whether the f32 value sits within 1e-6 relative (9 f32
    # ulps of the 2^16 between bf16 neighbours) of a rounding tie
    diff = o32.bfloat16().view(torch.int16) != o16.view(torch.int16)
    low = o32.view(torch.int32) & 0xFFFF
    near_tie = (low - 0x8000).abs() <= 9
    n_tie, n_other = int((diff & near_tie).sum()), int((diff & ~near_tie).sum())
    print(f"  bf16 store vs rounded f32 store: {n_tie} differ at a tie, {n_other} elsewhere")
    assert n_other == 0 and n_tie == 0


def test_tail_is_the_infer_kernels_tail(dev):
    """Both entry points compile one tail function: with a zero aggregate (z_l = 0 on a ring graph)
    bgnn_sage_infer_bf16 of z = [0 | y] gives the tail's bits."""
    from bgnn.graph import Graph
    n, H = 203, 200
    y, xp, bias, scale, shift = (t[:n].to(dev) if t.dim() == 2 else t.to(dev) for t in inputs(N_ROWS, H))
    i = torch.arange(n, device=dev)
    g = Graph.build(torch.stack([torch.cat([i, i]), torch.cat([(i + 1) % n, (i + 2) % n])]), n)
    assert g.fwd.plan.n_chunks == 0
    z = torch.cat([torch.zeros_like(y), y], 1).contiguous()
    outs = []
    for out_f32 in (True, False):
        a = torch.empty(n, H, dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
        b = torch.empty_like(a)
        _lib.call("bgnn_sage_infer_bf16", g.fwd.ref(), z.data_ptr(), 2 * H, bias.data_ptr(), scale.data_ptr(),
                  shift.data_ptr(), xp.data_ptr(), xp.stride(0), H, 0, a.data_ptr(), H, int(out_f32), None, _stream())
        _lib.call("bgnn_sage_tail_bf16", y.data_ptr(), H, bias.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                  xp.data_ptr(), xp.stride(0), n, H, b.data_ptr(), H, int(out_f32), _stream())
        torch.cuda.synchronize()
        outs.append((a, b))
    for a, b in outs:
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ----------------------------------------------------------------------------- model level
def model_graphs():
    return [S.make_mesh_graph(18, seed=40 + s, super_node=(s % 2 == 1)) for s in range(6)]


def make_model(name, h, dev, seed=77):
    from recipe import make_weights
    torch.manual_seed(0)
    model = bgnn.BuckGNN(16, 5, h, 6, "mean", model_name=name)
    sd = model.state_dict()
    w = make_weights({k: tuple(v.shape) for k, v in sd.items()}, seed)   # non-trivial running statistics
    sd = {k: torch.from_numpy(w[k]) if k in w else sd[k] for k in sd}
    model.load_state_dict(sd)
    return model.to(dev).eval(), sd


def torch_bf16_max_forward(sd, x, ei, batch, num_graphs, L=6):
    """The max path's arithmetic in torch: f32 encoder, x rounded to bf16, per layer an exact max
    over the in-edges (0 for isolated rows), F.linear on [agg | x] with the bf16 [W_l | W_r] and a
    bf16 output, the tail in f32, one bf16 round; the last layer stays f32."""
    from oracle import buckgnn_ref as R
    attr, aggr, use_bn = R.SAGE["GraphSage_maxAggr"]
    assert aggr == "max" and use_bn
    x = R._mlp(sd, "node_encoder", x)
    n, H = x.shape
    src, dst = ei
    idx = dst.view(-1, 1).expand(-1, H)
    for i in range(L):
        pre = f"{attr}.{i}"
        xb = x.bfloat16()
        agg = torch.zeros(n, H, dtype=torch.bfloat16, device=x.device).scatter_reduce(
            0, idx, xb[src], "amax", include_self=False)
        w = torch.cat([sd[pre + ".lin_l.weight"], sd[pre + ".lin_r.weight"]], 1).bfloat16()
        y = F.linear(torch.cat([agg, xb], 1), w)
        o = F.normalize(y.float() + sd[pre + ".lin_l.bias"], p=2.0, dim=-1)
        b = f"batch_norms.{i}"
        o = F.batch_norm(o, sd[b + ".running_mean"], sd[b + ".running_var"], sd[b + ".weight"], sd[b + ".bias"],
                         False, 0.1, 1e-5)
        v = torch.relu(o)
        if 0 < i < L - 1:
            v = v + xb.float()
        x = v if i == L - 1 else v.bfloat16().float()
    cnt = torch.bincount(batch, minlength=num_graphs).clamp_min(1).float().unsqueeze(1)
    pooled = torch.zeros(num_graphs, H, device=x.device).index_add_(0, batch, x) / cnt
    return R._mlp(sd, "decoder", pooled).squeeze()


def rel(a, r):
    return float((a.double().cpu() - r).norm() / r.norm())


@pytest.fixture
def layer_calls(monkeypatch):
    """Counts of the two inference layers' calls: {"max": ..., "sum": ...}."""
    calls = {"max": 0, "sum": 0}
    real_max, real_sum = fused.sage_infer_max_layer, fused.sage_infer_layer

    def counted_max(*a, **k):
        calls["max"] += 1
        return real_max(*a, **k)

    def counted_sum(*a, **k):
        calls["sum"] += 1
        return real_sum(*a, **k)
    monkeypatch.setattr(fused, "sage_infer_max_layer", counted_max)
    monkeypatch.setattr(fused, "sage_infer_layer", counted_sum)
    return calls


@pytest.mark.parametrize("h", [64, 512])
def test_max_model_bf16_close_to_oracle(dev, layer_calls, h):
    from oracle import buckgnn_ref as R
    name = "GraphSage_maxAggr"
    gs = model_graphs()
    model, sd = make_model(name, h, dev)
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    sdd = {k: v.to(dev) for k, v in sd.items()}
    batches = [Batch.from_data_list(gs[0:4]), Batch.from_data_list(gs[4:6])]
    ref, ours, f32, tor = [], [], [], []
    for hb in batches:
        ref.append(R.forward(sd64, name, hb.x.double(), hb.edge_index, hb.batch, False, "mean", 0.0))
        b = hb.to(dev)
        with torch.no_grad():
            f32.append(model(b.x, b.edge_index, b.edge_attr, b.batch)[0])
            model.infer_bf16 = True   # True keeps its meaning: a max model stays on the f32 path
            under_true = model(b.x, b.edge_index, b.edge_attr, b.batch)[0]
            assert layer_calls == {"max": 0, "sum": 0} and torch.equal(under_true, f32[-1])
            model.infer_bf16 = "all"
            ours.append(model(b.x, b.edge_index, b.edge_attr, b.batch)[0])
            model.infer_bf16 = False
            assert layer_calls == {"max": 6, "sum": 0}   # the bf16 path really ran: one call per layer
            layer_calls["max"] = 0
            tor.append(torch_bf16_max_forward(sdd, b.x, b.edge_index, b.batch, hb.num_graphs))
    ref = torch.cat(ref)
    r_ours, r_torch, r_f32 = rel(torch.cat(ours), ref), rel(torch.cat(tor), ref), rel(torch.cat(f32), ref)
    print(f"{name} h={h}: rel L2 vs the fp64 oracle: bf16 path {r_ours:.3e}, torch bf16 {r_torch:.3e}, "
          f"f32 path {r_f32:.3e}")
    assert r_ours <= 1.5 * r_torch + 1e-4, (r_ours, r_torch)

    # the inference driver's switch: metrics of a direct computation from its predictions, and the
    # model's own flag is left as it was
    scaler = bgnn.EigenvalueScaler(2.0, 0.75)
    r = bgnn.evaluate(model, batches, scaler, device=dev, bf16="all")
    assert model.infer_bf16 is False
    assert layer_calls == {"max": 12, "sum": 0}
    torch.testing.assert_close(r["predictions"], scaler.denormalize_eigenvalue(torch.cat(ours)), rtol=0, atol=0)
    t = scaler.denormalize_eigenvalue(torch.cat([hb.y for hb in batches])).double().numpy()
    p = r["predictions"].view(-1).double().cpu().numpy()
    ape = np.abs((t.reshape(-1) - p) / t.reshape(-1)) * 100
    assert r["mape"] == pytest.approx(ape.mean(), rel=1e-5)
    assert r["max_mape"] == pytest.approx(ape.max(), rel=1e-5)
    assert r["min_mape"] == pytest.approx(ape.min(), rel=1e-5)
    assert r["graphs"] == 6
    layer_calls["max"] = 0
    model.infer_bf16 = "all"
    bgnn.evaluate(model, batches[:1], scaler, device=dev, bf16=True)
    assert model.infer_bf16 == "all" and layer_calls == {"max": 0, "sum": 0}
    bgnn.evaluate(model, batches[:1], scaler, device=dev)
    assert model.infer_bf16 == "all" and layer_calls == {"max": 6, "sum": 0}


# ----------------------------------------------------------------------------- switches
def test_sum_model_under_all_is_the_path_under_true(dev, layer_calls):
    b = Batch.from_data_list(model_graphs()[0:4]).to(dev)
    model, _ = make_model("GraphSage_addAggr", 64, dev)
    preds = []
    with torch.no_grad():
        for flag in (True, "all"):
            model.infer_bf16 = flag
            preds.append(model(b.x, b.edge_index, b.edge_attr, b.batch)[0])
    assert layer_calls == {"max": 0, "sum": 12}
    assert torch.equal(preds[0], preds[1])


def _fallback_model(case, dev):
    name, h = "GraphSage_maxAggr", 64
    if case == "sag":
        name = "GraphSAGE_SAG"
    elif case == "h68":
        h = 68
    torch.manual_seed(3)
    model = bgnn.BuckGNN(16, 5, h, 6, "mean", model_name=name).to(dev)
    if case == "bn_no_running_stats":
        model.batch_norms[2] = torch.nn.BatchNorm1d(h, track_running_stats=False).to(dev)
    return model.train() if case == "train" else model.eval()


@pytest.mark.parametrize("case", ["train", "grad", "sag", "h68", "bn_no_running_stats"])
def test_fallbacks_under_all_are_bit_identical(dev, layer_calls, case):
    b = Batch.from_data_list(model_graphs()[0:4]).to(dev)
    preds = []
    for flag in (False, "all"):
        model = _fallback_model(case, dev)   # the same weights both times (seeded)
        model.infer_bf16 = flag
        torch.manual_seed(11)   # the train-mode dropout seeds
        with torch.set_grad_enabled(case in ("train", "grad")):
            preds.append(model(b.x, b.edge_index, b.edge_attr, b.batch)[0].detach())
    assert layer_calls == {"max": 0, "sum": 0}
    assert torch.equal(preds[0], preds[1])


# ----------------------------------------------------------------------------- weight cache
def test_max_weight_cache_follows_the_weights(dev):
    """[W_l | W_r] as bf16 is built once per weight version, not per call, beside infer_weights'."""
    model, _ = make_model("GraphSage_maxAggr", 64, dev)
    conv = model.sage_blocks_max[0]
    w0 = fused.infer_weights_max(conv)
    assert fused.infer_weights_max(conv) is w0
    assert w0.shape == (64, 128) and w0.dtype == torch.bfloat16
    assert torch.equal(w0, torch.cat([conv.lin_l.weight, conv.lin_r.weight], 1).detach().bfloat16())
    assert fused.infer_weights(conv) is not w0 and fused.infer_weights_max(conv) is w0   # its own attribute
    with torch.no_grad():
        conv.lin_r.weight.mul_(2.0)
    w1 = fused.infer_weights_max(conv)
    assert w1 is not w0 and torch.equal(w1[:, 64:], conv.lin_r.weight.detach().bfloat16())
    assert fused.infer_weights_max(conv) is w1
