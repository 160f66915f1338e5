"""GPU: the bf16 inference path of the GraphSAGE models (BuckGNN.infer_bf16).

Kernel level: bgnn_sage_infer_bf16 against the formula of include/bgnn.h evaluated in fp64 on the
same bf16 inputs -- isolated rows, duplicated edges, rows at the chunk boundary (in-degree 64 and
65), a row of several chunks, a last group of fewer rows than the plan's, a GraphStore batch (group
starts given explicitly) -- on every kernel the entry point can take (row groups of 4 and 8, one
row per wave). Model level: the 6-layer models against the fp64 oracle, with torch's own bf16
arithmetic as the yardstick. Fall-backs: every case outside the path is bit-identical to the flag
being off."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bgnn
from bgnn import _lib, fused
from bgnn import synthetic as S
from bgnn.data import Batch
from bgnn.graph import Csr, Graph, _graph_cache, _stream, enqueue_groups

pytestmark = pytest.mark.gpu

# the tolerance of the bgnn_sage_fwd-against-fp64 test (tests/test_gpu_fused.py TOL)
RTOL, ATOL = 1e-4, 1e-4
N_HAND = 1003


# ----------------------------------------------------------------------------- kernel level
@functools.lru_cache(maxsize=None)
def hand_edges():
    """[2, E] int64: N = 1,003 (251 groups of 4, the last of 3 rows). Rows 0..899 draw 1..8 sources
    (repeats allowed); row 20 holds duplicated edges; row 10 has in-degree exactly 64, row 11 65
    (the chunk boundary), row 500 in-degree 700 (11 chunks); rows 900..999 and 1001 are isolated;
    rows 1000 and 1002 (the short last group) have edges."""
    g = torch.Generator().manual_seed(5)
    src, dst = [], []

    def add(d, s):
        s = torch.as_tensor(s, dtype=torch.int64)
        src.append(s)
        dst.append(torch.full_like(s, d))

    for d in range(900):
        if d in (10, 11, 20, 500):
            continue
        add(d, torch.randint(0, N_HAND, (int(torch.randint(1, 9, (1,), generator=g)),), generator=g))
    add(20, [3, 3, 3, 7, 7, 1002])
    add(10, torch.randint(0, N_HAND, (64,), generator=g))
    add(11, torch.randint(0, N_HAND, (65,), generator=g))
    add(500, torch.randint(0, N_HAND, (700,), generator=g))
    add(1000, [0, 999, 1001])
    add(1002, [1002, 5])
    ei = torch.stack([torch.cat(src), torch.cat(dst)])
    return ei[:, torch.randperm(ei.size(1), generator=g)]


@functools.lru_cache(maxsize=None)
def store_batch_host():
    return S.make_batch(18, 3, super_node=True)


_graphs = {}


def graph_case(kind, dev):
    """(edge_index on the host, N, forward Csr) of a structure case, built once."""
    if kind in _graphs:
        return _graphs[kind]
    if kind == "store":   # gathered per-graph plans: grow is non-NULL
        hb = store_batch_host()
        store = bgnn.GraphStore([S.make_mesh_graph(18, s, super_node=True) for s in range(3)], dev)
        b = store.batch([0, 1, 2])
        assert torch.equal(b.edge_index.cpu(), hb.edge_index)
        g = _graph_cache.peek(b.edge_index, (b.num_nodes, 64))
        assert g is not None and g.fwd.groups is not None and g.fwd.groups.grow is not None
        assert g.fwd.plan.n_heavy == 3
        out = (hb.edge_index, hb.num_nodes, g.fwd, (store, b, g))
    else:
        ei = hand_edges()
        g = Graph.build(ei.to(dev), N_HAND)
        f = g.fwd
        deg = f.degree().cpu()
        assert (int(deg[10]), int(deg[11]), int(deg[500]), int(deg[950])) == (64, 65, 700, 0)
        assert f.plan.n_heavy == 2 and f.plan.n_chunks == 2 + 11
        assert f.groups is not None and f.groups.grow is None and f.groups.rows == 4
        if kind == "hand":
            csr = f
        elif kind == "hand_r8":
            csr = Csr(f.rowptr, f.col, f.n_rows, f.nnz, f.plan,
                      enqueue_groups(f.rowptr, f.col, f.n_rows, f.nnz, f.plan.chunk, rows=8))
        else:   # no row-group plan: one row per wave
            csr = Csr(f.rowptr, f.col, f.n_rows, f.nnz, f.plan, None)
        out = (ei, N_HAND, csr, g)
    _graphs[kind] = out
    return out


@functools.lru_cache(maxsize=None)
def inputs(n, H):
    g = torch.Generator().manual_seed(1000 + H + n)
    z = torch.randn(n, 2 * H, generator=g).bfloat16()
    xp = torch.randn(n, H, generator=g).bfloat16()
    bias = 0.1 * torch.randn(H, generator=g)
    sign = torch.where(torch.rand(H, generator=g) < 0.5, -1.0, 1.0)
    scale = H ** 0.5 * (0.5 + torch.rand(H, generator=g)) * sign
    shift = 0.5 * torch.randn(H, generator=g)
    return z, xp, bias, scale, shift


@functools.lru_cache(maxsize=None)
def reference(kind, n, H, mean, bn, skip):
    """fp64, from the same bf16 inputs (computed once per case, shared by the kernel variants)."""
    ei = hand_edges() if kind == "hand" else store_batch_host().edge_index
    z, xp, bias, scale, shift = inputs(n, H)
    zl, zr = z[:, :H].double(), z[:, H:].double()
    agg = torch.zeros(n, H, dtype=torch.float64).index_add_(0, ei[1], zl[ei[0]])
    if mean:
        agg = agg / torch.bincount(ei[1], minlength=n).clamp_min(1).double().unsqueeze(1)
    h = agg + zr + bias.double()
    o = h / h.norm(dim=1, keepdim=True).clamp_min(1e-12)
    y = torch.relu(o * scale.double() + shift.double()) if bn else torch.relu(o)
    return y + xp.double() if skip else y


def run_kernel(csr, n, H, mean, bn, skip, out_f32, dev):
    z, xp, bias, scale, shift = (t.to(dev) for t in inputs(n, H))
    out = torch.full((n, H), float("nan"), dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
    part = torch.empty(max(csr.plan.n_chunks, 1) * H, dtype=torch.float32, device=dev)
    _lib.call("bgnn_sage_infer_bf16", csr.ref(), z.data_ptr(), 2 * H, bias.data_ptr(),
              scale.data_ptr() if bn else None, shift.data_ptr() if bn else None,
              xp.data_ptr() if skip else None, H, H, int(mean), out.data_ptr(), H, int(out_f32),
              part.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu()


def check_case(kind, H, mean, bn, skip, dev):
    ref_kind = "store" if kind == "store" else "hand"
    _, n, csr, _keep = graph_case(kind, dev)
    ref = reference(ref_kind, n, H, mean, bn, skip)
    if bn and not skip:   # the inputs do what the test wants: about half the ReLUs fire
        assert 0.3 < float((ref > 0).double().mean()) < 0.7
    o32 = run_kernel(csr, n, H, mean, bn, skip, True, dev)
    o16 = run_kernel(csr, n, H, mean, bn, skip, False, dev)
    e32 = (o32.double() - ref).abs()
    e16 = (o16.double() - ref).abs()
    print(f"{kind} H={H} mean={mean} bn={bn} skip={skip}: max f32 err {float(e32.max()):.3e}, "
          f"max bf16 err / bound {float((e16 / (2.0 ** -8 * ref.abs() + ATOL)).max()):.3f}")
    # every element, none excluded
    assert bool(torch.isfinite(o32).all()) and bool(torch.isfinite(o16.float()).all())
    assert bool((e32 <= ATOL + RTOL * ref.abs()).all()), float((e32 - RTOL * ref.abs()).max())
    assert bool((e16 <= 2.0 ** -8 * ref.abs() + ATOL).all())
    # deterministic run to run
    assert torch.equal(o32, run_kernel(csr, n, H, mean, bn, skip, True, dev))
    assert torch.equal(o16.view(torch.int16), run_kernel(csr, n, H, mean, bn, skip, False, dev).view(torch.int16))
    # the bf16 store is the f32 result rounded once: elements that differ from torch's rounding of
    # the f32 output are counted, split by whether the f32 value sits within 1e-6 relative (9 f32
    # ulps of the 2^16 between bf16 neighbours) of a rounding tie
    diff = o32.bfloat16().view(torch.int16) != o16.view(torch.int16)
    low = o32.view(torch.int32) & 0xFFFF
    near_tie = (low - 0x8000).abs() <= 9
    n_tie, n_other = int((diff & near_tie).sum()), int((diff & ~near_tie).sum())
    print(f"  bf16 store vs rounded f32 store: {n_tie} differ at a tie, {n_other} elsewhere")
    assert n_other == 0 and n_tie == 0


@pytest.mark.parametrize("skip", [False, True])
@pytest.mark.parametrize("bn", [False, True])
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("H", [64, 200, 512])
@pytest.mark.parametrize("kind", ["hand", "store"])
def test_kernel_matches_fp64(dev, kind, H, mean, bn, skip):
    check_case(kind, H, mean, bn, skip, dev)


@pytest.mark.parametrize("mean,bn,skip", [(False, True, True), (True, False, False)])
@pytest.mark.parametrize("H", [200, 512])
@pytest.mark.parametrize("kind", ["hand_r8", "hand_rows"])
def test_kernel_other_plans(dev, kind, H, mean, bn, skip):
    """Row groups of 8 and a CSR without a row-group plan (one row per wave)."""
    check_case(kind, H, mean, bn, skip, dev)


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


def torch_bf16_forward(sd, name, x, ei, batch, num_graphs, L=6):
    """What autocast would store: f32 encoder, then per layer bf16 x, bf16 weights, F.linear with a
    bf16 output, f32 index_add aggregation, f32 tail, one bf16 round; the last layer stays f32."""
    from oracle import buckgnn_ref as R
    attr, aggr, use_bn = R.SAGE[name]
    x = R._mlp(sd, "node_encoder", x)
    n = x.size(0)
    src, dst = ei
    deg = torch.bincount(dst, minlength=n).clamp_min(1).float().unsqueeze(1)
    for i in range(L):
        pre = attr if name.endswith("_Shared") else f"{attr}.{i}"
        xb = x.bfloat16()
        zl = F.linear(xb, sd[pre + ".lin_l.weight"].bfloat16())
        zr = F.linear(xb, sd[pre + ".lin_r.weight"].bfloat16())
        agg = torch.zeros(n, x.size(1), device=x.device).index_add_(0, dst, zl.float()[src])
        if aggr == "mean":
            agg = agg / deg
        o = F.normalize(agg + zr.float() + sd[pre + ".lin_l.bias"], p=2.0, dim=-1)
        if use_bn:
            b = f"batch_norms.{i}"
            o = F.batch_norm(o, sd[b + ".running_mean"], sd[b + ".running_var"], sd[b + ".weight"], sd[b + ".bias"],
                             False, 0.1, 1e-5)
        y = torch.relu(o)
        if 0 < i < L - 1:
            y = y + xb.float()
        x = y if i == L - 1 else y.bfloat16().float()
    cnt = torch.bincount(batch, minlength=num_graphs).clamp_min(1).float().unsqueeze(1)
    pooled = torch.zeros(num_graphs, x.size(1), device=x.device).index_add_(0, batch, x) / cnt
    return R._mlp(sd, "decoder", pooled).squeeze()


def rel(a, r):
    return float((a.double().cpu() - r).norm() / r.norm())


@pytest.fixture
def layer_calls(monkeypatch):
    calls = []
    real = fused.sage_infer_layer

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(fused, "sage_infer_layer", counted)
    return calls


@pytest.mark.parametrize("name,h", [("GraphSage_addAggr", 64), ("GraphSage_meanAggr", 64),
                                    ("GraphSage_addAggr", 512), ("GraphSage_meanAggr", 512),
                                    ("GraphSage_addAggr_Shared", 64)])
def test_model_bf16_close_to_oracle(dev, layer_calls, name, h):
    from oracle import buckgnn_ref as R
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
            assert not layer_calls
            model.infer_bf16 = True
            ours.append(model(b.x, b.edge_index, b.edge_attr, b.batch)[0])
            model.infer_bf16 = False
            assert len(layer_calls) == 6   # the bf16 path really ran: one call per layer
            layer_calls.clear()
            tor.append(torch_bf16_forward(sdd, name, b.x, b.edge_index, b.batch, hb.num_graphs))
    ref = torch.cat(ref)
    r_ours, r_torch, r_f32 = rel(torch.cat(ours), ref), rel(torch.cat(tor), ref), rel(torch.cat(f32), ref)
    print(f"{name} h={h}: rel L2 vs the fp64 oracle: bf16 path {r_ours:.3e}, torch bf16 {r_torch:.3e}, "
          f"f32 path {r_f32:.3e}")
    assert r_ours <= 1.5 * r_torch + 1e-4, (r_ours, r_torch)

    # the inference driver's switch: metrics of a direct computation from its predictions, and the
    # model's own flag is left as it was
    scaler = bgnn.EigenvalueScaler(2.0, 0.75)
    r = bgnn.evaluate(model, batches, scaler, device=dev, bf16=True)
    assert model.infer_bf16 is False
    assert len(layer_calls) == 12
    torch.testing.assert_close(r["predictions"], scaler.denormalize_eigenvalue(torch.cat(ours)), rtol=0, atol=0)
    t = scaler.denormalize_eigenvalue(torch.cat([hb.y for hb in batches])).double().numpy()
    p = r["predictions"].view(-1).double().cpu().numpy()
    ape = np.abs((t.reshape(-1) - p) / t.reshape(-1)) * 100
    assert r["mape"] == pytest.approx(ape.mean(), rel=1e-5)
    assert r["max_mape"] == pytest.approx(ape.max(), rel=1e-5)
    assert r["min_mape"] == pytest.approx(ape.min(), rel=1e-5)
    assert r["graphs"] == 6
    layer_calls.clear()
    model.infer_bf16 = True
    bgnn.evaluate(model, batches[:1], scaler, device=dev, bf16=False)
    assert model.infer_bf16 is True and not layer_calls
    bgnn.evaluate(model, batches[:1], scaler, device=dev)
    assert model.infer_bf16 is True and len(layer_calls) == 6


def test_weight_cache_follows_the_weights(dev):
    """[W_l ; W_r] as bf16 is built once per weight version, not per call."""
    model, _ = make_model("GraphSage_addAggr", 64, dev)
    conv = model.sage_blocks_add[0]
    w0 = fused.infer_weights(conv)
    assert fused.infer_weights(conv) is w0
    assert torch.equal(w0, torch.cat([conv.lin_l.weight, conv.lin_r.weight]).detach().bfloat16())
    with torch.no_grad():
        conv.lin_r.weight.mul_(2.0)
    w1 = fused.infer_weights(conv)
    assert w1 is not w0 and torch.equal(w1[64:], conv.lin_r.weight.detach().bfloat16())


# ----------------------------------------------------------------------------- fall-backs
def _fallback_model(case, dev):
    name, h = "GraphSage_addAggr", 64
    if case == "max":
        name = "GraphSage_maxAggr"
    elif case == "sag":
        name = "GraphSAGE_SAG"
    elif case == "h68":
        h = 68
    torch.manual_seed(3)
    model = bgnn.BuckGNN(16, 5, h, 6, "mean", model_name=name).to(dev)
    if case == "bn_no_running_stats":
        model.batch_norms[2] = torch.nn.BatchNorm1d(h, track_running_stats=False).to(dev)
    return model.train() if case == "train" else model.eval()


@pytest.mark.parametrize("case", ["train", "grad", "max", "sag", "h68", "bn_no_running_stats"])
def test_fallbacks_are_bit_identical(dev, layer_calls, case):
    b = Batch.from_data_list(model_graphs()[0:4]).to(dev)
    preds = []
    for flag in (False, True):
        model = _fallback_model(case, dev)   # the same weights both times (seeded)
        model.infer_bf16 = flag
        torch.manual_seed(11)   # the train-mode dropout seeds
        with torch.set_grad_enabled(case in ("train", "grad")):
            preds.append(model(b.x, b.edge_index, b.edge_attr, b.batch)[0].detach())
    assert not layer_calls
    assert torch.equal(preds[0], preds[1])
