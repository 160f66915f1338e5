"""GPU: bf16 node features on the PyG surface -- the bf16 aggregation kernels
(bgnn_spmm_fwd_bf16 / bgnn_spmm_bwd_bf16), bgnn.aggregate, bgnn.nn.SAGEConv and the per-module
models under torch.autocast(bfloat16).

Kernel level: both entry points against their formulas (include/bgnn.h) evaluated in fp64 on the
same bf16 inputs, on the structure cases of tests/test_gpu_sage_infer.py (restated here): a hand
graph with isolated rows, duplicated edges, rows at the chunk boundary (in-degree 64 and 65), a row
of 11 chunks and a short last group; a GraphStore batch with super nodes (group starts given
explicitly) -- on every kernel an entry point can take (row groups of 4 and 8, one row per wave).
The f32 output is held to the worst-case bound of f32 accumulation, so no measured tolerance is
involved. Module and model level: the fp64 oracle, with torch's own bf16 arithmetic as the
yardstick."""
import functools

import pytest
import torch
import torch.nn.functional as F

import bgnn
from bgnn import _lib, fused, ops
from bgnn import synthetic as S
from bgnn.data import Batch
from bgnn.graph import Csr, Graph, _graph_cache, _stream, enqueue_groups, graph_for

pytestmark = pytest.mark.gpu

N_HAND = 1003
U = 2.0 ** -24   # unit roundoff of f32


# ----------------------------------------------------------------------------- structure cases
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
_keep_alive = []


def _variant(c, kind):
    if kind == "hand":
        return c
    groups = enqueue_groups(c.rowptr, c.col, c.n_rows, c.nnz, c.plan.chunk, rows=8) if kind == "hand_r8" else None
    return Csr(c.rowptr, c.col, c.n_rows, c.nnz, c.plan, groups)   # None: one row per wave


def graph_case(kind, dev):
    """(edge_index on the host, N, forward Csr, transpose Csr, forward rowptr, Graph) of a structure
    case, built once."""
    if kind in _graphs:
        return _graphs[kind]
    if kind == "store":   # gathered per-graph plans: grow is non-NULL
        hb = store_batch_host()
        store = bgnn.GraphStore([S.make_mesh_graph(18, s, super_node=True) for s in range(3)], dev)
        b = store.batch([0, 1, 2])
        assert torch.equal(b.edge_index.cpu(), hb.edge_index)
        g = _graph_cache.peek(b.edge_index, (b.num_nodes, 64))
        assert g is not None
        for c in (g.fwd, g.bwd):
            assert c.groups is not None and c.groups.grow is not None
            assert c.plan.n_heavy == 3
        _keep_alive.append((store, b))
        out = (hb.edge_index, hb.num_nodes, g.fwd, g.bwd, g.fwd.rowptr, g)
    else:
        ei = hand_edges()
        g = Graph.build(ei.to(dev), N_HAND)
        f = g.fwd
        deg = f.degree().cpu()
        assert (int(deg[10]), int(deg[11]), int(deg[500]), int(deg[950])) == (64, 65, 700, 0)
        assert f.plan.n_heavy == 2 and f.plan.n_chunks == 2 + 11
        assert f.groups is not None and f.groups.grow is None and f.groups.rows == 4
        assert g.bwd.groups is not None and g.bwd.groups.rows == 4
        out = (ei, N_HAND, _variant(f, kind), _variant(g.bwd, kind), f.rowptr, g)
    _graphs[kind] = out
    return out


def host_edges(kind):
    return store_batch_host().edge_index if kind == "store" else hand_edges()


@functools.lru_cache(maxsize=None)
def rows_bf16(n, H, seed):
    g = torch.Generator().manual_seed(seed + 7 * H + n)
    return torch.randn(n, H, generator=g).bfloat16()


@functools.lru_cache(maxsize=None)
def reference(kind, n, H, mean, transposed):
    """(fp64 result, fp64 sum of |terms|, entry count per row) of the header's formula on the bf16
    inputs; computed once per case and shared by the kernel variants."""
    ei = host_edges(kind)
    v = rows_bf16(n, H, 11 if transposed else 3).double()
    deg = torch.bincount(ei[1], minlength=n).clamp_min(1).double()
    if transposed:   # gx[j] = sum over edges j -> t of w(t) g[t]
        w = (1.0 / deg) if mean else torch.ones(n, dtype=torch.float64)
        terms = w[ei[1]].unsqueeze(1) * v[ei[1]]
        rows, scale = ei[0], torch.ones(n, 1, dtype=torch.float64)
    else:
        terms = v[ei[0]]
        rows, scale = ei[1], ((1.0 / deg) if mean else torch.ones(n, dtype=torch.float64)).unsqueeze(1)
    ref = scale * torch.zeros(n, H, dtype=torch.float64).index_add_(0, rows, terms)
    mag = scale * torch.zeros(n, H, dtype=torch.float64).index_add_(0, rows, terms.abs())
    return ref, mag, torch.bincount(rows, minlength=n)


def run_kernel(fwd, bwd, fwd_rowptr, n, H, mean, transposed, out_f32, dev, v=None):
    v = rows_bf16(n, H, 11 if transposed else 3).to(dev) if v is None else v
    out = torch.full((n, H), float("nan"), dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
    csr = bwd if transposed else fwd
    part = torch.empty(max(csr.plan.n_chunks, 1) * H, dtype=torch.float32, device=dev)
    if transposed:
        _lib.call("bgnn_spmm_bwd_bf16", csr.ref(), fwd_rowptr.data_ptr(), v.data_ptr(), v.stride(0), H, int(mean),
                  out.data_ptr(), H, int(out_f32), part.data_ptr(), _stream())
    else:
        _lib.call("bgnn_spmm_fwd_bf16", csr.ref(), v.data_ptr(), v.stride(0), H, int(mean), out.data_ptr(), H,
                  int(out_f32), part.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out


def check_case(kind, H, mean, transposed, dev):
    _, n, fwd, bwd, frp, _keep = graph_case(kind, dev)
    ref, mag, cnt = reference("store" if kind == "store" else "hand", n, H, mean, transposed)
    args = (fwd, bwd, frp, n, H, mean, transposed)
    o32 = run_kernel(*args, True, dev).cpu()
    o16 = run_kernel(*args, False, dev).cpu()
    # worst case of f32 accumulation in any order, plus the weight and scale roundings
    bound = (cnt.double().unsqueeze(1) + 4) * U * mag
    err = (o32.double() - ref).abs()
    print(f"{kind} H={H} mean={mean} transposed={transposed}: max err {float(err.max()):.3e}, "
          f"max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool(torch.isfinite(o32).all())
    assert bool((err <= bound).all())   # every element, none excluded
    empty = cnt == 0
    if kind != "store" and not transposed:
        assert int(empty.sum()) == 101   # the isolated rows 900..999 and 1001
    assert bool((o32[empty] == 0).all()) and bool((o16[empty].float() == 0).all())
    # the bf16 store is the f32 result rounded once, to nearest even
    assert torch.equal(o16.view(torch.int16), o32.bfloat16().view(torch.int16))
    # bit-identical run to run
    assert torch.equal(o32, run_kernel(*args, True, dev).cpu())
    assert torch.equal(o16.view(torch.int16), run_kernel(*args, False, dev).cpu().view(torch.int16))


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("H", [64, 200, 512])
@pytest.mark.parametrize("kind", ["hand", "store"])
def test_kernel_within_the_f32_bound(dev, kind, H, mean, transposed):
    check_case(kind, H, mean, transposed, dev)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("H", [200, 512])
@pytest.mark.parametrize("kind", ["hand_r8", "hand_rows"])
def test_kernel_other_plans(dev, kind, H, mean, transposed):
    """Row groups of 8 and a CSR without a row-group plan (one row per wave)."""
    check_case(kind, H, mean, transposed, dev)


@pytest.mark.parametrize("mean", [False, True])
def test_transpose_is_the_adjoint(dev, mean):
    """<A x, y> = <x, A^T y> with f32 outputs at H = 512 on the store batch."""
    _, n, fwd, bwd, frp, _keep = graph_case("store", dev)
    x, y = rows_bf16(n, 512, 3).to(dev), rows_bf16(n, 512, 11).to(dev)
    ax = run_kernel(fwd, bwd, frp, n, 512, mean, False, True, dev)
    aty = run_kernel(fwd, bwd, frp, n, 512, mean, True, True, dev)
    lhs = (ax.double() * y.double()).sum()
    rhs = (x.double() * aty.double()).sum()
    assert abs(float(lhs - rhs)) <= 1e-6 * float(ax.double().abs().sum() * y.double().abs().max())


# ----------------------------------------------------------------------------- aggregate
def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_aggregate_takes_bf16(dev, reduce):
    """bf16 in, bf16 out (float32 with out_dtype): a TypeError before this feature."""
    _, n, fwd, bwd, frp, g = graph_case("hand", dev)
    x = rows_bf16(n, 64, 3).to(dev)
    out = bgnn.aggregate(x, g, reduce)
    assert out.dtype == torch.bfloat16 and out.shape == (n, 64)
    o32 = bgnn.aggregate(x, g, reduce, out_dtype=torch.float32)
    assert o32.dtype == torch.float32
    assert torch.equal(bits(out), bits(o32.bfloat16()))
    if reduce != "max":   # the bf16 kernels' own result
        assert torch.equal(bits(o32), bits(run_kernel(fwd, bwd, frp, n, 64, reduce == "mean", False, True, dev)))
    else:   # exact: the maximum of bf16 values is one of them
        assert torch.equal(o32, bgnn.aggregate(x.float(), g, reduce))
    with pytest.raises(TypeError):
        bgnn.aggregate(x.half(), g, reduce)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_aggregate_reads_a_column_slice_in_place(dev, reduce, monkeypatch):
    _, n, _, _, _, g = graph_case("store", dev)
    H = 200
    z = rows_bf16(n, 2 * H, 3).to(dev)
    seen = []
    real = ops.spmm_fwd_bf16

    def spy(csr, x, *a, **k):
        seen.append((x.data_ptr(), x.stride(0)))
        return real(csr, x, *a, **k)
    monkeypatch.setattr(ops, "spmm_fwd_bf16", spy)
    for view in (z[:, :H], z[:, H:]):
        seen.clear()
        out = bgnn.aggregate(view, g, reduce)
        assert seen == [(view.data_ptr(), 2 * H)]   # no copy was made
        assert torch.equal(bits(out), bits(bgnn.aggregate(view.contiguous(), g, reduce)))


@pytest.mark.parametrize("H,reduce", [(68, "sum"), (68, "mean"), (64, "max"), (68, "max")])
def test_upcast_route_is_the_f32_path_rounded_once(dev, H, reduce, monkeypatch):
    """Widths outside the bf16 kernels and max: upcast, the float32 kernels, one rounding --
    bit for bit, forward and gradient."""
    monkeypatch.setattr(ops, "spmm_fwd_bf16", None)   # (must not be reached)
    _, n, _, _, _, g = graph_case("hand", dev)
    x = rows_bf16(n, H, 3).to(dev).requires_grad_(True)
    gy = rows_bf16(n, H, 11).to(dev)
    out = bgnn.aggregate(x, g, reduce)
    out.backward(gy)
    xf = x.detach().float().requires_grad_(True)
    ref = bgnn.aggregate(xf, g, reduce)
    ref.backward(gy.float())
    assert out.dtype == torch.bfloat16 and x.grad.dtype == torch.bfloat16
    assert torch.equal(bits(out), bits(ref.bfloat16()))
    assert torch.equal(bits(x.grad), bits(xf.grad.bfloat16()))


def test_max_ties_go_to_the_first_edge(dev):
    ei = torch.tensor([[3, 1, 2, 0], [0, 0, 0, 1]], device=dev)   # row 0: sources 3, 1, 2 in CSR order
    x = torch.zeros(4, 8, dtype=torch.bfloat16, device=dev)
    x[1] = 2.0
    x[2] = 2.0   # ties with row 1 in every column
    x[3, :4] = 2.0   # ... and with row 3, the first edge, in the first four
    x[3, 4:] = -1.0
    x.requires_grad_(True)
    g = Graph.build(ei, 4)
    out = bgnn.aggregate(x, g, "max")
    assert torch.equal(out[0].float().cpu(), torch.full((8,), 2.0))
    gy = torch.arange(1, 33, dtype=torch.float32, device=dev).view(4, 8).bfloat16()
    out.backward(gy)
    want = torch.zeros(4, 8)
    want[3, :4] = gy[0, :4].float().cpu()
    want[1, 4:] = gy[0, 4:].float().cpu()
    want[0] = gy[1].float().cpu()   # row 1's only source
    assert torch.equal(x.grad.float().cpu(), want)


@pytest.mark.parametrize("g_f32", [False, True])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_aggregate_gradient_is_the_transposed_kernel(dev, reduce, g_f32):
    _, n, fwd, bwd, frp, g = graph_case("store", dev)
    x = rows_bf16(n, 512, 3).to(dev).requires_grad_(True)
    gy = rows_bf16(n, 512, 11).to(dev)
    out = bgnn.aggregate(x, g, reduce, out_dtype=torch.float32 if g_f32 else None)
    out.backward(gy.float() if g_f32 else gy)   # a f32 gradient is rounded to bf16 once (exact here)
    assert x.grad.dtype == torch.bfloat16
    assert torch.equal(bits(x.grad), bits(run_kernel(fwd, bwd, frp, n, 512, reduce == "mean", True, False, dev, v=gy)))


def test_segment_reduce_bf16(dev):
    """max takes the upcast route (exact); sum / mean keep their f32 output (EA_GNN's)."""
    gen = torch.Generator().manual_seed(9)
    idx = torch.randint(0, 9, (500,), generator=gen).to(dev)
    seg = bgnn.segments_for(idx, 12)
    src = torch.randn(500, 64, generator=gen).bfloat16().to(dev).requires_grad_(True)
    gy = torch.randn(12, 64, generator=gen).bfloat16().to(dev)
    out = bgnn.segment_reduce(src, seg, "max")
    out.backward(gy)
    sf = src.detach().float().requires_grad_(True)
    ref = bgnn.segment_reduce(sf, seg, "max")
    ref.backward(gy.float())
    assert out.dtype == torch.bfloat16 and torch.equal(out.float(), ref)
    assert torch.equal(bits(src.grad), bits(sf.grad.bfloat16()))
    assert bgnn.segment_reduce(src.detach(), seg, "mean").dtype == torch.float32


# ----------------------------------------------------------------------------- SAGEConv
@functools.lru_cache(maxsize=None)
def mesh_batch_host():
    return Batch.from_data_list([S.make_mesh_graph(18, seed=40 + s, super_node=(s % 2 == 1)) for s in range(4)])


def rel(a, r):
    return float((a.detach().double().cpu() - r).norm() / r.norm())


@pytest.fixture
def linear_calls(monkeypatch):
    calls = []
    real = fused.linear_bf16

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(fused, "linear_bf16", counted)
    return calls


def restated_conv(x, w_l, b_l, w_r, ei, aggr, normalize, autocast):
    """torch's bf16 arithmetic for the module: bf16 operands, F.linear with a bf16 output, f32
    index_add_ and tail for sum / mean (transform first); max aggregates first (exact) and adds the
    two bf16 Linear outputs as torch does. The output has the module's dtype: the input's outside
    autocast; under autocast f32 after F.normalize, else a Linear's bf16."""
    from oracle import pyg_ref as P
    n = x.size(0)
    src, dst = ei
    xb = x.bfloat16()
    if aggr == "max":
        agg = P.scatter(xb.index_select(0, src), dst, n, "max")
        h = F.linear(agg, w_l.bfloat16(), b_l.bfloat16()) + F.linear(xb, w_r.bfloat16())
        if autocast:
            h = h.float()
    else:
        z_l, z_r = F.linear(xb, w_l.bfloat16()), F.linear(xb, w_r.bfloat16())
        h = torch.zeros(n, w_l.size(0), device=x.device).index_add_(0, dst, z_l.float().index_select(0, src))
        if aggr == "mean":
            h = h / torch.bincount(dst, minlength=n).clamp_min(1).float().unsqueeze(1)
        h = h + z_r.float() + b_l
    if normalize:
        h = F.normalize(h, p=2.0, dim=-1)
    return h if (autocast and normalize) else h.bfloat16()


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("aggr", ["add", "mean", "max"])
@pytest.mark.parametrize("h", [64, 512])
def test_sageconv_bf16(dev, linear_calls, h, aggr, normalize, autocast):
    """bf16 input outside autocast, and f32 input inside torch.autocast(bfloat16): output dtype, the
    path taken, and forward / gradients against the fp64 oracle with torch's bf16 as the yardstick."""
    from oracle import pyg_ref as P
    hb = mesh_batch_host()
    n = hb.num_nodes
    torch.manual_seed(h + 3)
    conv = bgnn.SAGEConv(h, h, aggr=aggr, normalize=normalize)
    gen = torch.Generator().manual_seed(17 + h)
    x_host = torch.randn(n, h, generator=gen)
    if not autocast:
        x_host = x_host.bfloat16().float()   # the bf16 input's values
    y_host = torch.randn(n, h, generator=gen)

    # fp64 oracle on the host
    ref = P.SAGEConv(h, h, aggr=aggr, normalize=normalize).double()
    ref.load_state_dict({k: v.double() for k, v in conv.state_dict().items()})
    xr = x_host.double().requires_grad_(True)
    out_r = ref(xr, hb.edge_index)
    (out_r * y_host.double()).sum().backward()
    want = [out_r.detach(), xr.grad, ref.lin_l.weight.grad, ref.lin_l.bias.grad, ref.lin_r.weight.grad]

    conv = conv.to(dev)
    ei = hb.edge_index.to(dev)
    y = y_host.to(dev)

    def run(fn):
        x = x_host.to(dev).to(torch.float32 if autocast else torch.bfloat16).requires_grad_(True)
        ps = [conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight]
        for p in ps:
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = fn(x)
            (out.float() * y).sum().backward()
        return out, [out, x.grad] + [p.grad.clone() for p in ps]

    out, ours = run(lambda x: conv(x, ei))
    if autocast:
        assert out.dtype == (torch.float32 if normalize else torch.bfloat16)
    else:
        assert out.dtype == torch.bfloat16
    assert len(linear_calls) == (0 if aggr == "max" else 1)   # the bf16 fast path ran / did not
    _, theirs = run(lambda x: restated_conv(x, conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, ei, aggr,
                                            normalize, autocast))
    for name, a, t, r in zip(("out", "dx", "dW_l", "db_l", "dW_r"), ours, theirs, want):
        assert bool(torch.isfinite(a.float()).all())
        r_ours, r_torch = rel(a, r), rel(t, r)
        print(f"h={h} {aggr} normalize={normalize} autocast={autocast} {name}: rel L2 vs fp64 ours {r_ours:.3e}, "
              f"torch bf16 {r_torch:.3e}")
        assert r_ours <= 1.5 * r_torch + 1e-4, (name, r_ours, r_torch)


@pytest.mark.parametrize("aggr", ["add", "mean", "max"])
def test_sageconv_f32_outside_autocast_is_unchanged(dev, linear_calls, aggr):
    """float32 input outside autocast: bit-identical to a direct fused.sage_conv call."""
    hb = mesh_batch_host()
    torch.manual_seed(5)
    conv = bgnn.SAGEConv(64, 64, aggr=aggr, normalize=True).to(dev)
    x = torch.randn(hb.num_nodes, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    ei = hb.edge_index.to(dev)
    with torch.no_grad():
        out = conv(x, ei)
        direct = fused.sage_conv(x, conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, graph_for(ei, x.size(0)),
                                 {"mean": 1, "max": 2}.get(aggr, 0))
    assert out.dtype == torch.float32 and not linear_calls
    assert torch.equal(out, direct)


def test_sageconv_no_grad_reuses_the_cached_bf16_weights(dev):
    hb = mesh_batch_host()
    torch.manual_seed(6)
    conv = bgnn.SAGEConv(64, 64, aggr="mean", normalize=True).to(dev)
    x = torch.randn(hb.num_nodes, 64, generator=torch.Generator().manual_seed(2)).to(dev)
    ei = hb.edge_index.to(dev)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with torch.no_grad():
            a = conv(x, ei)
            w = conv._bgnn_infer_wcat[1]
            conv(x, ei)
            assert conv._bgnn_infer_wcat[1] is w
        b = conv(x, ei)   # the autograd form: the same bf16 operands, rounded inside the GEMM
    assert a.dtype == b.dtype == torch.float32
    # rows of unit norm: at most a bf16 ulp of 1 apart where a z element rounds the other way
    torch.testing.assert_close(a, b.detach(), rtol=0, atol=2.0 ** -8)


# ----------------------------------------------------------------------------- model
@pytest.mark.parametrize("name", ["GraphSage_addAggr", "GraphSage_meanAggr", "GraphSage_maxAggr"])
def test_per_module_model_trains_under_autocast(dev, name):
    """use_fused = False, train mode, forward + loss + backward inside autocast: a TypeError at the
    first conv before this feature. Prediction and gradients against the fp64 oracle, with the
    oracle's own ops run under torch.autocast on the device as the yardstick."""
    from oracle import buckgnn_ref as R
    hb = mesh_batch_host()
    torch.manual_seed(21)
    model = bgnn.BuckGNN(16, 5, 64, 6, "mean", dropout_rate=0.0, model_name=name)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    params = [k for k, _ in model.named_parameters()]

    def oracle(sd_, x, ei, batch, y):
        pred = R.forward(sd_, name, x, ei, batch, True, "mean", 0.0)
        loss = ((pred.float() - y) ** 2).mean()
        loss.backward()
        return pred.detach()

    sd64 = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    for k in params:
        sd64[k].requires_grad_(True)
    p_ref = oracle(sd64, hb.x.double(), hb.edge_index, hb.batch, hb.y.double())
    used = [k for k in params if sd64[k].grad is not None and float(sd64[k].grad.norm()) > 0]
    assert len(used) >= 6 * 3
    g_ref = torch.cat([sd64[k].grad.flatten() for k in used])

    b = hb.to(dev)
    sdd = {k: v.to(dev) for k, v in sd.items()}
    for k in params:
        sdd[k].requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        p_torch = oracle(sdd, b.x, b.edge_index, b.batch, b.y)
    g_torch = torch.cat([sdd[k].grad.flatten() for k in used])

    model = model.to(dev).train()
    model.use_fused = False
    with torch.autocast("cuda", dtype=torch.bfloat16):
        pred, _ = model(b.x, b.edge_index, b.edge_attr, b.batch)
        ((pred.float() - b.y) ** 2).mean().backward()
    named = dict(model.named_parameters())
    assert bool(torch.isfinite(pred.float()).all())
    for k in used:
        assert named[k].grad is not None and bool(torch.isfinite(named[k].grad).all()), k
    g_ours = torch.cat([named[k].grad.flatten() for k in used])

    for what, a, t, r in (("pred", pred, p_torch, p_ref), ("grad", g_ours, g_torch, g_ref)):
        r_ours, r_torch = rel(a.float(), r), rel(t.float(), r)
        print(f"{name} {what}: rel L2 vs the fp64 oracle: ours {r_ours:.3e}, torch autocast {r_torch:.3e}")
        assert r_ours <= 1.5 * r_torch + 1e-4, (what, r_ours, r_torch)


def test_fused_path_refuses_non_f32_activations(dev):
    """Host only: a bf16 activation takes the per-module loop instead of the f32 kernels."""
    model = bgnn.BuckGNN(16, 5, 64, 6, "mean", dropout_rate=0.0, model_name="GraphSage_addAggr").to(dev)
    assert model.use_fused
    assert model._fused_ok(torch.empty(8, 64, dtype=torch.bfloat16, device=dev)) is False
    assert model._fused_ok(torch.empty(8, 64, dtype=torch.float32, device=dev)) is True
