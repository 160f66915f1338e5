"""GPU: the bf16 max aggregation (bgnn_spmm_max_bf16) and its place in bgnn.aggregate.

The maximum of bf16 values is one of them, so everything here is compared bit for bit: the kernel
against torch's scatter_reduce(amax) on the same values -- isolated rows, duplicated edges, rows at
the chunk boundary (in-degree 64 and 65), a row of 11 chunks, a short last group, a GraphStore
batch with 3 super nodes -- on every kernel the entry point can take (row groups of 4 and 8, one
row per wave, with and without the argmax state); the argmax state against the float32 kernel's
with half of all entries tied; aggregate's values and gradients against the upcast route."""
import functools

import pytest
import torch

import bgnn
from bgnn import ops
from bgnn import synthetic as S
from bgnn.graph import Csr, Graph, _graph_cache, enqueue_groups

pytestmark = pytest.mark.gpu

N_HAND = 1003


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


def graph_case(kind, dev):
    """(edge_index on the host, N, forward Csr, Graph) of a structure case, built once."""
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
        _keep_alive.append((store, b))
        out = (hb.edge_index, hb.num_nodes, g.fwd, g)
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
        else:   # "hand_rows": no row-group plan, one row per wave
            csr = Csr(f.rowptr, f.col, f.n_rows, f.nnz, f.plan, None)
        out = (ei, N_HAND, csr, g)
    _graphs[kind] = out
    return out


def host_edges(kind):
    return store_batch_host().edge_index if kind == "store" else hand_edges()


@functools.lru_cache(maxsize=None)
def rows_bf16(n, H, seed, relu=False):
    g = torch.Generator().manual_seed(seed + 7 * H + n)
    x = torch.randn(n, H, generator=g)
    return (torch.relu(x) if relu else x).bfloat16()


@functools.lru_cache(maxsize=None)
def reference(kind, n, H, relu=False):
    """torch's amax over each row's in-edges on the same bf16 values, upcast (exact), 0 for empty
    rows; on the CPU, computed once per case and shared by the kernel variants."""
    ei = host_edges(kind)
    x = rows_bf16(n, H, 3, relu).float()
    idx = ei[1].view(-1, 1).expand(-1, H)
    return torch.zeros(n, H).scatter_reduce(0, idx, x[ei[0]], "amax", include_self=False)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def run_kernel(csr, x, n, want_arg):
    out = torch.full((n, x.size(1)), float("nan"), dtype=torch.bfloat16, device=x.device)
    res, arg = ops.spmm_max_bf16(csr, x, n, want_arg, out=out)
    torch.cuda.synchronize()
    assert res is out and (arg is not None) == want_arg
    return out, arg


# ----------------------------------------------------------------------------- kernel against torch
@pytest.mark.parametrize("H", [8, 64, 200, 512])
@pytest.mark.parametrize("kind", ["hand", "hand_r8", "hand_rows"])
def test_kernel_equals_torch_amax(dev, kind, H):
    _, n, csr, _ = graph_case(kind, dev)
    ref = reference("hand", n, H)
    out, _ = run_kernel(csr, rows_bf16(n, H, 3).to(dev), n, False)
    assert torch.equal(out.float().cpu(), ref)   # exact, every element (a NaN left behind fails)
    assert bool((ref[950] == 0).all()) and bool((out[950] == 0).all())   # an isolated row


@pytest.mark.parametrize("H", [64, 512])
def test_kernel_equals_torch_amax_on_a_store_batch(dev, H):
    _, n, csr, _ = graph_case("store", dev)
    out, _ = run_kernel(csr, rows_bf16(n, H, 3).to(dev), n, False)
    assert torch.equal(out.float().cpu(), reference("store", n, H))


# ----------------------------------------------------------------------------- argmax state
@pytest.mark.parametrize("kind,H", [("hand", 8), ("hand", 200), ("hand", 512), ("hand_rows", 64), ("store", 64),
                                    ("store", 512)])
def test_argmax_state_is_the_f32_kernels(dev, kind, H):
    """ReLU inputs: about half of all entries tie at 0, so the first-edge rule decides most of the
    positions. The decoded state equals bgnn_spmm_fwd(MAX)'s on the upcast input, and asking for
    it does not change the values."""
    _, n, csr, _ = graph_case(kind, dev)
    xh = rows_bf16(n, H, 3, True)
    assert 0.4 < float((xh == 0).float().mean()) < 0.6
    x = xh.to(dev)
    out, arg = run_kernel(csr, x, n, True)
    plain, _ = run_kernel(csr, x, n, False)
    ref_out, ref_arg = ops.spmm_fwd(csr, x.float(), 2, n, want_arg=True)
    pos = ops.max_arg_positions(csr, arg, n, H).cpu()
    ref_pos = ops.max_arg_positions(csr, ref_arg, n, H).cpu()
    deg = csr.degree().cpu()
    light, heavy, empty = (deg > 0) & (deg <= csr.plan.chunk), deg > csr.plan.chunk, deg == 0
    assert int(light.sum()) > 0 and int(heavy.sum()) == csr.plan.n_heavy > 0
    assert int(empty.sum()) > 0 or kind == "store"   # (a mesh batch has no isolated node)
    for rows in (light, heavy, empty):
        assert torch.equal(pos[rows], ref_pos[rows])
    assert bool((pos[empty] == -1).all())
    # the positions are what they claim: the source at a heavy row's positions holds its maximum
    col = csr.col.cpu().long()
    r = int(torch.nonzero(heavy)[0])
    assert torch.equal(xh[col[pos[r]], torch.arange(H)].float(), ref_out[r].cpu())
    assert torch.equal(bits(out), bits(plain))
    assert torch.equal(out.float(), ref_out)
    assert torch.equal(out.float().cpu(), reference("store" if kind == "store" else "hand", n, H, True))


# ----------------------------------------------------------------------------- strides
@pytest.mark.parametrize("kind", ["hand", "hand_rows", "store"])
def test_planes_of_one_buffer(dev, kind):
    """x = plane 1 and out = plane 0 of one [N, 2H] allocation (the model path's layout): plane 1
    and a sentinel row behind the last one stay as they were."""
    H = 200
    _, n, csr, _ = graph_case(kind, dev)
    x = rows_bf16(n, H, 3).to(dev)
    buf = torch.full((n + 1, 2 * H), float("nan"), dtype=torch.bfloat16, device=dev)
    buf[:n, H:] = x
    buf[n] = -7.0
    ops.spmm_max_bf16(csr, buf[:n, H:], n, False, out=buf[:n, :H])
    torch.cuda.synchronize()
    assert torch.equal(buf[:n, :H].float().cpu(), reference("store" if kind == "store" else "hand", n, H))
    assert torch.equal(bits(buf[:n, H:]), bits(x))
    assert bool((buf[n] == -7.0).all())


# ----------------------------------------------------------------------------- host
@pytest.fixture
def max_calls(monkeypatch):
    seen = []
    real = ops.spmm_max_bf16

    def spy(csr, x, *a, **k):
        seen.append((x.data_ptr(), x.stride(0)))
        return real(csr, x, *a, **k)
    monkeypatch.setattr(ops, "spmm_max_bf16", spy)
    return seen


def test_aggregate_max_reads_a_column_slice_in_place(dev, max_calls):
    """aggregate(x_bf16, "max") reaches the bf16 kernel with the view itself, and allocates less
    than a float32 copy of it would take."""
    _, n, _, g = graph_case("store", dev)
    H = 200
    z = rows_bf16(n, 2 * H, 3).to(dev)
    for view in (z[:, :H], z[:, H:]):
        max_calls.clear()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = bgnn.aggregate(view, g, "max")
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        assert max_calls == [(view.data_ptr(), 2 * H)]   # no copy was made
        assert grown < n * H * 4, grown                  # (the bf16 result and the chunk scratch)
        assert out.dtype == torch.bfloat16
        assert torch.equal(out.float(), bgnn.aggregate(view.float().contiguous(), g, "max"))


@pytest.mark.parametrize("g_f32", [False, True])
@pytest.mark.parametrize("kind,H", [("hand", 64), ("store", 512)])
def test_aggregate_max_is_the_f32_route_rounded_once(dev, max_calls, kind, H, g_f32):
    """Values and gradients, bit for bit, with tied inputs; out_dtype=float32 is the exact widening."""
    _, n, _, g = graph_case(kind, dev)
    x = rows_bf16(n, H, 3, True).to(dev).requires_grad_(True)
    gy = rows_bf16(n, H, 11).to(dev)
    out = bgnn.aggregate(x, g, "max", out_dtype=torch.float32 if g_f32 else None)
    out.backward(gy.float() if g_f32 else gy)
    assert len(max_calls) == 1
    xf = x.detach().float().requires_grad_(True)
    ref = bgnn.aggregate(xf, g, "max")
    ref.backward(gy.float())
    assert len(max_calls) == 1   # (the float32 input took the float32 kernel)
    assert out.dtype == (torch.float32 if g_f32 else torch.bfloat16) and x.grad.dtype == torch.bfloat16
    assert torch.equal(out.float(), ref)
    assert torch.equal(bits(x.grad), bits(xf.grad.bfloat16()))
    assert int((x.grad != 0).sum()) > 0


def test_other_widths_keep_the_upcast_route(dev, monkeypatch):
    monkeypatch.setattr(ops, "spmm_max_bf16", None)   # (must not be reached)
    _, n, _, g = graph_case("hand", dev)
    x = rows_bf16(n, 68, 3).to(dev).requires_grad_(True)
    gy = rows_bf16(n, 68, 11).to(dev)
    out = bgnn.aggregate(x, g, "max")
    out.backward(gy)
    xf = x.detach().float().requires_grad_(True)
    ref = bgnn.aggregate(xf, g, "max")
    ref.backward(gy.float())
    assert out.dtype == torch.bfloat16 and torch.equal(out.float(), ref)
    assert torch.equal(bits(x.grad), bits(xf.grad.bfloat16()))


# ----------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("want_arg", [False, True])
@pytest.mark.parametrize("kind", ["hand", "store"])
def test_two_runs_are_bit_equal(dev, kind, want_arg):
    _, n, csr, _ = graph_case(kind, dev)
    x = rows_bf16(n, 512, 3, True).to(dev)
    a, arg_a = run_kernel(csr, x, n, want_arg)
    b, arg_b = run_kernel(csr, x, n, want_arg)
    assert torch.equal(bits(a), bits(b))
    if want_arg:
        assert torch.equal(ops.max_arg_positions(csr, arg_a, n, 512), ops.max_arg_positions(csr, arg_b, n, 512))
