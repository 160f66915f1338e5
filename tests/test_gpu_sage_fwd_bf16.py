"""GPU: bgnn_sage_fwd_bf16, the training-mode aggregation over bf16 z, against the formula of
include/bgnn.h evaluated in fp64 on the same bf16 inputs -- isolated rows, duplicated edges, rows at
the chunk boundary (in-degree 64 and 65), a row of several chunks, a last group of fewer rows than
the plan's, a GraphStore batch (group starts given explicitly) -- on every kernel the entry point can
take (row groups of 4 and 8, one row per wave). o and nrm: every element within the tolerance of the
bgnn_sage_fwd-against-fp64 test. bn_partial: the slots summed in fp64 against the fp64 column sums of
the kernel's own stored o and o^2, within the worst case of n_rows f32 additions of those values.
(The structure helpers are those of tests/test_gpu_sage_infer.py.)"""
import functools

import pytest
import torch

import bgnn
from bgnn import _lib
from bgnn import synthetic as S
from bgnn.graph import Csr, Graph, _graph_cache, _stream, enqueue_groups

pytestmark = pytest.mark.gpu

# the tolerance of the bgnn_sage_fwd-against-fp64 test (tests/test_gpu_fused.py TOL)
RTOL, ATOL = 1e-4, 1e-4
N_HAND = 1003


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
    g = torch.Generator().manual_seed(1900 + H + n)
    z = torch.randn(n, 2 * H, generator=g).bfloat16()
    bias = 0.1 * torch.randn(H, generator=g)
    return z, bias


@functools.lru_cache(maxsize=None)
def reference(kind, n, H, mean):
    """fp64 (o, nrm) from the same bf16 z (computed once per case, shared by the kernel variants)."""
    ei = hand_edges() if kind == "hand" else store_batch_host().edge_index
    z, bias = inputs(n, H)
    zl, zr = z[:, :H].double(), z[:, H:].double()
    agg = torch.zeros(n, H, dtype=torch.float64).index_add_(0, ei[1], zl[ei[0]])
    if mean:
        agg = agg / torch.bincount(ei[1], minlength=n).clamp_min(1).double().unsqueeze(1)
    h = agg + zr + bias.double()
    nrm = h.norm(dim=1)
    return h / nrm.clamp_min(1e-12).unsqueeze(1), nrm


def run_kernel(csr, z, bias, H, mean, stats=True):
    """(o, nrm, bn_partial) on the host; o, nrm and the slots are pre-filled with NaN."""
    n, dev = z.size(0), z.device
    o = torch.full((n, H), float("nan"), dtype=torch.float32, device=dev)
    nrm = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    slots = _lib.query("bgnn_sage_fwd_bf16_slots", csr.ref())
    assert slots >= 8 + (csr.plan.n_heavy if csr.plan.n_chunks else 0)
    bnp = torch.full((slots, 2, H), float("nan"), dtype=torch.float32, device=dev)
    part = torch.empty(max(csr.plan.n_chunks, 1) * H, dtype=torch.float32, device=dev)
    _lib.call("bgnn_sage_fwd_bf16", csr.ref(), z.data_ptr(), z.stride(0), bias.data_ptr(), H, int(mean),
              o.data_ptr(), nrm.data_ptr(), bnp.data_ptr() if stats else None, part.data_ptr(), _stream())
    torch.cuda.synchronize()
    return o.cpu(), nrm.cpu(), bnp.cpu()


def check_case(kind, H, mean, dev):
    ref_kind = "store" if kind == "store" else "hand"
    _, n, csr, _keep = graph_case(kind, dev)
    o_ref, n_ref = reference(ref_kind, n, H, mean)
    z, bias = (t.to(dev) for t in inputs(n, H))
    o, nrm, bnp = run_kernel(csr, z, bias, H, mean)
    eo = (o.double() - o_ref).abs()
    en = (nrm.double() - n_ref).abs()
    # every element, none excluded (a NaN left from the pre-fill fails the comparison)
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(nrm).all()) and bool(torch.isfinite(bnp).all())
    print(f"{kind} H={H} mean={mean}: max o err {float(eo.max()):.3e}, max nrm err {float(en.max()):.3e} "
          f"(max nrm {float(n_ref.max()):.1f})")
    assert bool((eo <= ATOL + RTOL * o_ref.abs()).all()), float((eo - RTOL * o_ref.abs()).max())
    assert bool((en <= ATOL + RTOL * n_ref.abs()).all()), float((en - RTOL * n_ref.abs()).max())
    # BatchNorm sums: over exactly the stored f32 values; n_rows f32 additions of v have an error of
    # at most n_rows * 2^-24 * sum |v| (one rounding of o * o included)
    od = o.double()
    for k, v in ((0, od), (1, od * od)):
        got = bnp[:, k, :].double().sum(0)
        bound = n * 2.0 ** -24 * v.abs().sum(0)
        err = (got - v.sum(0)).abs()
        print(f"  sum o^{k + 1}: max err / bound {float((err / bound).max()):.3e}")
        assert bool((err <= bound).all()), (k, float((err / bound).max()))
    # deterministic run to run
    o2, nrm2, bnp2 = run_kernel(csr, z, bias, H, mean)
    assert torch.equal(o, o2) and torch.equal(nrm, nrm2) and torch.equal(bnp, bnp2)
    # without the statistics: the same o and nrm, and no slot written
    o3, nrm3, bnp3 = run_kernel(csr, z, bias, H, mean, stats=False)
    assert torch.equal(o, o3) and torch.equal(nrm, nrm3) and bool(torch.isnan(bnp3).all())


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("H", [64, 200, 512])
@pytest.mark.parametrize("kind", ["hand", "store", "hand_r8", "hand_rows"])
def test_kernel_matches_fp64(dev, kind, H, mean):
    """Row groups of 4 (hand, store), of 8 (hand_r8) and a CSR without a row-group plan (hand_rows)."""
    check_case(kind, H, mean, dev)


@pytest.mark.parametrize("kind", ["hand", "hand_r8", "hand_rows"])
def test_all_zero_row(dev, kind):
    """An isolated row with z_r = 0 and bias = 0: h = 0, so nrm = 0 and o = 0 / 1e-12 = 0."""
    H = 64
    _, n, csr, _keep = graph_case(kind, dev)
    z = inputs(n, H)[0].clone()
    z[950, H:] = 0
    o, nrm, bnp = run_kernel(csr, z.to(dev), torch.zeros(H, device=dev), H, False)
    assert float(nrm[950]) == 0.0 and bool((o[950] == 0).all())
    assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(nrm).all()) and bool(torch.isfinite(bnp).all())
    assert float(nrm[951]) > 0.0   # (an isolated row with its own z_r is not zero)
