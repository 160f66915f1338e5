"""GPU: exact conformance matrix of the SAG pooling kernels of csrc/pool.hip -- bgnn_topk_rank,
bgnn_topk_select, bgnn_gather_scale, bgnn_gather_scale_bwd, bgnn_filter_edges -- and of the plan kernels
of csrc/graph.hip -- bgnn_heavy_plan, bgnn_group_plan -- each on its raw entry point (_lib.call).

References, inputs and case lists are tests/pool_ref.py's. Every integer output is an IntWin: a window
pre-filled with a sentinel no valid result can equal, inside guards of a second pattern, sized as
include/bgnn.h says (or larger, where the header gives a capacity), so that a write one element past an
output, or a slot left unwritten, shows; the workspaces are IntWins of exactly the queried size. Float
outputs are NaN-filled Wins, float inputs Bufs with NaN in the padding, around the rows and in every
row the index vectors do not name. Every element of every output is compared: integers must be equal,
out / dx and the dropped rows' zeros are compared as bits, dscore under H u sum |g x| (derived; the
section's largest err / bound is printed). Each section runs its first case twice and compares bits.

Section G is the one wrapper-level check: bgnn.pool.topk_select on scores with NaN must give the
oracle's perm, duplicate-free and inside [0, N), and only then is the gather run on it. No gather
anywhere in this file runs on a perm that was not compared with its reference first."""
import pytest
import torch

import pool_ref as P
from bgnn import _lib, pool
from bgnn.graph import _stream
from matrix_util import RATIOS, Buf, IntWin, Win, check, inp, ptr
from oracle import pyg_ref

pytestmark = pytest.mark.gpu

F32, I32, I64, U8 = torch.float32, torch.int32, torch.int64, torch.uint8


@pytest.fixture(autouse=True)
def _stop_after_a_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault is sticky: nothing more of this session runs on the GPU
        pytest.exit(f"GPU fault in the pooling matrix, session ended: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\nsection: largest err / bound")
    for k in sorted(RATIOS):
        if k.startswith("pool"):
            print(f"  {k}: {RATIOS[k]:.3f}")


def equal(got, want, what):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} elements, the reference has {tuple(want.shape)}"
    d = got != want
    if bool(d.any()):
        i = d.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} elements differ; first at {i}: got "
                             f"{got[tuple(i)].item()}, reference {want[tuple(i)].item()}")


def same_bits(a, b, what):
    equal(a.contiguous().view(I32), b.contiguous().view(I32), what + " (as bits)")


# ============================================================================ A. bgnn_topk_rank
def run_rank(dev, s, sizes):
    ptr_, batch = P.graph_arrays(sizes)
    sc, rank = inp(dev, s), IntWin(dev, s.numel(), I32)           # NaN after the last score
    batch, ptr_ = batch.to(dev), ptr_.to(dev)
    _lib.call("bgnn_topk_rank", sc.data_ptr(), batch.data_ptr(), ptr_.data_ptr(), s.numel(), ptr(rank), _stream())
    torch.cuda.synchronize()
    rank.guard("rank")
    return rank


@pytest.mark.parametrize("case", list(P.RANK_SIZES))
def test_a_rank(dev, case):
    sizes = P.RANK_SIZES[case]
    for j, kind in enumerate(P.SCORE_KINDS):
        s = P.scores(case, kind)
        label = f"bgnn_topk_rank sizes={case} N={s.numel()} scores={kind}"
        rank = run_rank(dev, s, sizes)
        rank.assert_all_written(label)
        got = rank.read()
        equal(got, P.rank_ref(s, sizes), label)
        if j == 0:
            equal(run_rank(dev, s, sizes).read(), got, label + ": two runs")


# ============================================================================ B. bgnn_topk_select
def run_select(dev, rank, sizes, k, with_batch_out):
    N = rank.numel()
    _, batch = P.graph_arrays(sizes)
    new_ptr = torch.cat([torch.zeros(1, dtype=I64), k.cumsum(0)])
    # perm and batch_out hold K elements; the windows hold N, so what lies behind the K-th shows as well
    perm, new_id, bo = IntWin(dev, N, I64), IntWin(dev, N, I32), IntWin(dev, N, I64)
    rank, batch, k, new_ptr = rank.to(dev), batch.to(dev), k.to(dev), new_ptr.to(dev)
    _lib.call("bgnn_topk_select", rank.data_ptr(), batch.data_ptr(), k.data_ptr(), new_ptr.data_ptr(), N, ptr(perm),
              ptr(new_id), ptr(bo) if with_batch_out else None, _stream())
    torch.cuda.synchronize()
    for w, what in ((perm, "perm"), (new_id, "new_id"), (bo, "batch_out")):
        w.guard(what)
    return perm, new_id, bo


@pytest.mark.parametrize("case", list(P.RANK_SIZES))
def test_b_select(dev, case):
    sizes = P.RANK_SIZES[case]
    first = True
    for kind in ("random", "nan_bits"):
        rank = P.rank_ref(P.scores(case, kind), sizes)           # the reference rank: independent of section A
        for kk in P.K_KINDS:
            k = P.k_of(sizes, kk)
            K = int(k.sum())
            want = P.select_ref(rank, sizes, k)
            for with_bo in (True, False):
                label = f"bgnn_topk_select sizes={case} scores={kind} k={kk} (K={K}) batch_out={'given' if with_bo else 'NULL'}"
                perm, new_id, bo = run_select(dev, rank, sizes, k, with_bo)
                perm.assert_all_written(label + " perm", K)
                perm.assert_untouched(label + " perm", K)        # k = 0 everywhere: the whole window keeps its sentinel
                new_id.assert_all_written(label + " new_id")
                equal(perm.read()[:K], want[0], label + " perm")
                equal(new_id.read(), want[1], label + " new_id")
                bo.assert_untouched(label + " batch_out", K if with_bo else 0)
                if with_bo:
                    bo.assert_all_written(label + " batch_out", K)
                    equal(bo.read()[:K], want[2], label + " batch_out")
                if first:
                    again = run_select(dev, rank, sizes, k, with_bo)
                    for a, b in zip(again, (perm, new_id, bo)):
                        equal(a.read(), b.read(), label + ": two runs")
                    first = False


# ============================================================================ C. bgnn_gather_scale / _bwd
def run_gather(dev, H, K, layout):
    _, dl, si, so = layout
    x, score, perm = P.gather_inputs(H, K)
    xin = Buf(dev, x, ld=H + dl, shift=si)
    out = Win(dev, K, H, H + dl, shift=so)
    sc, perm = inp(dev, score), perm.to(dev)
    _lib.call("bgnn_gather_scale", ptr(xin), xin.ld, H, perm.data_ptr(), sc.data_ptr(), K, ptr(out), out.ld, _stream())
    torch.cuda.synchronize()
    out.guard("gather_scale out (padding columns, guard rows)")
    return out.read()


def run_gather_bwd(dev, H, n, drop, layout, with_dscore=True):
    _, dl, si, so = layout
    g, x, new_id, score = P.gather_bwd_inputs(H, n, drop)
    gin, xin = Buf(dev, g, ld=H + dl, shift=si), Buf(dev, x, ld=H + dl, shift=si)
    dx, ds = Win(dev, n, H, H + dl, shift=so), Win(dev, 1, n, n)
    sc, new_id = inp(dev, score), new_id.to(dev)
    _lib.call("bgnn_gather_scale_bwd", ptr(gin), gin.ld, ptr(xin), xin.ld, H, new_id.data_ptr(), sc.data_ptr(), n,
              ptr(dx), dx.ld, ptr(ds) if with_dscore else None, _stream())
    torch.cuda.synchronize()
    dx.guard("gather_scale_bwd dx (padding columns, guard rows)")
    ds.guard("gather_scale_bwd dscore")
    return dx.read(), ds.read().view(-1)


@pytest.mark.parametrize("H", P.GATHER_H)
def test_c_gather(dev, H):
    first = True
    for rows in P.GATHER_ROWS:
        for layout in P.GATHER_LAYOUTS:
            x, score, perm = P.gather_inputs(H, rows)
            label = f"bgnn_gather_scale H={H} K={rows} N={x.size(0)} {layout[0]}"
            out = run_gather(dev, H, rows, layout)
            assert bool(torch.isfinite(out).all()), f"{label}: not finite (an element never written, or a row perm does not name was read)"
            same_bits(out, P.gather_scale_ref(x, perm, score), label)
            if first:
                same_bits(run_gather(dev, H, rows, layout), out, label + ": two runs")
            for drop in P.DROP_KINDS:
                g, x, new_id, score = P.gather_bwd_inputs(H, rows, drop)
                label = f"bgnn_gather_scale_bwd H={H} n={rows} dropped={drop} ({int((new_id < 0).sum())} rows) {layout[0]}"
                rdx, rds, bound = P.gather_scale_bwd_ref(g, x, new_id, score)
                dx, ds = run_gather_bwd(dev, H, rows, drop, layout)
                assert bool(torch.isfinite(dx).all()), f"{label}: dx not finite"
                same_bits(dx, rdx, label + " dx")
                check("pool C dscore", ds, rds, bound, label + " dscore")
                same_bits(ds[new_id < 0], torch.zeros(int((new_id < 0).sum())), label + " dscore of the dropped rows")
                if drop == "half":
                    dx2, ds2 = run_gather_bwd(dev, H, rows, drop, layout, with_dscore=False)
                    same_bits(dx2, dx, label + ": dx with dscore = NULL")
                    assert bool(torch.isnan(ds2).all()), f"{label}: dscore = NULL, yet it was written"
                    if first:
                        dx3, ds3 = run_gather_bwd(dev, H, rows, drop, layout)
                        same_bits(dx3, dx, label + ": two runs")
                        same_bits(ds3, ds, label + ": two runs")
            first = False


# ============================================================================ D. bgnn_filter_edges
def run_filter(dev, ei, new_id, N, with_kept=True):
    E = ei.size(1)
    ws_bytes = _lib.query("bgnn_filter_edges_ws_bytes", E)
    ws = IntWin(dev, ws_bytes, U8, pad=512)                      # exactly the queried size
    out, kept, nk = IntWin(dev, 2 * E, I64), IntWin(dev, E, I64), IntWin(dev, 1, I64)
    ei, new_id = ei.contiguous().to(dev), new_id.to(dev)
    _lib.call("bgnn_filter_edges", ei.data_ptr(), E, new_id.data_ptr(), N, ptr(out),
              ptr(kept) if with_kept else None, ptr(nk), ptr(ws) if E else None, ws_bytes if E else 0, _stream())
    torch.cuda.synchronize()
    for w, what in ((ws, "workspace"), (out, "out_edges"), (kept, "kept"), (nk, "n_kept")):
        w.guard("filter_edges " + what)
    return out, kept, nk


def check_filter(label, got, want, E, with_kept=True):
    out, kept, nk = got
    r_out, r_kept, n = want
    equal(nk.read(), torch.tensor([n]), label + " n_kept")
    out.assert_all_written(label + " out_edges", 2 * n)
    out.assert_untouched(label + " out_edges", 2 * n)
    equal(out.read()[:2 * n].view(2, n), r_out, label + " out_edges")
    kept.assert_untouched(label + " kept", n if with_kept else 0)
    if with_kept:
        kept.assert_all_written(label + " kept", n)
        equal(kept.read()[:n], r_kept, label + " kept")


@pytest.mark.parametrize("E", P.FILTER_E)
def test_d_filter(dev, E):
    N = P.FILTER_N
    for j, kind in enumerate(P.FILTER_KEPT):
        ei, new_id = P.filter_inputs(E, kind)
        want = P.filter_ref(ei, new_id, N)
        label = f"bgnn_filter_edges E={E} kept={kind} ({want[2]} edges)"
        got = run_filter(dev, ei, new_id, N)
        check_filter(label, got, want, E)
        if j == 0:
            again = run_filter(dev, ei, new_id, N)
            for a, b in zip(again, got):
                equal(a.read(), b.read(), label + ": two runs")
        if kind == "half":
            check_filter(label + " kept=NULL", run_filter(dev, ei, new_id, N, with_kept=False), want, E, with_kept=False)


def test_d_filter_no_edges(dev):
    """E = 0: only *n_kept is written (0); no workspace is needed"""
    assert _lib.query("bgnn_filter_edges_ws_bytes", 0) >= 0
    _, new_id = P.filter_inputs(1, "half")
    out, kept, nk = run_filter(dev, torch.zeros(2, 0, dtype=I64), new_id, P.FILTER_N)
    equal(nk.read(), torch.tensor([0]), "bgnn_filter_edges E=0 n_kept")
    out.assert_untouched("E=0 out_edges")
    kept.assert_untouched("E=0 kept")


# ============================================================================ E. bgnn_heavy_plan
def run_heavy(dev, rowptr, chunk):
    R, nnz = len(rowptr) - 1, int(rowptr[-1])
    cap = 2 * (nnz // chunk) + 2
    ws_bytes = _lib.query("bgnn_heavy_plan_ws_bytes", R)
    ws = IntWin(dev, ws_bytes, U8, pad=512)
    hr, c0, owner, counts = IntWin(dev, R, I32), IntWin(dev, R + 1, I32), IntWin(dev, cap, I32), IntWin(dev, 2, I32)
    rp = torch.from_numpy(rowptr).to(dev)
    _lib.call("bgnn_heavy_plan", rp.data_ptr(), R, nnz, chunk, ptr(hr), ptr(c0), ptr(owner), ptr(counts), ptr(ws), ws_bytes,
              _stream())
    torch.cuda.synchronize()
    for w, what in ((ws, "workspace"), (hr, "heavy_row"), (c0, "heavy_chunk0"), (owner, "chunk_heavy"), (counts, "counts")):
        w.guard("heavy_plan " + what)
    return hr, c0, owner, counts


@pytest.mark.parametrize("chunk", P.HEAVY_CHUNKS)
def test_e_heavy_plan(dev, chunk):
    for j, (name, rowptr) in enumerate(P.heavy_cases(chunk).items()):
        r_hr, r_c0, r_owner, r_counts = P.heavy_plan_ref(rowptr, chunk)
        nh, nc = int(r_counts[0]), int(r_counts[1])
        label = f"bgnn_heavy_plan chunk={chunk} {name} R={len(rowptr) - 1} nnz={int(rowptr[-1])} ({nh} heavy rows, {nc} chunks)"
        got = run_heavy(dev, rowptr, chunk)
        hr, c0, owner, counts = got
        equal(counts.read(), torch.from_numpy(r_counts), label + " counts")
        for w, ref, upto, what in ((hr, r_hr, nh, "heavy_row"), (c0, r_c0, nh + 1, "heavy_chunk0"), (owner, r_owner, nc, "chunk_heavy")):
            w.assert_all_written(f"{label} {what}", upto)
            w.assert_untouched(f"{label} {what}", upto)          # nothing behind the prefix
            equal(w.read()[:upto], torch.from_numpy(ref), f"{label} {what}")
        if j == 0:
            for a, b in zip(run_heavy(dev, rowptr, chunk), got):
                equal(a.read(), b.read(), label + ": two runs")


# ============================================================================ F. bgnn_group_plan
def run_groups(dev, R, chunk, grow):
    rowptr, col, n, _ = P.group_csr(R, chunk)
    G = len(grow) - 1 if grow is not None else -(-n // R)
    gsrc, gmask, gcnt = IntWin(dev, len(col), I32), IntWin(dev, len(col), U8), IntWin(dev, G, I32)
    gr = torch.tensor(grow, dtype=I32, device=dev) if grow is not None else None
    rp, cl = torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)
    _lib.call("bgnn_group_plan", rp.data_ptr(), cl.data_ptr(), n, chunk, R, None if gr is None else gr.data_ptr(), G,
              ptr(gsrc), ptr(gmask), ptr(gcnt), _stream())
    torch.cuda.synchronize()
    for w, what in ((gsrc, "gsrc"), (gmask, "gmask"), (gcnt, "gcnt")):
        w.guard("group_plan " + what)
    return gsrc, gmask, gcnt


@pytest.mark.parametrize("R,chunk", P.GROUP_CASES, ids=[f"R{r}-chunk{c}" for r, c in P.GROUP_CASES])
def test_f_group_plan(dev, R, chunk):
    for grow in (None, P.group_starts(R, chunk)):
        label = f"bgnn_group_plan R={R} chunk={chunk} grow={'NULL' if grow is None else 'given'}"
        r_src, r_mask, r_cnt = P.group_plan_ref(R, chunk, grow)
        got = run_groups(dev, R, chunk, grow)
        gsrc, gmask, gcnt = got
        gcnt.assert_all_written(label + " gcnt")
        equal(gcnt.read(), torch.from_numpy(r_cnt), label + " gcnt")
        # the whole windows: per group its gcnt[g] keys from the group's base, the sentinel from there to the
        # next group's base
        equal(gsrc.read(), torch.from_numpy(r_src), label + " gsrc")
        equal(gmask.read(), torch.from_numpy(r_mask), label + " gmask")
        if grow is None:
            for a, b in zip(run_groups(dev, R, chunk, grow), got):
                equal(a.read(), b.read(), label + ": two runs")


# ============================================================================ G. the wrapper, NaN scores
def test_g_topk_select_with_nan_scores(dev):
    """graph 0 all NaN, graph 1 with one NaN: perm is the oracle's (NaN first, ties by index), every slot a
    node of its graph; the gather runs only on a perm that passed"""
    sizes = [6, 9]
    N, H = sum(sizes), 8
    _, batch = P.graph_arrays(sizes)
    g = torch.Generator().manual_seed(5)
    score = torch.randn(N, generator=g)
    score[:6] = float("nan")
    score[6 + 4] = float("nan")
    perm, new_id, batch_out = pool.topk_select(score.to(dev), 0.5, batch.to(dev))
    torch.cuda.synchronize()
    perm_h = perm.cpu()
    want = pyg_ref.topk(score, 0.5, batch)
    assert want.tolist()[:4] == [0, 1, 2, 10]
    equal(perm_h, want, "topk_select with NaN scores: perm")
    assert bool(((perm_h >= 0) & (perm_h < N)).all()) and perm_h.unique().numel() == perm_h.numel()
    equal(batch_out.cpu(), batch[want], "topk_select with NaN scores: batch_out")
    back = torch.full((N,), -1, dtype=I32)
    back[want] = torch.arange(want.numel(), dtype=I32)
    equal(new_id.cpu(), back, "topk_select with NaN scores: new_id")
    # only now: the gather on the checked perm
    x = torch.randn(N, H, generator=g)
    out = pool.gather_scale(x.to(dev), score.to(dev), perm, new_id).cpu()
    nan_rows = torch.isnan(score[want])
    assert bool(torch.isnan(out[nan_rows]).all()) and bool(torch.isfinite(out[~nan_rows]).all())
    same_bits(out[~nan_rows], (x[want] * score[want].view(-1, 1))[~nan_rows], "gather_scale on the checked perm")
