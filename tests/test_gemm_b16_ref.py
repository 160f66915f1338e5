"""The bounds of the bf16-storage conformance matrix have teeth (no GPU): the references of
tests/gemm_b16_ref.py equal plain fp64 torch on every matrix case, an f32 host evaluation in either
k-slice order stays inside every bound (and is bit-equal on the exact cases), and every mutation
leaves the reference by more than 8 bounds -- or changes a bit of an exact case -- at every case that
is meant to show it. A mutation that no case shows fails here: that is a hole in the matrix."""
import numpy as np
import pytest
import torch

import gemm_b16_ref as R
from gemm_b16_ref import D

GEMM_IDS = [R.gid(c) for c in R.GEMM_CASES]


def test_case_ids_are_unique():
    assert len(set(GEMM_IDS)) == len(GEMM_IDS)
    assert len({R.did(c) for c in R.C_CASES}) == len(R.C_CASES)


def _plain(c, d):
    """the same formula in plain fp64 torch (@, index_select, clamp_min)"""
    A, B = d["a"].bfloat16().double(), d["b"].bfloat16().double()
    v = c["alpha"] * ((A.t() if c["ta"] else A) @ (B.t() if c["tb"] else B))
    if c["beta"] != 0.0:
        v = v + c["beta"] * d["c0"].double()
    if d["bias"] is not None:
        v = v + d["bias"].double().unsqueeze(0)
    for t, i in ((d["add0"], d["idx0"]), (d["add1"], d["idx1"])):
        if t is not None:
            v = v + torch.index_select(t.double(), 0, i)
    return torch.clamp_min(v, 0) if c["relu"] else v


@pytest.mark.parametrize("c", R.GEMM_CASES, ids=GEMM_IDS)
def test_gemm_reference_plain_torch_and_f32_host(c):
    d = R.gemm_inputs(c)
    kw = R.gemm_kw(c, d)
    ref, mag = R.gemm_ref(d["a"], d["b"], c["ta"], c["tb"], **kw)
    assert ref.shape == (c["M"], c["N"])
    assert float((ref - _plain(c, d)).abs().max()) <= 1e-12 * max(1.0, float(mag.max()))
    if c["data"] == "round":     # the product with the identity IS bf16(A); zeros arrive as +0
        want = R.rounding_want(d["a"])
        assert torch.equal(ref, R.r16(d["a"]).to(D)) and not bool(torch.signbit(want[want == 0]).any())
        for rev in (False, True):
            h = R.host_f32(d["a"], d["b"], 0, 1, reverse=rev)
            assert torch.equal(h.view(torch.int32), want.view(torch.int32))
        return
    if c["exact"]:
        R.assert_exact_data(ref)
        assert c["K"] <= 512
    for rev in (False, True):
        h = R.host_f32(d["a"], d["b"], c["ta"], c["tb"], reverse=rev, **kw)
        if c["exact"]:
            assert torch.equal(h.to(D), ref)
            assert torch.equal(h.bfloat16(), R.round_c(ref).bfloat16())
        else:
            assert R.ratio((h.to(D) - ref).abs(), R.c_bound(ref, mag, False)) <= 1.0
            assert R.ratio((h.bfloat16().to(D) - ref).abs(), R.c_bound(ref, mag, True)) <= 1.0


def test_exact_cases_round_and_tie():
    """the exact bf16 C cases really round (values that need more than 8 bits) and meet ties"""
    rounds = ties = 0
    for c in R.GEMM_CASES:
        if c["exact"] and not c["data"] and any(s & 4 for s in c["sts"]):
            d = R.gemm_inputs(c)
            ref, _ = R.gemm_ref(d["a"], d["b"], c["ta"], c["tb"], **R.gemm_kw(c, d))
            err = (R.round_c(ref).to(D) - ref).abs()
            lo, hi = R.r16(ref.float(), True).to(D), None
            rounds += int((err > 0).sum())
            hi = torch.where(ref >= 0, torch.nextafter(lo.float().bfloat16(), torch.tensor(float("inf")).bfloat16()),
                             torch.nextafter(lo.float().bfloat16(), torch.tensor(float("-inf")).bfloat16())).to(D)
            ties += int(((ref != lo) & ((ref - lo).abs() == (hi - ref).abs())).sum())
    assert rounds > 1000 and ties > 100, (rounds, ties)


GEMM_MUTS = ("drop_last_k64", "clamp_row", "idx_prev", "idx_swap", "bias_256", "relu_early", "trunc_operand", "trunc_c")


@pytest.mark.parametrize("mut", GEMM_MUTS)
def test_gemm_mutations_show(mut):
    shown = 0
    for c in R.GEMM_CASES:
        if not R.shows(mut, c):
            continue
        d = R.gemm_inputs(c)
        kw = R.gemm_kw(c, d)
        ref, mag = R.gemm_ref(d["a"], d["b"], c["ta"], c["tb"], **kw)
        bad, _ = R.gemm_ref(d["a"], d["b"], c["ta"], c["tb"], mut=mut, **kw)
        if c["data"] == "round":
            want = R.rounding_want(d["a"])
            got = R.r16(d["a"], True) if mut == "trunc_operand" else R.r16(want, False)
            if mut == "trunc_c":   # the f32 C (storage 0) is bf16(A) exactly, so a truncated bf16 C cannot differ ...
                continue           # ... the exact cases below show it
            assert not torch.equal(got, want), R.gid(c)
        elif mut == "trunc_c":
            assert not torch.equal(R.round_c(ref, "trunc_c"), R.round_c(ref)), R.gid(c)
        elif c["exact"]:
            assert not torch.equal(bad, ref), R.gid(c)
        else:
            assert R.away(bad, ref, R.c_bound(ref, mag, False)) > 8, R.gid(c)
            if any(s & 4 for s in c["sts"]):
                assert R.away(R.r16(bad.float()), ref, R.c_bound(ref, mag, True)) > 8, R.gid(c)
        shown += 1
    assert shown > 0, f"no case of the matrix shows {mut}"


def test_every_mutation_is_covered():
    assert set(R.MUTATIONS) == set(GEMM_MUTS) | {"no_first_round", "group_shift", "no_ik", "deg_plus_1", "no_clamp",
                                                   "drop_ninth"}


# ---------------------------------------------------------------------------- drop-add
@pytest.mark.parametrize("c", R.C_CASES, ids=[R.did(c) for c in R.C_CASES])
def test_dropadd_reference(c):
    a, b, src = R.dropadd_inputs(c["M"], c["N"], c["K"], c["data"])
    ref, bound, exact, keep = R.dropadd_ref(a, b, src, c["p"], c["seed"])
    prod = (a.double() @ b.double().t()).float().bfloat16().double()
    ik = float(R.inv_keep(c["p"]))
    plain = prod + torch.where(keep, src.double() * ik, torch.zeros((), dtype=D))
    assert float((ref - plain).abs().max()) <= 1e-12 * 4096
    R.assert_exact_data(prod)
    assert exact == (c["p"] in (0.0, 0.5))
    if c["p"] == 0.0:
        assert bool(keep.all())
    # an f32 host evaluation: the product and the sum rounded separately, and as one fused operation
    w32 = np.where(keep.numpy(), src.numpy() * R.inv_keep(c["p"]), np.float32(0)).astype(np.float32)
    two = torch.from_numpy(prod.float().numpy() + w32).bfloat16()
    fused = plain.float().bfloat16()      # (one rounding of the fp64 value to f32, then bf16: the fma's result)
    for h in (two, fused):
        if exact:
            assert torch.equal(h, R.r16(ref.float()).bfloat16())
        assert R.ratio((h.to(D) - ref).abs(), bound) <= 1.0
    if c["data"]:     # A = 0: the zero pattern is the kept set
        assert torch.equal(two != 0, keep)


@pytest.mark.parametrize("mut", ["no_first_round", "group_shift", "no_ik"])
def test_dropadd_mutations_show(mut):
    shown = 0
    for c in R.C_CASES:
        a, b, src = R.dropadd_inputs(c["M"], c["N"], c["K"], c["data"])
        ref, bound, exact, keep = R.dropadd_ref(a, b, src, c["p"], c["seed"])
        # under the 2^-8 |ref| of an inexact ik only a zero product (A = 0) lets the addend's mistakes show
        if (mut != "no_first_round" and (c["p"] == 0.0 or not (exact or c["data"]))) or \
                (mut == "no_first_round" and (c["data"] or c["K"] < 96 or not exact)):
            continue
        bad = R.dropadd_ref(a, b, src, c["p"], c["seed"], mut=mut)[0]
        if exact:
            assert not torch.equal(R.r16(bad.float()), R.r16(ref.float())), R.did(c)
        else:
            assert R.away(bad, ref, bound) > 8, R.did(c)
        shown += 1
    assert shown > 0


# ---------------------------------------------------------------------------- csrc/elem.hip
SMALL = [e for e in R.ELEM_CASES if e[1] < 10 ** 6]


@pytest.mark.parametrize("k,n,p,seed,flag", SMALL, ids=[f"{e[0]}-{e[1]}-p{e[2]}-s{e[3] % 1000}-{e[4]}" for e in SMALL])
def test_elem_references(k, n, p, seed, flag):
    a, b = R.elem_inputs(n)
    keep = R.keep_mask(seed, 1, n, p).view(-1)
    ik = float(R.inv_keep(p))
    if k == "dropout":
        out, kp = R.add_dropout_ref(a, b if flag else None, p, seed)
        assert torch.equal(kp, keep)
        s = a.double() + (b.double() if flag else 0)
        plain = torch.where(keep, s * ik, torch.zeros((), dtype=D))
        # the f32 sum is exact on this data, so round16 of the f32 product is within one f32 rounding of plain
        assert R.ratio((out.double() - plain).abs(), R.E16 * plain.abs() + 2 * R.U * plain.abs() + 1e-300) <= 1.0
        if p > 0 and n > 8:
            for mut in ("group_shift", "no_ik"):
                assert not torch.equal(R.add_dropout_ref(a, b if flag else None, p, seed, mut=mut)[0], out)
    else:
        ref, bound, kp = R.add_dropped_ref(a, b, p, seed)
        plain = a.double() + torch.where(keep, b.double() * ik, torch.zeros((), dtype=D))
        assert float((ref - plain).abs().max()) <= 1e-12 * 16
        untouched = ~keep | (b == 0)
        assert torch.equal(ref[untouched], a.double()[untouched])
        if p > 0 and n > 8:
            for mut in ("group_shift", "no_ik"):
                bad = R.add_dropped_ref(a, b, p, seed, mut=mut)[0]
                assert R.away(bad, ref, bound) > 8 or not torch.equal(bad[untouched], a.double()[untouched])


def test_elem_large_size_passes_the_grid_cap():
    n = R.ELEM_N[2]
    assert n % 8 == 0 and n // 8 == 256 * 8192 + 1


@pytest.mark.parametrize("Rr,H,mean,exact", R.SEG_CASES, ids=[f"R{c[0]}-H{c[1]}-mean{c[2]}-exact{c[3]}" for c in R.SEG_CASES])
def test_segment_references(Rr, H, mean, exact):
    rowptr, col, E = R.seg_csr(Rr)
    x, g = R.seg_inputs(Rr, H, exact)
    deg = (rowptr[1:] - rowptr[:-1]).long()
    assert int(deg[-1]) == 0 and col.numel() == E and torch.equal(torch.sort(col.long()).values, torch.arange(E))
    if Rr == len(R.SEG_DEG):
        assert deg.tolist() == list(R.SEG_DEG)
    ref, bound = R.segment_sum_ref(rowptr, col, x, mean, exact)
    seg = torch.repeat_interleave(torch.arange(Rr), deg)
    plain = torch.zeros(Rr, H, dtype=D).index_add_(0, seg, x.double()[col.long()])
    if mean:
        plain = plain / deg.clamp_min(1).double().unsqueeze(1)
    assert float((ref - plain).abs().max()) <= 1e-12 * 4096
    # an f32 host evaluation: sequential f32 sums in CSR order and reversed, the reciprocal and the product
    if Rr <= 64:
        for rev in (False, True):
            h = torch.zeros(Rr, H)
            for r in range(Rr):
                rows = col.long()[int(rowptr[r]):int(rowptr[r + 1])]
                acc = torch.zeros(H)
                for j in (reversed(rows.tolist()) if rev else rows.tolist()):
                    acc = acc + x[j].float()
                h[r] = acc * (np.float32(1) / np.float32(max(int(deg[r]), 1))) if mean else acc
            assert R.ratio((h.double() - ref).abs(), bound) <= 1.0 or (bool(((h.double() - ref).abs() <= bound).all()))
    for mut in ("drop_ninth",) + (("deg_plus_1", "no_clamp") if mean else ()):
        bad = R.segment_sum_ref(rowptr, col, x, mean, exact, mut=mut)[0]
        # (a long row's random mean is small against its summation bound: deg + 1 shows there on exact data)
        rows = {"drop_ninth": deg >= 9, "deg_plus_1": (deg > 0) & ((deg <= 17) | bool(exact)), "no_clamp": deg == 0}[mut]
        if not bool(rows.any()):
            continue
        err = (bad - ref).abs()[rows]
        b = bound[rows]
        assert not bool(torch.isfinite(err).all()) or bool(((err > 8 * b).sum(1) > 0).all()), (mut, Rr, H)
    # the broadcast: torch's own expression per position
    out = R.segment_bcast_ref(rowptr, col, g, mean)
    want = (g / deg.clamp_min(1).float().unsqueeze(1) if mean else g).to(torch.bfloat16).index_select(0, seg)
    assert torch.equal(out[col.long()], want)


def test_segment_mutations_have_rows():
    deg = torch.tensor(R.SEG_DEG)
    assert bool((deg >= 9).any()) and bool((deg == 0).any()) and {0, 1, 7, 8, 9, 16, 17, 700} <= set(R.SEG_DEG)
