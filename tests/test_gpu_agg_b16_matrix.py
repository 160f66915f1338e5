"""GPU: fp64 conformance matrix of the bf16 gather skeleton (csrc/b16_gather.h) -- bgnn_spmm_fwd_bf16,
bgnn_spmm_bwd_bf16, bgnn_spmm_max_bf16 (arg NULL and non-NULL), bgnn_spmm_max_pack_bf16,
bgnn_sage_infer_bf16, bgnn_sage_fwd_bf16 -- and of bgnn_sage_tail_bf16, each on its raw entry point
(_lib.call).

References, bounds, inputs and case lists are tests/agg_b16_ref.py's (fp64 evaluations of the
header's formulas on the upcast bf16 rows; bounds from operation counts, u = 2^-24, none measured).
Structures: the kinds of the f32 aggregation matrix (tests/spmm_ref.py) and `dense`, planned with 4
and 8 rows per group; the device CSR is compared with the host's first (dev_graph), the device's
gcnt and chunk counts with the host's restatement here. Every output is a NaN-filled window inside
a guarded allocation (bf16: ld = H + 8, the packed planes 2H + 8; f32: ld = H + 4; the ld-less o of
bgnn_sage_fwd_bf16: guard rows above and below), every bf16 input a Buf with ld = H + 8 (z: 2H + 8),
NaN in its padding, before its first and after its last row, and NaN in every row of the gathered
plane that no edge names. The chunk scratch, the second plane of the argmax runs and bn_partial
start as NaN with a guard behind them. Every element of every output is compared; nothing is
excluded. Each test runs its first configuration twice and compares bits; each section prints its
largest err / bound."""
import pytest
import torch

import agg_b16_ref as A
import sage_rows_ref as SR
import spmm_ref as R
import test_gpu_spmm_matrix as M
from bgnn import _lib
from bgnn.graph import Csr, Plan, _stream, enqueue_groups
from matrix_util import RATIOS, Buf, Out, Win, check, inp, ptr
from test_gpu_spmm_matrix import ArgState, check_state, dev_graph, max_backward

pytestmark = pytest.mark.gpu

D, BF, F32 = torch.float64, torch.bfloat16, torch.float32
SUM, MEAN, MAX = R.SUM, R.MEAN, R.MAX


@pytest.fixture(autouse=True)
def _restore_knobs():
    for k in M.KNOBS:        # (max_backward sets the f32 kernels' knobs from these)
        if k not in M._defaults:
            M._defaults[k] = _lib.query("bgnn_get_tuning", k)
    yield
    for k in M.KNOBS:
        _lib.call("bgnn_set_tuning", k, M._defaults[k])
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault is sticky: nothing more of this session runs on the GPU
        pytest.exit(f"GPU fault in the bf16 aggregation matrix, session ended: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\nsection: largest err / bound")
    for k in sorted(RATIOS):
        if k.startswith("aggb16"):
            print(f"  {k}: {RATIOS[k]:.3f}")


# ============================================================================ structure on the device
_dev = {}


def graph(kind, dev):
    """dev_graph's dict for a kind of this matrix (dense_r8: the dense graph with plans of 8 rows)"""
    if kind in _dev:
        return _dev[kind]
    if kind == "dense_r8":
        G = dict(dev_graph("dense", dev))
        for k in ("fwd", "bwd"):
            c = G[k]
            G[k] = Csr(c.rowptr, c.col, c.n_rows, c.nnz, c.plan,
                       enqueue_groups(c.rowptr, c.col, c.n_rows, c.nnz, c.plan.chunk, rows=8))
        G["kind"], G["S"] = kind, R.struct(kind)
    else:
        G = dev_graph(kind, dev)
    for c in (G["fwd"], G["bwd"]):
        assert (c.groups.rows if c.groups is not None else 0) == A.group_rows(kind)
    _dev[kind] = G
    return G


def test_structure_on_the_device(dev):
    """the device plans hold the combine and key-batch cases: chunk counts of 16, 17, 175 and 44, and
    gcnt equal to the host's restatement with 64, 65, 256 (groups of 4) and 512 keys (a group of 8)"""
    for kind, rows, want in (("hand_c4", (10, 11, 500), (16, 17, 175)), ("hand_c16", (500,), (44,))):
        p = graph(kind, dev)["fwd"].plan
        hr = p.heavy_row[:p.n_heavy].cpu().tolist()
        c0 = p.heavy_chunk0[:p.n_heavy + 1].cpu().long()
        got = tuple(int(c0[hr.index(r) + 1] - c0[hr.index(r)]) for r in rows)
        assert got == want, f"{kind}: rows {rows} hold {got} chunks"
        assert {hr[h]: int(c0[h + 1] - c0[h]) for h in range(p.n_heavy)} == A.chunks_of(kind)
    seen = {}
    for kind in ("dense", "dense_r8", "hand", "hand_r8", "hand_t", "hand_c4", "hand_c16", "tiny5", "tiny9"):
        G = graph(kind, dev)
        for csr, tr in ((G["fwd"], False), (G["bwd"], True)):
            gr = csr.groups
            assert gr.grow is None and gr.n_groups == -(-G["n"] // gr.rows)
            host = A.edge_keys(kind, gr.rows, tr)[1]
            got = gr.gcnt[:gr.n_groups].cpu().long()
            assert torch.equal(got, host), f"{kind} {'transpose' if tr else 'forward'}: gcnt differs from the host's keys"
            seen[(kind, tr)] = set(got.tolist())
    assert {64, 65, 256} <= seen[("dense", False)] and 512 in seen[("dense_r8", False)]
    assert any(c % 8 for c in seen[("dense", False)]) and any(c % 4 for c in seen[("dense_r8", False)])
    assert max(seen[("hand", False)]) == 67          # what the old tests reach: one group past 64 keys


# ============================================================================ helpers
def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def same_bits(a, b, what):
    d = bits(a) != bits(b)
    assert not bool(d.any()), f"{what}: {int(d.sum())} elements differ in bits; first at {d.nonzero()[0].tolist()}"


def out_win(dev, n, H, f32, planes=1):
    return Win(dev, n, planes * H, H + 4 if f32 else planes * H + 8, F32 if f32 else BF)


def scratch(dev, csr, H, planes=1):
    part = M.scratch_for(dev, csr, H, planes)
    return part, (ptr(part) if csr.plan.n_chunks else None)


def vec(dev, t):
    return None if t is None else inp(dev, t)


def rounds_to(o16, o32, what):
    """the bf16 output is torch's nearest-even rounding of the kernel's own f32 output, bit for bit"""
    same_bits(o16, o32.to(BF), what + ": the bf16 store against the rounded f32 store")


# ============================================================================ A. the sums
def run_sum(dev, G, xb, H, reduce, transposed, f32):
    csr = G["bwd"] if transposed else G["fwd"]
    xin = Buf(dev, xb, ld=H + 8, dtype=BF)
    out = out_win(dev, G["n"], H, f32)
    part, pp = scratch(dev, csr, H)
    if transposed:
        _lib.call("bgnn_spmm_bwd_bf16", csr.ref(), G["frp"].data_ptr(), ptr(xin), xin.ld, H, reduce, ptr(out), out.ld,
                  int(f32), pp, _stream())
    else:
        _lib.call("bgnn_spmm_fwd_bf16", csr.ref(), ptr(xin), xin.ld, H, reduce, ptr(out), out.ld, int(f32), pp, _stream())
    torch.cuda.synchronize()
    out.guard("sum out")
    part.guard("sum chunk scratch")
    return out.read()


@pytest.mark.parametrize("transposed", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("kind,H", A.CASES, ids=A.IDS)
def test_a_sums(dev, kind, H, transposed):
    G = graph(kind, dev)
    S = G["S"]
    name = "bgnn_spmm_bwd_bf16" if transposed else "bgnn_spmm_fwd_bf16"
    deg = S.deg_t if transposed else S.deg
    empty, heavy = deg == 0, deg > S.chunk
    xb, xe = A.randn_b16(kind, H, int(transposed), transposed), A.exact_b16(kind, H, transposed)
    assert int(torch.isnan(xb).any(1).sum()) == int(A.unnamed(kind, transposed).sum()) == int(torch.isnan(xe).any(1).sum())
    first = None
    for reduce in (SUM, MEAN):
        label = f"{name} {kind} N={G['n']} H={H} {'mean' if reduce else 'sum'}"
        ref, bound = A.sum_ref(kind, xb, reduce, transposed)
        o32 = run_sum(dev, G, xb, H, reduce, transposed, True)
        check(f"aggb16 A {name[10:13]} {'mean' if reduce else 'sum'}", o32, ref, bound, label)
        o16 = run_sum(dev, G, xb, H, reduce, transposed, False)
        rounds_to(o16, o32, label)
        assert bool((bits(o32)[empty] == 0).all()) and bool((bits(o16)[empty] == 0).all()), f"{label}: an empty row is not +0"
        if first is None:
            first = o32
            same_bits(run_sum(dev, G, xb, H, reduce, transposed, True), o32, label + ": two runs")
        if kind == "hand" and bool(heavy.any()):   # the chunk and combine path does not depend on the light family
            other = run_sum(dev, graph("hand_nogroups", dev), xb, H, reduce, transposed, True)
            same_bits(other[heavy], o32[heavy], label + ": heavy rows, with and without a row-group plan")
    # the exact input: integers, every partial sum below 2^24 -- SUM equals the fp64 sum bit for bit
    label = f"{name} {kind} N={G['n']} H={H} sum, exact input"
    ref, _ = A.sum_ref(kind, xe, SUM, transposed)
    o32 = run_sum(dev, G, xe, H, SUM, transposed, True)
    assert bool(torch.isfinite(o32).all()), f"{label}: not finite"
    wrong = o32.to(D) != ref
    assert not bool(wrong.any()), f"{label}: {int(wrong.sum())} elements differ from the integer sum; first at {wrong.nonzero()[0].tolist()}"
    rounds_to(run_sum(dev, G, xe, H, SUM, transposed, False), o32, label)


# ============================================================================ B. the max kernels
def run_max(dev, G, xb, H, state):
    csr = G["fwd"]
    xin = Buf(dev, xb, ld=H + 8, dtype=BF)
    out = out_win(dev, G["n"], H, False)
    part, pp = scratch(dev, csr, H, 2)
    _lib.call("bgnn_spmm_max_bf16", csr.ref(), ptr(xin), xin.ld, H, ptr(out), out.ld, ptr(state), pp, _stream())
    torch.cuda.synchronize()
    out.guard("max out")
    part.guard("max chunk scratch (values and positions)")
    return out.read()


def run_pack(dev, G, x, H, state):
    csr = G["fwd"]
    xin = Buf(dev, x, ld=H + 4, dtype=F32)
    out = out_win(dev, G["n"], H, False, planes=2)
    part, pp = scratch(dev, csr, H, 2)
    _lib.call("bgnn_spmm_max_pack_bf16", csr.ref(), ptr(xin), xin.ld, H, ptr(out), out.ld, ptr(state), pp, _stream())
    torch.cuda.synchronize()
    out.guard("pack out (columns from 2H on)")
    part.guard("pack chunk scratch (values and positions)")
    o = out.read()
    return o[:, :H].contiguous(), o[:, H:].contiguous()


def backward(dev, G, kind, x, H, state, label, i, ref):
    """bgnn_spmm_bwd_max on a state that passed check_state: the f32 matrix's max_backward where its
    geometry table knows H, else the same comparison under the default knobs"""
    if (H, "") in R.EXPECT_GEOMETRY:
        return max_backward(dev, G, kind, x, (H, ""), state, label, i, ref)
    g, a = R.randn_rows(kind, H, 1), R.randn_rows(kind, H, 2)
    for addend in (None, a):
        r, b = R.max_bwd_ref(kind, x, g, addend, fwd=ref)
        o = M.run_bwd(dev, G, g, (H, ""), MAX, addend, None, state)
        check(f"aggb16 B bwd_max{' + addend' if addend is not None else ''}", o, r, b, label + " bwd_max")


def same_state(a, b, label):
    for p, q in zip(a.decode(label), b.decode(label)):
        assert torch.equal(p, q), f"{label}: the state differs between two runs"


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=A.IDS)
def test_b_max(dev, i):
    kind, H = A.CASES[i]
    G = graph(kind, dev)
    S, csr = G["S"], G["fwd"]
    for which in ("randn", "ties", "nonfinite"):
        xb = A.max_input(kind, H, which).to(BF)
        x = xb.float()
        ref = R.max_fwd_ref(kind, x)
        want = ref["out"].float().to(BF)
        label = f"bgnn_spmm_max_bf16 {kind} N={G['n']} H={H}, {which} inputs"
        same_bits(run_max(dev, G, xb, H, None), want, label + " arg=NULL")
        state = ArgState(dev, S.n, H, csr.plan.n_heavy)
        o = run_max(dev, G, xb, H, state)
        same_bits(o, want, label + " with arg")
        check_state(state, S, csr, x, o.float(), ref, label)      # on the host, before any backward sees it
        backward(dev, G, kind, x, H, state, label, i, ref)
        if which == "randn":
            again = ArgState(dev, S.n, H, csr.plan.n_heavy)
            same_bits(run_max(dev, G, xb, H, again), o, label + ": two runs")
            same_state(again, state, label)


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=A.IDS)
def test_b_max_pack(dev, i):
    kind, H = A.CASES[i]
    G = graph(kind, dev)
    S, csr = G["S"], G["fwd"]
    for which in ("subbf16", "ties", "nonfinite"):
        x = A.max_input(kind, H, which)
        ref = R.max_fwd_ref(kind, x)                               # the f32 maximum and its first maximiser
        label = f"bgnn_spmm_max_pack_bf16 {kind} N={G['n']} H={H}, {which} inputs"
        state = ArgState(dev, S.n, H, csr.plan.n_heavy)
        p0, p1 = run_pack(dev, G, x, H, state)
        same_bits(p0, ref["out"].float().to(BF), label + " plane 0 = bf16(the f32 maximum)")
        nan = torch.isnan(x)
        assert bool(torch.isnan(p1[nan]).all()), f"{label}: a NaN of x is not one in plane 1"
        same_bits(torch.where(nan, torch.zeros((), dtype=BF), p1), torch.where(nan, torch.zeros(()), x).to(BF),
                  label + " plane 1 = bf16(x)")
        check_state(state, S, csr, x.to(BF).float(), p0.float(), ref, label)
        backward(dev, G, kind, x, H, state, label, i, ref)
        if which == "subbf16":
            again = ArgState(dev, S.n, H, csr.plan.n_heavy)
            q0, q1 = run_pack(dev, G, x, H, again)
            same_bits(q0, p0, label + ": two runs")
            same_bits(q1, p1, label + ": two runs")
            same_state(again, state, label)


# ============================================================================ C. the eval-mode layer
def run_infer(dev, G, d, H, flags, f32):
    mean, affine, skip, bias = flags
    csr = G["fwd"]
    zin = Buf(dev, d["z"], ld=2 * H + 8, dtype=BF)
    xp = Buf(dev, d["xprev"], ld=H + 8, dtype=BF) if skip else None
    b, sc, sh = vec(dev, d["bias"] if bias else None), vec(dev, d["scale"] if affine else None), vec(dev, d["shift"] if affine else None)
    out = out_win(dev, G["n"], H, f32)
    part, pp = scratch(dev, csr, H)
    _lib.call("bgnn_sage_infer_bf16", csr.ref(), ptr(zin), zin.ld, ptr(b), ptr(sc), ptr(sh), ptr(xp), xp.ld if skip else 0,
              H, mean, ptr(out), out.ld, int(f32), pp, _stream())
    torch.cuda.synchronize()
    out.guard("infer out")
    part.guard("infer chunk scratch")
    return out.read()


def run_tail(dev, y, d, H, flags, f32, plane=False):
    """bgnn_sage_tail_bf16 on y [n, H]; plane: y is the z_r plane of a [n, 2H] buffer, read in place"""
    affine, skip, bias = flags
    n = y.size(0)
    if plane:
        yin = Buf(dev, y, ld=2 * H + 8, dtype=BF)
        yp, ldy = yin.ptr + 2 * H, yin.ld
    else:
        yin = Buf(dev, y, ld=H + 8, dtype=BF)
        yp, ldy = yin.ptr, yin.ld
    xp = Buf(dev, d["xprev"], ld=H + 8, dtype=BF) if skip else None
    b, sc, sh = vec(dev, d["bias"] if bias else None), vec(dev, d["scale"] if affine else None), vec(dev, d["shift"] if affine else None)
    out = out_win(dev, n, H, f32)
    _lib.call("bgnn_sage_tail_bf16", yp, ldy, ptr(b), ptr(sc), ptr(sh), ptr(xp), xp.ld if skip else 0, n, H, ptr(out), out.ld,
              int(f32), _stream())
    torch.cuda.synchronize()
    out.guard("tail out")
    return out.read()


def zero_norm_value(d, r, affine, skip, H):
    """ReLU(shift) + x_prev of a row with h = 0, in f32 (one rounding at most: the kernel's)"""
    v = torch.relu(d["shift"]) if affine else torch.zeros(H)
    return v + d["xprev"][r].float() if skip else v


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=A.IDS)
def test_c_infer(dev, i):
    kind, H = A.CASES[i]
    G = graph(kind, dev)
    S = G["S"]
    d = A.layer_inputs(kind, H)
    assert int(torch.isnan(d["z"][:, :H]).any(1).sum()) == int(A.unnamed(kind).sum())
    runs = [f for c, f in A.INFER_CASES if c == (kind, H)]
    assert len(runs) == 4
    iso = (S.deg == 0).nonzero().flatten()
    for j, flags in enumerate(runs):
        mean, affine, skip, bias = flags
        label = f"bgnn_sage_infer_bf16 {kind} N={G['n']} H={H} mean={mean} affine={affine} skip={skip} bias={bias}"
        ref, bound = A.infer_ref(kind, d, *flags)
        y32 = run_infer(dev, G, d, H, flags, True)
        check(f"aggb16 C infer{' affine' if affine else ''}{' skip' if skip else ''}", y32, ref, bound, label)
        rounds_to(run_infer(dev, G, d, H, flags, False), y32, label)
        zr = A.zero_row(kind)
        if zr is not None and not bias:
            same_bits(y32[zr], zero_norm_value(d, zr, affine, skip, H), label + f": the zero-norm row {zr}")
        if j == 0:
            same_bits(run_infer(dev, G, d, H, flags, True), y32, label + ": two runs")
        if kind == "hand":   # a row with a zero aggregate gets the same bits from the tail alone
            assert iso.numel() == 101
            for f32 in (True, False):
                t = run_tail(dev, d["z"], d, H, flags[1:], f32, plane=True)
                yk = y32 if f32 else run_infer(dev, G, d, H, flags, False)
                same_bits(t[iso], yk[iso], label + f": isolated rows, infer against tail (out_f32={int(f32)})")


@pytest.mark.parametrize("i", range(0, len(A.TAIL_CASES), 4), ids=[f"{n}-{h}" for (n, h), _ in A.TAIL_CASES[::4]])
def test_c_tail(dev, i):
    (n, H), _ = A.TAIL_CASES[i]
    d = A.tail_inputs(n, H)
    for j, ((_n, _h), flags) in enumerate(A.TAIL_CASES[i:i + 4]):
        affine, skip, bias = flags
        label = f"bgnn_sage_tail_bf16 N={n} H={H} affine={affine} skip={skip} bias={bias}"
        ref, bound = A.tail_ref(d, *flags)
        y32 = run_tail(dev, d["y"], d, H, flags, True)
        check(f"aggb16 C tail{' affine' if affine else ''}{' skip' if skip else ''}", y32, ref, bound, label)
        rounds_to(run_tail(dev, d["y"], d, H, flags, False), y32, label)
        if not bias:
            same_bits(y32[n // 2], zero_norm_value(d, n // 2, affine, skip, H), label + ": the zero-norm row")
        if j == 0:
            same_bits(run_tail(dev, d["y"], d, H, flags, True), y32, label + ": two runs")


# ============================================================================ D. the training-mode layer
def run_fwd(dev, G, d, H, mean, bias, slots, stats=True):
    csr = G["fwd"]
    n = G["n"]
    zin = Buf(dev, d["z"], ld=2 * H + 8, dtype=BF)
    b = vec(dev, d["bias"] if bias else None)
    o, nrm, bnp = Win(dev, n, H, H, F32), Out(dev, 1, n), Out(dev, 1, slots * 2 * H)
    part, pp = scratch(dev, csr, H)
    _lib.call("bgnn_sage_fwd_bf16", csr.ref(), ptr(zin), zin.ld, ptr(b), H, mean, ptr(o), ptr(nrm), ptr(bnp) if stats else None,
              pp, _stream())
    torch.cuda.synchronize()
    o.guard("sage_fwd_bf16 o")
    nrm.guard("sage_fwd_bf16 nrm")
    bnp.guard("sage_fwd_bf16 bn_partial")
    part.guard("sage_fwd_bf16 chunk scratch")
    return o.read(), nrm.read().view(-1), bnp.read().view(slots, 2, H)


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=A.IDS)
def test_d_fwd(dev, i):
    kind, H = A.CASES[i]
    G = graph(kind, dev)
    S, csr = G["S"], G["fwd"]
    d = A.layer_inputs(kind, H)
    slots = _lib.query("bgnn_sage_fwd_bf16_slots", csr.ref())
    light, nh, groups = A.expect_slots(kind, csr.groups.n_groups if kind == "store" else None)
    assert slots == light + nh, f"{kind}: {slots} slots, the rule written out gives {light} + {nh}"
    assert nh == csr.plan.n_heavy and (groups is None) == (csr.groups is None)
    rmax = SR.fwd_rows_per_slot(S.n, slots, nh, groups)
    heavy = csr.plan.heavy_row[:nh].cpu().long()
    for j, (mean, bias) in enumerate(f for c, f in A.FWD_CASES if c == (kind, H)):
        label = f"bgnn_sage_fwd_bf16 {kind} N={G['n']} H={H} mean={mean} bias={bias}"
        ref = A.layer_ref(kind, d["z"], d["bias"] if bias else None, mean)
        o, nrm, P = run_fwd(dev, G, d, H, mean, bias, slots)
        check("aggb16 D fwd o", o, ref["o"], ref["o_bound"], label + " o")
        check("aggb16 D fwd nrm", nrm, ref["nrm"], ref["nrm_bound"], label + " nrm (every row, heavy rows included)")
        zr = A.zero_row(kind)
        if zr is not None and not bias:
            assert float(nrm[zr]) == 0.0 and bool((bits(o[zr]) == 0).all()), f"{label}: the zero-norm row {zr}"
        assert bool(torch.isfinite(P).all()), f"{label}: {int((~torch.isfinite(P)).any(2).any(1).sum())} of the {slots} slots not written"
        if nh:
            same_bits(P[light:, 0], o[heavy], label + ": a heavy row's slot is its stored o")
            sq = o[heavy].to(D) ** 2
            check("aggb16 D heavy slot o^2", P[light:, 1], sq, SR.U * sq, label + " heavy slots' squares")
        (s0, b0), (s1, b1) = A.slot_sums_ref(o, rmax)
        check("aggb16 D sum o", P[:, 0].to(D).sum(0), s0, b0, f"{label} slot sums of o (Rmax = {rmax}, {slots} slots)")
        check("aggb16 D sum o^2", P[:, 1].to(D).sum(0), s1, b1, f"{label} slot sums of o^2 (Rmax = {rmax})")
        o2, nrm2, P2 = run_fwd(dev, G, d, H, mean, bias, slots, stats=False)
        same_bits(o2, o, label + ": o with bn_partial = NULL")
        same_bits(nrm2, nrm, label + ": nrm with bn_partial = NULL")
        assert bool(torch.isnan(P2).all()), f"{label}: bn_partial = NULL, yet a slot was written"
        if j == 0:
            o3, nrm3, P3 = run_fwd(dev, G, d, H, mean, bias, slots)
            same_bits(o3, o, label + ": two runs")
            same_bits(nrm3, nrm, label + ": two runs")
            same_bits(P3, P, label + ": two runs")


# ============================================================================ E. no rows
def test_e_no_rows(dev):
    """N = 0: every entry point returns BGNN_OK and writes nothing"""
    H = 8
    zi = torch.zeros(2, dtype=torch.int32, device=dev)
    csr = Csr(zi[:1], zi[:1], 0, 0, Plan(zi[:1], zi, zi[:1], 0, 0, 64))
    x16, x32 = Buf(dev, torch.zeros(0, 2 * H), ld=2 * H + 8, dtype=BF), Buf(dev, torch.zeros(0, H), ld=H + 4, dtype=F32)
    b = vec(dev, torch.zeros(H))
    wins = []
    for f32 in (True, False):
        for reduce in (SUM, MEAN):
            out = out_win(dev, 0, H, f32)
            _lib.call("bgnn_spmm_fwd_bf16", csr.ref(), ptr(x16), x16.ld, H, reduce, ptr(out), out.ld, int(f32), None, _stream())
            _lib.call("bgnn_spmm_bwd_bf16", csr.ref(), zi.data_ptr(), ptr(x16), x16.ld, H, reduce, ptr(out), out.ld, int(f32),
                      None, _stream())
            _lib.call("bgnn_sage_infer_bf16", csr.ref(), ptr(x16), x16.ld, ptr(b), ptr(b), ptr(b), ptr(x16), x16.ld, H, reduce,
                      ptr(out), out.ld, int(f32), None, _stream())
            wins.append(out)
        out = out_win(dev, 0, H, f32)
        _lib.call("bgnn_sage_tail_bf16", ptr(x16), x16.ld, ptr(b), ptr(b), ptr(b), ptr(x16), x16.ld, 0, H, ptr(out), out.ld,
                  int(f32), _stream())
        wins.append(out)
    state = ArgState(dev, 0, H, 0)
    for arg in (None, state):
        out = out_win(dev, 0, H, False)
        _lib.call("bgnn_spmm_max_bf16", csr.ref(), ptr(x16), x16.ld, H, ptr(out), out.ld, ptr(arg), None, _stream())
        wins.append(out)
    out = out_win(dev, 0, H, False, planes=2)
    _lib.call("bgnn_spmm_max_pack_bf16", csr.ref(), ptr(x32), x32.ld, H, ptr(out), out.ld, ptr(state), None, _stream())
    wins.append(out)
    slots = _lib.query("bgnn_sage_fwd_bf16_slots", csr.ref())
    assert slots == 8                                  # the count is the grid's, at least 8; no slot is written
    o, nrm, bnp = Win(dev, 0, H, H, F32), Out(dev, 1, 1), Out(dev, 1, slots * 2 * H)
    for reduce in (SUM, MEAN):
        _lib.call("bgnn_sage_fwd_bf16", csr.ref(), ptr(x16), x16.ld, ptr(b), H, reduce, ptr(o), ptr(nrm), ptr(bnp), None, _stream())
    torch.cuda.synchronize()
    for w in wins + [o]:
        w.guard("N = 0")
    state.decode("N = 0")
    nrm.guard("N = 0 nrm")
    bnp.guard("N = 0 bn_partial")
    assert bool(torch.isnan(nrm.read()).all()) and bool(torch.isnan(bnp.read()).all())
