"""GPU: fp64 conformance matrix of the f32 SAGE layer row kernels -- bgnn_sage_fwd (the aggregation
with the SAGE epilogue, csrc/spmm.hip) and every entry point of csrc/sage.hip -- each on its raw
entry point (_lib.call), at the smallest shapes that reach every branch: partly filled lanes
(H = 4, 12, 100, 252, 260, 508), the one / two float4 per lane dispatch edge (H = 256 / 260), fewer
rows than waves, more than 4 * 1024 rows (row blocks of 5 rows and trailing blocks without rows),
the reversed row walks, zero-norm rows, every optional argument, the slot-count boundaries of the
reductions, and the dropout mask against its host restatement.

References, bounds, inputs and the case lists are tests/sage_rows_ref.py's (fp64 evaluations of the
header's formulas; bounds from the operation counts, u = 2^-24, none measured); the mask is the
host restatement there, never a kernel's. Every output is a window pre-filled with NaN inside a
larger allocation whose guard rows and ld padding hold a fixed bit pattern that must survive the
call; partial buffers start as NaN, so a slot that is not written poisons its reduction; inputs carry
NaN in the rows after n_rows. Column sums are checked where the header fixes their structure: the
slots are summed in fp64 on the host and compared with the fp64 column sum of the rows the kernel
itself wrote (o, dh, x_next: each held to its own bound per element), within (R + 3) u sum |terms|, R
the rows per slot of the documented partition. Each section prints its largest err / bound ratio.

Sections: A sage_fwd, B sage_apply, C sage_bwd_stats + reduce_partials, D sage_bwd_rows,
E l2norm_bwd, F bn_finalize / bn_finalize_shifted / bn_eval_coeffs / reduce_partials on synthetic
partials, G linear_bwd_prep, H one dropout mask for every consumer."""
import pytest
import torch

import sage_rows_ref as R
from bgnn import _lib
from bgnn.graph import Csr, _stream
from matrix_util import RATIOS, Out, amax_prev, check, check_amax, inp, ptr, scalar
from test_gpu_spmm_b16 import graph_case

pytestmark = pytest.mark.gpu

D = torch.float64
KNOBS = (1, 3, 13)      # BGNN_TUNE_SEG_KERNEL, BGNN_TUNE_SEG_U, BGNN_TUNE_ROWS_REV
_defaults = {}


@pytest.fixture(autouse=True)
def _restore_knobs():
    for k in KNOBS:
        if k not in _defaults:
            _defaults[k] = _lib.query("bgnn_get_tuning", k)
    yield
    for k in KNOBS:
        _lib.call("bgnn_set_tuning", k, _defaults[k])
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault is sticky: nothing more of this session runs on the GPU
        pytest.exit(f"GPU fault in the SAGE row-kernel matrix, session ended: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\nsection: largest err / bound")
    for k in sorted(RATIOS):
        print(f"  {k}: {RATIOS[k]:.3f}")


def slots_sum(part, S, H, label):
    """the [S, 2, H] partial window summed over its slots in fp64 on the host"""
    part.guard(label + " partials")
    return part.read().view(S, 2, H)


def reduce_check(dev, P, S, H, accumulate, null, label, sec="C reduce_partials"):
    """bgnn_reduce_partials on the kernel's own partials P [S, 2, H] against their fp64 sums"""
    pbuf = inp(dev, P.reshape(S, 2 * H))
    prev = [torch.randn(H, generator=torch.Generator().manual_seed(S + H + k)) if accumulate else None for k in (0, 1)]
    outs = [None if null == k else Out(dev, 1, H, init=prev[k]) for k in (0, 1)]
    _lib.call("bgnn_reduce_partials", ptr(pbuf), S, H, ptr(outs[0]), ptr(outs[1]), accumulate, _stream())
    for k in (0, 1):
        if outs[k] is None:
            continue
        outs[k].guard(label)
        ref, bound = R.reduce_partials_ref(P, k, prev[k])
        check(sec, outs[k].read().view(H), ref, bound, f"{label} reduce_partials half {k} accumulate={accumulate}")


# ============================================================================ A. bgnn_sage_fwd
_csrs = {}


def fwd_graph(kind, dev):
    """(host edge_index, N, Csr, knob settings, (group_rows, n_groups) of the row-group kernel or None)"""
    base = {"hand": "hand", "hand_r8": "hand_r8", "blocked": "hand", "store": "store", "store_hagg": "store"}.get(
        kind, "hand_rows")
    ei, n, fwd, _bwd, _frp, _keep = graph_case(base, dev)
    knobs = {}
    if kind.startswith("rows_u"):
        knobs[3] = int(kind[6:])
    if kind == "blocked":
        knobs[1] = 1
    if kind not in _csrs:
        c = Csr(fwd.rowptr, fwd.col, fwd.n_rows, fwd.nnz, fwd.plan, fwd.groups)   # a copy: ranges stay off the shared one
        if kind == "store_hagg":
            c.ensure_ranges()
            assert c.ranges_all == 1
        _csrs[kind] = c
    c = _csrs[kind]
    groups = None
    if c.groups is not None and kind != "blocked":
        gr = c.groups
        groups = (gr.rows, gr.n_groups if gr.grow is not None else -(-n // gr.rows))
    return ei, n, c, knobs, groups


@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.case_id)
def test_a_sage_fwd(dev, case):
    kind, H, mean, inter, rev = case
    ei, n, csr, knobs, groups = fwd_graph(kind, dev)
    for k, v in knobs.items():
        _lib.call("bgnn_set_tuning", k, v)
    _lib.call("bgnn_set_tuning", 13, (_defaults[13] & ~4) | (4 if rev else 0))
    label = f"bgnn_sage_fwd {kind} N={n} H={H} mean={mean} z={'[N, 2H]' if inter else 'planes'} rev={rev} " \
            f"kernel={'row groups of %d' % groups[0] if groups else ('blocked' if kind == 'blocked' else 'one row per wave')}"
    d = R.fwd_inputs(n, H)
    zl, zr, b = d["z"][:, :H].contiguous(), d["z"][:, H:].contiguous(), d["b"]
    if inter:
        zbuf = inp(dev, d["z"])
        pzl, pzr, ldz = zbuf.data_ptr(), zbuf.data_ptr() + 4 * H, 2 * H
    else:
        zbuf = (inp(dev, zl), inp(dev, zr))
        pzl, pzr, ldz = zbuf[0].data_ptr(), zbuf[1].data_ptr(), H
    bbuf = inp(dev, b)
    nh, nck = csr.plan.n_heavy, csr.plan.n_chunks
    hagg = heavy = hbuf = None
    if kind == "store_hagg":   # the range rows' aggregates: fp64 sums of their z_l rows, rounded to f32
        rg = csr.ranges.cpu()
        heavy = csr.plan.heavy_row[:nh].cpu().long()
        hagg = torch.zeros(nh, H)
        for k in range(int(rg[0])):
            a, e, h = rg[2 + 3 * k:5 + 3 * k].tolist()
            hagg[h] = zl[a:e].to(D).sum(0).float()
        hbuf = Out(dev, nh, H, init=hagg)          # ld = H + 4, padding PATTERN
    ref = R.sage_fwd_ref(ei, n, zl, zr, b, mean, hagg, heavy)
    slots = _lib.query("bgnn_sage_fwd_slots", csr.ref())
    assert slots == R.fwd_slots(n, nh if nck else 0, groups), f"{label}: {slots} slots"
    assert slots > (nh if nck else 0) and (slots - (nh if nck else 0)) % 8 == 0

    def run():
        o, nrm, part = Out(dev, n, H, ld=H), Out(dev, 1, n), Out(dev, slots, 2 * H, ld=2 * H)
        scratch = Out(dev, 1, max(nck, 1) * H)
        _lib.call("bgnn_sage_fwd", csr.ref(), pzl, ldz, pzr, ldz, ptr(bbuf), H, mean, ptr(o), ptr(nrm), ptr(part),
                  ptr(scratch) if nck else None, ptr(hbuf), hbuf.ld if hbuf else 0, _stream())
        torch.cuda.synchronize()
        for w, nm in ((o, "o"), (nrm, "nrm"), (part, "bn_partial"), (scratch, "chunk scratch")):
            w.guard(f"{label} {nm}")
        return o.read(), nrm.read().view(n), part.read().view(slots, 2, H)

    runs = [run(), run()]
    ko, kn, P = runs[0]
    check("A sage_fwd o", ko, ref["o"], ref["o_bound"], label + " o")
    check("A sage_fwd nrm", kn, ref["nrm"], ref["nrm_bound"], label + " nrm")
    assert int((ref["cnt"] == 0).sum()) == (101 if not kind.startswith("store") else 0)   # empty rows: h = z_r + b
    Rr = R.fwd_rows_per_slot(n, slots, nh if nck else 0, groups)
    assert bool(torch.isfinite(P).all()), f"{label}: a BatchNorm slot of the {slots} was not written"
    s, bound = R.colsum(ko, Rr)
    check("A sage_fwd sum o", P[:, 0].to(D).sum(0), s, bound, f"{label} column sums of o (R = {Rr}, {slots} slots)")
    s, bound = R.colsum(ko.to(D) ** 2, Rr)
    check("A sage_fwd sum o^2", P[:, 1].to(D).sum(0), s, bound, f"{label} column sums of o^2 (R = {Rr})")
    for a, b2, nm in zip(runs[0], runs[1], ("o", "nrm", "bn_partial")):
        assert torch.equal(a, b2), f"{label}: {nm} differs between two runs"
    if kind == "blocked":
        # every kernel runs one row arithmetic (seg_common.h): the one-row-per-wave kernel's o and nrm are the
        # blocked kernel's bit for bit (bn_partial is not compared: the slots partition the rows differently)
        _lib.call("bgnn_set_tuning", 1, 2)
        assert _lib.query("bgnn_sage_fwd_slots", csr.ref()) == slots
        so, sn, _ = run()
        assert torch.equal(so, ko), f"{label}: o differs from the one-row-per-wave kernel's"
        assert torch.equal(sn, kn), f"{label}: nrm differs from the one-row-per-wave kernel's"


# ============================================================================ B. bgnn_sage_apply
def run_apply(dev, d, n, H, aff, skip, p, seed, prev, ranges=None, rpart=None):
    bufs = [inp(dev, d["o"]), inp(dev, d["scale"]) if aff else None, inp(dev, d["shift"]) if aff else None,
            inp(dev, d["xprev"])]
    x, am = Out(dev, n, H, ld=H), scalar(dev, prev)
    _lib.call("bgnn_sage_apply", ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), skip, p, seed, n, H, ptr(x),
              ptr(am), ptr(ranges), ptr(rpart), _stream())
    torch.cuda.synchronize()
    return x, am


def check_apply(sec, d, n, H, aff, skip, p, seed, prev, x, am, label):
    ref, bound, keep = R.sage_apply_ref(d["o"], d["scale"] if aff else None, d["shift"] if aff else None, d["xprev"],
                                        skip, p, seed)
    x.guard(label)
    out = x.read()
    check(sec, out, ref, bound, label)
    assert bool((out[~keep] == 0).all()), f"{label}: a dropped element is not 0"
    assert torch.equal(out != 0, keep & (ref != 0)), f"{label}: the kept set differs from the host mask"
    check_amax(am, prev, out, label)
    return out


@pytest.mark.parametrize("i", range(len(R.APPLY_CASES)), ids=[R.case_id(c) for c in R.APPLY_CASES])
def test_b_sage_apply(dev, i):
    (n, H), (aff, skip, p, seed, rev) = R.APPLY_CASES[i]
    _lib.call("bgnn_set_tuning", 13, (_defaults[13] & ~2) | (2 if rev else 0))
    label = f"bgnn_sage_apply N={n} H={H} scale/shift={'given' if aff else 'NULL'} skip={skip} p={p} seed={seed} " \
            f"rev={rev} grid form"
    d = R.layer_inputs(n, H)
    x, am = run_apply(dev, d, n, H, aff, skip, p, seed, amax_prev(i))
    check_apply("B sage_apply", d, n, H, aff, skip, p, seed, amax_prev(i), x, am, label)


def range_depth(rpb, a, e):
    """depth of the f32 summation tree behind one range sum: a wave's rows of the block, the 4 waves,
    the blocks a wave of the finish walks (every fourth), its 4 waves"""
    nb = (e - 1) // rpb - a // rpb + 1
    return -(-rpb // 4) + 3 + -(-nb // 4) + 3


def store_csr(dev, transposed):
    key = "store_t" if transposed else "store_f"
    ei, n, fwd, bwd, frp, _keep = graph_case("store", dev)
    if key not in _csrs:
        s = bwd if transposed else fwd
        c = Csr(s.rowptr, s.col, s.n_rows, s.nnz, s.plan, s.groups)
        c.ensure_ranges()
        _csrs[key] = c
    return n, _csrs[key], frp


@pytest.mark.parametrize("aff,p,seed", [(1, 0.1, 77), (0, 0.5, 2 ** 64 - 1)])
@pytest.mark.parametrize("H", R.APPLY_ROWS_H)
def test_b_sage_apply_rows_form(dev, H, aff, p, seed):
    """the row-blocked form (a ranges buffer): x_next bit for bit the grid form's, the range partials
    finished by bgnn_range_sums_finish mode 0 against the fp64 sums of the rows it wrote"""
    n, csr, _ = store_csr(dev, False)
    label = f"bgnn_sage_apply N={n} H={H} scale/shift={'given' if aff else 'NULL'} skip=1 p={p} seed={seed} rows form"
    d = R.layer_inputs(n, H)
    x0, am0 = run_apply(dev, d, n, H, aff, 1, p, seed, 0.0)
    out0 = check_apply("B sage_apply", d, n, H, aff, 1, p, seed, 0.0, x0, am0, label + " (grid)")
    nbytes = _lib.query("bgnn_range_partial_bytes", n, H)
    S = R.rows_slots(n)
    assert nbytes == S * 3 * H * 4
    rp = Out(dev, S, 3 * H, ld=3 * H)
    x1, am1 = run_apply(dev, d, n, H, aff, 1, p, seed, 0.0, csr.ranges, rp)
    rp.guard(label + " range partials")
    out1 = x1.read()
    x1.guard(label)
    assert torch.equal(out1.view(torch.int32), out0.view(torch.int32)), f"{label}: x_next differs from the grid form"
    assert am1.read().item() == am0.read().item()
    assert bool(torch.isfinite(rp.read()).all()), f"{label}: a range partial slot was not written"
    nh = csr.plan.n_heavy
    sums, aug = Out(dev, nh, H), scalar(dev, 0.0)
    _lib.call("bgnn_range_sums_finish", ptr(rp), n, H, csr.ref(), 0, ptr(sums), sums.ld, ptr(am1), ptr(aug), _stream())
    torch.cuda.synchronize()
    sums.guard(label + " range sums")
    got, rg = sums.read(), csr.ranges.cpu()
    assert int(rg[0]) == nh == 3
    for k in range(nh):
        a, e, h = rg[2 + 3 * k:5 + 3 * k].tolist()
        t = out1[a:e].to(D)
        s = t.sum(0)
        check("B range sums (mode 0)", got[h], s, R.tree_bound(range_depth(R.rows_rpb(n), a, e), t.abs().sum(0), s),
              f"{label} range row {h} = rows [{a}, {e})")
    assert aug.read().item() == max(am1.read().item(), got.abs().max().item())


# ============================================================================ C. bgnn_sage_bwd_stats
@pytest.mark.parametrize("i", range(len(R.STATS_CASES)), ids=[R.case_id(c) for c in R.STATS_CASES])
def test_c_sage_bwd_stats(dev, i):
    (n, H), (p, pooled, accumulate, null) = R.STATS_CASES[i]
    seed = R.SEEDS[i % 3]
    label = f"bgnn_sage_bwd_stats N={n} H={H} p={p} seed={seed} g_rows={'set' if pooled else 'NULL'}"
    d = R.layer_inputs(n, H, n_pool=3 if pooled else 0)
    S = _lib.query("bgnn_rows_slots", n)
    assert S == R.rows_slots(n)
    part = Out(dev, S, 2 * H, ld=2 * H)
    bufs = [inp(dev, d[k]) for k in ("g", "g_rows", "o", "scale", "shift", "mean", "invstd")]
    _lib.call("bgnn_sage_bwd_stats", *[ptr(t) for t in bufs], p, seed, n, H, ptr(part), _stream())
    torch.cuda.synchronize()
    P = slots_sum(part, S, H, label)
    assert bool(torch.isfinite(P).all()), f"{label}: a slot of the {S} was not written"
    rpb = R.rows_rpb(n)
    used = -(-n // rpb)
    assert bool((P[used:] == 0).all()), f"{label}: a block without rows wrote a non-zero slot"
    g2, g2x = R.bwd_stats_ref(d["g"], d["g_rows"], d["o"], d["scale"], d["shift"], d["mean"], d["invstd"], p, seed)
    for k, (t, nm) in enumerate(((g2, "sum g2"), (g2x, "sum g2 xhat"))):
        s, bound = R.colsum(t, rpb)
        check(f"C sage_bwd_stats {nm}", P[:, k].to(D).sum(0), s, bound, f"{label} {nm} (R = {rpb}, {S} slots)")
    reduce_check(dev, P, S, H, accumulate, null, label)


# ============================================================================ D. bgnn_sage_bwd_rows
def run_rows(dev, d, n, H, bn, gam, skip, p, seed, ldf, w_mode, prev, ranges=None, rw=None, rpart=None):
    args = R.rows_args(d, bn, gam)
    order = ("g", "g_rows", "o", "nrm", "scale", "shift", "gamma", "mean", "invstd", "sum_g2", "sum_g2xhat")
    bufs = [inp(dev, args[k]) for k in order]
    S = R.rows_slots(n)
    dh, gs = Out(dev, n, H, ld=ldf * H), (Out(dev, n, H, ld=H) if skip else None)
    part, am = Out(dev, S, 2 * H, ld=2 * H), scalar(dev, prev)
    wr = inp(dev, d["w_rowptr"]) if w_mode else None
    _lib.call("bgnn_sage_bwd_rows", *[ptr(t) for t in bufs], p, seed, skip, n, H, ptr(dh), ldf * H, ptr(gs), ptr(part),
              ptr(am), ptr(wr), w_mode, ptr(ranges), ptr(rw), ptr(rpart), _stream())
    torch.cuda.synchronize()
    return args, dh, gs, part, am


def check_rows(sec, dev, args, d, n, H, p, seed, skip, w_mode, prev, dh, gs, part, am, label, accumulate=0, null=None,
               relu=True):
    ref = R.bwd_rows_ref(args["g"], args["g_rows"], args["o"], args["nrm"], args["scale"], args["shift"], args["gamma"],
                         args["mean"], args["invstd"], args["sum_g2"], args["sum_g2xhat"], p, seed, relu=relu)
    dh.guard(label + " dh")
    out = dh.read()
    check(f"{sec} dh", out, ref["dh"], ref["bound"], label + " dh")
    if skip:
        gs.guard(label + " gskip")
        assert torch.equal(gs.read(), ref["gskip"]), f"{label}: gskip != dropout'(g) computed in f32"
    S, rpb = R.rows_slots(n), R.rows_rpb(n)
    P = slots_sum(part, S, H, label)
    assert bool(torch.isfinite(P).all()), f"{label}: a partial_db slot of the {S} was not written"
    assert bool((P[-(-n // rpb):] == 0).all()), f"{label}: a block without rows wrote a non-zero slot"
    s, bound = R.colsum(out, rpb)
    check(f"{sec} sum dh", P[:, 0].to(D).sum(0), s, bound, f"{label} column sums of dh (R = {rpb}, {S} slots)")
    if w_mode:
        s, bound = R.colsum(out, rpb, w=R.row_weights(d["w_rowptr"], w_mode))
        check(f"{sec} sum w dh", P[:, 1].to(D).sum(0), s, bound, f"{label} column sums of w_r dh_r, w_mode {w_mode}")
    else:
        assert bool((P[:, 1] == 0).all()), f"{label}: partial_db[.][1] must be 0 without row weights"
    check_amax(am, prev, out, label)
    reduce_check(dev, P, S, H, accumulate, null, label, "D reduce_partials")
    return out


@pytest.mark.parametrize("i", range(len(R.ROWS_CASES)), ids=[R.case_id(c) for c in R.ROWS_CASES])
def test_d_sage_bwd_rows(dev, i):
    (n, H), (bn, gam, skip, p, pooled, ldf, w_mode, rev) = R.ROWS_CASES[i]
    seed = R.SEEDS[i % 3]
    _lib.call("bgnn_set_tuning", 13, (_defaults[13] & ~1) | rev)
    label = f"bgnn_sage_bwd_rows N={n} H={H} NV={2 if H > 256 else 1} bn={bn} gamma={'given' if gam else 'NULL'} " \
            f"skip={skip} p={p} seed={seed} g_rows={'set' if pooled else 'NULL'} lddh={ldf * H} w_mode={w_mode} rev={rev}"
    d = R.layer_inputs(n, H, n_pool=3 if pooled else 0)
    res = run_rows(dev, d, n, H, bn, gam, skip, p, seed, ldf, w_mode, amax_prev(i))
    check_rows("D sage_bwd_rows", dev, res[0], d, n, H, p, seed, skip, w_mode, amax_prev(i), *res[1:], label,
               accumulate=i % 2, null=(None, 0, 1)[i % 3])


@pytest.mark.parametrize("bn", ["train", "off"])
@pytest.mark.parametrize("H", [100, 260])
def test_d_zero_norm_rows(dev, H, bn):
    """three rows with o = 0, nrm = 0: dh = d * 1e12 (F.normalize's clamped denominator), amax accordingly"""
    n = 67
    _lib.call("bgnn_set_tuning", 13, _defaults[13] | 1)
    label = f"bgnn_sage_bwd_rows N={n} H={H} bn={bn} zero-norm rows"
    d = R.layer_inputs(n, H, zero_norm=True)
    res = run_rows(dev, d, n, H, bn, 1, 1, 0.25, 77, 1, 1, 0.0)
    out = check_rows("D zero-norm rows", dev, res[0], d, n, H, 0.25, 77, 1, 1, 0.0, *res[1:], label)
    assert out[0].abs().max().item() > 1e9 and res[4].read().item() == out.abs().max().item()


@pytest.mark.parametrize("mean_w", [0, 1])
@pytest.mark.parametrize("H", [100, 260, 512])
def test_d_sage_bwd_rows_ranges(dev, H, mean_w):
    """the transpose CSR's ranges: range partials of rw dh (rw = 1, or 1 / max(deg, 1) from the forward
    rowptr), finished by bgnn_range_sums_finish mode 1 into the super nodes' rows"""
    n, csr, frp = store_csr(dev, True)
    label = f"bgnn_sage_bwd_rows N={n} H={H} bn=train skip=1 p=0.25 ranges, range_w_rowptr={'set' if mean_w else 'NULL'}"
    d = R.layer_inputs(n, H)
    S = R.rows_slots(n)
    rp = Out(dev, S, 3 * H, ld=3 * H)
    res = run_rows(dev, d, n, H, "train", 1, 1, 0.25, 77, 1, 2, 0.0, csr.ranges, frp if mean_w else None, rp)
    out = check_rows("D sage_bwd_rows", dev, res[0], d, n, H, 0.25, 77, 1, 2, 0.0, *res[1:], label)
    rp.guard(label + " range partials")
    assert bool(torch.isfinite(rp.read()).all()), f"{label}: a range partial slot was not written"
    dz, aug = Out(dev, n, H, ld=H), scalar(dev, 0.0)
    _lib.call("bgnn_range_sums_finish", ptr(rp), n, H, csr.ref(), 1, ptr(dz), H, None, ptr(aug), _stream())
    torch.cuda.synchronize()
    dz.guard(label + " range sums")
    got, rg = dz.read(), csr.ranges.cpu()
    nh = csr.plan.n_heavy
    heavy = csr.plan.heavy_row[:nh].cpu().tolist()
    deg = (frp[1:] - frp[:-1]).cpu().clamp_min(1).to(D)
    written = torch.zeros(n, dtype=torch.bool)
    assert int(rg[0]) == nh == 3
    for k in range(nh):
        a, e, h = rg[2 + 3 * k:5 + 3 * k].tolist()
        t = out[a:e].to(D) * ((1.0 / deg[a:e]).unsqueeze(1) if mean_w else 1.0)
        s = t.sum(0)
        check("D range sums (mode 1)", got[heavy[h]], s, R.tree_bound(range_depth(R.rows_rpb(n), a, e), t.abs().sum(0), s),
              f"{label} range row {heavy[h]} = rows [{a}, {e})")
        written[heavy[h]] = True
    assert bool(torch.isnan(got[~written]).all()), f"{label}: the finish wrote a row that is no range row"
    assert aug.read().item() == got[written].abs().max().item()


# ============================================================================ E. bgnn_l2norm_bwd
def run_l2(dev, d, n, H, ldf, prev):
    bufs = [inp(dev, d[k]) for k in ("g", "o", "nrm")]
    S = R.rows_slots(n)
    dh, part, am = Out(dev, n, H, ld=ldf * H), Out(dev, S, 2 * H, ld=2 * H), scalar(dev, prev)
    _lib.call("bgnn_l2norm_bwd", *[ptr(t) for t in bufs], n, H, ptr(dh), ldf * H, ptr(part), ptr(am), _stream())
    torch.cuda.synchronize()
    args = R.l2_args(d)
    return args, dh, None, part, am


@pytest.mark.parametrize("i", range(len(R.L2_CASES)), ids=[R.case_id(c) for c in R.L2_CASES])
def test_e_l2norm_bwd(dev, i):
    (n, H), (ldf, rev) = R.L2_CASES[i]
    _lib.call("bgnn_set_tuning", 13, (_defaults[13] & ~1) | rev)
    label = f"bgnn_l2norm_bwd N={n} H={H} NV={2 if H > 256 else 1} lddh={ldf * H} rev={rev}"
    d = R.layer_inputs(n, H)
    res = run_l2(dev, d, n, H, ldf, amax_prev(i))
    check_rows("E l2norm_bwd", dev, res[0], d, n, H, 0.0, 0, 0, 0, amax_prev(i), *res[1:], label, relu=False)


def test_e_zero_norm_rows(dev):
    n, H = 67, 260
    label = f"bgnn_l2norm_bwd N={n} H={H} zero-norm rows"
    d = R.layer_inputs(n, H, zero_norm=True)
    res = run_l2(dev, d, n, H, 1, 0.0)
    out = check_rows("E zero-norm rows", dev, res[0], d, n, H, 0.0, 0, 0, 0, 0.0, *res[1:], label, relu=False)
    assert out[0].abs().max().item() > 1e9


# ============================================================================ F. the reductions on synthetic partials
@pytest.mark.parametrize("i", range(len(R.FIN_CASES)), ids=[R.case_id(c) for c in R.FIN_CASES])
def test_f_bn_finalize(dev, i):
    (S, H), (one, aff, mom, running) = R.FIN_CASES[i]
    count = R.fin_count(S, one)
    eps = 1e-5
    label = f"S={S} H={H} count={count} gamma/beta={'given' if aff else 'NULL'} momentum={mom} " \
            f"running={'given' if running else 'NULL'}"
    P = R.partials(S, H, count)
    gamma, beta, rm, rv, ks = R.fin_inputs(S, H, aff)
    gb, bb = inp(dev, gamma), inp(dev, beta)
    for name, kshift in (("bgnn_bn_finalize", None), ("bgnn_bn_finalize_shifted", ks)):
        pbuf = inp(dev, P.reshape(S, 2 * H))
        outs = {k: Out(dev, 1, H) for k in ("mean", "invstd", "scale", "shift")}
        run = {k: Out(dev, 1, H, init=v) for k, v in (("rmean", rm), ("rvar", rv))} if running else {}
        kb = inp(dev, kshift)
        head = (ptr(pbuf), S, H, count) + ((ptr(kb),) if kshift is not None else ())
        _lib.call(name, *head, ptr(gb), ptr(bb), eps, mom, ptr(run.get("rmean")), ptr(run.get("rvar")),
                  *[ptr(outs[k]) for k in ("mean", "invstd", "scale", "shift")], _stream())
        torch.cuda.synchronize()
        ref = R.bn_finalize_ref(P, count, gamma, beta, eps, mom, rm if running else None, rv if running else None, kshift)
        assert bool((ref["var"] >= 1e-3 * P[:, 1].to(D).sum(0) / count).all())   # the input condition
        for k, w in outs.items():
            w.guard(f"{name} {label} {k}")
            check(f"F {name[5:]}", w.read().view(H), *ref[k], f"{name} {label} {k}")
        for k, w in run.items():
            w.guard(f"{name} {label} {k}")
            if mom == 0.0:   # the running statistics keep their bits
                assert torch.equal(w.read().view(H).view(torch.int32), (rm if k == "rmean" else rv).view(torch.int32))
            else:
                check(f"F {name[5:]}", w.read().view(H), *ref[k], f"{name} {label} {k}")
    # eval coefficients from the running statistics
    sc, sh = Out(dev, 1, H), Out(dev, 1, H)
    rmb, rvb = inp(dev, rm), inp(dev, rv)
    _lib.call("bgnn_bn_eval_coeffs", H, ptr(gb), ptr(bb), eps, ptr(rmb), ptr(rvb), ptr(sc), ptr(sh), _stream())
    torch.cuda.synchronize()
    ref = R.bn_eval_ref(gamma, beta, eps, rm, rv)
    for w, k in ((sc, "scale"), (sh, "shift")):
        w.guard(f"bgnn_bn_eval_coeffs {label} {k}")
        check("F bn_eval_coeffs", w.read().view(H), *ref[k], f"bgnn_bn_eval_coeffs {label} {k}")
    reduce_check(dev, P, S, H, i % 2, (None, 0, 1)[i % 3], f"synthetic partials {label}", "F reduce_partials")


# ============================================================================ G. bgnn_linear_bwd_prep
@pytest.mark.parametrize("i", range(len(R.PREP_CASES)), ids=[R.case_id(c) for c in R.PREP_CASES])
def test_g_linear_bwd_prep(dev, i):
    (n, C), (has_y, has_out) = R.PREP_CASES[i]
    label = f"bgnn_linear_bwd_prep N={n} C={C} y={'given' if has_y else 'NULL'} g_out={'given' if has_out else 'NULL'}"
    g, y = R.prep_inputs(n, C)
    S = _lib.query("bgnn_linear_bwd_prep_slots")
    assert S == R.PREP_SLOTS
    gb, yb = inp(dev, g), inp(dev, y) if has_y else None
    go = Out(dev, n, C, ld=C) if has_out else None
    part, am = Out(dev, S, 2 * C, ld=2 * C), scalar(dev, amax_prev(i))
    _lib.call("bgnn_linear_bwd_prep", ptr(gb), ptr(yb), n, C, ptr(go), ptr(part), ptr(am), _stream())
    torch.cuda.synchronize()
    want = R.prep_ref(g, y if has_y else None)
    if has_out:
        go.guard(label)
        assert torch.equal(go.read().view(torch.int32), want.view(torch.int32)), f"{label}: g_out != the masked g"
    P = slots_sum(part, S, C, label)
    assert bool(torch.isfinite(P[:, 0]).all()), f"{label}: a slot was not written"
    assert bool(torch.isnan(P[:, 1]).all()), f"{label}: the second half of a slot is not this kernel's to write"
    Rr = R.prep_rows_per_slot(n, C)
    s, bound = R.colsum(want, Rr)
    check("G linear_bwd_prep sums", P[:, 0].to(D).sum(0), s, bound, f"{label} column sums (R = {Rr})")
    check_amax(am, amax_prev(i), want, label)
    pbuf = inp(dev, P.reshape(S, 2 * C))
    out0 = Out(dev, 1, C)
    _lib.call("bgnn_reduce_partials", ptr(pbuf), S, C, ptr(out0), None, 0, _stream())
    torch.cuda.synchronize()
    out0.guard(label)
    check("G reduce_partials", out0.read().view(C), *R.reduce_partials_ref(P, 0), f"{label} reduce_partials")


# ============================================================================ H. one mask, every consumer
@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n,H", [(67, 100), (5, 512)])
def test_h_one_mask_every_consumer(dev, n, H, p, seed):
    label = f"N={n} H={H} p={p} seed={seed}"
    keep = R.keep_mask(seed, n, H, p)
    assert 0 < int(keep.sum()) < n * H
    d = R.layer_inputs(n, H)
    d["xprev"] = d["xprev"].abs() + 1.0              # relu(.) + x_prev > 0: every kept element is non-zero
    x, _am = run_apply(dev, d, n, H, 1, 1, p, seed, 0.0)
    assert torch.equal(x.read() != 0, keep), f"bgnn_sage_apply {label}: kept set differs from the host mask"
    d["g"] = torch.ones(n, H)
    _args, _dh, gs, _part, _am = run_rows(dev, d, n, H, "train", 1, 1, p, seed, 1, 0, 0.0)
    gsk = gs.read()
    assert torch.equal(gsk != 0, keep), f"bgnn_sage_bwd_rows {label}: non-zero set of gskip differs from the host mask"
    assert bool((gsk[keep] == float(R.inv_keep(p))).all())
    a, out = inp(dev, torch.ones(n, H)), Out(dev, 1, n * H)
    _lib.call("bgnn_add_dropout", ptr(a), None, n * H, p, seed, ptr(out), _stream())
    torch.cuda.synchronize()
    out.guard(f"bgnn_add_dropout {label}")
    assert torch.equal(out.read().view(n, H) != 0, keep), f"bgnn_add_dropout {label}: kept set differs from the host mask"
