"""GPU: fp64 conformance matrix of the LDS-resident VALU kernels at the two ends of every model and
of the per-module BatchNorm -- csrc/mlp.hip (bgnn_mlp2_fwd / _bwd, bgnn_small_linear_fwd / _bwd,
bgnn_linear_bwd_prep_bf16), csrc/head.hip (bgnn_head2_fwd / _bwd) and csrc/bn.hip (bgnn_bn_stats /
_apply / _bwd_stats / _bwd_dx) -- each on its raw entry point (_lib.call), at the smallest shapes that
reach every branch: ragged and full tiles, a workgroup's second tile, 17 slots (sum groups of 2
followed by empty groups), NULL biases and optional outputs, W2 off a 16-byte boundary, partly idle
lanes (K / 4 below and off a multiple of 64), a partly filled last block, every C of the head's
cg / cg + 4 split, BatchNorm's capped grid and the grid-stride pass of its row kernels, N = 0.

References, bounds, inputs and case lists are tests/dense_rows_ref.py's (fp64 evaluations of the
header's formulas; bounds from the operation counts, u = 2^-24, none measured; no element is left out
of a comparison: the ReLU masks are exact by construction of the inputs, with exact-zero
pre-activations under non-zero gradients). Every output is a window pre-filled with NaN inside a
larger allocation whose guards hold a fixed bit pattern that must survive the call; workspaces and
partial buffers start as NaN inside guards, sized exactly to the *_ws_bytes / *_slots answer; float
inputs carry NaN after their last row. Each section prints its largest err / bound ratio.

Sections: A mlp2_fwd, B mlp2_bwd, C small_linear, D head2, E linear_bwd_prep_bf16, F bn."""
import pytest
import torch

import dense_rows_ref as R
from bgnn import _lib
from bgnn.graph import _stream
from matrix_util import RATIOS, In, Out, OutB16, amax_prev, check, check_amax, inp, inp16, ptr, scalar

pytestmark = pytest.mark.gpu

D = torch.float64
F, D1, D2 = R.MLP_F, R.MLP_D1, R.MLP_D2


@pytest.fixture(autouse=True)
def _sticky_fault_ends_the_session():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault is sticky: nothing more of this session runs on the GPU
        pytest.exit(f"GPU fault in the dense-kernel matrix, session ended: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\nsection: largest err / bound")
    for k in sorted(RATIOS):
        if k[:2] in ("A ", "B ", "C ", "D ", "E ", "F "):
            print(f"  {k}: {RATIOS[k]:.3f}")


def geometry():
    return tuple(_lib.query("bgnn_head2_geometry", i) for i in range(3))


def flat(dev, n):
    """a contiguous output of n floats as a one-row window"""
    return Out(dev, 1, n)


def sync():
    torch.cuda.synchronize()


def slots_of(ws, slots, L, Lp, label):
    """the per-workgroup partials [slots, L] of a workspace window of (slots + 16) slots of stride Lp: every
    slot and every group sum written (the Lp - L padding floats of a slot may hold anything)"""
    ws.guard(label + " workspace")
    w = ws.read().view(slots + R.SUM_GROUPS, Lp)[:, :L]
    assert bool(torch.isfinite(w[:slots]).all()), f"{label}: a partial slot of the {slots} was not fully written"
    assert bool(torch.isfinite(w[slots:]).all()), f"{label}: a group sum of the {R.SUM_GROUPS} was not written"
    return w[:slots]


# ============================================================================ A. bgnn_mlp2_fwd
def enc(N, grid):
    return R.two_layer_inputs(N, F, D1, D2, grid)


@pytest.mark.parametrize("i", range(len(R.MLP_FWD_CASES)), ids=[R.case_id(c) for c in R.MLP_FWD_CASES])
def test_a_mlp2_fwd(dev, i):
    N, (nullb, w2off, am_mode, grid) = R.MLP_FWD_CASES[i]
    label = f"bgnn_mlp2_fwd N={N} b1={'NULL' if nullb & 1 else 'given'} b2={'NULL' if nullb & 2 else 'given'} " \
            f"W2 {'4 bytes off' if w2off else 'on'} a 16-byte boundary " \
            f"amax={('NULL', 'previous 0', 'previous 3e30')[am_mode]} " \
            f"{'dyadic' if grid else 'randn'} inputs"
    d = enc(N, grid)
    b1, b2 = (None if nullb & 1 else d["b1"]), (None if nullb & 2 else d["b2"])
    xb, W1b, b1b, b2b = inp(dev, d["x"]), inp(dev, d["W1"]), inp(dev, b1), inp(dev, b2)
    W2b = In(dev, d["W2"], ld=D1, lead=w2off)
    assert W2b.ptr % 16 == (4 if w2off else 0)
    h = flat(dev, N * D2)
    prev = (None, 0.0, 3.0e30)[am_mode]
    am = scalar(dev, prev) if prev is not None else None
    _lib.call("bgnn_mlp2_fwd", ptr(xb), N, F, D1, D2, ptr(W1b), ptr(b1b), ptr(W2b), ptr(b2b), ptr(h), ptr(am), _stream())
    sync()
    h.guard(label)
    out = h.read().view(N, D2)
    ref, bound = R.mlp2_fwd_ref(d["x"], d["W1"], b1, d["W2"], b2)
    check("A mlp2_fwd h", out, ref, bound, label)
    assert bool((out >= 0).all())
    if am is not None:
        check_amax(am, prev, out, label)
        assert am.read().item() == R.amax_ref(prev, out)


def test_a_mlp2_fwd_no_rows(dev):
    h, am = flat(dev, D2), scalar(dev, 1.5)
    W = inp(dev, torch.zeros(D2, D1))
    assert _lib.call("bgnn_mlp2_fwd", None, 0, F, D1, D2, None, None, None, None, None, None, _stream()) == 0
    assert _lib.call("bgnn_mlp2_fwd", ptr(W), 0, F, D1, D2, ptr(W), None, ptr(W), None, ptr(h), ptr(am), _stream()) == 0
    sync()
    h.guard("bgnn_mlp2_fwd N=0")
    assert bool(torch.isnan(h.read()).all()) and am.read().item() == 1.5, "bgnn_mlp2_fwd N=0 wrote"


# ============================================================================ B. bgnn_mlp2_bwd
MLP_L = D2 * D1 + D2 + D1 * F + D1   # a slot: [dW2 | db2 | dW1 | db1]
MLP_OUTS = (("dW1", (D1, F)), ("db1", (D1,)), ("dW2", (D2, D1)), ("db2", (D2,)))


def run_mlp2_bwd(dev, d, N, b1, label):
    bufs = [inp(dev, d["x"]), inp(dev, d["W1"]), inp(dev, b1), inp(dev, d["W2"]), inp(dev, d["h"]), inp(dev, d["g"])]
    slots, _ = R.tile_partition(N, R.KT, R.MLP_BLOCKS)
    nbytes = _lib.query("bgnn_mlp2_bwd_ws_bytes", N)
    assert nbytes == (slots + R.SUM_GROUPS) * MLP_L * 4, f"{label}: workspace of {nbytes} bytes"
    ws = flat(dev, nbytes // 4)
    outs = {k: flat(dev, int(torch.Size(s).numel())) for k, s in MLP_OUTS}
    x, W1, b1b, W2, h, dh = bufs
    _lib.call("bgnn_mlp2_bwd", ptr(x), N, F, D1, D2, ptr(W1), ptr(b1b), ptr(W2), ptr(h), ptr(dh),
              *[ptr(outs[k]) for k, _ in MLP_OUTS], ptr(ws), nbytes, _stream())
    sync()
    for k, w in outs.items():
        w.guard(f"{label} {k}")
    part = slots_of(ws, slots, MLP_L, MLP_L, label)
    return {k: outs[k].read().view(s) for k, s in MLP_OUTS}, part


@pytest.mark.parametrize("N,nb1", R.MLP_BWD_CASES, ids=[R.case_id(c) for c in R.MLP_BWD_CASES])
def test_b_mlp2_bwd(dev, N, nb1):
    slots, Rr = R.tile_partition(N, R.KT, R.MLP_BLOCKS)
    label = f"bgnn_mlp2_bwd N={N} b1={'NULL' if nb1 else 'given'} dyadic hidden layer, host-made h " \
            f"({slots} slots of <= {Rr} rows)"
    d = enc(N, 1)
    b1 = None if nb1 else d["b1"]
    got, part = run_mlp2_bwd(dev, d, N, b1, label)
    ref = R.mlp2_bwd_ref(d["x"], d["W1"], b1, d["W2"], d["h"], d["g"])
    for k, _ in MLP_OUTS:
        check(f"B mlp2_bwd {k}", got[k], ref[k][0], ref[k][1], f"{label} {k}")
    again, part2 = run_mlp2_bwd(dev, d, N, b1, label)
    for k, _ in MLP_OUTS:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{label}: {k} differs between two runs"
    assert torch.equal(part.view(torch.int32), part2.view(torch.int32)), f"{label}: the partials differ between two runs"


def test_b_mlp2_bwd_no_rows(dev):
    outs = {k: flat(dev, int(torch.Size(s).numel())) for k, s in MLP_OUTS}
    _lib.call("bgnn_mlp2_bwd", None, 0, F, D1, D2, None, None, None, None, None, *[ptr(outs[k]) for k, _ in MLP_OUTS],
              None, 0, _stream())
    sync()
    for k, w in outs.items():
        w.guard(f"bgnn_mlp2_bwd N=0 {k}")
        assert bool((w.read() == 0).all()), f"bgnn_mlp2_bwd N=0: {k} is not zero-filled"


# ============================================================================ C. bgnn_small_linear_fwd / _bwd
@pytest.mark.parametrize("i", range(len(R.SL_FWD_CASES)), ids=[R.case_id(c) for c in R.SL_FWD_CASES])
def test_c_small_linear_fwd(dev, i):
    (B, K, N), (relu, nobias) = R.SL_FWD_CASES[i]
    label = f"bgnn_small_linear_fwd B={B} K={K} N={N} relu={relu} bias={'NULL' if nobias else 'given'} " \
            f"({K // 4} float4 per row, {B * N % 4 or 4} of 4 waves in the last block)"
    d = R.small_linear_inputs(B, K, N)
    bias = None if nobias else d["bias"]
    xb, Wb, bb = inp(dev, d["x"]), inp(dev, d["W"]), inp(dev, bias)
    y = flat(dev, B * N)
    _lib.call("bgnn_small_linear_fwd", ptr(xb), B, K, ptr(Wb), ptr(bb), N, relu, ptr(y), _stream())
    sync()
    y.guard(label)
    ref, bound = R.small_linear_fwd_ref(d["x"], d["W"], bias, relu)
    check("C small_linear_fwd", y.read().view(B, N), ref, bound, label)


@pytest.mark.parametrize("i", range(len(R.SL_BWD_CASES)), ids=[R.case_id(c) for c in R.SL_BWD_CASES])
def test_c_small_linear_bwd(dev, i):
    (B, K, N), (noy, nodb, nodx) = R.SL_BWD_CASES[i]
    label = f"bgnn_small_linear_bwd B={B} K={K} N={N} y={'NULL' if noy else 'host-made'} db={'NULL' if nodb else 'given'} " \
            f"dx={'NULL' if nodx else 'given'}"
    d = R.small_linear_inputs(B, K, N)
    y = None if noy else d["y"]
    gb, yb, xb, Wb = inp(dev, d["gy"]), inp(dev, y), inp(dev, d["x"]), inp(dev, d["W"])
    dx, dW, db = (None if nodx else flat(dev, B * K)), flat(dev, N * K), (None if nodb else flat(dev, N))
    _lib.call("bgnn_small_linear_bwd", ptr(gb), ptr(yb), ptr(xb), B, K, ptr(Wb), N, ptr(dx), ptr(dW), ptr(db), _stream())
    sync()
    ref = R.small_linear_bwd_ref(d["gy"], y, d["x"], d["W"])
    for w, k, shape in ((dW, "dW", (N, K)), (db, "db", (N,)), (dx, "dx", (B, K))):
        if w is not None:
            w.guard(f"{label} {k}")
            check(f"C small_linear_bwd {k}", w.read().view(shape), ref[k][0], ref[k][1], f"{label} {k}")


@pytest.mark.parametrize("K,N", [(4, 1), (260, 65)])
def test_c_small_linear_bwd_no_rows(dev, K, N):
    """B = 0: dW and db are zeros, dx is untouched"""
    label = f"bgnn_small_linear_bwd B=0 K={K} N={N}"
    some = inp(dev, torch.zeros(4, K))
    Wb = inp(dev, torch.ones(N, K))
    dx, dW, db = flat(dev, K), flat(dev, N * K), flat(dev, N)
    _lib.call("bgnn_small_linear_bwd", ptr(some), ptr(some), ptr(some), 0, K, ptr(Wb), N, ptr(dx), ptr(dW), ptr(db),
              _stream())
    sync()
    for w, k in ((dx, "dx"), (dW, "dW"), (db, "db")):
        w.guard(f"{label} {k}")
    assert bool((dW.read() == 0).all()) and bool((db.read() == 0).all()), f"{label}: dW / db not zero"
    assert bool(torch.isnan(dx.read()).all()), f"{label}: dx was written"


# ============================================================================ D. bgnn_head2_fwd / _bwd
def head_case(i, which):
    T, fwd, bwd = geometry()
    (D0, C), ni, (nb1, nb2) = R.HEAD_CASES[i]
    N = R.head_ns(T, (fwd, bwd)[which])[ni]
    return T, bwd, D0, C, N, nb1, nb2


@pytest.mark.parametrize("i", range(len(R.HEAD_CASES)), ids=[R.case_id(c) for c in R.HEAD_CASES])
def test_d_head2_fwd(dev, i):
    T, bwd, D0, C, N, nb1, nb2 = head_case(i, 0)
    grid = i % 2
    label = f"bgnn_head2_fwd D0={D0} C={C} N={N} b1={'NULL' if nb1 else 'given'} b2={'NULL' if nb2 else 'given'} " \
            f"{'dyadic' if grid else 'randn'} inputs"
    d = R.two_layer_inputs(N, D0, R.HEAD_D1, C, grid, T=T, cap=bwd)
    b1, b2 = (None if nb1 else d["b1"]), (None if nb2 else d["b2"])
    bufs = [inp(dev, t) for t in (d["x"], d["W1"], b1, d["W2"], b2)]
    y = flat(dev, N * C)
    _lib.call("bgnn_head2_fwd", ptr(bufs[0]), N, D0, R.HEAD_D1, C, *[ptr(t) for t in bufs[1:]], ptr(y), _stream())
    sync()
    y.guard(label)
    ref, bound = R.head2_fwd_ref(d["x"], d["W1"], b1, d["W2"], b2)
    check("D head2_fwd y", y.read().view(N, C), ref, bound, label)


@pytest.mark.parametrize("i", range(len(R.HEAD_CASES)), ids=[R.case_id(c) for c in R.HEAD_CASES])
def test_d_head2_bwd(dev, i):
    T, bwd, D0, C, N, nb1, _ = head_case(i, 1)
    slots, Rr = R.tile_partition(N, T, bwd)
    label = f"bgnn_head2_bwd D0={D0} C={C} N={N} b1={'NULL' if nb1 else 'given'} dyadic hidden layer " \
            f"({slots} slots of <= {Rr} rows)"
    d = R.two_layer_inputs(N, D0, R.HEAD_D1, C, 1, T=T, cap=bwd)
    b1 = None if nb1 else d["b1"]
    shapes = (("dW1", (R.HEAD_D1, D0)), ("db1", (R.HEAD_D1,)), ("dW2", (C, R.HEAD_D1)), ("db2", (C,)))
    L = sum(int(torch.Size(s).numel()) for _, s in shapes)
    Lp = (L + 3) // 4 * 4
    nbytes = _lib.query("bgnn_head2_bwd_ws_bytes", N, D0, C)
    assert nbytes == (slots + R.SUM_GROUPS) * Lp * 4, f"{label}: workspace of {nbytes} bytes"

    def run():
        bufs = [inp(dev, t) for t in (d["x"], d["W1"], b1, d["W2"], d["g"])]
        ws, dx = flat(dev, nbytes // 4), flat(dev, N * D0)
        outs = {k: flat(dev, int(torch.Size(s).numel())) for k, s in shapes}
        _lib.call("bgnn_head2_bwd", ptr(bufs[0]), N, D0, R.HEAD_D1, C, *[ptr(t) for t in bufs[1:]], ptr(dx),
                  *[ptr(outs[k]) for k, _ in shapes], ptr(ws), nbytes, _stream())
        sync()
        dx.guard(f"{label} dx (rows past N)")
        for k, w in outs.items():
            w.guard(f"{label} {k}")
        slots_of(ws, slots, L, Lp, label)
        got = {k: outs[k].read().view(s) for k, s in shapes}
        got["dx"] = dx.read().view(N, D0)
        return got

    got = run()
    ref = R.head2_bwd_ref(d["x"], d["W1"], b1, d["W2"], d["g"], T, bwd)
    for k in ("dx", "dW1", "db1", "dW2", "db2"):
        check(f"D head2_bwd {k}", got[k], ref[k][0], ref[k][1], f"{label} {k}")
    again = run()
    for k in got:
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{label}: {k} differs between two runs"


def test_d_head2_no_rows(dev):
    D0, C = 64, 5
    shapes = (R.HEAD_D1 * D0, R.HEAD_D1, C * R.HEAD_D1, C)
    outs = [flat(dev, n) for n in shapes]
    y = flat(dev, C)
    assert _lib.call("bgnn_head2_fwd", None, 0, D0, R.HEAD_D1, C, None, None, None, None, ptr(y), _stream()) == 0
    _lib.call("bgnn_head2_bwd", None, 0, D0, R.HEAD_D1, C, None, None, None, None, None, *[ptr(w) for w in outs], None, 0,
              _stream())
    sync()
    y.guard("bgnn_head2_fwd N=0")
    assert bool(torch.isnan(y.read()).all())
    for w in outs:
        w.guard("bgnn_head2_bwd N=0")
        assert bool((w.read() == 0).all()), "bgnn_head2_bwd N=0: a gradient is not zero-filled"


# ============================================================================ E. bgnn_linear_bwd_prep_bf16
@pytest.mark.parametrize("i", range(len(R.PREP16_CASES)), ids=[R.case_id(c) for c in R.PREP16_CASES])
def test_e_linear_bwd_prep_bf16(dev, i):
    (n, C), has_y = R.PREP16_CASES[i]
    label = f"bgnn_linear_bwd_prep_bf16 N={n} C={C} " + ("y host-made" if has_y else "bias only (y, g_out NULL)")
    g, y = R.prep_bf16_inputs(n, C)
    S = _lib.query("bgnn_linear_bwd_prep_slots")
    assert S == R.PREP_BLOCKS
    gb, yb = inp16(dev, g), (inp16(dev, y) if has_y else None)
    go = OutB16(dev, n * C) if has_y else None
    part = Out(dev, S, 2 * C, ld=2 * C)
    _lib.call("bgnn_linear_bwd_prep_bf16", ptr(gb), ptr(yb), n, C, ptr(go), ptr(part), _stream())
    sync()
    want, s, bound = R.prep_bf16_ref(g, y if has_y else None)
    if has_y:
        go.guard(label)
        assert torch.equal(go.read().view(torch.int16), want.reshape(-1).view(torch.int16)), \
            f"{label}: g_out != the masked g"
    part.guard(label + " partials")
    P = part.read().view(S, 2, C)
    assert bool(torch.isfinite(P[:, 0]).all()), f"{label}: a slot of the {S} was not written"
    assert bool(torch.isnan(P[:, 1]).all()), f"{label}: the second half of a slot is not this kernel's to write"
    check("E linear_bwd_prep_bf16 sums", P[:, 0].to(D).sum(0), s, bound,
          f"{label} column sums (R = {R.prep_bf16_rows_per_slot(n, C)})")


# ============================================================================ F. csrc/bn.hip
def bn_partials(dev, name, args, slots, C, label):
    part = Out(dev, slots, 2 * C, ld=2 * C)
    _lib.call(name, *args, ptr(part), _stream())
    sync()
    part.guard(label + " partials")
    P = part.read().view(slots, 2, C)
    assert bool(torch.isfinite(P).all()), f"{label}: a slot of the {slots} was not written"
    return P.to(D).sum(0)


def bn_rows_kernels(dev, d, n, C, gnull, label):
    """bgnn_bn_apply and bgnn_bn_bwd_dx, per element"""
    xb, gb = inp(dev, d["x"]), inp(dev, d["g"])
    sc, sh, mean, invstd, sums = (inp(dev, d[k]) for k in ("scale", "shift", "mean", "invstd", "sums"))
    gamma = None if gnull else d["gamma"]
    gmb = inp(dev, gamma)
    y = flat(dev, n * C)
    _lib.call("bgnn_bn_apply", ptr(xb), n, C, ptr(sc), ptr(sh), ptr(y), _stream())
    sync()
    y.guard(label + " bn_apply")
    check("F bn_apply", y.read().view(n, C), *R.bn_apply_ref(d["x"], d["scale"], d["shift"]), f"bgnn_bn_apply {label}")
    del y
    dx = flat(dev, n * C)
    _lib.call("bgnn_bn_bwd_dx", ptr(gb), ptr(xb), ptr(mean), ptr(invstd), ptr(gmb), ptr(sums), n, C, ptr(dx), _stream())
    sync()
    dx.guard(label + " bn_bwd_dx")
    check("F bn_bwd_dx", dx.read().view(n, C), *R.bn_bwd_dx_ref(d["g"], d["x"], d["mean"], d["invstd"], gamma, d["sums"]),
          f"bgnn_bn_bwd_dx {label} gamma={'NULL' if gnull else 'given'}")


@pytest.mark.parametrize("i", range(len(R.BN_CASES)), ids=[R.case_id(c) for c in R.BN_CASES])
def test_f_bn(dev, i):
    (C, n), kind, gnull = R.BN_CASES[i]
    slots, rpb, rpi = R.bn_slots(n, C)
    label = f"C={C} n_rows={n} x={'randn * 0.3 + 0.05' if kind == 0 else '1e3 + randn'} ({slots} slots of <= {rpb} rows, " \
            f"{rpi} rows per block step)"
    assert _lib.query("bgnn_bn_slots", n, C) == slots, label
    d = R.bn_inputs(n, C, kind)
    xb, gb, mean, invstd = inp(dev, d["x"]), inp(dev, d["g"]), inp(dev, d["mean"]), inp(dev, d["invstd"])
    S = bn_partials(dev, "bgnn_bn_stats", (ptr(xb), n, C), slots, C, f"bgnn_bn_stats {label}")
    for k, (s, bound), nm in zip((0, 1), R.bn_stats_ref(d["x"]), ("sum x - k", "sum (x - k)^2")):
        check(f"F bn_stats {nm}", S[k], s, bound, f"bgnn_bn_stats {label} {nm}")
    S = bn_partials(dev, "bgnn_bn_bwd_stats", (ptr(gb), ptr(xb), ptr(mean), ptr(invstd), n, C), slots, C,
                    f"bgnn_bn_bwd_stats {label}")
    refs = R.bn_bwd_stats_ref(d["g"], d["x"], d["mean"], d["invstd"])
    for k, (s, bound), nm in zip((0, 1), refs, ("sum g", "sum g xhat")):
        check(f"F bn_bwd_stats {nm}", S[k], s, bound, f"bgnn_bn_bwd_stats {label} {nm}")
    bn_rows_kernels(dev, d, n, C, gnull, label)


def test_f_bn_rows_grid_stride(dev):
    """more than 8192 * 256 float4: the grid-stride second pass of bgnn_bn_apply / bgnn_bn_bwd_dx"""
    C, n = R.BN_STRIDE_CASE
    assert n * C // 4 > R.BN_ROWS_BLOCKS * 256
    bn_rows_kernels(dev, R.bn_inputs(n, C, 0), n, C, 0, f"C={C} n_rows={n} (grid-stride)")


@pytest.mark.parametrize("C", [4, 1024])
def test_f_bn_bwd_stats_no_rows(dev, C):
    """n_rows = 0: one slot of zeros"""
    assert _lib.query("bgnn_bn_slots", 0, C) == 1
    some = inp(dev, torch.ones(2, C))
    S = bn_partials(dev, "bgnn_bn_bwd_stats", (ptr(some), ptr(some), ptr(some), ptr(some), 0, C), 1, C,
                    f"bgnn_bn_bwd_stats C={C} n_rows=0")
    assert bool((S == 0).all())
