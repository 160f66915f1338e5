"""CPU: the references of tests/sage_rows_ref.py are right and their bounds have teeth.

- Each formula reference equals fp64 torch autograd of the composition F.normalize -> F.batch_norm
  (training / eval / none) -> relu -> (+ x_prev) -> mask * inv_keep to 1e-12 relative: sum g2 and
  sum g2 xhat are autograd's dbeta and dgamma, dh the gradient with respect to h, sum dh the
  gradient with respect to the bias.
- The mask restatement keeps the right fraction.
- No backward case has an element of o scale + shift whose ReLU sign an f32 kernel could
  legitimately take the other way; exact zeros are present and give g2 = 0.
- For every case of the GPU matrix (the lists are shared) every mutation that can show in that case
  moves the fp64 result by more than 8 x the bound on at least one element; the unmutated fp64
  result against itself stays at 0. A mutation is skipped for a case only where it cannot show:
  the case does not use what it changes (no dropout, no row weights, no empty row, one slot ...),
  or the mutated mask happens to equal the true one on so few elements (each line says so)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sage_rows_ref as R

D = torch.float64
TEETH = 8.0


# ----------------------------------------------------------------------------- references vs autograd
def close(a, b, what):
    a, b = a.to(D), b.to(D)
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-30), what


@pytest.mark.parametrize("p,seed", [(0.0, 0), (0.25, 77), (0.5, 2 ** 64 - 1)])
@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("bn", ["train", "eval", "off"])
def test_references_agree_with_autograd(bn, skip, p, seed):
    n, H, eps = 37, 20, float(np.float32(1e-5))
    q = torch.Generator().manual_seed(11)
    z, b = torch.randn(n, H, generator=q, dtype=D), torch.randn(H, generator=q, dtype=D).requires_grad_(True)
    z.requires_grad_(True)
    xprev = torch.randn(n, H, generator=q, dtype=D).requires_grad_(True)
    gamma = (torch.rand(H, generator=q, dtype=D) + 0.5).requires_grad_(True)
    beta = torch.randn(H, generator=q, dtype=D).requires_grad_(True)
    rm, rv = torch.randn(H, generator=q, dtype=D) * 0.1, torch.rand(H, generator=q, dtype=D) * 0.05 + 0.01
    G = torch.randn(n, H, generator=q, dtype=D)
    keep, ik = R.keep_mask(seed, n, H, p), float(R.inv_keep(p))
    h = z + b
    h.retain_grad()
    o = F.normalize(h, dim=1)
    if bn == "train":
        y = F.batch_norm(o, None, None, gamma, beta, training=True, eps=eps)
    elif bn == "eval":
        y = F.batch_norm(o, rm, rv, gamma, beta, training=False, eps=eps)
    else:
        y = o
    x = (torch.relu(y) + (xprev if skip else 0)) * keep * ik
    (x * G).sum().backward()

    od, nrm = o.detach(), h.detach().norm(dim=1)
    if bn == "train":
        part = torch.stack([od.sum(0), od.pow(2).sum(0)]).unsqueeze(0)
        fin = R.bn_finalize_ref(part, n, gamma.detach(), beta.detach(), eps, 0.1, rm, rv)
        mean, invstd, scale, shift = (fin[k][0] for k in ("mean", "invstd", "scale", "shift"))
        m = float(np.float32(0.1))   # the entry point takes an f32 momentum
        close(fin["rmean"][0], (1 - m) * rm + m * od.mean(0), "running_mean")
        close(fin["rvar"][0], (1 - m) * rv + m * od.var(0, unbiased=True), "running_var")
    elif bn == "eval":
        ev = R.bn_eval_ref(gamma.detach(), beta.detach(), eps, rm, rv)
        mean, invstd, scale, shift = rm, 1.0 / (rv + eps).sqrt(), ev["scale"][0], ev["shift"][0]
    else:
        mean = invstd = scale = shift = None
    close(R.sage_apply_ref(od, scale, shift, xprev.detach(), skip, p, seed)[0], x.detach(), "x_next")
    sg2 = sg2x = None
    if bn != "off":
        g2, g2x = R.bwd_stats_ref(G, None, od, scale, shift, mean, invstd, p, seed)
        close(g2.sum(0), beta.grad, "sum g2 = dbeta")
        close(g2x.sum(0), gamma.grad, "sum g2 xhat = dgamma")
        sg2, sg2x = (g2.sum(0), g2x.sum(0)) if bn == "train" else (torch.zeros(H, dtype=D), torch.zeros(H, dtype=D))
    ref = R.bwd_rows_ref(G, None, od, nrm, scale, shift, gamma.detach() if bn != "off" else None, mean, invstd, sg2,
                         sg2x, p, seed)
    close(ref["dh"], h.grad, "dh")
    close(ref["dh"].sum(0), b.grad, "sum dh = db")
    if skip:
        close(ref["gskip"], xprev.grad, "gskip")


def test_l2norm_reference_agrees_with_autograd():
    q = torch.Generator().manual_seed(3)
    h = torch.randn(23, 12, generator=q, dtype=D).requires_grad_(True)
    G = torch.randn(23, 12, generator=q, dtype=D)
    o = F.normalize(h, dim=1)
    (o * G).sum().backward()
    ref = R.bwd_rows_ref(G, None, o.detach(), h.detach().norm(dim=1), *([None] * 7), 0.0, 0, relu=False)
    close(ref["dh"], h.grad, "dh")


def test_zero_norm_rows_follow_the_clamped_denominator():
    """F.normalize's max(||h||, 1e-12): at h = 0 the gradient is g / 1e-12"""
    h = torch.zeros(2, 8, dtype=D, requires_grad=True)
    G = torch.randn(2, 8, generator=torch.Generator().manual_seed(1), dtype=D)
    (F.normalize(h, dim=1) * G).sum().backward()
    ref = R.bwd_rows_ref(G, None, torch.zeros(2, 8, dtype=D), torch.zeros(2, dtype=D), *([None] * 7), 0.0, 0, relu=False)
    close(ref["dh"], h.grad, "dh")


def test_linear_prep_reference_is_threshold_backward():
    g, y = R.prep_inputs(257, 8)
    yy = y.clone().requires_grad_(True)
    torch.relu(yy).backward(g)
    assert torch.equal(R.prep_ref(g, y), yy.grad)


# ----------------------------------------------------------------------------- the mask
def test_threshold_and_scale():
    assert [R.dropout_threshold(p) for p in (0.0, -1.0, 0.1, 0.25, 0.5, 0.999999)] == [0, 0, 6554, 16384, 32768, 65536]
    assert R.inv_keep(0.0) == 1 and R.inv_keep(0.5) == 2 and R.inv_keep(0.1) == np.float32(1) / np.float32(0.9)


@pytest.mark.parametrize("seed", R.SEEDS)
@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_mask_keep_fraction(p, seed):
    n = 1 << 20
    kept = int(R.keep_mask(seed, 1024, 1024, p).sum())
    q = 1.0 - R.dropout_threshold(p) / 65536.0
    assert abs(kept - n * q) <= 4.0 * (n * q * (1 - q)) ** 0.5
    assert bool(R.keep_mask(seed, 8, 8, 0.0).all())


def test_mask_is_a_function_of_the_flat_group_index():
    """[N, H] and the flat array of the same elements share one mask (bgnn_add_dropout's view)"""
    assert torch.equal(R.keep_mask(77, 67, 100, 0.5).view(-1), R.keep_mask(77, 1, 6700, 0.5).view(-1))


# ----------------------------------------------------------------------------- no ambiguous ReLU signs
SHAPES = sorted({(c[0], 3 if c[1][1] else 0) for c in R.STATS_CASES} | {(c[0], 3 if c[1][4] else 0) for c in R.ROWS_CASES}
                | {((975, H), 0) for H in (100, 260, 512)} | {((67, 100), 0), ((5, 512), 0)})


@pytest.mark.parametrize("shape,pool", SHAPES)
def test_no_ambiguous_relu_signs(shape, pool):
    n, H = shape
    for zn in ((False, True) if shape in ((67, 100), (67, 260)) else (False,)):
        d = R.layer_inputs(n, H, n_pool=pool, zero_norm=zn)
        amb, zeros = R.relu_ambiguous(d["o"], d["scale"], d["shift"])
        assert amb == 0 and zeros > 0
        g2, _ = R.bwd_stats_ref(d["g"], d["g_rows"], d["o"], d["scale"], d["shift"], d["mean"], d["invstd"], 0.0, 0)
        yp = d["o"].to(D) * d["scale"].to(D) + d["shift"].to(D)
        assert bool((g2[yp == 0] == 0).all())


# ----------------------------------------------------------------------------- the bounds have teeth
def show(label, mut, r, note=""):
    print(f"{label}: {mut}: {'%.3g' % r if r is not None else 'n/a'} {note}")
    assert r is None or r > TEETH, f"{label}: mutation {mut} stays within {r:.3g} x the bound"


@pytest.mark.parametrize("case", R.FWD_CASES, ids=R.case_id)
def test_teeth_sage_fwd(case):
    kind, H, mean, _inter, _rev = case
    label = f"sage_fwd {kind} H={H} mean={mean}"
    ei, n, heavy, groups = R.host_graph(kind)
    d = R.fwd_inputs(n, H)
    zl, zr, b = d["z"][:, :H], d["z"][:, H:], d["b"]
    hg = kind == "store_hagg"

    def ref(mut=None, drop=(), skip_first=False):
        return R.sage_fwd_ref(ei, n, zl, zr, b, mean, R.host_hagg(ei, n, zl, heavy, skip_first) if hg else None,
                              heavy if hg else None, mut, drop)
    true = ref()
    assert R.away(ref()["o"], true["o"], true["o_bound"]) == 0.0

    def far(m):
        return max(R.away(m["o"], true["o"], true["o_bound"]), R.away(m["nrm"], true["nrm"], true["nrm_bound"]))
    big = int(heavy[1]) if not kind.startswith("store") else int(heavy[0])      # the in-degree-700 row / a super node
    at = (ei[1] == big).nonzero().flatten()
    e700 = int(at[zl[ei[0][at]].abs().amax(1).argmax()])                        # its entry with the largest |z_l|
    show(label, "drop_entry_700", far(ref(skip_first=True) if hg else ref(drop=(e700,))))
    # the stable sort keeps edge_index order within a row: its last / first entry
    r64, rshort = (10, 1000) if not kind.startswith("store") else (10, n - 2)
    show(label, "drop_last_of_64", far(ref(drop=(int((ei[1] == r64).nonzero()[-1]),))))
    show(label, "drop_first_short_group", far(ref(drop=(int((ei[1] == rshort).nonzero()[0]),))))
    empty = int((true["cnt"] == 0).sum())
    show(label, "deg0", far(ref("deg0")) if mean and empty else None, "" if mean and empty else "(sum, or no empty row)")
    show(label, "bias_tail", far(ref("bias_tail")))
    slots = R.fwd_slots(n, len(heavy), groups if kind != "blocked" else None)
    Rr = R.fwd_rows_per_slot(n, slots, len(heavy), groups if kind != "blocked" else None)
    for t, nm in ((true["o"], "o"), (true["o"] ** 2, "o^2")):
        s, bound = R.colsum(t, Rr)
        assert R.away(R.colsum(t, Rr)[0], s, bound) == 0.0
        show(label, f"skip_row (sum {nm}, R = {Rr})", R.away(R.colsum(t, Rr, mut="skip_row")[0], s, bound))


def mask_teeth(label, n, H, p, seed, value_of):
    """the two mask mutations on a case with dropout: value_of(mut) -> (mutated result, true, bound)"""
    if R.dropout_threshold(p) == 0:
        for m in ("group_shift", "thr_minus_1"):
            show(label, m, None, "(no dropout)")
        return
    true = R.keep_mask(seed, n, H, p)
    for m in ("group_shift", "thr_minus_1"):
        differ = int((R.keep_mask(seed, n, H, p, m) != true).sum())
        if differ == 0:
            # group_shift: every 4-bit group equal to its neighbour's; thr_minus_1: no 16-bit field equal to thr - 1
            # (one element in 65,536): only at shapes with few elements
            assert n * H < (1 << 12 if m == "group_shift" else 1 << 20), f"{label}: {m} leaves the mask unchanged"
            show(label, m, None, f"(the mutated mask equals the true one on all {n * H} elements)")
            continue
        a, t, bound = value_of(m)
        r = R.away(a, t, bound)
        if r == 0.0 and differ <= 8:   # every differing element sits where the ReLU passes nothing
            show(label, m, None, f"(the {differ} differing mask elements are blocked by the ReLU)")
            continue
        show(label, m, r, f"({differ} mask elements differ)")


@pytest.mark.parametrize("i", range(len(R.APPLY_CASES)), ids=[R.case_id(c) for c in R.APPLY_CASES])
def test_teeth_sage_apply(i):
    (n, H), (aff, skip, p, seed, _rev) = R.APPLY_CASES[i]
    label = f"sage_apply N={n} H={H} affine={aff} skip={skip} p={p} seed={seed}"
    d = R.layer_inputs(n, H)
    if not skip:   # without the skip a kept element can be relu(.) = 0: let the mask act on non-zero values
        d = dict(d, o=d["o"].abs() + 0.5)

    def run(mut=None):
        return R.sage_apply_ref(d["o"], d["scale"] if aff else None, d["shift"] if aff else None, d["xprev"], skip, p,
                                seed, mut)
    ref, bound, _ = run()
    assert R.away(run()[0], ref, bound) == 0.0
    mask_teeth(label, n, H, p, seed, lambda m: (run(m)[0], ref, bound + 5 * R.U * run(m)[0].abs()))


@pytest.mark.parametrize("H", R.APPLY_ROWS_H)
def test_teeth_apply_range_sums(H):
    ei, n, heavy, _ = R.host_graph("store")
    d = R.layer_inputs(n, H)
    x = R.sage_apply_ref(d["o"], d["scale"], d["shift"], d["xprev"], 1, 0.1, 77)[0]
    a, e = 0, int((ei[1] == int(heavy[0])).sum())
    s = x[a:e].sum(0)
    bound = R.tree_bound(4 + 3 + -(-(e - a) // 16) + 3, x[a:e].abs().sum(0), s)
    show(f"apply range sums H={H}", "skip_row", R.away(x[a:e - 1].sum(0), s, bound))


@pytest.mark.parametrize("i", range(len(R.STATS_CASES)), ids=[R.case_id(c) for c in R.STATS_CASES])
def test_teeth_sage_bwd_stats(i):
    (n, H), (p, pooled, _acc, _null) = R.STATS_CASES[i]
    seed = R.SEEDS[i % 3]
    label = f"sage_bwd_stats N={n} H={H} p={p} seed={seed} pooled={pooled}"
    d = R.layer_inputs(n, H, n_pool=3 if pooled else 0)
    rpb = R.rows_rpb(n)

    def run(mut=None):
        t = R.bwd_stats_ref(d["g"], d["g_rows"], d["o"], d["scale"], d["shift"], d["mean"], d["invstd"], p, seed, mut)
        return [R.colsum(x, rpb, mut=mut) for x in t]
    true = run()
    assert all(R.away(a[0], t[0], t[1]) == 0.0 for a, t in zip(run(), true))

    def far(m):
        return max(R.away(a[0], t[0], t[1]) for a, t in zip(run(m), true))
    show(label, "skip_row", far("skip_row"))
    mask_teeth(label, n, H, p, seed, lambda m: (run(m)[0][0], true[0][0], true[0][1]))
    can = pooled and n >= 3
    show(label, "g_rows_prev", far("g_rows_prev") if can else None, "" if can else "(no g_rows, or one row)")
    P = torch.stack([d["g"][:1].expand(5, H), d["o"][:1].expand(5, H)], 1)[:, :, :H].contiguous()   # any 5 slots
    s, bound = R.reduce_partials_ref(P, 0)
    show(label, "omit_slot (reduce_partials)", R.away(R.reduce_partials_ref(P, 0, mut="omit_slot")[0], s, bound))


@pytest.mark.parametrize("i", range(len(R.ROWS_CASES) + len(R.L2_CASES)),
                         ids=["D-" + R.case_id(c) for c in R.ROWS_CASES] + ["E-" + R.case_id(c) for c in R.L2_CASES])
def test_teeth_sage_bwd_rows(i):
    if i < len(R.ROWS_CASES):
        (n, H), (bn, gam, skip, p, pooled, _ldf, w_mode, _rev) = R.ROWS_CASES[i]
        seed, relu = R.SEEDS[i % 3], True
        d = R.layer_inputs(n, H, n_pool=3 if pooled else 0)
        args = R.rows_args(d, bn, gam)
        label = f"sage_bwd_rows N={n} H={H} bn={bn} gamma={gam} skip={skip} p={p} seed={seed} pooled={pooled} w_mode={w_mode}"
    else:
        (n, H), _ = R.L2_CASES[i - len(R.ROWS_CASES)]
        bn, p, seed, pooled, w_mode, relu = "off", 0.0, 0, 0, 0, False
        d = R.layer_inputs(n, H)
        args = R.l2_args(d)
        label = f"l2norm_bwd N={n} H={H}"
    rpb = R.rows_rpb(n)

    def run(mut=None):
        return R.bwd_rows_ref(*[args[k] for k in ("g", "g_rows", "o", "nrm", "scale", "shift", "gamma", "mean", "invstd",
                                                  "sum_g2", "sum_g2xhat")], p, seed, relu=relu, mut=mut)
    true = run()
    assert R.away(run()["dh"], true["dh"], true["bound"]) == 0.0
    s, bound = R.colsum(true["dh"], rpb)
    show(label, "skip_row (sum dh)", R.away(R.colsum(true["dh"], rpb, mut="skip_row")[0], s, bound))
    if relu:
        mask_teeth(label, n, H, p, seed, lambda m: (run(m)["dh"], true["dh"], true["bound"] + run(m)["bound"]))
        can = pooled and n >= 3
        show(label, "g_rows_prev", R.away(run("g_rows_prev")["dh"], true["dh"], true["bound"]) if can else None,
             "" if can else "(no g_rows, or one row)")
        can = w_mode == 1 and n >= 3
        if can:
            s, bound = R.colsum(true["dh"], rpb, w=R.row_weights(d["w_rowptr"], 1))
            r = R.away(R.colsum(true["dh"], rpb, w=R.row_weights(d["w_rowptr"], 1, "w_mode_2"))[0], s, bound)
        show(label, "w_mode_2", r if can else None, "" if can else "(w_mode is not 1, or no row of in-degree 2)")


@pytest.mark.parametrize("i", range(len(R.FIN_CASES)), ids=[R.case_id(c) for c in R.FIN_CASES])
def test_teeth_bn_finalize(i):
    (S, H), (one, aff, mom, running) = R.FIN_CASES[i]
    count = R.fin_count(S, one)
    label = f"bn_finalize S={S} H={H} count={count} affine={aff} momentum={mom} running={running}"
    P = R.partials(S, H, count)
    gamma, beta, rm, rv, ks = R.fin_inputs(S, H, aff)
    for kshift in (None, ks):
        def run(mut=None):
            return R.bn_finalize_ref(P, count, gamma, beta, 1e-5, mom, rm if running else None, rv if running else None,
                                     kshift, mut)
        true = run()
        assert bool((true["var"] >= 1e-3 * P[:, 1].to(D).sum(0) / count).all())
        keys = [k for k in true if k != "var"]
        assert all(R.away(run()[k][0], *true[k]) == 0.0 for k in keys)
        show(label, "omit_slot", max(R.away(run("omit_slot")[k][0], *true[k]) for k in ("mean", "invstd", "scale", "shift")))
        can = "rvar" in true and count > 1
        show(label, "biased", R.away(run("biased")["rvar"][0], *true["rvar"]) if can else None,
             "" if can else "(no running statistics, momentum 0, or count 1)")
    for half in (0, 1):
        s, bound = R.reduce_partials_ref(P, half)
        show(label, f"omit_slot (reduce_partials half {half})",
             R.away(R.reduce_partials_ref(P, half, mut="omit_slot")[0], s, bound))


@pytest.mark.parametrize("i", range(len(R.PREP_CASES)), ids=[R.case_id(c) for c in R.PREP_CASES])
def test_teeth_linear_bwd_prep(i):
    (n, C), (has_y, _has_out) = R.PREP_CASES[i]
    g, y = R.prep_inputs(n, C)
    want = R.prep_ref(g, y if has_y else None)
    Rr = R.prep_rows_per_slot(n, C)
    s, bound = R.colsum(want, Rr)
    assert R.away(R.colsum(want, Rr)[0], s, bound) == 0.0
    show(f"linear_bwd_prep N={n} C={C} y={has_y}", f"skip_row (R = {Rr})",
         R.away(R.colsum(want, Rr, mut="skip_row")[0], s, bound))
