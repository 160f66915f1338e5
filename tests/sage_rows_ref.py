"""Host references for the f32 SAGE layer row kernels (bgnn_sage_fwd and csrc/sage.hip): the
dropout mask restated from the text of include/bgnn.h and csrc/common.h, fp64 evaluations of the
header's formulas on the same f32 inputs (each with `mag`, the fp64 sum of the absolute values of
the terms behind every output element), the bounds that follow from the operation count of each
formula under the standard f32 model (u = 2^-24; nothing here is a measured tolerance), the case
lists shared by tests/test_gpu_sage_rows_matrix.py (GPU) and tests/test_sage_rows_ref.py (CPU:
autograd agreement, mutations), and the input generators. No GPU is touched here.

Mutations: every reference takes `mut`, the name of one deliberate mistake (MUTATIONS below), and
then computes what a subtly wrong kernel would; the CPU test shows that each leaves the true result
by more than 8 x the bound."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of f32
E64 = 2.0 ** -53        # ... of f64
SEEDS = (0, 77, 2 ** 64 - 1)
D = torch.float64


# ============================================================================ the dropout mask
def dropout_threshold(p):
    """thr = floor(p * 65536 + 0.5) of the f32 p, clamped to 65536; p <= 0 gives 0 (no dropout)."""
    p = float(np.float32(p))
    if not p > 0.0:
        return 0
    return int(min(math.floor(p * 65536.0 + 0.5), 65536))


def inv_keep(p):
    """The f32 1.f / (1.f - p) kept values are multiplied by (1 without dropout)."""
    if dropout_threshold(p) == 0:
        return np.float32(1.0)
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def mix64(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def keep_mask(seed, n_rows, H, p, mut=None):
    """bool [n_rows, H]: the hash covers groups of 4 consecutive elements of the dense array; element
    k of group g is kept when bits [16k, 16k + 16) of mix64(seed ^ g * 0xD1B54A32D192ED03) are >= thr."""
    thr = dropout_threshold(p)
    n = n_rows * H
    assert n % 4 == 0
    if thr == 0:
        return torch.ones(n_rows, H, dtype=torch.bool)
    if mut == "thr_minus_1":
        thr -= 1
    g = np.arange(n // 4, dtype=np.uint64)
    if mut == "group_shift":
        g = g + np.uint64(1)
    with np.errstate(over="ignore"):
        h = mix64(np.uint64(seed) ^ (g * np.uint64(0xD1B54A32D192ED03)))
    k = np.arange(4, dtype=np.uint64) * np.uint64(16)
    field = (h[:, None] >> k[None, :]) & np.uint64(0xFFFF)
    return torch.from_numpy((field >= np.uint64(thr)).reshape(n_rows, H))


# ============================================================================ shared pieces
def rows_slots(n):
    """bgnn_rows_slots: ceil(n / 4) row blocks, at most 1024 (include/bgnn.h, csrc/ranges.h)."""
    return max(1, min((n + 3) // 4, 1024))


def rows_rpb(n):
    return -(-n // rows_slots(n))


def colsum(x, R, w=None, rows=None, mut=None):
    """(fp64 column sum of w_r x_r over `rows`, bound). The header fixes the structure of every
    column sum over rows: f32 within a slot, fp64 across slots. A slot adds at most R terms in some
    order: at most R - 1 roundings touch a term, plus up to 3 in forming the term (weight, product,
    square), so |err| <= (R + 3) u sum |terms|, plus u |result| for a final rounding to f32 and the
    fp64 summation over the slots, which is below u^2 * slots * sum |terms|: absorbed by the + 3.
    mut 'skip_row': the last row of the last non-empty row block (blocks of rpb rows) is left out."""
    x = x.to(D)
    t = x if w is None else x * w.to(D).unsqueeze(1)
    if rows is not None:
        t = t[rows[0]:rows[1]]
    if mut == "skip_row" and t.size(0):
        t = t[:-1]
    s = t.sum(0)
    return s, (R + 3) * U * t.abs().sum(0) + U * s.abs()


def tree_bound(depth, terms_abs, s):
    """an f32 summation tree of the given depth: |err| <= depth u sum |terms| (+ 3 for forming a term,
    + u |result|)"""
    return (depth + 3) * U * terms_abs + U * s.abs()


def ratio(err, bound):
    """largest err / bound; a non-finite error counts as infinite"""
    err = torch.as_tensor(err, dtype=D)
    if err.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    return float((err / bound.clamp_min(1e-300)).max())


def away(a, b, bound):
    """how far a mutated result is from the true one, in bounds"""
    return ratio((a.to(D) - b.to(D)).abs(), bound)


# ============================================================================ sage_fwd
def sage_fwd_ref(ei, n, zl, zr, b, mean, hagg=None, heavy_rows=None, mut=None, drop=()):
    """h = s_r sum z_l[col] + z_r + b, nrm = ||h||, o = h / max(nrm, 1e-12) in fp64, with the
    bounds:
      h: a row with cnt entries adds cnt terms (cnt - 1 roundings), scales (s_r rounded + the
         product) and adds z_r and b: (cnt + 4) u mag, mag = s_r sum |z_l| + |z_r| + |b|.
      nrm = sqrt(sum h^2): first order sum |h| dh / nrm, plus (H + 8) u nrm for the length-H sum
         of squares in any order, the squares and the root.
      o = h / den: dh / den + |o| dnrm / den + 2 u |o| (den = max(nrm, 1e-12) is exact when clamped).
    heavy_rows / hagg: those rows take the given f32 aggregate in place of their sum.
    drop: edge positions left out (a mutation); mut 'deg0': 1 / deg, 'bias_tail': no bias on the last
    4 columns."""
    src, dst = ei[0], ei[1]
    if len(drop):
        keep = torch.ones(src.numel(), dtype=torch.bool)
        keep[list(drop)] = False
        src, dst = src[keep], dst[keep]
    H = zl.size(1)
    zl, zr, b = zl.to(D), zr.to(D), b.to(D).clone()
    cnt = torch.bincount(dst, minlength=n)
    agg = torch.zeros(n, H, dtype=D).index_add_(0, dst, zl[src])
    amag = torch.zeros(n, H, dtype=D).index_add_(0, dst, zl[src].abs())
    if hagg is not None:
        agg[heavy_rows] = hagg.to(D)
        amag[heavy_rows] = hagg.to(D).abs()
    if mean:
        s = 1.0 / (cnt.to(D) if mut == "deg0" else cnt.clamp_min(1).to(D))
    else:
        s = torch.ones(n, dtype=D)
    s = s.unsqueeze(1)
    if mut == "bias_tail":
        b[-4:] = 0
    h = s * agg + zr + b          # (an empty row: s = 1, agg = 0, so h = z_r + b)
    mag = torch.where(cnt.unsqueeze(1) > 0, s * amag, torch.zeros((), dtype=D)) + zr.abs() + b.abs()
    nrm = h.pow(2).sum(1).sqrt()
    den = nrm.clamp_min(1e-12)
    o = h / den.unsqueeze(1)
    cb = cnt.clone()
    if hagg is not None:
        cb[heavy_rows] = 1        # one given term
    dh = (cb.to(D).unsqueeze(1) + 4) * U * mag
    dn = (h.abs() * dh).sum(1) / den + (H + 8) * U * nrm
    do = dh / den.unsqueeze(1) + o.abs() * (torch.where(nrm >= 1e-12, dn, torch.zeros((), dtype=D)) / den).unsqueeze(1) \
        + 2 * U * o.abs()
    return dict(h=h, mag=mag, cnt=cnt, nrm=nrm, nrm_bound=dn + U * nrm, o=o, o_bound=do)


def fwd_rows_per_slot(n, slots, n_heavy, groups=None):
    """R of the aggregation kernels' BatchNorm slots, from the documented partition: the light
    rows (or row groups) are dealt over slots - n_heavy blocks, a heavy row has a slot of its own.
    groups = (group_rows, n_groups) for the row-group kernel."""
    light = slots - n_heavy

    def per(x):   # contiguous blocks of ceil(x / light), or the sweep: each eighth of the items dealt
        return max(-(-x // light), 4 * -(-(-(-x // 8)) // (light // 2)))   # to light / 8 blocks of 4 waves
    return groups[0] * per(groups[1]) if groups else per(n)


# ============================================================================ sage_apply
def sage_apply_ref(o, scale, shift, xprev, skip, p, seed, mut=None):
    """x_next = drop(relu(o scale + shift) + x_prev): (ref, bound, keep mask). Kept elements:
    a = fl(o scale), b = fl(a + shift) (or one fma), c = fl(relu(b) + x_prev), fl(c inv_keep) with
    the f32 inv_keep: |err| <= (4 u |o scale| + 3 u |shift| + 2 u |x_prev|) inv_keep to first
    order; the bound takes 5 u mag, mag = (|o scale| + |shift| + |x_prev|) inv_keep. Dropped
    elements are exactly 0 (bound 0)."""
    n, H = o.shape
    o = o.to(D)
    t = o * scale.to(D) if scale is not None else o
    y = t + shift.to(D) if shift is not None else t
    mag = t.abs() + (shift.to(D).abs() if shift is not None else 0)
    exact = scale is None                      # no arithmetic before the ReLU
    y = y.clamp_min(0)
    if skip:
        y = y + xprev.to(D)
        mag = mag + xprev.to(D).abs()
        exact = False
    keep = keep_mask(seed, n, H, p, mut)
    ik = float(inv_keep(p))
    ref = torch.where(keep, y * ik, torch.zeros((), dtype=D))
    mag = torch.where(keep, mag * ik, torch.zeros((), dtype=D))
    return ref, (U if exact and ik == 1.0 else 5 * U) * mag, keep


# ============================================================================ the backward
def _g1(g, g_rows, keep, p, mut=None):
    """dropout'(g) = keep ? g inv_keep : 0 -- one f32 product, so for f32 inputs it is computed in
    f32 and is exact (this is also gskip). mut 'g_rows_prev': one row reads g_rows[r - 1]."""
    if g_rows is not None:
        idx = g_rows.clone()
        if mut == "g_rows_prev":
            r = int((g_rows[1:] != g_rows[:-1]).nonzero()[0]) + 1 if bool((g_rows[1:] != g_rows[:-1]).any()) else 0
            if r:
                idx[r] = g_rows[r - 1]
        g = g[idx]
    ik = float(inv_keep(p))
    g1 = (g * ik) if g.dtype == torch.float32 else g * ik
    return torch.where(keep, g1, torch.zeros((), dtype=g1.dtype))


def relu_ambiguous(o, scale, shift):
    """(count of elements of yp = o scale + shift with 0 < |yp| <= 4 u (|o scale| + |shift|), where an
    f32 kernel could take the other side of the ReLU; count of exact zeros)"""
    t = o.to(D) * scale.to(D) if scale is not None else o.to(D)
    yp = t + shift.to(D) if shift is not None else t
    slack = 4 * U * (t.abs() + (shift.to(D).abs() if shift is not None else 0))
    if scale is None:
        slack = torch.zeros_like(yp)          # yp = o is exact
    return int(((yp.abs() <= slack) & (yp != 0)).sum()), int((yp == 0).sum())


def bwd_stats_ref(g, g_rows, o, scale, shift, mean, invstd, p, seed, mut=None):
    """per element g2 = relu'(o scale + shift) dropout'(g) (exact for f32 inputs, the ReLU sign
    being unambiguous) and g2 xhat, xhat = (o - mean) invstd (3 roundings: the + 3 of colsum)."""
    n, H = o.shape
    keep = keep_mask(seed, n, H, p, mut)
    g1 = _g1(g, g_rows, keep, p, mut).to(D)
    yp = o.to(D) * scale.to(D) + shift.to(D)
    g2 = torch.where(yp > 0, g1, torch.zeros((), dtype=D))
    return g2, g2 * ((o.to(D) - mean.to(D)) * invstd.to(D))


def bwd_rows_ref(g, g_rows, o, nrm, scale, shift, gamma, mean, invstd, sum_g2, sum_g2xhat, p, seed, relu=True,
                 mut=None):
    """dh of bgnn_sage_bwd_rows (relu=False, no BN, p = 0: bgnn_l2norm_bwd) in fp64 with its bound.
      d (BN) = kA g2 - kB - xhat kC, kA = gamma invstd, kB = kA sum_g2 / N, kC = kA sum_g2xhat / N:
         kA 1 rounding, kB and kC 3 more (1 / N, two products), xhat 2, the three products and two
         differences: at most 10 u (|kA g2| + |kB| + |xhat kC|). Without BN d = g2, exact.
      dot = <o, d>: sum |o| dd + (H + 8) u sum |o d| (length-H sum, any order).
      dh = (d - o dot) / nrm: (dd + |o| ddot) / nrm + 4 u (|d| + |o| |dot|) / nrm (product, difference,
         reciprocal, product); nrm < 1e-12: d 1e12, dd 1e12 + 4 u |d| 1e12.
    Returns dict(dh, bound, mag, gskip (f32-exact), d)."""
    n, H = o.shape
    keep = keep_mask(seed, n, H, p, mut)
    g1 = _g1(g, g_rows, keep, p, mut)
    g1d, od = g1.to(D), o.to(D)
    if relu:
        t = od * scale.to(D) if scale is not None else od
        yp = t + shift.to(D) if shift is not None else t
        g2 = torch.where(yp > 0, g1d, torch.zeros((), dtype=D))
    else:
        g2 = g1d
    if mean is not None:
        kA = (gamma.to(D) if gamma is not None else 1.0) * invstd.to(D)
        kB = kA * sum_g2.to(D) / n
        kC = kA * sum_g2xhat.to(D) / n
        t3 = (od - mean.to(D)) * invstd.to(D) * kC
        d = kA * g2 - kB - t3
        dd = 10 * U * ((kA * g2).abs() + kB.abs() + t3.abs())
    else:
        d, dd = g2, torch.zeros_like(g2)
    dot = (od * d).sum(1, keepdim=True)
    ddot = (od.abs() * dd).sum(1, keepdim=True) + (H + 8) * U * (od * d).abs().sum(1, keepdim=True)
    nr = nrm.to(D).unsqueeze(1)
    through = (nrm >= float(np.float32(1e-12))).unsqueeze(1) if nrm.dtype == torch.float32 else nr >= 1e-12
    safe = torch.where(through, nr, torch.ones((), dtype=D))
    dh = torch.where(through, (d - od * dot) / safe, d * 1e12)
    mag = torch.where(through, (d.abs() + od.abs() * dot.abs()) / safe, d.abs() * 1e12)
    bound = torch.where(through, (dd + od.abs() * ddot) / safe, dd * 1e12) + 4 * U * mag
    return dict(dh=dh, bound=bound, mag=mag, gskip=g1, d=d)


def row_weights(rowptr, w_mode, mut=None):
    """w_r of partial_db[.][1]: 1 = in-degree, 2 = [in-degree > 0], 0 = none (the half is 0)"""
    deg = (rowptr[1:] - rowptr[:-1]).to(D)
    if w_mode == 1 and mut != "w_mode_2":
        return deg
    if w_mode in (1, 2):
        return (deg > 0).to(D)
    return torch.zeros_like(deg)


# ============================================================================ BatchNorm coefficients
def bn_finalize_ref(part, count, gamma, beta, eps, momentum, rmean, rvar, kshift=None, mut=None):
    """torch.nn.BatchNorm1d's training arithmetic on [S, 2, H] partials (sums of x - k and (x - k)^2;
    k = 0 without kshift) in fp64: mean, invstd (biased variance), scale = gamma invstd, shift =
    beta - mean scale, running statistics with the unbiased variance (count == 1: the variance
    itself). eps and momentum are the f32 values the entry point receives. Bounds: every output is
    one rounding of an fp64 value: 4 u relative (4 u of the two terms for the differences), plus the
    first-order effect of the kernel's own fp64 sums over the slots, (S + 4) 2^-53 sum |partials|.
    mut 'omit_slot': one slot left out; 'biased': the biased variance into running_var."""
    p = part.to(D)
    if mut == "omit_slot":
        p = torch.cat([p[:p.size(0) // 2], p[p.size(0) // 2 + 1:]])
    S, n = part.size(0), float(count)
    eps, m = float(np.float32(eps)), float(np.float32(momentum))
    s0, s1, a0, a1 = p[:, 0].sum(0), p[:, 1].sum(0), p[:, 0].abs().sum(0), p[:, 1].abs().sum(0)
    mu0 = s0 / n
    var = (s1 / n - mu0 * mu0).clamp_min(0)
    mu = mu0 + (kshift.to(D) if kshift is not None else 0)
    is_ = 1.0 / (var + eps).sqrt()
    g = gamma.to(D) if gamma is not None else torch.ones_like(mu)
    b = beta.to(D) if beta is not None else torch.zeros_like(mu)
    e = (S + 4) * E64
    dmu = e * a0 / n + (E64 * mu.abs() if kshift is not None else 0)
    dvar = e * (a1 / n + 2 * mu0.abs() * a0 / n)
    dis = is_ * dvar / (2 * (var + eps))
    out = dict(mean=(mu, 4 * U * mu.abs() + dmu), invstd=(is_, 4 * U * is_ + dis),
               scale=(g * is_, 4 * U * (g * is_).abs() + g.abs() * dis),
               shift=(b - mu * g * is_, 4 * U * (b.abs() + (mu * g * is_).abs()) + g.abs() * (dmu * is_ + mu.abs() * dis)),
               var=var)
    if rmean is not None and rvar is not None and m > 0:
        unb = var * n / (n - 1.0) if count > 1 and mut != "biased" else var
        k = n / (n - 1.0) if count > 1 else 1.0
        out["rmean"] = ((1 - m) * rmean.to(D) + m * mu, 4 * U * (((1 - m) * rmean.to(D)).abs() + (m * mu).abs()) + m * dmu)
        out["rvar"] = ((1 - m) * rvar.to(D) + m * unb, 4 * U * (((1 - m) * rvar.to(D)).abs() + m * unb) + m * k * dvar)
    return out


def bn_eval_ref(gamma, beta, eps, rmean, rvar):
    is_ = 1.0 / (rvar.to(D) + float(np.float32(eps))).sqrt()
    g = gamma.to(D) if gamma is not None else torch.ones_like(is_)
    b = beta.to(D) if beta is not None else torch.zeros_like(is_)
    t = rmean.to(D) * g * is_
    return dict(scale=(g * is_, 4 * U * (g * is_).abs()), shift=(b - t, 4 * U * (b.abs() + t.abs())))


def reduce_partials_ref(part, half, prev=None, mut=None):
    """out = (float) fp64 sum of the slots (+ the previous f32 value with accumulate): one rounding
    of the sum and one of the f32 addition, plus the fp64 summation term."""
    p = part.to(D)[:, half]
    if mut == "omit_slot":
        p = torch.cat([p[:p.size(0) // 2], p[p.size(0) // 2 + 1:]])
    s = p.sum(0)
    bound = U * s.abs() + (part.size(0) + 4) * E64 * p.abs().sum(0)
    if prev is not None:
        s = s + prev.to(D)
        bound = bound + U * s.abs()
    return s, bound


# ============================================================================ linear_bwd_prep
def prep_ref(g, y):
    """g_out = y > 0 ? g : 0 (exact)"""
    return g if y is None else torch.where(y > 0, g, torch.zeros((), dtype=g.dtype))


PREP_SLOTS = 512


def prep_rows_per_slot(n, C):
    """a block takes 256 / (C / 4) rows per step, the grid of 512 blocks strides over the rows"""
    rpi = 256 // (C // 4)
    return rpi * -(-n // (PREP_SLOTS * rpi))


# ============================================================================ inputs
def _seed(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return s


def layer_inputs(n, H, n_pool=0, zero_norm=False):
    d = dict(_layer_inputs(n, H, n_pool))
    if zero_norm:   # three rows with o = 0, nrm = 0 (first, middle, last)
        d["o"], d["nrm"] = d["o"].clone(), d["nrm"].clone()
        for r in sorted({0, n // 2, n - 1}):
            d["o"][r] = 0
            d["nrm"][r] = 0
    return d


@functools.lru_cache(maxsize=4)
def _layer_inputs(n, H, n_pool=0, bn=True, tag=0):
    """f32 inputs of the apply / backward kernels for an [n, H] layer, drawn so that no element of
    yp = o scale + shift is ambiguous for the ReLU (the seed is advanced until the count is 0;
    tests/test_sage_rows_ref.py asserts it), with a few exact zeros (o = 0, shift = 0 there); the last
    row has o = 1 (it passes the ReLU, so leaving it out of a column sum shows).
    n_pool > 0: g is [n_pool, H] and g_rows a non-decreasing batch vector."""
    for attempt in range(64):
        q = torch.Generator().manual_seed(_seed(n, H, bn, n_pool, tag, attempt))
        o = torch.randn(n, H, generator=q) * 0.3
        scale = torch.rand(H, generator=q) + 0.5
        shift = torch.randn(H, generator=q) * 0.1
        zc = sorted({0, H - 1} | ({H // 2} if H >= 12 else set()))   # columns with exact zeros
        shift[zc] = 0
        o[n - 1] = 1.0                                        # the last row passes the ReLU (column-sum mutations)
        o[: max(n - 1, 1): max(1, n // 3), zc] = 0            # (not in the last row, unless it is the only one)
        if relu_ambiguous(o, scale, shift)[0] == 0 and relu_ambiguous(o, None, None)[0] == 0:
            break
    else:
        raise AssertionError("no unambiguous draw")
    ng = n_pool if n_pool else n
    d = dict(o=o, scale=scale, shift=shift, xprev=torch.randn(n, H, generator=q),
             g=torch.randn(ng, H, generator=q), nrm=torch.rand(n, generator=q) + 0.5,
             gamma=torch.rand(H, generator=q) + 0.5, mean=torch.randn(H, generator=q) * 0.1,
             invstd=torch.rand(H, generator=q) * 2 + 1, sum_g2=torch.randn(H, generator=q) * n ** 0.5,
             sum_g2xhat=torch.randn(H, generator=q) * n ** 0.5, g_rows=None)
    if n_pool:
        d["g_rows"] = (torch.arange(n) * n_pool // n).to(torch.int64)
    # a rowptr with empty rows for the row weights: in-degree r % 4 (every fourth row empty)
    d["w_rowptr"] = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.arange(n) % 4, 0)]).to(torch.int32)
    return d


def fwd_inputs(n, H, tag=0):
    q = torch.Generator().manual_seed(_seed(n, H, tag, 99))
    return dict(z=torch.randn(n, 2 * H, generator=q), b=torch.randn(H, generator=q) * 0.5)


def partials(S, H, count, tag=0):
    """[S, 2, H] synthetic BatchNorm partials whose variance s1 / n - (s0 / n)^2 is at least 1e-3 of
    E[x^2] = s1 / n (a condition on the inputs: the kernel's fp64 difference is then not
    cancellation-limited)"""
    q = torch.Generator().manual_seed(_seed(S, H, count, tag, 5))
    p0 = torch.randn(S, H, generator=q) * (count / S) ** 0.5 + 0.3 * count / S
    p1 = torch.rand(S, H, generator=q) + 0.5
    mu0 = p0.to(D).sum(0) / count
    want = mu0 * mu0 + (0.25 + torch.rand(H, generator=q).to(D)) * mu0.pow(2).clamp_min(0.1)   # E[x^2]
    p1 = (p1.to(D) * (want * count / p1.to(D).sum(0))).float()
    return torch.stack([p0, p1], 1).contiguous()


# ============================================================================ the matrix
def _cycle(shapes, flags, per_shape):
    """per_shape flag tuples for every shape, walking the full flag product cyclically so that every
    flag value meets several shapes and every shape several flag values"""
    out, i = [], 0
    for s in shapes:
        for _ in range(per_shape):
            out.append((s, flags[i % len(flags)]))
            i += 1
    return out


def _prod(*axes):
    import itertools
    return list(itertools.product(*axes))


NS = (1, 3, 5, 67, 4099)

# B: (N, H), (affine, skip, p, seed, rev)
APPLY_CASES = _cycle(_prod(NS, (4, 100, 256, 260, 512, 1028)),
                     [f for f in _prod((1, 0), (0, 1), (0.0, 0.1, 0.5), SEEDS, (0, 1))][::5], 3)
APPLY_ROWS_H = (100, 260, 512)
# C: (N, H), (p, pooled g_rows, accumulate, NULL output)
STATS_CASES = _cycle(_prod(NS, (4, 12, 100, 256, 512, 516, 1024)),
                     _prod((0.0, 0.25), (0, 1), (0, 1), (None, 0, 1)), 2)
# D: (N, H), (bn: 'train' / 'eval' (zero sums) / 'off', gamma, skip, p, pooled, lddh factor, w_mode, rev)
ROWS_H = (4, 100, 252, 256, 260, 508, 512)
ROWS_CASES = _cycle(_prod(NS, ROWS_H),
                    _prod(("train", "eval", "off"), (1, 0), (0, 1), (0.0, 0.25), (0, 1), (1, 2), (0, 1, 2), (0, 1))[::7],
                    3)
# E: (N, H), (lddh factor, rev)
L2_CASES = _cycle(_prod(NS, ROWS_H), _prod((1, 2), (0, 1)), 1)
# F: (S, H), (count == 1, affine, momentum, running stats given)
FIN_CASES = _cycle(_prod((1, 31, 32, 33, 224, 225, 256, 257, 1027), (4, 12, 100, 512)),
                   _prod((0, 1), (1, 0), (0.0, 0.1), (1, 0)), 2)
# G: (N, C), (y given, g_out given)
PREP_CASES = [((n, c), f) for n in (1, 5, 257, 5000) for c in (4, 8, 64, 128, 1024)
              for f in ((1, 1), (0, 1), (0, 0))]
# A: (graph, plan kind, H, mean, interleaved z, rev bit 2)
FWD_H = (4, 64, 100, 256, 260, 512)
FWD_KINDS = ("hand", "hand_r8", "rows_u8", "rows_u12", "rows_u16", "blocked", "store", "store_hagg")
FWD_CASES = [(k, H, mean, (i + j + m) % 2, (i + 2 * j + m) % 2)
             for i, k in enumerate(FWD_KINDS) for j, H in enumerate(FWD_H) for m, mean in enumerate((0, 1))]

MUTATIONS = ("drop_entry_700", "drop_last_of_64", "drop_first_short_group", "deg0", "bias_tail", "skip_row",
             "group_shift", "thr_minus_1", "g_rows_prev", "w_mode_2", "omit_slot", "biased")


def case_id(c):
    return "-".join(str(x) for x in (c[0] if isinstance(c[0], tuple) else (c[0],))) + "-" + \
        "-".join(str(x) for x in (c[1] if isinstance(c[1], tuple) else c[1:]))


def rows_args(d, bn, gam):
    """the arguments of a bgnn_sage_bwd_rows case: bn 'train' (arbitrary reduced statistics), 'eval'
    (zeros: the eval-mode call) or 'off' (mean == NULL; scale / shift NULL too unless gam)"""
    aff = bn != "off" or gam
    H = d["o"].size(1)
    zero = torch.zeros(H)
    return dict(g=d["g"], g_rows=d["g_rows"], o=d["o"], nrm=d["nrm"], scale=d["scale"] if aff else None,
                shift=d["shift"] if aff else None, gamma=d["gamma"] if gam else None,
                mean=d["mean"] if bn != "off" else None, invstd=d["invstd"] if bn != "off" else None,
                sum_g2=None if bn == "off" else (zero if bn == "eval" else d["sum_g2"]),
                sum_g2xhat=None if bn == "off" else (zero if bn == "eval" else d["sum_g2xhat"]))


def l2_args(d):
    return dict(g=d["g"], g_rows=None, o=d["o"], nrm=d["nrm"], scale=None, shift=None, gamma=None, mean=None,
                invstd=None, sum_g2=None, sum_g2xhat=None)


def fin_count(S, one):
    return 1 if one else 2 * S + 1


def fin_inputs(S, H, aff):
    """gamma, beta, running_mean, running_var (small, so that the unbiased-variance term shows), kshift"""
    q = torch.Generator().manual_seed(_seed(S, H, 3))
    gamma, beta = (torch.rand(H, generator=q) + 0.5, torch.randn(H, generator=q)) if aff else (None, None)
    return gamma, beta, torch.randn(H, generator=q), torch.rand(H, generator=q) * 1e-2 + 1e-3, torch.randn(H, generator=q)


def prep_inputs(n, C):
    """g, y of a bgnn_linear_bwd_prep case: y has exact zeros (masked: y > 0 is false); the last row
    passes the mask with |g| = 2 (leaving it out of a column sum shows)"""
    q = torch.Generator().manual_seed(_seed(n, C, 8))
    g = torch.randn(n, C, generator=q)
    y = torch.randn(n, C, generator=q)
    y[::3, ::5] = 0
    y[n - 1] = 1.0
    g[n - 1] = torch.where(g[n - 1] < 0, -2.0, 2.0)
    return g, y


def host_graph(kind):
    """(edge_index, N, heavy rows, (group_rows, n_groups) or None) of a structure case, on the host"""
    from test_gpu_spmm_b16 import N_HAND, hand_edges, store_batch_host
    if kind.startswith("store"):
        b = store_batch_host()
        ei, n = b.edge_index, b.num_nodes
        sizes = (b.ptr[1:] - b.ptr[:-1]).tolist()
        groups = (4, sum(-(-s // 4) for s in sizes))
    else:
        ei, n = hand_edges(), N_HAND
        groups = {"hand": (4, -(-n // 4)), "hand_r8": (8, -(-n // 8))}.get(kind)
    deg = torch.bincount(ei[1], minlength=n)
    return ei, n, (deg > 64).nonzero().flatten(), groups


def host_hagg(ei, n, zl, heavy, skip_first=False):
    """the range rows' aggregates: fp64 sums of their z_l rows [a, e), rounded to f32 (skip_first: a
    mutation, the first row of each range is left out)"""
    out = torch.zeros(len(heavy), zl.size(1))
    for k, r in enumerate(heavy.tolist()):
        src = ei[0][ei[1] == r]
        a, e = int(src.min()), int(src.max()) + 1
        assert torch.equal(src, torch.arange(a, e))
        out[k] = zl[a + int(skip_first):e].to(D).sum(0).float()
    return out


def fwd_slots(n, heavy_slots, groups):
    """bgnn_sage_fwd_slots restated: the light rows' (row groups') grid -- one item per wave, at most
    1024 blocks, a multiple of 8 -- plus one slot per heavy row"""
    x = groups[1] if groups else n
    return max(8, (min(-(-x // 4), 1024) + 7) // 8 * 8) + heavy_slots
