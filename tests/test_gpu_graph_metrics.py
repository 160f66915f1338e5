"""bgnn_graph_metrics (the per-graph error table of the static heads, bgnn.losses.graph_metrics)
against an oracle written out here: a per-graph loop over the float32 element values computed with
torch on the CPU, reductions in fp64, torch.quantile on the float32 values for the four quantiles.

The kernel's element values equal the oracle's bit for bit: v * scale + center (product rounded, sum
rounded), a = |t - p|, r = a / (|t| + 1e-8), t^2 - p^2 and, for static_disp, the row magnitude as the
sequential rounded sum of rounded squares with a correctly rounded root (`_norm_rows`: include/bgnn.h
defines it so; torch.norm itself rounds differently on the CPU and on the GPU). So the bounds are
derived, not measured:
* sum-type columns (mape, re, mae, mse, regional forms, std_mae): both sides sum the same values in
  double; a relative 1e-12 plus the two summation orders' own error, 2 n 2^-53, relative to the sum of
  the terms' magnitudes (rb below). re is a ratio of two such sums: 2 rb. std_mae is checked on its
  square, the variance: a mean off by rb * mean moves sum (a - mean)^2 / (n - 1) by at most about
  rb * mean^2, which is added;
* rmse on its square with the same bound; before that the oracle asserts that no per-graph
  mean(t^2 - p^2) lies within 1e-9 * mean(t^2 + p^2) of zero, so NaN-ness agrees exactly;
* maxima columns and max_mae: equal after conversion to double (first row of a tie wins);
* quantile columns: |got - torch.quantile| <= 2^-22 * max(|v_lo|, |v_hi|) with the two order
  statistics from a CPU sort (the restated f32 lerp and torch's differ by at most 1 ulp, from
  contraction; the bound gives 2), and bit-equal where the f32 rank 0.9f * (n - 1) is integral;
* counts exact; a NaN or an infinity in the oracle must be the same NaN / infinity in the table."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
THR = {0: 0.2, 1: 1e-4}
KIND = {0: "static_stress", 1: "static_disp"}
# column maps (include/bgnn.h): per region mape, re, rmse, mae, p90
REGION_COLS = {0: (9, 10, 11, 12, 13), 1: (14, 15, 16, 17, 18), 2: (19, 20, 21, 22, 24)}
MSE, MAX_MAE, STD, P90_ABS, N_HI, N_LO = 23, 25, 26, 27, 28, 29


def _norm_rows(v):
    """sqrt(sum_c v_c^2) per row of a float32 [n, C] tensor: squares and sums rounded one by one in
    column order, the root correctly rounded."""
    acc = v[:, 0] * v[:, 0]
    for c in range(1, v.size(1)):
        acc = acc + v[:, c] * v[:, c]
    # (numpy's float32 sqrt is the correctly rounded one; torch.sqrt on the CPU is off by an ulp for
    # some float32 inputs, e.g. 1.1599200661294162e-05)
    return torch.from_numpy(np.sqrt(acc.numpy()))


def _quantile(vals):
    """(torch.quantile(vals, 0.9) as a double, the absolute bound, whether the f32 rank is integral)."""
    q = torch.quantile(vals, 0.9).item()
    if np.isnan(q):
        return q, 0.0, False
    vs = torch.sort(vals).values
    rank = np.float32(0.9) * np.float32(vals.numel() - 1)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    if lo == hi:
        assert q == vs[lo].item()
        return q, 0.0, True
    return q, 2.0 ** -22 * max(abs(vs[lo].item()), abs(vs[hi].item())), False


def _oracle(p, t, batch, B, mode, thr):
    """p, t: the float32 values the formulas see (already denormalised), on the CPU. Returns
    (want [B, 30], tol [B, 30] absolute, square [B, 30]: for the rmse / std columns the value whose
    root `want` is, checked on the square; n_exact: how many quantiles had an integral rank)."""
    C = t.size(1)
    thr32 = torch.tensor(thr, dtype=torch.float32)
    want = np.full((B, 30), np.nan)
    tol = np.zeros((B, 30))
    square = np.full((B, 30), np.nan)
    n_exact = 0
    for g in range(B):
        rows = torch.nonzero(batch == g).flatten()   # ascending row index
        if rows.numel() == 0:
            want[g, N_HI:] = 0
            continue
        tg, pg = t[rows], p[rows]
        a = (tg - pg).abs()
        r = a / (tg.abs() + 1e-8)
        sq = tg ** 2 - pg ** 2
        trip = []
        if mode == 1:
            mag = _norm_rows(tg)
            i = int(torch.argmax(mag))
            err = _norm_rows(a[i:i + 1])[0]
            trip.append((mag[i], err, err / (mag[i] + 1e-8) * 100))
            comps = (0, 1)
            hi = (mag >= thr32)[:, None].expand_as(tg)
        else:
            comps = (0, 1, 2)
            hi = tg.abs() >= thr32
        for c in comps:
            i = int(torch.argmax(tg[:, c].abs()))   # the first of several maxima
            trip.append((tg[i, c].abs(), a[i, c], r[i, c] * 100))
        for k, (v, e, rl) in enumerate(trip):
            want[g, 3 * k:3 * k + 3] = v.item(), e.item(), rl.item()
        for ri, m in enumerate((hi, ~hi, torch.ones_like(hi))):
            cm, cr, crm, cma, cq = REGION_COLS[ri]
            n = int(m.sum())
            if ri < 2:
                want[g, N_HI + ri] = n
            if n == 0:
                want[g, [cm, cr, crm, cma, cq]] = 0
                continue
            am, rm, tm, sm = a[m].double(), r[m].double(), tg[m].abs().double(), sq[m].double()
            rb = 1e-12 + 2 * n * 2.0 ** -53
            want[g, cm] = (rm.sum() / n * 100).item()
            tol[g, cm] = rb * abs(want[g, cm])
            want[g, cr] = (am.sum() / tm.sum() * 100).item()
            tol[g, cr] = 2 * rb * abs(want[g, cr])
            want[g, cma] = (am.sum() / n).item()
            tol[g, cma] = rb * abs(want[g, cma])
            mean_sq = (sm.sum() / n).item()
            scale_sq = ((tg[m] ** 2).double().sum() + (pg[m] ** 2).double().sum()).item() / n
            # the sign of the mean is not in doubt, so sqrt's NaN-ness must agree exactly
            assert not np.isfinite(mean_sq) or abs(mean_sq) > 1e-9 * scale_sq, (g, ri, mean_sq, scale_sq)
            square[g, crm] = mean_sq
            want[g, crm] = np.sqrt(mean_sq) if not mean_sq < 0 else np.nan
            tol[g, crm] = rb * (sm.abs().sum() / n).item()
            if ri == 2:
                want[g, MSE], tol[g, MSE] = mean_sq, tol[g, crm]
            q, qb, exact = _quantile(r[m])
            n_exact += exact
            want[g, cq], tol[g, cq] = q * 100, qb * 100
        n = tg.numel()
        ad = a.double().flatten()
        rb = 1e-12 + 2 * n * 2.0 ** -53
        want[g, MAX_MAE] = a.max().item()
        mean = ad.sum() / n
        var = (((ad - mean) ** 2).sum() / torch.tensor(float(n - 1), dtype=torch.float64)).item()   # n = 1: NaN
        square[g, STD], want[g, STD] = var, np.sqrt(var)
        tol[g, STD] = rb * (abs(var) + mean.item() ** 2) if np.isfinite(var) else 0.0
        q, qb, exact = _quantile(a.flatten())
        n_exact += exact
        want[g, P90_ABS], tol[g, P90_ABS] = q, qb
    return want, tol, square, n_exact


def _compare(got, want, tol, square, tag):
    got = got.cpu().numpy()
    assert got.shape == want.shape
    for g in range(want.shape[0]):
        for c in range(30):
            w, x = want[g, c], got[g, c]
            if np.isnan(w):
                assert np.isnan(x), (tag, g, c, x)
            elif np.isinf(w):
                assert x == w, (tag, g, c, x, w)
            elif not np.isnan(square[g, c]):
                assert abs(x * x - square[g, c]) <= tol[g, c], (tag, g, c, x * x, square[g, c], tol[g, c])
            else:
                assert abs(x - w) <= tol[g, c], (tag, g, c, x, w, tol[g, c])


def _inputs(sizes, C, mode, seed, shuffle):
    """(pred, target, batch) on the CPU: graphs of the given row counts, |target| spread over two
    decades around the mode's threshold, pred = target * (1 + delta) with 1e-3 <= |delta| <= 0.2, a
    tenth of the rows of the larger graphs with pred == target (zeros among the errors: ties at the
    bottom)."""
    g = torch.Generator().manual_seed(seed)
    N = int(sum(sizes))
    sign = torch.where(torch.rand(N, C, generator=g) < 0.5, -1.0, 1.0)
    mag = (torch.rand(N, C, generator=g) * 0.9 + 0.1) * torch.pow(10.0, torch.rand(N, 1, generator=g) * 2 - 1.0)
    target = sign * mag * THR[mode] * 3
    delta = (torch.rand(N, C, generator=g) * 0.2 + 1e-3) * torch.where(torch.rand(N, C, generator=g) < 0.5, -1.0, 1.0)
    pred = target * (1 + delta)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    if shuffle:
        batch = batch[torch.randperm(N, generator=g)]
    # (not in graphs of fewer than 30 rows: a region of nothing but exact zeros has mean(t^2 - p^2) = 0)
    same = (torch.rand(N, generator=g) < 0.1) & (torch.tensor(sizes)[batch] >= 30)
    pred[same] = target[same]
    return pred, target, batch


CASES = {
    # name: (graph sizes, shuffle the batch vector)
    "one_graph": ([37], False),
    "one_row_graphs": ([1, 5, 1, 300, 1], False),
    "long_graph": ([20011, 40], False),
    "b300": ([((7 * i) % 23) + 1 for i in range(300)], False),
    "unsorted": ([120, 1, 77, 300, 9], True),
    # element counts n with n - 1 a multiple of 10 at C = 3 (21, 51, 111): an integral f32 rank
    "integral_rank": ([7, 17, 37], False),
}
MODE_C = [(0, 3), (0, 6), (1, 2), (1, 3), (1, 6)]


@functools.lru_cache(maxsize=None)
def _case(name, mode, C, with_scaler):
    """Inputs and the oracle's table of one case, computed once."""
    import bgnn
    sizes, shuffle = CASES[name]
    pred, target, batch = _inputs(sizes, C, mode, 100 + 10 * mode + C, shuffle)
    scaler = None
    p32, t32 = pred, target
    if with_scaler:
        # (centers well below the thresholds' scale would not move anything; these do)
        scaler = bgnn.ColumnScaler(center=[0.05 * THR[mode] * (c + 1) for c in range(C)],
                                   scale=[0.5 + 0.37 * c for c in range(C)])
        p32, t32 = scaler.denormalize(pred), scaler.denormalize(target)
    return pred, target, batch, scaler, _oracle(p32, t32, batch, len(sizes), mode, THR[mode])


def _table(dev, pred, target, batch, mode, scaler=None, thr=None):
    from bgnn import losses
    scale, center = scaler._at(dev) if scaler is not None else (None, None)
    out = losses.graph_metrics(pred.to(dev), target.to(dev), batch.to(dev), KIND[mode],
                               THR[mode] if thr is None else thr, scale, center)
    assert out is not None and out.dtype == torch.float64 and out.shape[1] == 30
    return out


@pytest.mark.parametrize("with_scaler", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("mode,C", MODE_C, ids=[f"{KIND[m]}-C{c}" for m, c in MODE_C])
@pytest.mark.parametrize("name", list(CASES))
def test_table_matches_the_oracle(dev, name, mode, C, with_scaler):
    pred, target, batch, scaler, (want, tol, square, n_exact) = _case(name, mode, C, with_scaler)
    got = _table(dev, pred, target, batch, mode, scaler)
    again = _table(dev, pred, target, batch, mode, scaler)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))   # bit-stable (NaNs included)
    _compare(got, want, tol, square, (name, mode, C, with_scaler))
    if name == "integral_rank" and C == 3:
        assert n_exact >= 6   # the all-element quantiles (rel and abs) of the three graphs: bit-equal
    assert bool((got[:, N_HI] + got[:, N_LO] == torch.bincount(batch, minlength=got.size(0)).to(dev) * C).all())


def _hand_made():
    """Tiny graphs for the select, mode 0 at C = 3 with target 0 (all elements low, a = |pred|
    exactly, r = |pred| / 1e-8f): every graph has 4 rows = 12 elements, so rank 0.9f * 11 = 9.9
    interpolates between sorted positions 9 and 10."""
    one = np.float32(1.0).view(np.uint32)
    sets = [
        [0.75] * 12,                                                          # all equal
        [1, 2, 3, 4, 5, 6, 7, 8, 9, 10.5, 10.5, 20],                           # a tie across ranks 9 and 10
        [1, 2, 3, 4, 5, 6, 7, 8, 9.5, 9.5, 11, 20],                            # the tie ends at rank 9
        [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12.5, 12.5],                           # the tie starts at rank 10
        list(np.array([one + k for k in (5, 0, 11, 3, 9, 1, 7, 2, 10, 4, 8, 6)], dtype=np.uint32).view(np.float32)),
        [0.0, 1e-45, 1e-40, 1e-38, 1.2e-38, 1e-20, 1e-5, 1.0, 3.0, 1e10, 1e20, float("inf")],
    ]
    g = torch.Generator().manual_seed(5)
    pred = torch.stack([torch.tensor(s, dtype=torch.float32)[torch.randperm(12, generator=g)] for s in sets])
    pred = pred.reshape(-1, 3)
    pred[::2] *= -1
    target = torch.zeros_like(pred)
    batch = torch.repeat_interleave(torch.arange(len(sets)), 4)
    # n = 1 and n = 2: graphs with exactly one / two high elements (0.5 >= 0.2) among low ones
    extra_t = torch.tensor([[0.5, 0.01, -0.02], [0.03, 0.01, 0.02],
                            [0.01, -0.7, 0.02], [0.9, 0.05, 0.01]])
    extra_p = extra_t * torch.tensor([[1.1, 0.9, 1.2], [0.8, 1.3, 0.7], [1.2, 0.6, 1.1], [0.75, 0.9, 1.3]])
    target = torch.cat([target, extra_t])
    pred = torch.cat([pred, extra_p])
    batch = torch.cat([batch, torch.tensor([6, 6, 7, 7])])
    return pred, target, batch, len(sets)


def test_selection_stress(dev):
    pred, target, batch, n_sets = _hand_made()
    B = n_sets + 2
    want, tol, square, _ = _oracle(pred, target, batch, B, 0, 0.2)
    got = _table(dev, pred, target, batch, 0)
    _compare(got, want, tol, square, "hand_made")
    g = got.cpu().numpy()
    assert (g[:n_sets, N_HI] == 0).all() and (g[:n_sets, N_LO] == 12).all()
    assert (g[:n_sets, 9:14] == 0).all()                        # no high elements: zeros
    assert g[0, P90_ABS] == 0.75 and g[1, P90_ABS] == 10.5      # ties: the value itself
    assert list(g[n_sets:, N_HI]) == [1, 2]                     # n = 1 and n = 2
    assert np.isfinite(g[:n_sets, P90_ABS]).all()
    assert np.isinf(g[n_sets - 1, MAX_MAE])                     # (the +inf sits above the two ranks)


def test_nan_prediction_stays_in_its_graph(dev):
    pred, target, batch = _inputs([30, 45, 12], 3, 0, 9, False)
    row = 30 + 7
    target[row, 1] = 0.9          # a high element
    pred[row, 1] = float("nan")
    want, tol, square, _ = _oracle(pred, target, batch, 3, 0, 0.2)
    got = _table(dev, pred, target, batch, 0)
    _compare(got, want, tol, square, "nan")
    g = got.cpu().numpy()
    hi_cols, lo_cols, all_cols = REGION_COLS[0], REGION_COLS[1], REGION_COLS[2]
    for c in (hi_cols[0], hi_cols[3], hi_cols[4], all_cols[0], all_cols[3], all_cols[4], MSE, MAX_MAE, STD, P90_ABS):
        assert np.isnan(g[1, c]), c
    # the low region holds no NaN (its rmse may be one of its own: the mean of t^2 - p^2 is signed)
    assert np.isfinite(g[1, [lo_cols[0], lo_cols[1], lo_cols[3], lo_cols[4]]]).all()
    assert np.isfinite(g[[0, 2]][:, [c for c in range(30) if c not in (11, 16, 21)]]).all()


def test_tie_of_the_maximum_takes_the_first_row(dev):
    for mode, C in ((0, 3), (1, 2)):
        pred, target, batch = _inputs([50, 64], C, mode, 21, True)
        rows = torch.nonzero(batch == 1).flatten()
        big = THR[mode] * 100
        first, later = int(rows[5]), int(rows[40])
        target[first] = torch.tensor([big, -big, big][:C])
        target[later] = target[first]
        pred[first] = target[first] * 1.25
        pred[later] = target[later] * 0.5
        want, tol, square, _ = _oracle(pred, target, batch, 2, mode, THR[mode])
        got = _table(dev, pred, target, batch, mode)
        _compare(got, want, tol, square, ("tie", mode))
        g = got.cpu().numpy()
        # max_*_mae of graph 1 comes from the first row (25 % off), not the later one (50 % off)
        k = 1 if mode == 0 else 4
        assert g[1, k] == float((target[first, 0] - pred[first, 0]).abs())


def test_empty_region_and_empty_graph(dev):
    pred, target, batch = _inputs([20, 33], 3, 0, 3, False)
    batch = batch * 2                                            # graph 1 has no rows
    got = _table(dev, pred, target, batch, 0, thr=1e6).cpu().numpy()   # nothing is high
    assert got.shape[0] == 3
    assert (got[[0, 2], 9:14] == 0).all() and (got[[0, 2], N_HI] == 0).all()
    assert list(got[[0, 2], N_LO]) == [60, 99]
    assert np.isnan(got[1, :28]).all() and (got[1, 28:] == 0).all()
    low = _table(dev, pred, target, batch, 0, thr=0.0).cpu().numpy()   # everything is high
    assert (low[[0, 2], 14:19] == 0).all() and (low[[0, 2], N_LO] == 0).all()
    # the high columns of one run are the low columns of the other, bit for bit
    assert np.array_equal(low[[0, 2], 9:14], got[[0, 2], 14:19], equal_nan=True)


def test_declines(dev):
    from bgnn import losses
    p = torch.randn(10, 3, device=dev)
    b = torch.zeros(10, dtype=torch.long, device=dev)
    assert losses.graph_metrics(p, p + 1, b, "static_stress", 0.2) is not None
    assert losses.graph_metrics(p, p + 1, None, "static_stress", 0.2) is None
    assert losses.graph_metrics(p.double(), p.double(), b, "static_stress", 0.2) is None
    assert losses.graph_metrics(p, p[:, :2], b, "static_stress", 0.2) is None
    assert losses.graph_metrics(p.cpu(), p.cpu(), b.cpu(), "static_stress", 0.2) is None
    assert losses.graph_metrics(p[:, :2], p[:, :2] + 1, b, "static_stress", 0.2) is None   # C = 2: disp only
    assert losses.graph_metrics(p[:, :2], p[:, :2] + 1, b, "static_disp", 1e-4) is not None
    w = torch.randn(10, 9, device=dev)
    assert losses.graph_metrics(w, w + 1, b, "static_disp", 1e-4) is None
    assert losses.graph_metrics(p, p + 1, b[:5], "static_stress", 0.2) is None
    d = losses.stress_errors(w, w + 1, b, "static_disp", 1e-4)   # C = 9: the torch code
    assert len(d) == 28 and d["mae"] == pytest.approx(1.0, rel=1e-5)
    with pytest.raises(NotImplementedError):
        losses.graph_metrics(p, p + 1, b, "buckling", 0.2)


def _spy(monkeypatch):
    from bgnn import _lib
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    return calls


def _same(d, ref, rel, tag):
    assert sorted(d) == sorted(ref), tag
    for k, v in ref.items():
        if np.isnan(v):
            assert np.isnan(d[k]), (tag, k, d[k])
        else:
            assert d[k] == pytest.approx(float(v), rel=rel, abs=1e-6), (tag, k, d[k], v)


@pytest.mark.parametrize("mode,C", [(0, 3), (1, 2), (1, 3)])
def test_switch_off_gives_the_torch_values(dev, monkeypatch, mode, C):
    """FUSED_STRESS_ERRORS = False runs the torch segment ops (no kernel call); with the switch on the
    values agree with them at tests/test_losses.py's tolerance, NaNs matching."""
    from bgnn import losses
    pred, target, batch = _inputs([120, 1, 77, 300, 9], C, mode, 31, True)
    # |pred| < |target| except in graph 2: no cancellation in any graph's sum of t^2 - p^2 (the torch
    # path takes it in f32), graph 2's is negative: every rmse key is NaN on both sides
    shrink = 1 - (pred - target).abs() / target.abs()
    pred = target * torch.where((batch == 2)[:, None], 2 - shrink, shrink)
    p, t, b = pred.to(dev), target.to(dev), batch.to(dev)
    calls = _spy(monkeypatch)
    on = losses.stress_errors(p, t, b, KIND[mode], THR[mode])
    assert calls.count("bgnn_graph_metrics") == 1
    monkeypatch.setattr(losses, "FUSED_STRESS_ERRORS", False)
    off = losses.stress_errors(p, t, b, KIND[mode], THR[mode])
    assert calls.count("bgnn_graph_metrics") == 1
    cpu = losses.stress_errors(pred, target, batch, KIND[mode], THR[mode])
    assert all(isinstance(v, float) for v in on.values())
    _same(off, cpu, 5e-5, "off-vs-cpu")
    _same(on, off, 5e-5, "on-vs-off")


def test_reference_golden_through_the_kernel(dev, monkeypatch):
    """The reference's own stress_errors values (tests/golden/heads/metrics.npz) through the kernel."""
    from bgnn import losses
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "heads", "metrics.npz"))
    calls = _spy(monkeypatch)
    for i, tag in enumerate(("stress", "disp")):
        p, t, b = (torch.from_numpy(gold[f"{tag}_{k}"]).to(dev) for k in ("pred", "target", "batch"))
        d = losses.stress_errors(p, t, b, str(gold[f"{tag}_kind"]), float(gold[f"{tag}_threshold"]))
        assert calls.count("bgnn_graph_metrics") == i + 1
        _same(d, dict(zip((str(k) for k in gold[f"{tag}_keys"]), gold[f"{tag}_vals"])), 5e-5, tag)
