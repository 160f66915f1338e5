"""bgnn_graph_loss_ex (kinds 3 ratio of sums, 4 mixed, 5 max component; kinds 0..2 with a device-side
multiplier) and bgnn_force_scale against fp64 restatements of the class formulas (bgnn/losses.py,
Utils/Losses.py:303-359, 403-443, 509-695), written out here, on the same float32 values; then the
five classes on the kernels, the switch, and one train_step per criterion.

Bounds (derived, not measured), u = 2^-24. The values the formulas see are the float32 denormalised
ones (v * scale + center as torch computes them; the kernel applies exactly that), so every bound
starts from the same float32 p, t. Sums are in double (no error at these sizes); the result is rounded
once and the multiplier applied in double: 2u |loss64| covers both.
  kind 3: |p - t| carries one rounding, |t| none: A_g is within u A_g, T_g exact:
          |loss - loss64| <= 3u |loss64|.
  kind 4: r = |p - t| / (|t| + eps) carries three roundings: |r32 - r64| <= 3u r64 (+ second order; 4u is
          used). An order statistic is 1-Lipschitz in the max norm, so the two selected values are off
          by at most 4u rmax_g, rmax_g the graph's largest r; the lerp adds three roundings of values
          <= rmax_g: |Q - Q64| <= 7u rmax_g. The MAE term has one rounding per element. With m = mult:
          |loss - loss64| <= m (0.2 * 7u mean_g rmax_g + 0.8 u mean_g mae_g) + 2u |loss64|.
          The restatement takes the rank q (n - 1) and the weight in float32, as the kernel and torch do.
  kind 5: three roundings in each selected term, all terms >= 0: |loss - loss64| <= 6u |loss64|.
  gradients: no cancellation; the divisor carries one rounding, the weight 1 - w one, the result one,
          the sum of the dense and the quantile part one: |dpred - dpred64| <= 1e-6 (|dense64| + |quantile64|)
          (1e-6 > 5u, the bound tests/test_gpu_graph_loss.py uses), and exactly 0 where the restatement is 0.
  bgnn_force_scale: a row norm over nc columns carries nc roundings under the root (halved by it)
          and the root's own: <= (nc / 2 + 1) u; the total is rounded once:
          |out - sum64| <= (nc / 2 + 2) u sum64.
Preconditions, asserted on the CPU: the f32 and fp64 signs of p - t agree; for kind 4 the f32 and fp64
orderings pick the same elements at ranks lo and lo + 1 (or both picks have p == t, whose gradient is 0)."""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
CASES = {
    # name: (graph sizes, shuffle the batch vector)
    "one_graph": ([37], False),
    "one_row_graphs": ([1, 5, 1, 300, 1], False),
    "long_graph": ([5003, 40], False),
    "b300": ([((7 * i) % 23) + 1 for i in range(300)], False),
    "unsorted": ([120, 1, 77, 300, 9], True),
}
QS = (0.0, 0.2, 0.9, 1.0)


def _inputs(sizes, C, seed, shuffle):
    """(pred, target, batch) on the CPU: graphs of the given row counts; C = 0 means a 1-D pred."""
    g = torch.Generator().manual_seed(seed)
    N = int(sum(sizes))
    shape = (N,) if C == 0 else (N, C)
    mag = torch.rand(shape, generator=g) * 1.5 + 0.5
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    target = mag * sign
    delta = (torch.rand(shape, generator=g) * 0.2 + 1e-3) * torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    pred = target * (1 + delta)
    same = torch.rand(N, generator=g) < 0.1   # rows with pred == target exactly
    pred[same] = target[same]
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    if shuffle:
        batch = batch[torch.randperm(N, generator=g)]
    return pred, target, batch


def _scaler(C):
    import bgnn
    cols = max(C, 1)
    return bgnn.ColumnScaler(center=[0.05 * (c + 1) for c in range(cols)], scale=[0.5 + 0.37 * c for c in range(cols)])


def _graph_elems(batch, B, C):
    """Per graph the flat indices row * C + c of its elements, ascending."""
    cols = torch.arange(C)
    return [((batch == g).nonzero().flatten()[:, None] * C + cols).flatten() for g in range(B)]


def _pick(r, idx, q):
    """torch.quantile's rank among the graph's elements (rank and weight in float32) and the elements
    picked at ranks lo and lo + 1 by the kernel's convention: of the elements that hold the selected
    value, the smallest flat index; the same value at both ranks: one element."""
    n = idx.numel()
    rank = np.float32(q) * np.float32(n - 1)
    lo = int(np.floor(rank))
    need_hi = int(np.ceil(rank)) > lo
    w = float(np.float32(rank - np.float32(lo)))
    v = r[idx]
    s, _ = torch.sort(v)
    e_lo = int(idx[(v == s[lo]).nonzero()[0, 0]])
    if not need_hi:
        return s[lo], s[lo], 0.0, e_lo, e_lo
    e_hi = int(idx[(v == s[lo + 1]).nonzero()[0, 0]])
    return s[lo], s[lo + 1], w, e_lo, e_hi


def _ref64(kind, p32, t32, batch, B, eps, q, m):
    """fp64 restatement on the float32 values p32, t32 (CPU). Returns loss, the two gradient parts
    (dense, sparse; with respect to the values the formula sees), the loss bound and the
    precondition flag."""
    C = 1 if p32.dim() == 1 else p32.size(1)
    p, t = p32.double().reshape(-1), t32.double().reshape(-1)
    d = p - t
    sg = torch.sign(d)
    ok = torch.equal(torch.sign((p32 - t32).reshape(-1)).double(), sg)
    elems = _graph_elems(batch, B, C)
    dense, sparse = torch.zeros_like(p), torch.zeros_like(p)
    eps = float(np.float32(eps))
    if kind in (1, 2):   # the per-graph means of |p - t| / |p^2 - t^2| (tests/test_gpu_graph_loss.py's bound)
        if kind == 2:
            d = p ** 2 - t ** 2
            sg = torch.sign(d)
            ok = torch.equal(torch.sign((p32 ** 2 - t32 ** 2).reshape(-1)).double(), sg)
        a = d.abs() if kind == 1 else p ** 2 + t ** 2
        loss = A = 0.0
        for idx in elems:
            loss += float(d[idx].abs().mean())
            A += float(a[idx].mean())
            dense[idx] = m / B / idx.numel() * sg[idx] * (2 * p[idx] if kind == 2 else 1.0)
        loss = m / B * loss
        return loss, dense, sparse, 4 * U * m / B * A + 2 * U * abs(loss), ok
    if kind == 3:
        loss = 0.0
        for idx in elems:
            T = t[idx].abs().sum() + 1e-8
            loss += float(d[idx].abs().sum() / T)
            dense[idx] = m / B * sg[idx] / T
        loss = m / B * loss
        return loss, dense, sparse, 3 * U * abs(loss), ok
    if kind == 4:
        r = d.abs() / (t.abs() + eps)
        r32 = ((p32 - t32).abs() / (t32.abs() + np.float32(eps))).reshape(-1)
        qsum = maesum = rmax = 0.0
        for idx in elems:
            a, b, w, e_lo, e_hi = _pick(r, idx, q)
            _, _, w32, f_lo, f_hi = _pick(r32, idx, q)
            ok = ok and w == w32 and all(e == f or (d[e] == 0 and d[f] == 0) for e, f in ((e_lo, f_lo), (e_hi, f_hi)))
            qsum += float(a + w * (b - a))
            maesum += float(d[idx].abs().mean())
            rmax += float(r[idx].max())
            dense[idx] = 0.8 * m / B / idx.numel() * sg[idx]
            for e, wt in ((e_lo, 1.0 - w), (e_hi, w)) if e_hi != e_lo else ((e_lo, 1.0),):
                sparse[e] += 0.2 * m / B * wt * sg[e] / (t[e].abs() + eps)
        loss = m * (0.2 / B * qsum + 0.8 / B * maesum)
        bound = m * (0.2 * 7 * U * rmax / B + 0.8 * U * maesum / B) + 2 * U * abs(loss)
        return loss, dense, sparse, bound, ok
    assert kind == 5
    t2 = t.reshape(-1, C)
    loss = 0.0
    for g in range(B):
        rows = (batch == g).nonzero().flatten()
        for c in range(C):
            e = int(rows[torch.argmax(t2[rows, c].abs())]) * C + c   # (argmax: the first maximum)
            den = t[e].abs() + eps
            loss += float(d[e].abs() / den)
            sparse[e] = m / (B * C) * sg[e] / den
    loss = m / (B * C) * loss
    return loss, dense, sparse, 6 * U * abs(loss), ok


def _run(dev, kind, pred, target, batch, eps, scaler=None, **kw):
    from bgnn import losses
    p = pred.to(dev).requires_grad_(True)
    scale, center = scaler._at(dev) if scaler is not None else (None, None)
    loss = losses.graph_loss(kind, eps, p, target.to(dev), batch.to(dev), scale, center, **kw)
    assert loss is not None
    g, = torch.autograd.grad(loss, p)
    return loss.detach(), g


def _check(dev, tag, kind, pred, target, batch, B, eps, scaler, q=0.0, m=1.0):
    loss, g = _run(dev, kind, pred, target, batch, eps, scaler, q=q, mult=m)
    again, g2 = _run(dev, kind, pred, target, batch, eps, scaler, q=q, mult=m)
    assert torch.equal(loss, again) and torch.equal(g, g2), tag   # bit-stable
    if scaler is not None:
        p32, t32 = scaler.denormalize(pred), scaler.denormalize(target)
        chain = scaler.scale.double().repeat(pred.size(0)) if pred.dim() == 2 else scaler.scale.double()
    else:
        p32, t32, chain = pred, target, 1.0
    loss64, dense, sparse, bound, ok = _ref64(kind, p32, t32, batch, B, eps, q, m)
    assert ok, tag   # the preconditions hold on these inputs (a CPU check of the restatement itself)
    err = abs(loss.item() - loss64)
    print(f"{tag}: loss {loss.item():.9g} fp64 {loss64:.12g} err {err:.3g} bound {bound:.3g}")
    assert err <= bound, (tag, err, bound)
    dense, sparse = dense * chain, sparse * chain
    gd = g.double().cpu().reshape(-1)
    gerr = (gd - (dense + sparse)).abs()
    gb = 1e-6 * (dense.abs() + sparse.abs())
    assert bool((gerr <= gb).all()), (tag, float((gerr - gb).max()))
    if kind == 5:   # exactly zero off the B C selected elements
        assert int((gd != 0).sum()) <= B * max(pred.dim() == 2 and pred.size(1), 1)
        assert bool((gd[sparse == 0] == 0).all())
    return loss, g


@pytest.mark.parametrize("with_scaler", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("C", [0, 3, 6])
@pytest.mark.parametrize("name", list(CASES))
def test_kinds_match_fp64(dev, name, C, with_scaler):
    sizes, shuffle = CASES[name]
    pred, target, batch = _inputs(sizes, C, 11 + C, shuffle)
    B = len(sizes)
    scaler = _scaler(C) if with_scaler else None
    tag = f"{name} C={C} scaled={with_scaler}"
    _check(dev, tag + " kind=3", 3, pred, target, batch, B, 0.0, scaler, m=100.0)
    for q in QS:
        for eps in ((1e-8, 0.1) if q == 0.2 else (1e-8,)):
            _check(dev, tag + f" kind=4 q={q} eps={eps}", 4, pred, target, batch, B, eps, scaler, q=q, m=1.0)
    _check(dev, tag + " kind=5", 5, pred, target, batch, B, 1e-8, scaler, m=10000.0)


def test_kinds_0_to_2_equal_bgnn_graph_loss(dev, monkeypatch):
    """Through the new entry point with mult_dev = None: the same bits as bgnn_graph_loss; with a
    device multiplier: the same loss and gradient times it (one more rounding each)."""
    from bgnn import _lib
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    md = torch.tensor([2.5], device=dev)
    for name in ("long_graph", "unsorted", "b300"):
        sizes, shuffle = CASES[name]
        for C in (0, 3):
            pred, target, batch = _inputs(sizes, C, 5, shuffle)
            scaler = _scaler(C)
            for kind in (0, 1, 2):
                n = len(calls)
                want, gw = _run(dev, kind, pred, target, batch, 0.1, scaler)
                got, gg = _run(dev, kind, pred, target, batch, 0.1, scaler, mult=10000.0)
                assert [c for c in calls[n:] if "graph_loss" in c] == ["bgnn_graph_loss", "bgnn_graph_loss_ex"]
                assert torch.equal(want, got) and torch.equal(gw, gg), (name, C, kind)
                sc, gs = _run(dev, kind, pred, target, batch, 0.1, scaler, mult=4000.0, mult_dev=md)
                assert abs(sc.item() - want.item()) <= 3 * U * abs(want.item())   # 4000 * 2.5 = 10000
                assert bool(((gs - gw).abs() <= 3 * U * gw.abs()).all())


def test_kind5_ties_take_the_first_row_in_any_row_order(dev):
    """Several rows hold the largest |target| of a column: the smallest row index takes the gradient,
    also when the graph's rows are not contiguous in the batch vector (a second graph's row in
    between) and when the rows come in the opposite order (then another physical row is first)."""
    target = torch.tensor([[1.0, -3.0], [-2.0, 3.0], [2.0, 0.5], [0.1, 0.2], [2.0, -3.0]])
    pred = target + torch.tensor([[0.1, 0.2], [0.3, -0.1], [-0.2, 0.1], [0.1, 0.1], [0.5, 0.5]])
    # column 0: |t| = 2 at rows 1, 2, 4 -> row 1; column 1: |t| = 3 at rows 0, 1, 4 -> row 0
    for batch in (torch.tensor([0, 0, 0, 0, 0]), torch.tensor([0, 0, 0, 1, 0])):
        _, g = _run(dev, 5, pred, target, batch, 1e-8)
        g = g.cpu()
        assert g[1, 0] != 0 and g[0, 1] != 0
        assert g[2, 0] == 0 and g[4, 0] == 0 and g[1, 1] == 0 and g[4, 1] == 0
        assert int((g != 0).sum()) == 2 * (int(batch.max()) + 1)   # (graph 1: its one row, both columns)
    # rows reversed: old row 4 is row 0 now and holds both maxima first
    _, g = _run(dev, 5, pred.flip(0), target.flip(0), torch.zeros(5, dtype=torch.long), 1e-8)
    g = g.cpu()
    assert g[0, 0] != 0 and g[0, 1] != 0 and int((g != 0).sum()) == 2


def test_kind4_ties_go_to_the_smallest_flat_index(dev):
    """A duplicated selected value: its whole weight sits on the smallest flat index. Nine elements
    (t = 1, eps = 0, so r = p - t exactly) with r * 8 = [5, 2, 2, 8, 1, 2, 7, 6, 9]: sorted
    [1, 2, 2, 2, 5, 6, 7, 8, 9] at indices [4, 1, 2, 5, 0, 7, 6, 3, 8]; the ranks q * 8 below are exact."""
    r = torch.tensor([5.0, 2.0, 2.0, 8.0, 1.0, 2.0, 7.0, 6.0, 9.0]) / 8
    for shape in ((9,), (3, 3)):
        t = torch.ones(shape)
        p = t + r.reshape(shape)
        b = torch.zeros(shape[0], dtype=torch.long)
        for q, elems in ((0.25, {1: 1.0}),             # rank 2: the value 2, copies at 1, 2, 5 -> index 1
                         (0.1875, {1: 1.0}),           # rank 1.5: ranks 1 and 2 hold the same value: weight 1
                         (0.0625, {4: 0.5, 1: 0.5}),   # rank 0.5: rank 0 (index 4) and rank 1 (the value 2 -> index 1)
                         (0.4375, {1: 0.5, 0: 0.5})):  # rank 3.5: rank 3 (the value 2 -> index 1) and rank 4 (index 0)
            _, g = _run(dev, 4, p, t, b, 0.0, q=q)
            g = g.double().cpu().reshape(-1)
            for e in range(9):
                want = 0.8 / 9 + 0.2 * elems.get(e, 0.0)
                assert abs(float(g[e]) - want) <= 1e-6 * want, (shape, q, e, float(g[e]), want)


def test_force_scale_matches_fp64(dev):
    from bgnn import losses
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5003, 16, generator=g)
    x[:, -1] = (torch.rand(5003, generator=g) < 0.1).float()
    xd = x.to(dev)

    def want(v, c0, nc, flag):
        rows = v.double()
        if flag is not None:
            rows = rows[rows[:, flag] == 0]
        return float(rows[:, c0:c0 + nc].pow(2).sum(1).sqrt().sum())

    for c0, nc, flag in ((3, 2, None), (3, 2, 15), (0, 8, 15), (5, 1, None)):
        out = losses.force_scale(xd, 0.1, flag, c0, nc)
        again = losses.force_scale(xd, 0.1, flag, c0, nc)
        assert out.shape == (1,) and torch.equal(out, again)   # bit-stable
        s = want(x, c0, nc, flag)
        assert abs(out.item() - s) <= (nc / 2 + 2) * U * s, (c0, nc, flag, out.item(), s)
    # a strided column slice of a wider matrix: the row stride is the parent's
    wide = torch.randn(300, 40, generator=g).to(dev)
    view = wide[:, 8:24]
    assert not view.is_contiguous()
    s = want(view.cpu(), 3, 2, None)
    assert abs(losses.force_scale(view, 0.1).item() - s) <= 3 * U * s
    # the clamp: small forces, and every row flagged
    small = xd * 1e-6
    assert losses.force_scale(small, 0.1).item() == np.float32(0.1)
    flagged = xd.clone()
    flagged[:, -1] = 1
    assert losses.force_scale(flagged, 0.25, 15).item() == 0.25
    # outside the cover
    assert losses.force_scale(x, 0.1) is None and losses.force_scale(xd.double(), 0.1) is None
    assert losses.force_scale(xd[:, :4], 0.1) is None


GOLD = os.path.join(os.path.dirname(__file__), "golden", "heads", "losses_scaled.npz")
NEW = {"mixed": ("GraphMixedError", 4), "maxc": ("GraphMaxComponentRelativeError", 5),
       "mae_scaled": ("ScaledGraphMAELoss", 1), "mse_scaled": ("ScaledGraphMSELoss", 2),
       "rel_scaled": ("ScaledGraphRELoss", 3)}


def _spy(monkeypatch):
    from bgnn import _lib
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a)), orig(name, *a))[1])
    return calls


def _names(calls):
    """The loss entry points among the recorded calls (the segment index of a new batch vector is
    built through the library too)."""
    return [c[0] for c in calls if c[0] in ("bgnn_graph_loss", "bgnn_graph_loss_ex", "bgnn_force_scale")]


def test_classes_take_the_kernels_and_match_the_reference_golden(dev, monkeypatch):
    """The five classes on the GPU go through bgnn_graph_loss_ex (the force-scaled ones through
    bgnn_force_scale too) and reproduce the reference's own values and gradients
    (tests/golden/heads/losses_scaled.npz) at tests/test_losses_scaled.py's rel=2e-5."""
    from bgnn import losses
    gold = np.load(GOLD)
    calls = _spy(monkeypatch)
    n = 0
    for tag in ("s3", "d3", "v1", "m3"):
        p, t, b, x = (torch.from_numpy(gold[f"{tag}_{k}"]).to(dev) for k in ("pred", "target", "batch", "x"))
        for name, (cls, _) in NEW.items():
            for suffix, kw in (("", {}), ("_noforce", {"force_scaling": False})) if "scaled" in name else (("", {}),):
                before = len(calls)
                pr = p.clone().requires_grad_(True)
                v = getattr(losses, cls)(**kw)(pr, t, b, x)
                g, = torch.autograd.grad(v, pr)
                want = ["bgnn_force_scale"] if "scaled" in name and not kw else []
                assert _names(calls[before:]) == want + ["bgnn_graph_loss_ex"], (tag, name, suffix)
                key = f"{tag}_{name}{suffix}"
                assert v.item() == pytest.approx(float(gold[key]), rel=2e-5), key
                np.testing.assert_allclose(g.cpu().numpy(), gold[key + "_grad"], rtol=2e-5, atol=0, err_msg=key)
                n += 1
                # without a batch vector: the torch formula, no kernel
                before = len(calls)
                v = getattr(losses, cls)(**kw)(p, t, None, x)
                assert v.item() == pytest.approx(float(gold[key + "_nobatch"]), rel=2e-5), key
                assert _names(calls[before:]) == []
    assert n == 4 * 8


@pytest.mark.parametrize("name", list(NEW))
def test_switch_off_gives_the_torch_value(dev, monkeypatch, name):
    """FUSED_GRAPH_LOSS = False (or the name taken out of FUSED_CRITERIA): the class runs its torch
    code; value and gradient agree with the kernel's within the bounds above (both sit that close to
    the fp64 value; the torch sums are f32 and atomic: n_max * u relative is allowed for them)."""
    from bgnn import losses
    cls, kind = NEW[name]
    sizes, shuffle = CASES["unsorted"]
    pred, target, batch = _inputs(sizes, 3, 5, shuffle)
    B = len(sizes)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(pred.size(0), 16, generator=g)
    mod = getattr(losses, cls)()
    out = []
    cname = losses._CRITERION_NAMES[getattr(losses, cls)]
    every = set(losses._CRITERION_NAMES.values())
    for setting in ("on", "off", "name_off"):
        monkeypatch.setattr(losses, "FUSED_GRAPH_LOSS", setting != "off")
        monkeypatch.setattr(losses, "FUSED_CRITERIA", every - {cname} if setting == "name_off" else every)
        p = pred.to(dev).requires_grad_(True)
        loss = mod(p, target.to(dev), batch.to(dev), x.to(dev))
        gr, = torch.autograd.grad(loss, p)
        out.append((loss.item(), gr.double().cpu().reshape(-1)))
    force = float(x[:, 3:5].double().pow(2).sum(1).sqrt().sum())
    m = {4: 1.0, 5: 10000.0}.get(kind, 100.0 * force)
    l64, dense, sparse, bound, ok = _ref64(kind, pred, target, batch, B, getattr(mod, "epsilon", 0.0),
                                           getattr(mod, "percentile", 0.0), m)
    assert ok
    gabs = dense.abs() + sparse.abs()
    bound += 4 * U * abs(l64)   # the force scale's own error, (nc / 2 + 2) u
    n_max = max(sizes) * 3
    assert abs(out[0][0] - l64) <= bound, (out[0][0], l64, bound)
    for loss_t, g_t in out[1:]:
        assert abs(loss_t - l64) <= bound + n_max * U * abs(l64)
        assert bool(((out[0][1] - g_t).abs() <= 2 * (1e-6 + 4 * U) * gabs + n_max * U * gabs).all())


def test_declines_and_empty_graph_ids(dev, monkeypatch):
    """Outside the kernels' cover graph_loss returns None (the classes then run torch); a graph id
    without rows gives NaN on the kernel and on the torch route (kind 3: 0 / 1e-8 = 0 from that graph,
    as the torch expression; kind 5's torch route indexes past the end for such a graph, undefined
    in the reference too, and is not run)."""
    from bgnn import losses
    p = torch.randn(10, 3, device=dev)
    b = torch.zeros(10, dtype=torch.long, device=dev)
    for kind in (3, 4, 5):
        assert losses.graph_loss(kind, 1e-8, p, p.clone(), b, q=0.2) is not None
        assert losses.graph_loss(kind, 1e-8, p, p.clone(), None) is None
        assert losses.graph_loss(kind, 1e-8, p.double(), p.double(), b) is None
        assert losses.graph_loss(kind, 1e-8, p.cpu(), p.cpu(), b.cpu()) is None
        assert losses.graph_loss(kind, 1e-8, p, p.clone(), b, mult_dev=torch.ones(1)) is None   # a CPU scalar
    assert losses.graph_loss(4, 1e-8, p, p.clone(), b, q=1.5) is None
    assert losses.graph_loss(6, 1e-8, p, p.clone(), b, mult=1.0) is None
    w = torch.randn(10, 9, device=dev)
    assert losses.graph_loss(4, 1e-8, w, w.clone(), b, q=0.2) is None
    x = torch.randn(10, 16, device=dev)
    assert losses.ScaledGraphRELoss()(w, w + 1, b, x).item() > 0   # C = 9: torch
    assert losses.GraphMixedError()(w, w + 1, b, None).item() > 0

    p = torch.rand(6, 2, device=dev) + 1
    t = torch.rand(6, 2, device=dev) + 1
    b = torch.tensor([0, 0, 2, 2, 2, 0], device=dev)   # graph 1 has no rows
    x = torch.randn(6, 16, device=dev)
    mods = [losses.GraphMixedError(), losses.ScaledGraphMAELoss(), losses.ScaledGraphMSELoss(),
            losses.ScaledGraphRELoss()]
    got = [m(p, t, b, x) for m in mods] + [losses.GraphMaxComponentRelativeError()(p, t, b, x)]
    monkeypatch.setattr(losses, "FUSED_GRAPH_LOSS", False)
    want = [m(p, t, b, x) for m in mods]
    for m, a, c in zip(mods, got, want):
        if type(m) is losses.ScaledGraphRELoss:
            assert torch.isfinite(a) and a.item() == pytest.approx(c.item(), rel=1e-5)
        else:
            assert torch.isnan(a) and torch.isnan(c), type(m).__name__
    assert torch.isnan(got[-1])


def _node_batch(dev, seed=0):
    """Six 19 x 19 meshes with super nodes (2,172 nodes) and a static_disp y: one row per real node."""
    from bgnn import synthetic
    b = synthetic.make_batch(19, 6, super_node=True, seed0=seed)
    g = torch.Generator().manual_seed(seed + 77)
    n_real = int((b.x[:, -1] == 0).sum())
    y = torch.rand(n_real, 2, generator=g) * 1.5 + 0.5
    b.y = y * torch.where(torch.rand(y.shape, generator=g) < 0.5, -1.0, 1.0)
    return b.to(dev)


@pytest.mark.parametrize("name", list(NEW))
def test_train_step_fused_against_torch_route(dev, monkeypatch, name):
    """One SGD train_step of a small static_disp model (h = 64, super-node pooling, ColumnScaler) with
    each criterion, the switch on and off, from the same state.
    Losses: both routes are within the loss bound above of the fp64 value of the same prediction (the
    forward is the same kernels on both routes), so they differ by at most twice that; the bound's
    terms are all <= 7u times sums of the positive terms that make up the loss or its MAE part, and
    the torch sums are f32: |on - off| <= (2 * 7u + n_max u) * |loss|, n_max the largest graph's elements.
    Parameters: p' = p - lr * g. The two dpred differ by <= 2e-6 relative elementwise (the gradient
    bound above, both routes against fp64); the backward is the same deterministic f32 kernels, whose
    own rounding this suite bounds at 2e-3 of a tensor's gradient scale (tests/test_gpu_model.py:86-97),
    once per route: |p'_on - p'_off| <= lr * 4e-3 * max|g| + 2 * 2^-24 * max|p'| per tensor.
    The fused route reads no device scalar back (torch.Tensor.item is not called on a GPU tensor; the
    model's host-side dropout seeds are CPU tensors and do not count) and calls bgnn_force_scale
    on the unfiltered x with the flag column instead of gathering the real nodes' rows."""
    import bgnn
    from bgnn import losses
    cls, kind = NEW[name]
    b = _node_batch(dev, seed=3)
    scaler = bgnn.ColumnScaler(center=[0.1, 0.2], scale=[0.8, 1.1])
    torch.manual_seed(1)
    model = bgnn.BuckGNN(16, 5, hidden_channels=64, num_layers=3, pooling_layer="supernode_only",
                         prediction_type="static_disp", dropout_rate=0.0, model_name="GraphSage_addAggr").to(dev).train()
    state = copy.deepcopy(model.state_dict())
    crit = getattr(losses, cls)()
    lr = 1e-3
    res = {}
    calls = _spy(monkeypatch)
    orig_item = torch.Tensor.item

    def step(criterion):
        """One train_step from the saved state; the loss, the library calls and the number of device
        scalars read back with .item() during it."""
        model.load_state_dict(state)
        opt = torch.optim.SGD(model.parameters(), lr=lr)
        items = []
        before = len(calls)
        with monkeypatch.context() as mp:
            mp.setattr(torch.Tensor, "item",
                       lambda self: (items.append(1) if self.is_cuda else None, orig_item(self))[1])
            loss = bgnn.train_step(model, b, opt, criterion, scaler)
        return loss, calls[before:], len(items)

    step(losses.GraphMAELoss())   # (builds the batch's graph structures, which reads their plan counts back once)
    for on in (True, False):
        monkeypatch.setattr(losses, "FUSED_GRAPH_LOSS", on)
        loss, step_calls, items = step(crit)
        names = _names(step_calls)
        print(f"{name} fused={on}: device .item() calls {items}")
        if on:
            assert items == 0, name
            assert names.count("bgnn_graph_loss_ex") == 1 and names.count("bgnn_graph_loss") == 0
            fs = [a for n_, a in step_calls if n_ == "bgnn_force_scale"]
            assert len(fs) == (1 if "scaled" in name else 0)
            for a in fs:   # (x, N, ldx, c0, nc, flag_col, ...): every row of batch.x, the flag column named
                assert a[1] == b.x.size(0) and a[2] == b.x.size(1) and a[3:6] == (3, 2, b.x.size(1) - 1)
        else:
            assert "bgnn_graph_loss_ex" not in names and "bgnn_force_scale" not in names
        res[on] = (loss.item(), {k: v.detach().clone() for k, v in model.named_parameters()})
    n_max = 361 * 2
    l_on, l_off = res[True][0], res[False][0]
    print(f"{name}: loss fused {l_on:.9g} torch {l_off:.9g}")
    assert abs(l_on - l_off) <= (14 * U + n_max * U) * abs(l_off), (name, l_on, l_off)
    for k, p_on in res[True][1].items():
        p_off = res[False][1][k]
        gmax = float((p_off - state[k]).abs().max()) / lr
        tol = lr * 4e-3 * gmax + 2 * U * float(p_off.abs().max())
        assert float((p_on - p_off).abs().max()) <= tol, (name, k, float((p_on - p_off).abs().max()), tol)


def test_evaluate_nodes_passes_x_to_the_criterion(dev, monkeypatch):
    """evaluate_nodes hands a force-scaled criterion the node features: on the kernels batch.x with the
    flag column named, on the torch route the rows without super nodes; either way the reported loss
    is the criterion's value on the model's denormalised prediction (the torch sums are f32 and
    atomic: (n_max + 14) u relative per route, as in the train-step test)."""
    import bgnn
    from bgnn import losses
    b = _node_batch(dev, seed=5)
    scaler = bgnn.ColumnScaler(center=[0.1, 0.2], scale=[0.8, 1.1])
    torch.manual_seed(2)
    model = bgnn.BuckGNN(16, 5, hidden_channels=64, num_layers=3, pooling_layer="supernode_only",
                         prediction_type="static_disp", dropout_rate=0.0, model_name="GraphSage_addAggr").to(dev)
    crit = losses.ScaledGraphMAELoss()
    calls = _spy(monkeypatch)
    got = bgnn.evaluate_nodes(model, [b], scaler, crit)["loss"]
    assert _names(calls).count("bgnn_force_scale") == 1 and _names(calls).count("bgnn_graph_loss_ex") == 1
    with torch.no_grad():
        pred, out_batch = model.eval()(b.x, b.edge_index, b.edge_attr, b.batch)
    monkeypatch.setattr(losses, "FUSED_GRAPH_LOSS", False)
    n = len(calls)
    want = crit(scaler.denormalize(pred), scaler.denormalize(b.y), out_batch, b.x[b.x[:, -1] == 0]).item()
    off = bgnn.evaluate_nodes(model, [b], scaler, crit)["loss"]
    assert _names(calls[n:]) == []
    tol = 2 * (361 * 2 + 14) * U * abs(want)
    assert want > 0 and abs(got - want) <= tol and abs(off - want) <= tol, (got, off, want)
