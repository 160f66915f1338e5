"""bgnn_graph_loss (the per-graph-mean losses GraphRelativeError / GraphMAELoss / GraphMSELoss of the
node-level heads as one HIP kernel, loss and d loss / d pred together) against an fp64 restatement
of the class formulas (bgnn/losses.py, Utils/Losses.py:362-401, 445-507), written out here, on the
same float32 values.

Bounds (derived, not measured). The kernel computes the element term f in f32 with at most 4
roundings (difference, |t| + eps, quotient; squares and difference for kind 2), sums in double (no
error at these sizes) and rounds the result once:
    |loss - loss64| <= 4 * 2^-24 * A + 2^-23 * |loss64|,
with A the same per-graph-mean reduction applied to f (kinds 0, 1) or to p^2 + t^2 (kind 2: p^2 - t^2
cancels, each square carries one rounding of its own size). The gradient has no cancellation:
    |dpred - dpred64| <= 1e-6 * |dpred64|   (+ 4 * 2^-24 * |dpred64| for kind 2's factor 2p),
and is exactly 0 where pred == target (sign(0) = 0).
With a ColumnScaler the values the formula sees are the float32 denormalised ones, v * scale +
center as torch computes them (product rounded, sum rounded): the kernel applies exactly that, the
restatement starts from the same float32 values and the chain-rule factor scale[c] is applied to its
gradient in fp64.
The sign of p - t (of p^2 - t^2) must agree between f32 and fp64 for the gradient check to mean
anything: pred = target * (1 + delta) with |delta| >= 1e-3, plus a block with pred == target."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
MULT = 10000.0
KINDS = {0: "GraphRelativeError", 1: "GraphMAELoss", 2: "GraphMSELoss"}


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


def _ref64(kind, p32, t32, batch, B, eps):
    """fp64 restatement on float32 values p32, t32 (CPU): loss, d loss / d p, A, and the sign source."""
    p = p32.double().requires_grad_(True)
    t = t32.double()
    if kind == 0:
        d = p - t
        f = d.abs() / (t.abs() + float(np.float32(eps)))
        a = f
    elif kind == 1:
        d = p - t
        f = d.abs()
        a = f
    else:
        d = p ** 2 - t ** 2
        f = d.abs()
        a = p ** 2 + t ** 2
    C = 1 if p.dim() == 1 else p.size(1)
    cnt = torch.bincount(batch, minlength=B).double() * C

    def reduce(v):
        rows = v if v.dim() == 1 else v.sum(1)
        return (torch.zeros(B, dtype=torch.float64).index_add_(0, batch, rows) / cnt).mean() * MULT
    loss = reduce(f)
    g, = torch.autograd.grad(loss, p)
    return loss.detach(), g, reduce(a.detach()), d.detach()


def _run(dev, kind, pred, target, batch, eps, scaler=None):
    from bgnn import losses
    p = pred.to(dev).requires_grad_(True)
    t = target.to(dev)
    b = batch.to(dev)
    scale, center = scaler._at(dev) if scaler is not None else (None, None)
    loss = losses.graph_loss(kind, eps, p, t, b, scale, center)
    assert loss is not None
    g, = torch.autograd.grad(loss, p)
    return loss.detach(), g


CASES = {
    # name: (graph sizes, shuffle the batch vector)
    "one_graph": ([37], False),
    "one_row_graphs": ([1, 5, 1, 300, 1], False),
    "long_graph": ([5003, 40], False),
    "b300": ([((7 * i) % 23) + 1 for i in range(300)], False),
    "unsorted": ([120, 1, 77, 300, 9], True),
}


@pytest.mark.parametrize("with_scaler", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("eps", [0.1, 1e-8])
@pytest.mark.parametrize("C", [0, 3, 6])
@pytest.mark.parametrize("name", list(CASES))
def test_graph_loss_matches_fp64(dev, name, C, eps, with_scaler):
    import bgnn
    sizes, shuffle = CASES[name]
    pred, target, batch = _inputs(sizes, C, 11 + C, shuffle)
    B = len(sizes)
    scaler = None
    if with_scaler:
        cols = max(C, 1)
        scaler = bgnn.ColumnScaler(center=[0.05 * (c + 1) for c in range(cols)],
                                   scale=[0.5 + 0.37 * c for c in range(cols)])
    for kind in KINDS:
        if kind != 0 and eps != 0.1:
            continue   # (eps enters kind 0 only)
        loss, g = _run(dev, kind, pred, target, batch, eps, scaler)
        again, g2 = _run(dev, kind, pred, target, batch, eps, scaler)
        assert torch.equal(loss, again) and torch.equal(g, g2)   # bit-stable
        # the float32 values the formula sees (torch's own f32 denormalisation)
        if scaler is not None:
            p32, t32 = scaler.denormalize(pred), scaler.denormalize(target)
            chain = scaler.scale.double()
        else:
            p32, t32, chain = pred, target, None
        loss64, g64, A, d64 = _ref64(kind, p32, t32, batch, B, eps)
        # no sign flips between f32 and fp64 on these inputs (CPU check of the restatement itself)
        d32 = (p32 - t32) if kind != 2 else (p32 ** 2 - t32 ** 2)
        assert torch.equal(torch.sign(d32).double(), torch.sign(d64)), (name, kind)
        assert int((d64 == 0).sum()) > 0 or name == "one_graph"
        if chain is not None:
            g64 = g64 * chain
        err = abs(loss.item() - loss64.item())
        bound = 4 * 2.0 ** -24 * A.item() + 2.0 ** -23 * abs(loss64.item())
        print(f"{name} C={C} eps={eps} kind={kind} scaled={with_scaler}: loss {loss.item():.9g} "
              f"fp64 {loss64.item():.12g} err {err:.3g} bound {bound:.3g}")
        assert err <= bound, (name, kind, err, bound)
        gd = g.double().cpu()
        assert gd.shape == g64.shape
        gb = (1e-6 + (4 * 2.0 ** -24 if kind == 2 else 0.0)) * g64.abs()
        gerr = (gd - g64).abs()
        print(f"    grad max rel err {(gerr / g64.abs().clamp_min(1e-300)).max().item():.3g}")
        assert bool((gerr <= gb).all()), (name, kind, float((gerr - gb).max()))
        assert bool((gd[d64 == 0] == 0).all())   # sign(0) = 0, exactly


def test_classes_take_the_kernel_and_match_the_reference_golden(dev, monkeypatch):
    """The three bgnn.losses classes on the GPU go through bgnn_graph_loss and reproduce the
    reference's own values (tests/golden/heads/losses.npz) at tests/test_losses.py's rel=2e-5."""
    import os
    from bgnn import _lib, losses
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "heads", "losses.npz"))
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), orig(name, *a))[1])
    mods = {"rel": losses.GraphRelativeError, "mse": losses.GraphMSELoss, "mae": losses.GraphMAELoss}
    n = 0
    for tag in ("s3", "d3", "v1"):
        p, t, b = (torch.from_numpy(gold[f"{tag}_{k}"]).to(dev) for k in ("pred", "target", "batch"))
        for name, cls in mods.items():
            before = calls.count("bgnn_graph_loss")
            got = cls()(p, t, b, None).item()
            assert calls.count("bgnn_graph_loss") == before + 1, (tag, name)
            assert got == pytest.approx(float(gold[f"{tag}_{name}"]), rel=2e-5), (tag, name)
            n += 1
            # without a batch vector: the torch formula, no kernel
            before = calls.count("bgnn_graph_loss")
            assert cls()(p, t, None, None).item() == pytest.approx(float(gold[f"{tag}_{name}_nobatch"]), rel=2e-5)
            assert calls.count("bgnn_graph_loss") == before
    assert n == 9


@pytest.mark.parametrize("kind", list(KINDS))
def test_switch_off_gives_the_torch_value(dev, monkeypatch, kind):
    """FUSED_GRAPH_LOSS = False: the class runs its torch code; value and gradient agree with the
    kernel's within the two bounds above (both sit that close to the fp64 value; the torch sums are
    f32 and atomic, so their own error is allowed for at the f32 sum bound N * 2^-24)."""
    from bgnn import losses
    sizes, shuffle = CASES["unsorted"]
    pred, target, batch = _inputs(sizes, 3, 5, shuffle)
    cls = getattr(losses, KINDS[kind])
    out = []
    for on in (True, False):
        monkeypatch.setattr(losses, "FUSED_GRAPH_LOSS", on)
        p = pred.to(dev).requires_grad_(True)
        loss = cls()(p, target.to(dev), batch.to(dev), None)
        g, = torch.autograd.grad(loss, p)
        out.append((loss.item(), g.double().cpu()))
    loss64, g64, A, _ = _ref64(kind, pred, target, batch, len(sizes), getattr(cls(), "epsilon", 0.0))
    bound = 4 * 2.0 ** -24 * A.item() + 2.0 ** -23 * abs(loss64.item())
    n_max = max(sizes) * 3
    assert abs(out[0][0] - loss64.item()) <= bound
    assert abs(out[1][0] - loss64.item()) <= bound + n_max * 2.0 ** -24 * abs(loss64.item())
    assert bool(((out[0][1] - out[1][1]).abs() <= 2 * (1e-6 + 4 * 2.0 ** -24) * g64.abs()).all())


def test_declines(dev):
    """Calls outside the kernel's cover return None from graph_loss (the classes then run torch)."""
    from bgnn import losses
    p = torch.randn(10, 3, device=dev)
    b = torch.zeros(10, dtype=torch.long, device=dev)
    assert losses.graph_loss(0, 0.1, p, p.clone(), b) is not None
    assert losses.graph_loss(0, 0.1, p, p.clone(), None) is None
    assert losses.graph_loss(0, 0.1, p.double(), p.double(), b) is None
    assert losses.graph_loss(0, 0.1, p, p[:, :2], b) is None
    assert losses.graph_loss(0, 0.1, p.cpu(), p.cpu(), b.cpu()) is None
    w = torch.randn(10, 9, device=dev)
    assert losses.graph_loss(0, 0.1, w, w.clone(), b) is None
    assert losses.GraphRelativeError()(w, w + 1, b, None).item() > 0   # C = 9: torch


def test_empty_graph_id_is_nan_like_torch(dev, monkeypatch):
    from bgnn import losses
    p = torch.rand(6, 2, device=dev) + 1
    t = torch.rand(6, 2, device=dev) + 1
    b = torch.tensor([0, 0, 2, 2, 2, 0], device=dev)   # graph 1 has no rows
    got = losses.GraphMAELoss()(p, t, b, None)
    monkeypatch.setattr(losses, "FUSED_GRAPH_LOSS", False)
    want = losses.GraphMAELoss()(p, t, b, None)
    assert torch.isnan(got) and torch.isnan(want)
