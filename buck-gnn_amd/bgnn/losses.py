"""Per-graph losses and error metrics of the node-level heads (static stress / displacement,
mode shapes), vectorised over the graphs of a batch.

The reference computes these with a Python loop over `range(batch.max().item() + 1)` and a
boolean mask per graph (`Utils/Losses.py:303-507`, `Dataset_Preparation/Metrics.py:4-191`):
one host sync plus O(B) small kernels per graph and call. Here every per-graph quantity is a
segment reduction over the batch vector (`index_add_` / `scatter_reduce_` over graph ids, ragged
per-graph quantiles as one `nanquantile` over a NaN-padded [B, max_len] view), so a call costs
a fixed handful of device ops, independent of B, and one host sync for the graph count (one
more for the padded width where a quantile is taken).
Results equal the reference's (tests/test_losses.py against the reference's own classes:
tests/golden/heads/losses.npz, made by tests/golden/make_golden_losses.py).

Semantics kept from the reference, including its quirks:
* the per-graph losses scale by 10000 when a batch vector is given, and not without one;
* `GraphMSELoss` averages |p^2 - t^2| per graph, but |p - t|^2 without a batch vector;
* `GraphMixedError` uses the 0.2-quantile of the relative error (its docstring says P90);
* `stress_errors` returns SUMS over graphs (its comment says means), and the `*_high` /
  `*_low` entries sum only over graphs that have such elements (0 when none has);
* per-component maxima take the first index of the largest |target| (torch.argmax);
* the force-scaled losses (`ScaledGraphMAELoss`, `ScaledGraphMSELoss`, `ScaledGraphRELoss`) scale by
  100, not 10000, sum the force over every row of the `x` they are given (one scale for the whole
  batch, not one per graph), and `ScaledGraphMSELoss` without a batch vector returns mean |p - t| times
  the scale (no squares).

All eight `criterion(pred, target, batch, x)` classes of the reference run on HIP when they are given
a batch vector and float32 GPU tensors of at most 8 columns (`graph_loss`, `criterion_loss`):
bgnn_graph_loss for the three per-graph means, bgnn_graph_loss_ex for the mixed (exact per-graph
quantile by radix select, with its gradient), max-component and force-scaled ones, the force scale
itself from bgnn_force_scale on the device (no `.item()`). Loss and gradient come from one call, sums
in double in a fixed order, bit-stable. `FUSED_GRAPH_LOSS = False`, a name taken out of
`FUSED_CRITERIA`, CPU tensors, doubles and more than 8 columns run the torch segment ops.
`get_loss_function` maps the reference's loss names to these classes.

`stress_errors` on float32 GPU tensors runs as one HIP entry point (`graph_metrics`,
bgnn_graph_metrics: the whole per-graph table of `METRIC_KEYS[prediction_type]` in two launches,
exact per-graph 0.9-quantiles by radix select, sums in double in a fixed order, bit-stable) and one
read-back; `FUSED_STRESS_ERRORS = False`, CPU tensors, doubles and more than 8 columns run the torch
segment ops. `StressErrorMeter` accumulates the same sums on the device over the batches of an
epoch (bgnn.train_step's `metrics=`, bgnn.evaluate_nodes) and reads them back once.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor, nn


# --------------------------------------------------------------------------------------------
# segment helpers over the batch vector (graph ids of the rows, any order)

def _num_graphs(batch: Tensor) -> int:
    return int(batch.max().item()) + 1 if batch.numel() else 0


def _seg_sum(v: Tensor, seg: Tensor, n: int) -> Tensor:
    """Σ of v over each segment; v and seg are 1-D of the same length."""
    return torch.zeros(n, dtype=v.dtype, device=v.device).index_add_(0, seg, v)


def _seg_count(seg: Tensor, n: int, dtype=torch.float32) -> Tensor:
    return torch.zeros(n, dtype=dtype, device=seg.device).index_add_(
        0, seg, torch.ones_like(seg, dtype=dtype))


def _seg_mean(v: Tensor, seg: Tensor, n: int) -> Tensor:
    return _seg_sum(v, seg, n) / _seg_count(seg, n, v.dtype)


def _seg_quantile(v: Tensor, seg: Tensor, n: int, q: float) -> Tensor:
    """torch.quantile (linear interpolation) of v within each segment; NaN for empty ones."""
    order = torch.argsort(seg, stable=True)
    vs, ss = v[order], seg[order]
    cnt = _seg_count(ss, n, torch.int64)
    start = torch.cumsum(cnt, 0) - cnt
    width = int(cnt.max().item()) if n else 0
    pad = torch.full((n, max(width, 1)), float("nan"), dtype=v.dtype, device=v.device)
    pos = torch.arange(vs.numel(), device=v.device) - start[ss]
    pad[ss, pos] = vs
    return torch.nanquantile(pad, q, dim=1)


def _seg_first_argmax(v: Tensor, seg: Tensor, n: int) -> Tensor:
    """Row index of the first maximum of v within each segment (rows ordered by position)."""
    mx = torch.full((n,), float("-inf"), dtype=v.dtype, device=v.device).scatter_reduce_(
        0, seg, v, "amax", include_self=True)
    idx = torch.arange(v.numel(), device=v.device)
    cand = torch.where(v == mx[seg], idx, torch.full_like(idx, v.numel()))
    return torch.full((n,), v.numel(), dtype=idx.dtype, device=v.device).scatter_reduce_(
        0, seg, cand, "amin", include_self=True)


def _elem_seg(batch: Tensor, x: Tensor) -> Tensor:
    """Graph id of every element of x ([N] or [N, C], row-major flattening)."""
    return batch if x.dim() == 1 else batch.repeat_interleave(x[0].numel())


# --------------------------------------------------------------------------------------------
# the three per-graph-mean losses as one HIP kernel (bgnn_graph_loss)

# GraphRelativeError / GraphMAELoss / GraphMSELoss with a batch vector on bgnn_graph_loss: loss and
# d loss / d pred in two launches, sums in a fixed order (bit-stable; index_add_ is atomic)
FUSED_GRAPH_LOSS = True
_MULT = 10000.0


class _GraphLossFn(torch.autograd.Function):
    """bgnn_graph_loss: the loss, with d loss / d pred computed in the same pass and kept for the
    backward (one multiply). scale / center: optional per-column affine applied to pred and target
    before the element term (the denormalisation of bgnn.train.ColumnScaler)."""

    @staticmethod
    def forward(ctx, pred, target, seg, kind: int, eps: float, scale, center):
        from . import _lib
        from .graph import _ptr, _stream
        shape = pred.shape
        p = pred.contiguous()
        t = target.contiguous()
        N = p.size(0)
        C = p.numel() // N
        B = seg.num_rows
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        dpred = torch.empty_like(p)
        ws_bytes = _lib.query("bgnn_graph_loss_ws_bytes", N, C, B)
        ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=p.device)
        _lib.call("bgnn_graph_loss", p.data_ptr(), t.data_ptr(), N, C, seg.fwd.rowptr.data_ptr(),
                  seg.fwd.col.data_ptr(), B, int(kind), float(eps), _MULT, _ptr(scale), _ptr(center),
                  loss.data_ptr(), dpred.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
        ctx.save_for_backward(dpred.view(shape))
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None, None, None, None


def _segments(batch: Tensor, num_graphs: Optional[int] = None):
    """The batch vector's segment index (cached); num_graphs: the graph count where the caller
    knows it (None: read back from the batch vector)."""
    from .graph import SegmentIndex, _index_cache

    def build():
        return SegmentIndex.build(batch, int(batch.max().item()) + 1 if num_graphs is None else int(num_graphs))
    return _index_cache.get(batch, ("batch",), build)


class _GraphLossExFn(torch.autograd.Function):
    """bgnn_graph_loss_ex: kinds 0..5 with the quantile q and the multiplier mult * mult_dev[0]
    (mult_dev: a float32 device scalar or None; no gradient flows through it), otherwise as
    _GraphLossFn."""

    @staticmethod
    def forward(ctx, pred, target, seg, kind: int, eps: float, scale, center, q: float, mult: float, mult_dev):
        from . import _lib
        from .graph import _ptr, _stream
        shape = pred.shape
        p = pred.contiguous()
        t = target.contiguous()
        N = p.size(0)
        C = p.numel() // N
        B = seg.num_rows
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        dpred = torch.empty_like(p)
        ws_bytes = _lib.query("bgnn_graph_loss_ex_ws_bytes", N, C, B)
        ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=p.device)
        _lib.call("bgnn_graph_loss_ex", p.data_ptr(), t.data_ptr(), N, C, seg.fwd.rowptr.data_ptr(),
                  seg.fwd.col.data_ptr(), B, int(kind), float(eps), float(mult), _ptr(scale), _ptr(center), float(q),
                  _ptr(mult_dev), loss.data_ptr(), dpred.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
        ctx.save_for_backward(dpred.view(shape))
        return loss

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return (dpred * g,) + (None,) * 9


# the reference's factor per kind: the per-graph means and the max-component loss x 10000, the
# force-scaled ratio of sums x 100, the mixed loss as it is
_KIND_MULT = {0: _MULT, 1: _MULT, 2: _MULT, 3: 100.0, 4: 1.0, 5: _MULT}


def graph_loss(kind: int, eps: float, pred: Tensor, target: Tensor, batch: Optional[Tensor], scale=None,
               center=None, q: float = 0.0, mult: Optional[float] = None, mult_dev: Optional[Tensor] = None,
               num_graphs: Optional[int] = None) -> Optional[Tensor]:
    """The per-graph loss `kind` (0 relative, 1 MAE, 2 squares: per-graph means; 3 ratio of sums, 4
    mixed with the `q`-quantile of the relative error, 5 relative error at each component's largest
    |target|) of pred * scale + center against target * scale + center (scale / center: [C] float32
    tensors or None), times mult (None: the reference's factor for the kind, 10000 / 100 / 1) and
    times mult_dev[0] (a float32 device scalar, e.g. force_scale's; None: 1), or None when the call
    does not qualify: float32 GPU pred and target of one [N] or [N, C <= 8] shape, a batch vector of
    N graph ids on the same device, no gradient wanted for target. num_graphs: the number of graphs
    where the caller knows it (it saves the read-back of batch.max()). Kinds 0..2 with the default
    multiplier run on bgnn_graph_loss, everything else on bgnn_graph_loss_ex (fewer than 2^31
    elements)."""
    if not (FUSED_GRAPH_LOSS and batch is not None and pred.is_cuda and pred.dtype == torch.float32
            and target.dtype == torch.float32 and target.device == pred.device and pred.shape == target.shape
            and pred.dim() in (1, 2) and pred.size(0) > 0 and batch.device == pred.device and batch.dim() == 1
            and batch.numel() == pred.size(0) and not batch.is_floating_point() and not target.requires_grad):
        return None
    C = pred.size(1) if pred.dim() == 2 else 1
    if not 1 <= C <= 8:
        return None
    for v in (scale, center):
        if v is not None and not (v.is_cuda and v.dtype == torch.float32 and v.numel() == C and v.is_contiguous()):
            return None
    if kind <= 2 and mult is None and mult_dev is None:
        return _GraphLossFn.apply(pred, target, _segments(batch, num_graphs), kind, eps, scale, center)
    if kind not in _KIND_MULT or pred.numel() >= 2 ** 31 or (kind == 4 and not 0.0 <= q <= 1.0):
        return None
    if mult_dev is not None and not (mult_dev.is_cuda and mult_dev.device == pred.device
                                     and mult_dev.dtype == torch.float32 and mult_dev.numel() == 1):
        return None
    return _GraphLossExFn.apply(pred, target, _segments(batch, num_graphs), kind, eps, scale, center, q,
                                _KIND_MULT[kind] if mult is None else mult, mult_dev)


def force_scale(x: Tensor, min_scale: float, flag_col: Optional[int] = None, c0: int = 3, nc: int = 2
                ) -> Optional[Tensor]:
    """max(sum over rows of ||x[:, c0 : c0 + nc]||_2, min_scale) as a float32 device scalar [1] on
    bgnn_force_scale (the Scaled* classes' compute_total_force and clamp, no host read); rows with a
    non-zero x[:, flag_col] are skipped (None: every row counts). None when the call does not
    qualify: a float32 GPU x [N >= 1, F >= c0 + nc] with unit column stride."""
    if not (FUSED_GRAPH_LOSS and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.size(0) > 0
            and x.stride(1) == 1 and x.stride(0) >= x.size(1) and 1 <= nc <= 8 and 0 <= c0
            and c0 + nc <= x.size(1) and (flag_col is None or 0 <= flag_col < x.size(1))):
        return None
    from . import _lib
    from .graph import _stream
    x = x.detach()
    N = x.size(0)
    out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws_bytes = _lib.query("bgnn_force_scale_ws_bytes", N)
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=x.device)
    _lib.call("bgnn_force_scale", x.data_ptr(), N, x.stride(0), c0, nc, -1 if flag_col is None else int(flag_col),
              float(min_scale), out.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
    return out


# --------------------------------------------------------------------------------------------
# losses (Utils/Losses.py)

class GraphRelativeError(nn.Module):
    """Per-graph mean of |p - t| / (|t| + eps), averaged over graphs, x 10000
    (Utils/Losses.py:362-401)."""

    def __init__(self, epsilon: float = 0.1):
        super().__init__()
        self.epsilon = epsilon

    def forward(self, pred: Tensor, target: Tensor, batch: Optional[Tensor], x=None) -> Tensor:
        out = graph_loss(0, self.epsilon, pred, target, batch)
        if out is not None:
            return out
        rel = torch.abs(pred - target) / (torch.abs(target) + self.epsilon)
        if batch is None:
            return torch.mean(rel)
        n = _num_graphs(batch)
        return torch.mean(_seg_mean(rel.reshape(-1), _elem_seg(batch, rel), n)) * 10000


class GraphMixedError(nn.Module):
    """0.2 x mean over graphs of the per-graph `percentile`-quantile of the relative error
    + 0.8 x mean over graphs of the per-graph MAE (Utils/Losses.py:403-443)."""

    def __init__(self, epsilon: float = 1e-8, percentile: float = 0.2):
        super().__init__()
        self.epsilon = epsilon
        self.percentile = percentile

    def forward(self, pred: Tensor, target: Tensor, batch: Optional[Tensor], x=None) -> Tensor:
        out = criterion_loss(self, pred, target, batch)
        if out is not None:
            return out
        diff = torch.abs(pred - target)
        rel = diff / (torch.abs(target) + self.epsilon)
        if batch is None:
            return 0.2 * torch.quantile(rel, self.percentile) + 0.8 * torch.mean(diff)
        n = _num_graphs(batch)
        seg = _elem_seg(batch, rel)
        q = _seg_quantile(rel.reshape(-1), seg, n, self.percentile)
        mae = _seg_mean(diff.reshape(-1), seg, n)
        return 0.2 * torch.mean(q) + 0.8 * torch.mean(mae)


class GraphMSELoss(nn.Module):
    """Per-graph mean of |p^2 - t^2|, averaged over graphs, x 10000; without a batch vector
    mean(|p - t|^2) (Utils/Losses.py:445-475)."""

    def __init__(self, alpha: float = 0.5):
        super().__init__()
        self.alpha = alpha

    def forward(self, pred: Tensor, target: Tensor, batch: Optional[Tensor], x=None) -> Tensor:
        if batch is None:
            return torch.mean(torch.abs(pred - target) ** 2)
        out = graph_loss(2, 0.0, pred, target, batch)
        if out is not None:
            return out
        d = torch.abs(pred ** 2 - target ** 2)
        return torch.mean(_seg_mean(d.reshape(-1), _elem_seg(batch, d), _num_graphs(batch))) * 10000


class GraphMAELoss(nn.Module):
    """Per-graph mean of |p - t|, averaged over graphs, x 10000 (Utils/Losses.py:477-507)."""

    def __init__(self, alpha: float = 0.5):
        super().__init__()
        self.alpha = alpha

    def forward(self, pred: Tensor, target: Tensor, batch: Optional[Tensor], x=None) -> Tensor:
        out = graph_loss(1, 0.0, pred, target, batch)
        if out is not None:
            return out
        d = torch.abs(pred - target)
        if batch is None:
            return torch.mean(d)
        return torch.mean(_seg_mean(d.reshape(-1), _elem_seg(batch, d), _num_graphs(batch))) * 10000


class GraphMaxComponentRelativeError(nn.Module):
    """Relative error at the location of each graph's largest |target| per component,
    averaged over components and graphs, x 10000 (Utils/Losses.py:303-359)."""

    def __init__(self, epsilon: float = 1e-8):
        super().__init__()
        self.epsilon = epsilon

    def forward(self, pred: Tensor, target: Tensor, batch: Optional[Tensor], x=None) -> Tensor:
        out = criterion_loss(self, pred, target, batch)
        if out is not None:
            return out
        p2 = pred if pred.dim() > 1 else pred.unsqueeze(1)
        t2 = target if target.dim() > 1 else target.unsqueeze(1)
        if batch is None:
            idx = torch.argmax(torch.abs(t2), dim=0)
            mt, mp = t2.gather(0, idx[None]).squeeze(0), p2.gather(0, idx[None]).squeeze(0)
            return torch.mean(torch.abs(mp - mt) / (torch.abs(mt) + self.epsilon))
        n = _num_graphs(batch)
        errs = []
        for c in range(t2.size(1)):
            i = _seg_first_argmax(torch.abs(t2[:, c]), batch, n)
            mt, mp = t2[i, c], p2[i, c]
            errs.append(torch.abs(mp - mt) / (torch.abs(mt) + self.epsilon))
        return torch.mean(torch.stack(errs, 1)) * 10000


class _ScaledGraphLoss(nn.Module):
    """The force-scaled per-graph losses (Utils/Losses.py:509-695): the per-graph term times
    max(total force, min_scale), averaged over graphs, x 100. The total force is the sum over ALL
    rows of the x passed in of ||x[:, 3:5]||_2, not per graph: one scale serves every graph of the
    batch, and no gradient flows through it. Without a batch vector: the term over all elements times
    the scale, not x 100."""

    _kind = 1   # the kernel's kind (graph_loss) of the per-graph term

    def __init__(self, force_scaling: bool = True, min_scale: float = 0.1):
        super().__init__()
        self.force_scaling = force_scaling
        self.min_scale = min_scale

    def compute_total_force(self, x: Tensor) -> Tensor:
        return torch.sum(torch.norm(x[:, 3:5], dim=1))

    def _scale(self, x: Optional[Tensor]):
        """max(total force, min_scale) as a tensor (the reference reads it back with .item()), or 1."""
        if not self.force_scaling:
            return 1.0
        if x is None:
            raise ValueError(f"{type(self).__name__}: force_scaling needs the node features x "
                             "(forces in columns 3:5); pass x or construct with force_scaling=False")
        return torch.clamp(self.compute_total_force(x.detach()), min=self.min_scale)

    def _term(self, pred: Tensor, target: Tensor) -> Tensor:
        return torch.abs(pred - target)

    def _all(self, pred: Tensor, target: Tensor) -> Tensor:
        """The term without a batch vector."""
        return torch.mean(torch.abs(pred - target))

    def _per_graph(self, pred: Tensor, target: Tensor, batch: Tensor, n: int) -> Tensor:
        d = self._term(pred, target)
        return _seg_mean(d.reshape(-1), _elem_seg(batch, d), n)

    def forward(self, pred: Tensor, target: Tensor, batch: Optional[Tensor], x: Optional[Tensor] = None) -> Tensor:
        out = criterion_loss(self, pred, target, batch, x)
        if out is not None:
            return out
        scale = self._scale(x)
        if batch is None:
            return self._all(pred, target) * scale
        return torch.mean(self._per_graph(pred, target, batch, _num_graphs(batch)) * scale) * 100


class ScaledGraphMAELoss(_ScaledGraphLoss):
    """Per-graph mean of |p - t| times the force scale, averaged over graphs, x 100
    (Utils/Losses.py:509-566)."""


class ScaledGraphMSELoss(_ScaledGraphLoss):
    """Per-graph mean of |p^2 - t^2| times the force scale, averaged over graphs, x 100; without a
    batch vector mean |p - t| times the scale (Utils/Losses.py:568-625)."""

    _kind = 2

    def _term(self, pred: Tensor, target: Tensor) -> Tensor:
        return torch.abs(pred ** 2 - target ** 2)


class ScaledGraphRELoss(_ScaledGraphLoss):
    """Per graph sum |p - t| / (sum |t| + 1e-8) times the force scale, averaged over graphs, x 100
    (Utils/Losses.py:627-695)."""

    _kind = 3

    def _all(self, pred: Tensor, target: Tensor) -> Tensor:
        return torch.abs(pred - target).sum() / (torch.abs(target).sum() + 1e-8)

    def _per_graph(self, pred: Tensor, target: Tensor, batch: Tensor, n: int) -> Tensor:
        seg = _elem_seg(batch, pred)
        return _seg_sum(torch.abs(pred - target).reshape(-1), seg, n) / (
            _seg_sum(torch.abs(target).reshape(-1), seg, n) + 1e-8)


# The reference's names (get_loss_function) of the classes whose batch-vector call takes the
# kernels of bgnn_graph_loss_ex while FUSED_GRAPH_LOSS is on. A name stays here only where
# tools/graph_loss_ab.py measured its fused train step faster than the torch route.
FUSED_CRITERIA = {"graph_mixed", "graph_max_rel", "graph_mae_scaled", "graph_mse_scaled", "graph_rel_scaled"}


def criterion_loss(criterion, pred: Tensor, target: Tensor, batch: Optional[Tensor], x: Optional[Tensor] = None,
                   scale=None, center=None, flag_col: Optional[int] = None, num_graphs: Optional[int] = None
                   ) -> Optional[Tensor]:
    """criterion(pred * scale + center, target * scale + center, batch, x) for one of this module's
    eight per-graph classes on the loss kernels (graph_loss), or None when the criterion is none of
    them, is switched off (FUSED_GRAPH_LOSS, FUSED_CRITERIA) or the call does not qualify. For the
    force-scaled classes x is the unfiltered node features and flag_col the column whose non-zero
    rows (super nodes) do not count: the scale comes from force_scale, with no host read. num_graphs:
    as graph_loss's."""
    cls = type(criterion)
    if batch is None:
        return None
    if cls in (GraphRelativeError, GraphMAELoss, GraphMSELoss):
        kind = {GraphRelativeError: 0, GraphMAELoss: 1, GraphMSELoss: 2}[cls]
        return graph_loss(kind, getattr(criterion, "epsilon", 0.0), pred, target, batch, scale, center,
                          num_graphs=num_graphs)
    name = _CRITERION_NAMES.get(cls)
    if name is None or name not in FUSED_CRITERIA:
        return None
    if cls is GraphMixedError:
        return graph_loss(4, criterion.epsilon, pred, target, batch, scale, center, q=criterion.percentile,
                          num_graphs=num_graphs)
    if cls is GraphMaxComponentRelativeError:
        return graph_loss(5, criterion.epsilon, pred, target, batch, scale, center, mult=_MULT,
                          num_graphs=num_graphs)
    mult_dev = None
    if criterion.force_scaling:
        if x is None:
            criterion._scale(None)   # raises
        mult_dev = force_scale(x, criterion.min_scale, flag_col)
        if mult_dev is None:
            return None
    return graph_loss(criterion._kind, 0.0, pred, target, batch, scale, center, mult=100.0, mult_dev=mult_dev,
                      num_graphs=num_graphs)


_CRITERION_NAMES = {GraphMixedError: "graph_mixed", GraphMaxComponentRelativeError: "graph_max_rel",
                    ScaledGraphMAELoss: "graph_mae_scaled", ScaledGraphMSELoss: "graph_mse_scaled",
                    ScaledGraphRELoss: "graph_rel_scaled"}
# the classes whose forward takes (pred, target, batch, x)
GRAPH_CRITERIA = (GraphRelativeError, GraphMAELoss, GraphMSELoss, GraphMixedError, GraphMaxComponentRelativeError,
                  ScaledGraphMAELoss, ScaledGraphMSELoss, ScaledGraphRELoss)

# get_loss_function's names that the reference maps to two-argument losses this package does not carry
_REFERENCE_ONLY = ("static_mixed", "static_mse", "static_relative", "static_stress", "static_mae", "log_cosh",
                   "eigenvalue", "order_preserving", "focal", "mape", "mae", "rse", "rrse", "rrse1", "msle",
                   "focal_rrse", "focal_mape")


def get_loss_function(loss_name: str, allValues=None, use_z_coord: bool = False, use_rotations: bool = False):
    """The reference's get_loss_function (Utils/Losses.py:8-66) for the losses this package carries:
    the eight graph_* names (criterion(pred, target, batch, x)), relative_error and mse. The
    reference's other names raise NotImplementedError, an unknown name its ValueError."""
    table = {"graph_mse": GraphMSELoss, "graph_mae": GraphMAELoss, "graph_rel": GraphRelativeError,
             "graph_mixed": GraphMixedError, "graph_max_rel": GraphMaxComponentRelativeError,
             "graph_rel_scaled": ScaledGraphRELoss, "graph_mae_scaled": ScaledGraphMAELoss,
             "graph_mse_scaled": ScaledGraphMSELoss, "mse": nn.MSELoss}
    if loss_name in table:
        return table[loss_name]()
    if loss_name == "relative_error":
        from .train import RelativeErrorLoss
        return RelativeErrorLoss()
    if loss_name in _REFERENCE_ONLY:
        raise NotImplementedError(f"get_loss_function: the reference's {loss_name!r} loss is not implemented in bgnn "
                                  "(the graph_* losses, relative_error and mse are)")
    raise ValueError(f"Unknown loss function: {loss_name}")


# --------------------------------------------------------------------------------------------
# metrics (Dataset_Preparation/Metrics.py)

def mape_error(predictions: Tensor, targets: Tensor, prediction_type: str = "buckling", normalizer=None,
               threshold: float = 0.1) -> Tensor:
    """MAPE_error (Dataset_Preparation/Metrics.py:4-23), every prediction type."""
    if prediction_type == "buckling":
        if normalizer is not None:
            p, t = normalizer.denormalize_eigenvalue(predictions), normalizer.denormalize_eigenvalue(targets)
            return torch.mean(torch.abs((t - p) / t)) * 100
        return torch.mean(torch.abs((targets - predictions) / targets)) * 100
    if prediction_type in ("static_disp", "static_stress"):
        m = torch.abs(targets) >= threshold
        return torch.mean(torch.abs((targets[m] - predictions[m]) / (targets[m] + 1e-8))) * 100
    if prediction_type == "mode_shape":
        pn = predictions / (torch.norm(predictions, dim=1, keepdim=True) + 1e-8)
        tn = targets / (torch.norm(targets, dim=1, keepdim=True) + 1e-8)
        return torch.mean(torch.abs(pn - tn)) * 100
    return None


def _region_metrics(abs_diff: Tensor, rel_diff: Tensor, target: Tensor, pred: Tensor, seg: Tensor, n: int,
                    mask: Optional[Tensor]) -> Dict[str, Tensor]:
    """mape / re / rmse / mae / p90 per graph over the selected elements (all when mask is
    None), with a per-graph 'present' flag (the reference appends only when the mask hits)."""
    if mask is not None:
        abs_diff, rel_diff, target, pred, seg = abs_diff[mask], rel_diff[mask], target[mask], pred[mask], seg[mask]
    cnt = _seg_count(seg, n, abs_diff.dtype)
    present = cnt > 0
    out = {
        "mape": _seg_sum(rel_diff, seg, n) / cnt * 100,
        "re": _seg_sum(abs_diff, seg, n) / _seg_sum(torch.abs(target), seg, n) * 100,
        "rmse": torch.sqrt(_seg_sum(target ** 2 - pred ** 2, seg, n) / cnt),
        "mae": _seg_sum(abs_diff, seg, n) / cnt,
        "p90": _seg_quantile(rel_diff, seg, n, 0.9) * 100,
    }
    return {k: torch.where(present, v, torch.zeros_like(v)) for k, v in out.items()}


# the per-graph metric table as one HIP entry point (bgnn_graph_metrics)

# stress_errors / StressErrorMeter on bgnn_graph_metrics where the call qualifies (graph_metrics)
FUSED_STRESS_ERRORS = True
_REGION = ("mape", "re", "rmse", "mae", "p90")
_TAIL = tuple(k + "_high" for k in _REGION) + tuple(k + "_low" for k in _REGION) + (
    "mape", "re", "rmse", "mae", "mse", "p90", "max_mae", "std_mae", "p90_abs")
# the table's metric columns in order (include/bgnn.h), = the reference's keys for the type; two
# more columns follow: the element counts of the high and of the low region
METRIC_KEYS = {
    "static_stress": tuple(f"max_{c}_{k}" for c in ("x", "y", "xy") for k in ("val", "mae", "rel")) + _TAIL,
    "static_disp": tuple(f"max_{c}_{k}" for c in ("disp", "x", "y") for k in ("val", "mae", "rel")) + _TAIL,
}
GRAPH_METRICS_COLS = 30
_N_KEYS = 28
# the reference's thresholds per type (TRAIN_FINAL.py:271-292)
DEFAULT_THRESHOLD = {"static_disp": 1e-4, "static_stress": 0.2}


def graph_metrics(pred: Tensor, target: Tensor, batch: Optional[Tensor], prediction_type: str, threshold: float,
                  scale=None, center=None) -> Optional[Tensor]:
    """The per-graph metric table [B, GRAPH_METRICS_COLS] (float64, on the device; columns
    METRIC_KEYS[prediction_type], then the high / low element counts) of pred * scale + center
    against target * scale + center on bgnn_graph_metrics, or None when the call does not qualify:
    graph_loss's conditions (float32 GPU pred and target of one [N, C <= 8] shape, a batch vector of
    N graph ids on the same device) with C >= 3 for static_stress and C >= 2 for static_disp. A
    graph id without rows gives a NaN row with zero counts. No host sync beyond the cached segment
    index of the batch vector."""
    if prediction_type not in METRIC_KEYS:
        raise NotImplementedError(f"Error metrics not implemented for prediction type: {prediction_type}")
    if not (batch is not None and pred.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32
            and target.device == pred.device and pred.shape == target.shape and pred.dim() == 2 and pred.size(0) > 0
            and batch.device == pred.device and batch.dim() == 1 and batch.numel() == pred.size(0)
            and not batch.is_floating_point()):
        return None
    C = pred.size(1)
    mode = 0 if prediction_type == "static_stress" else 1
    if not (3 if mode == 0 else 2) <= C <= 8 or pred.numel() >= 2 ** 31:
        return None
    for v in (scale, center):
        if v is not None and not (v.is_cuda and v.dtype == torch.float32 and v.numel() == C and v.is_contiguous()):
            return None
    from . import _lib
    from .graph import _ptr, _stream
    p = pred.detach().contiguous()
    t = target.detach().contiguous()
    seg = _segments(batch)
    N, B = p.size(0), seg.num_rows
    out = torch.empty((B, GRAPH_METRICS_COLS), dtype=torch.float64, device=p.device)
    ws_bytes = _lib.query("bgnn_graph_metrics_ws_bytes", N, C, B)
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.float64, device=p.device)
    _lib.call("bgnn_graph_metrics", p.data_ptr(), t.data_ptr(), N, C, seg.fwd.rowptr.data_ptr(),
              seg.fwd.col.data_ptr(), B, mode, float(threshold), _ptr(scale), _ptr(center), out.data_ptr(),
              ws.data_ptr(), ws_bytes, _stream())
    return out


def _fused_table(pred, target, batch, prediction_type, threshold, scale=None, center=None):
    return graph_metrics(pred, target, batch, prediction_type, threshold, scale, center) if FUSED_STRESS_ERRORS \
        else None


class StressErrorMeter:
    """stress_errors over the batches of an epoch, accumulated on the device: the reference adds the
    per-batch dicts key by key (TRAIN_FINAL.py:300-304) and divides by the number of graphs
    (TRAIN_FINAL.py:319,384) or of batches (INFERENCE.py:190).
    update() adds a batch's sums over graphs and its graph count with no host sync (the table of
    bgnn_graph_metrics; inputs that kernel declines go through the torch stress_errors, which
    syncs); compute() is the one read-back. state() is the accumulator itself, [30] float64:
    the 28 sums in METRIC_KEYS order, the graph count, the update count (a caller may all-reduce it)."""

    def __init__(self, prediction_type: str, threshold: Optional[float] = None):
        if prediction_type not in METRIC_KEYS:
            raise ValueError(f"StressErrorMeter: no error metrics for prediction type {prediction_type!r} "
                             "(static_stress or static_disp)")
        self.prediction_type = prediction_type
        self.threshold = DEFAULT_THRESHOLD[prediction_type] if threshold is None else float(threshold)
        self.keys = METRIC_KEYS[prediction_type]
        self._acc: Optional[Tensor] = None

    def _state_on(self, device) -> Tensor:
        if self._acc is None:
            self._acc = torch.zeros(_N_KEYS + 2, dtype=torch.float64, device=device)
        return self._acc

    def update(self, pred: Tensor, target: Tensor, batch: Optional[Tensor], scale=None, center=None) -> None:
        """Add one batch. scale / center: the ColumnScaler's per-column affine ([C] float32 on the
        device), applied to pred and target before the metrics (None: the values as they are)."""
        acc = self._state_on(pred.device)
        table = _fused_table(pred, target, batch, self.prediction_type, self.threshold, scale, center)
        if table is not None:
            acc[:_N_KEYS] += table[:, :_N_KEYS].sum(0)
            acc[_N_KEYS] += table.size(0)
        else:
            p, t = pred.detach(), target
            if scale is not None:
                p, t = p * scale, t * scale
            if center is not None:
                p, t = p + center, t + center
            d = stress_errors(p, t, batch, self.prediction_type, self.threshold)
            acc[:_N_KEYS] += torch.tensor([d[k] for k in self.keys], dtype=torch.float64).to(acc.device)
            acc[_N_KEYS] += _num_graphs(batch) if batch is not None else 1
        acc[_N_KEYS + 1] += 1

    def state(self) -> Optional[Tensor]:
        return self._acc

    def reset(self) -> None:
        if self._acc is not None:
            self._acc.zero_()

    @property
    def counts(self):
        """(graphs, updates) so far (a host read)."""
        if self._acc is None:
            return 0, 0
        g, u = self._acc[_N_KEYS:].tolist()
        return int(g), int(u)

    def compute(self, per: str = "graph") -> Dict[str, float]:
        """The accumulated sums divided by the number of graphs (per="graph") or of updates
        (per="batch"); NaN before the first update."""
        if per not in ("graph", "batch"):
            raise ValueError("StressErrorMeter.compute: per must be 'graph' or 'batch'")
        if self._acc is None:
            return {k: float("nan") for k in self.keys}
        vals = self._acc.tolist()
        den = vals[_N_KEYS] if per == "graph" else vals[_N_KEYS + 1]
        return {k: (v / den if den else float("nan")) for k, v in zip(self.keys, vals)}


def stress_errors(predictions: Tensor, targets: Tensor, batch: Optional[Tensor] = None,
                  prediction_type: str = "static_stress", threshold: float = 0.1) -> Dict[str, float]:
    """stress_errors (Dataset_Preparation/Metrics.py:25-191): per-graph error metrics of the
    static stress ([N, 3]: x, y, xy) or displacement ([N, >= 2]) heads, summed over graphs.
    float32 GPU tensors of at most 8 columns: bgnn_graph_metrics and one read-back of the sums."""
    if prediction_type not in ("static_stress", "static_disp"):
        raise NotImplementedError(f"Error metrics not implemented for prediction type: {prediction_type}")
    if batch is None:
        batch = torch.zeros(len(predictions), dtype=torch.long, device=predictions.device)
    table = _fused_table(predictions, targets, batch, prediction_type, threshold)
    if table is not None:
        return dict(zip(METRIC_KEYS[prediction_type], table[:, :_N_KEYS].sum(0).tolist()))
    n = _num_graphs(batch)
    p, t = predictions, targets
    abs_diff = torch.abs(t - p)
    rel_diff = abs_diff / (torch.abs(t) + 1e-8)
    C = t.size(1)
    seg = batch.repeat_interleave(C)
    flat = lambda v: v.reshape(-1)   # noqa: E731
    res: Dict[str, Tensor] = {}
    if prediction_type == "static_disp":
        mag = torch.norm(t, dim=1)
        i = _seg_first_argmax(mag, batch, n)
        err = torch.norm(abs_diff[i], dim=1)
        res["max_disp_val"] = mag[i]
        res["max_disp_mae"] = err
        res["max_disp_rel"] = err / (mag[i] + 1e-8) * 100
        comps = ["x", "y"]
        row_hi = mag >= threshold
        hi_mask = flat(row_hi[:, None].expand_as(t))
        lo_mask = flat((~row_hi)[:, None].expand_as(t))
    else:
        comps = ["x", "y", "xy"]
        hi_mask = flat(torch.abs(t) >= threshold)
        lo_mask = flat(torch.abs(t) < threshold)
    for c, name in enumerate(comps):
        i = _seg_first_argmax(torch.abs(t[:, c]), batch, n)
        res[f"max_{name}_val"] = torch.abs(t[i, c])
        res[f"max_{name}_mae"] = abs_diff[i, c]
        res[f"max_{name}_rel"] = abs_diff[i, c] / (torch.abs(t[i, c]) + 1e-8) * 100
    a, r, tt, pp = flat(abs_diff), flat(rel_diff), flat(t), flat(p)
    for suffix, mask in (("_high", hi_mask), ("_low", lo_mask)):
        for k, v in _region_metrics(a, r, tt, pp, seg, n, mask).items():
            res[k + suffix] = v
    for k, v in _region_metrics(a, r, tt, pp, seg, n, None).items():
        res[k] = v
    cnt = _seg_count(seg, n, a.dtype)
    res["mse"] = _seg_sum(tt ** 2 - pp ** 2, seg, n) / cnt
    res["max_mae"] = torch.full((n,), float("-inf"), dtype=a.dtype, device=a.device).scatter_reduce_(
        0, seg, a, "amax", include_self=True)
    mean = _seg_sum(a, seg, n) / cnt
    res["std_mae"] = torch.sqrt(_seg_sum((a - mean[seg]) ** 2, seg, n) / (cnt - 1))
    res["p90_abs"] = _seg_quantile(a, seg, n, 0.9)
    # the reference sums Python floats (float64) over graphs
    return {k: float(v.double().sum().item()) for k, v in res.items()}
