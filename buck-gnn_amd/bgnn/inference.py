"""Inference driver: INFERENCE.py's buckling evaluation on the
bgnn path.

INFERENCE.py:133-150,176-186 runs the model in eval mode under no_grad over a DataLoader
and reports, on denormalised eigenvalues, the MAPE summed over graphs divided by the
number of graphs, and the smallest and largest per-graph APE, all in percent. `evaluate`
does the same over any iterable of batches: host-collated `Batch`es, or
`GraphStore.loader(...)` batches gathered on the GPU.

INFERENCE.py:153-172,189-199 does the same for the static heads with stress_errors per batch,
summed key by key and divided by the number of batches: `evaluate_nodes`, on a device-side
bgnn.losses.StressErrorMeter (one read-back at the end).
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch

from .graph import prepare
from .train import ColumnScaler, EigenvalueScaler, _denormalize_nodes, _node_criterion


def _flags_set(model, flags: dict, run):
    """run() with the model attributes `flags` set, each put back after (removed again where the
    model did not carry it)."""
    before = {k: vars(model)[k] for k in flags if k in vars(model)}
    for k, v in flags.items():
        setattr(model, k, v)
    try:
        return run()
    finally:
        for k in flags:
            if k in before:
                setattr(model, k, before[k])
            else:
                delattr(model, k)


def _bf16_value(bf16):
    return "all" if isinstance(bf16, str) and bf16 == "all" else bool(bf16)


@torch.no_grad()
def evaluate(model, batches: Iterable, normalizer: Optional[EigenvalueScaler] = None,
             device=None, bf16=None, bf16_sag: Optional[bool] = None) -> Dict[str, float]:
    """Buckling-eigenvalue metrics of INFERENCE.py: mean / min / max APE in percent.
    bf16: None leaves the model's `infer_bf16` flag alone; True / False sets it for this call (the
    GraphSAGE sum / mean models' bf16 inference path, BuckGNN.infer_bf16) and restores it after;
    "all" is passed through as it is (the max-aggregation model's bf16 path too).
    bf16_sag: the same for `infer_bf16_sag` (GraphSAGE_SAG on bf16 rows where infer_bf16 is set):
    None leaves it alone, True / False sets it for this call and restores it after."""
    model.eval()
    flags = {}
    if bf16 is not None:
        flags["infer_bf16"] = _bf16_value(bf16)
    if bf16_sag is not None:
        flags["infer_bf16_sag"] = bool(bf16_sag)
    return _flags_set(model, flags, lambda: _evaluate(model, batches, normalizer, device))


def _evaluate(model, batches, normalizer, device) -> Dict[str, float]:
    total, n, lo, hi = 0.0, 0, float("inf"), 0.0
    preds = []
    for batch in batches:
        if device is not None:
            batch = batch.to(device)
        prepare(batch.edge_index, batch.x.size(0), batch.batch, getattr(batch, "num_graphs", None) or None)
        pred, _ = model(batch.x, batch.edge_index, batch.edge_attr, batch.batch)
        true = batch.y
        if normalizer is not None:
            true, pred = normalizer.denormalize_eigenvalue(true), normalizer.denormalize_eigenvalue(pred)
        apes = torch.abs((true - pred.view_as(true)) / true)
        # one host read per batch for the three statistics (INFERENCE.py reads them per batch too)
        s, mx, mn = torch.stack([apes.sum(), apes.max(), apes.min()]).tolist()
        total += s * 100
        hi, lo = max(hi, mx * 100), min(lo, mn * 100)
        n += apes.numel()
        preds.append(pred.detach())
    return {"mape": total / max(n, 1), "min_mape": lo if n else 0.0, "max_mape": hi, "graphs": n,
            "predictions": torch.cat(preds) if preds else None}


@torch.no_grad()
def evaluate_nodes(model, batches: Iterable, normalizer=None, criterion=None, threshold: Optional[float] = None,
                   device=None, bf16=None, return_predictions: bool = False,
                   bf16_sag: Optional[bool] = None) -> Dict[str, object]:
    """The static heads' evaluation (INFERENCE.py:153-172,189-199; the validation loop of
    TRAIN_FINAL.py:349-384): eval mode, no_grad, per batch the model's prediction and its returned
    (super-node adjusted) batch vector, stress_errors of the denormalised values accumulated in a
    StressErrorMeter (threshold None: the reference's, 1e-4 for static_disp and 0.2 for
    static_stress), and criterion(denorm(pred), denorm(y), batch, x) as the train step calls it (x: the
    node features without the super nodes, for a criterion that reads the forces) when a criterion is
    given.
    normalizer: a bgnn.ColumnScaler (folded into the metric kernel), a reference-style object with
    denormalize_displacement / denormalize_gp_stresses, or None.
    bf16: None leaves the model's flags alone; True / "all" / False sets `infer_bf16` to that value
    and `infer_bf16_decoder` to its truth value for this call (the bf16 layer loop with the decoder
    on bf16 rows, BuckGNN.infer_bf16_decoder) and restores both after, as `evaluate` does.
    bf16_sag: None leaves `infer_bf16_sag` alone; True / False sets it for this call and restores it
    after (GraphSAGE_SAG on bf16 rows; the decoder there reads f32 rows either way).
    return_predictions: also return the fields, not only their metrics.
    Returns {"metrics_per_graph": sums / graphs, "metrics_per_batch": sums / batches, "graphs",
    "batches", "loss": the mean criterion value over batches or None}, and with return_predictions
    "predictions": one (denormalised prediction [n, C], returned batch vector) per batch."""
    flags = {}
    if bf16 is not None:
        flags.update(infer_bf16=_bf16_value(bf16), infer_bf16_decoder=bool(bf16))
    if bf16_sag is not None:
        flags["infer_bf16_sag"] = bool(bf16_sag)
    return _flags_set(model, flags, lambda: _evaluate_nodes(model, batches, normalizer, criterion, threshold, device,
                                                            return_predictions))


def _evaluate_nodes(model, batches, normalizer, criterion, threshold, device, return_predictions):
    from . import losses
    ptype = getattr(model, "prediction_type", "buckling")
    if ptype not in losses.METRIC_KEYS:
        raise ValueError(f"evaluate_nodes: a {ptype!r} model has no stress_errors metrics (static_disp or "
                         "static_stress); bgnn.evaluate covers buckling")
    model.eval()
    meter = losses.StressErrorMeter(ptype, threshold)
    loss_sum = None
    preds = []
    for batch in batches:
        if device is not None:
            batch = batch.to(device)
        prepare(batch.edge_index, batch.x.size(0), batch.batch, getattr(batch, "num_graphs", None) or None)
        pred, out_batch = model(batch.x, batch.edge_index, batch.edge_attr, batch.batch)
        if return_predictions:
            preds.append((_denormalize_nodes(normalizer, ptype, pred).detach(), out_batch))
        y = batch.y.contiguous() if ptype == "static_stress" else batch.y
        if normalizer is None or type(normalizer) is ColumnScaler:
            scale, center = normalizer._at(pred.device) if normalizer is not None else (None, None)
            meter.update(pred, y, out_batch, scale, center)
        else:
            meter.update(_denormalize_nodes(normalizer, ptype, pred), _denormalize_nodes(normalizer, ptype, y),
                         out_batch)
        if criterion is not None:
            v = _node_criterion(model, batch, criterion, normalizer, pred, y, out_batch).detach().double()
            loss_sum = v if loss_sum is None else loss_sum + v
    graphs, n = meter.counts
    out = {"metrics_per_graph": meter.compute("graph"), "metrics_per_batch": meter.compute("batch"), "graphs": graphs,
           "batches": n, "loss": float(loss_sum.item()) / n if loss_sum is not None else None}
    if return_predictions:
        out["predictions"] = preds
    return out
