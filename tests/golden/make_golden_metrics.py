#!/usr/bin/env python
"""Generate tests/golden/heads/metrics.npz from the REFERENCE's own stress_errors
(Dataset_Preparation/Metrics.py:25-191), at the thresholds its training loop uses
(TRAIN_FINAL.py:271-292: 0.2 for static_stress, 1e-4 for static_disp).

Runs only in the build container, where /root/reference exists; the reference module is imported
unchanged, as tests/golden/make_golden_losses.py does. The fixture holds only data: the seeded
inputs and the reference's outputs.

Two cases, each a ragged batch of graphs of 1 to 300 rows:
  stress: C = 3, threshold 0.2; |pred| < |target| everywhere, so every rmse is finite;
  disp:   C = 2, threshold 1e-4; additive noise (some per-graph mean(t^2 - p^2) < 0: rmse NaN).
In each, graph 7 lies entirely in the high region, graph 8 entirely in the low region, and graph 3
has exact ties of the largest |target| (of the largest row magnitude too, for disp) at rows with
different predictions: the first row wins.

    python tests/golden/make_golden_metrics.py [--out tests/golden/heads/metrics.npz]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
SIZES = [1, 37, 5, 300, 64, 18, 7, 40, 23]
ALL_HIGH, ALL_LOW, TIES = 7, 8, 3


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def inputs(seed, C, threshold, multiplicative):
    """Targets spread over two decades around the threshold; graphs ALL_HIGH / ALL_LOW a decade
    above / below it."""
    g = torch.Generator().manual_seed(seed)
    batch = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(SIZES)])
    N = batch.numel()
    sign = torch.where(torch.rand(N, C, generator=g) < 0.5, -1.0, 1.0)
    mag = (torch.rand(N, C, generator=g) * 0.9 + 0.1) * torch.pow(10.0, torch.rand(N, 1, generator=g) * 2 - 1.0)
    t = sign * mag * threshold * 3
    hi, lo = batch == ALL_HIGH, batch == ALL_LOW
    t[hi] = sign[hi] * (torch.rand(int(hi.sum()), C, generator=g) + 1.5) * threshold * 10
    t[lo] = sign[lo] * (torch.rand(int(lo.sum()), C, generator=g) * 0.5 + 0.1) * threshold * 0.1
    off = sum(SIZES[:TIES])
    n = SIZES[TIES]
    rows = t[off:off + n]
    # the row of the largest magnitude, copied to the graph's last row (a tie of the magnitude and of
    # every component's largest |target| that lies in that row); one more tie in column 0 alone
    top = int(torch.norm(rows, dim=1).argmax())
    rows[top] = rows[top] * 1.5
    rows[n - 1] = rows[top]
    rows[n - 2, 0] = -rows[:, 0].abs().max()
    if multiplicative:
        p = t * (1 - (torch.rand(N, C, generator=g) * 0.3 + 0.01))
    else:
        p = t + 0.3 * threshold * torch.randn(N, C, generator=g)
    return p, t, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "heads", "metrics.npz"))
    args = ap.parse_args()
    M = load(os.path.join(REF, "Dataset_Preparation", "Metrics.py"), "ref_metrics")
    out = {}
    for tag, (seed, C, kind, thr, mult) in {"stress": (11, 3, "static_stress", 0.2, True),
                                            "disp": (12, 2, "static_disp", 1e-4, False)}.items():
        p, t, b = inputs(seed, C, thr, mult)
        d = M.stress_errors(p, t, b, prediction_type=kind, threshold=thr)
        out[f"{tag}_pred"], out[f"{tag}_target"], out[f"{tag}_batch"] = p.numpy(), t.numpy(), b.numpy()
        out[f"{tag}_kind"] = np.array(kind)
        out[f"{tag}_threshold"] = np.float64(thr)
        out[f"{tag}_keys"] = np.array(sorted(d))
        out[f"{tag}_vals"] = np.array([d[k] for k in sorted(d)], dtype=np.float64)
    np.savez(args.out, **out)
    print("wrote", args.out, len(out), "arrays")


if __name__ == "__main__":
    main()
