#!/usr/bin/env python
"""Generate tests/golden/heads/losses_scaled.npz from the REFERENCE's own eight
criterion(pred, target, batch, x) classes (Utils/Losses.py:303-695: GraphRelativeError,
GraphMixedError, GraphMSELoss, GraphMAELoss, GraphMaxComponentRelativeError, ScaledGraphMAELoss,
ScaledGraphMSELoss, ScaledGraphRELoss): values with and without a batch vector, the force-scaled
ones also with force_scaling=False, and the reference's own autograd gradient with respect to pred.

Runs only where a checkout of the reference exists (--ref, or the environment's BGNN_REFERENCE); its
modules are imported unchanged (torch_scatter, which Losses.py imports, comes from the oracle's CPU
restatement, oracle/shim.py). The fixture holds only data: the seeded inputs and the reference's
outputs.

    python tests/golden/make_golden_losses_scaled.py --ref /path/to/reference
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_losses import inputs, load  # noqa: E402

# the three shape families of losses.npz, and one whose forces are small enough that min_scale wins
CASES = {"s3": (1, [37, 5, 64, 18], 3, 1.0), "d3": (2, [23, 41, 9], 3, 1.0), "v1": (3, [30, 12, 25], 1, 1.0),
         "m3": (4, [11, 29], 3, 1e-4)}
NAMES = {"rel": "GraphRelativeError", "mixed": "GraphMixedError", "mse": "GraphMSELoss", "mae": "GraphMAELoss",
         "maxc": "GraphMaxComponentRelativeError", "mae_scaled": "ScaledGraphMAELoss",
         "mse_scaled": "ScaledGraphMSELoss", "rel_scaled": "ScaledGraphRELoss"}


def features(seed, N, force):
    """x [N, 16]: forces in columns 3:5 (zero on most rows, as point loads), the last column the
    super-node flag (a few rows set; the classes do not look at it: they sum what they are given)."""
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.randn(N, 16, generator=g)
    loaded = torch.rand(N, generator=g) < 0.2
    x[:, 3:5] = torch.randn(N, 2, generator=g) * force * loaded[:, None]
    x[:, -1] = (torch.rand(N, generator=g) < 0.05).float()
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("BGNN_REFERENCE"), required="BGNN_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=os.path.join(HERE, "heads", "losses_scaled.npz"))
    args = ap.parse_args()
    from oracle import shim
    shim.install()
    L = load(os.path.join(args.ref, "Utils", "Losses.py"), "ref_losses")
    shim.uninstall()
    out = {}
    for tag, (seed, sizes, C, force) in CASES.items():
        p, t, b = inputs(seed, sizes, C)
        if C == 1:
            p, t = p[:, 0].contiguous(), t[:, 0].contiguous()
        x = features(seed, b.numel(), force)
        out[f"{tag}_pred"], out[f"{tag}_target"], out[f"{tag}_batch"], out[f"{tag}_x"] = (
            p.numpy(), t.numpy(), b.numpy(), x.numpy())
        for name, cls in NAMES.items():
            variants = {"": {}}
            if name.endswith("_scaled"):
                variants["_noforce"] = {"force_scaling": False}
            for suffix, kw in variants.items():
                mod = getattr(L, cls)(**kw)
                for bsuffix, bv in (("", b), ("_nobatch", None)):
                    pr = p.clone().requires_grad_(True)
                    v = mod(pr, t, bv, x)
                    g, = torch.autograd.grad(v, pr)
                    out[f"{tag}_{name}{suffix}{bsuffix}"] = np.float64(v.item())
                    out[f"{tag}_{name}{suffix}{bsuffix}_grad"] = g.numpy()
    np.savez(args.out, **out)
    print("wrote", args.out, len(out), "arrays")


if __name__ == "__main__":
    main()
