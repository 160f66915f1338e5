#!/usr/bin/env python
"""Compare two `bench.py --dump-outputs DIR` directories bit for bit: the same file names, and per
file the same dtype, shape and bytes (NaNs must match by bits too). Prints one line per differing
file and exits 1 when any differs. Usage: tools/compare_dumps.py DIR_A DIR_B"""
import os
import sys

import numpy as np


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    a = sorted(f for f in os.listdir(a_dir) if f.endswith(".npy"))
    b = sorted(f for f in os.listdir(b_dir) if f.endswith(".npy"))
    bad = 0
    for f in sorted(set(a) ^ set(b)):
        print(f"only in one directory: {f}")
        bad += 1
    for f in sorted(set(a) & set(b)):
        x, y = np.load(os.path.join(a_dir, f)), np.load(os.path.join(b_dir, f))
        if x.dtype != y.dtype or x.shape != y.shape:
            print(f"{f}: {x.dtype}{x.shape} vs {y.dtype}{y.shape}")
            bad += 1
        elif x.tobytes() != y.tobytes():
            d = np.flatnonzero(x.reshape(-1).view(np.uint8).reshape(x.size, -1)
                               != y.reshape(-1).view(np.uint8).reshape(y.size, -1)).size
            with np.errstate(all="ignore"):
                m = float(np.nanmax(np.abs(x.astype(np.float64) - y.astype(np.float64))))
            print(f"{f}: {d} differing bytes of {x.nbytes}, max |a - b| = {m:.3e}")
            bad += 1
    print(f"{len(set(a) & set(b))} files compared, {bad} differ")
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(main())
