#!/usr/bin/env python
"""Inventory of the kernels one cfg2 train step launches that are not the library's own (`bgnn::`):
count and time per step and the torch op behind each, from a torch.profiler run, then the call sites
of those ops in this repository, recorded by wrapping the torch entry points for one step (as
tools/count_fills.py does for the fills). The library's launches go through ctypes, not through
torch ops, so every kernel listed here is one torch launched.
Usage: tools/kernel_inventory.py [steps]   (default 4 profiled steps after 3 warm-up steps)"""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "buck-gnn_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

import bgnn  # noqa: E402
from bgnn import synthetic  # noqa: E402


# torch entry points behind the kernels above, wrapped to record the innermost call site in this
# repository (the profiler's own stacks come back empty for ops run by the autograd thread)
TORCH_FNS = ("zeros", "zeros_like", "ones", "ones_like", "full", "full_like", "empty_like", "cat", "stack", "outer",
             "index_select", "_foreach_copy_", "_foreach_add_", "_foreach_zero_", "div", "mul", "sub", "clamp_min",
             "reshape", "flatten", "clone", "tensor", "as_tensor")
TENSOR_FNS = ("zero_", "fill_", "new_zeros", "new_full", "clone", "copy_", "to", "float", "long", "int", "contiguous",
              "reshape", "flatten", "index_select", "div", "mul", "sub", "add_", "mul_", "clamp_min", "clamp_min_",
              "__truediv__", "__mul__", "__rmul__", "__sub__", "__rsub__", "__add__", "__radd__")
calls = collections.Counter()
recording = [False]


def call_site():
    import traceback
    for fr in reversed(traceback.extract_stack()[:-2]):
        if fr.filename.startswith(ROOT) and not fr.filename.endswith("kernel_inventory.py"):
            return f"{os.path.relpath(fr.filename, ROOT)}:{fr.lineno}"
    return "the step loop of this tool (torch.optim.Adam, batch ids)"


def wrap(obj, name):
    orig = getattr(obj, name, None)
    if orig is None:
        return

    def f(*a, **k):
        if recording[0]:
            calls[(name.strip("_") if name.startswith("__") else name, call_site())] += 1
        return orig(*a, **k)
    setattr(obj, name, f)


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    dev = torch.device("cuda", 0)
    c = synthetic.CONFIGS["cfg2"]
    pool = [synthetic.make_mesh_graph(c["n"], g) for g in range(32)]
    store = bgnn.GraphStore(pool, dev)
    torch.manual_seed(0)
    model = bgnn.BuckGNN(synthetic.NUM_NODE_FEATURES, synthetic.NUM_EDGE_FEATURES, hidden_channels=512,
                         num_layers=6, pooling_layer="mean", prediction_type="buckling", dropout_rate=0.1,
                         model_name="GraphSage_addAggr").to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, weight_decay=1e-8, fused=True)
    crit, norm = bgnn.RelativeErrorLoss(), bgnn.EigenvalueScaler(center=1.0, scale=0.5)
    rng = np.random.default_rng(0)

    def step():
        ids = rng.permutation(32)[:16].tolist()
        bgnn.train_step(model, store.batch(ids), opt, crit, norm)

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    for n in TORCH_FNS:
        wrap(torch, n)
    for n in TENSOR_FNS:
        wrap(torch.Tensor, n)
    recording[0] = True
    step()
    torch.cuda.synchronize()
    recording[0] = False
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
    counts, times = collections.Counter(), collections.Counter()
    for ev in prof.events():
        for k in ev.kernels:
            if "bgnn::" in k.name:
                continue
            if ev.name.startswith("hip"):   # a runtime call the profiler could not pair with its op
                continue
            chain, par = [ev.name], getattr(ev, "cpu_parent", None)
            while par is not None and len(chain) < 4:   # the enclosing ops, innermost first
                chain.append(par.name)
                par = getattr(par, "cpu_parent", None)
            key = (k.name[:110], " < ".join(chain))
            counts[key] += 1
            times[key] += k.duration
    print(f"{steps} profiled steps; per step: count, us, kernel | torch op < enclosing ops")
    for key, n in sorted(counts.items(), key=lambda kv: -times[kv[0]]):
        print(f"{n / steps:6.2f} {times[key] / steps:8.1f}  {key[0]} | {key[1]}")
    report_sites()


def report_sites():
    print("one step: calls of the wrapped torch entry points by call site (views and no-op casts included)")
    for (name, where), n in sorted(calls.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print(f"{n:4d}  {name:14s} {where}")


if __name__ == "__main__":
    main()
