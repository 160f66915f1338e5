#!/usr/bin/env python
"""Same-process A/B of the node-level train step (static_disp on cfg2: N = 80,656, h = 512, C = 2,
GraphRelativeError, ColumnScaler): the torch decoder and torch per-graph loss (both switches off: the
computation the code had before the head kernels) against the bgnn_head2 tail and bgnn_graph_loss.
The settings alternate for R rounds of S steps, the order reversed every other round; per setting the
fastest, median and slowest round in ms/step.

    python tools/node_head_ab.py                 # the A/B (AB_ROUNDS, AB_STEPS)
    python tools/node_head_ab.py fused|torch     # a few steps of one setting, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/node_head_ab.py fused
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "buck-gnn_amd"))
import torch  # noqa: E402

import bgnn  # noqa: E402
from bgnn import fused, losses, synthetic  # noqa: E402

SETTINGS = {"torch": (False, False), "fused": (True, True), "head_only": (True, False), "loss_only": (False, True)}


def apply(name):
    fused.FUSED_NODE_HEAD, losses.FUSED_GRAPH_LOSS = SETTINGS[name]


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
    rounds, steps = int(os.environ.get("AB_ROUNDS", "6")), int(os.environ.get("AB_STEPS", "8"))
    dev = torch.device("cuda", 0)
    batch = synthetic.make_config_batch(os.environ.get("AB_CONFIG", "cfg2")).to(dev)
    torch.manual_seed(0)
    batch.y = torch.randn(batch.x.size(0), 2, device=dev)
    model = bgnn.BuckGNN(16, 5, hidden_channels=int(os.environ.get("AB_HIDDEN", "512")), num_layers=6,
                         dropout_rate=0.1, prediction_type="static_disp",
                         model_name=os.environ.get("AB_MODEL", "GraphSage_addAggr")).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-8, fused=True)
    crit, norm = bgnn.GraphRelativeError(), bgnn.ColumnScaler([0.1, -0.2], [0.5, 1.5])
    # a buffer larger than the 256 MB Infinity Cache, rewritten before every step: each step starts
    # from the same (cold) cache state whatever ran before it
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

    def step():
        flush.fill_(1)
        bgnn.clear_caches()
        bgnn.train_step(model, batch, opt, crit, norm)

    if mode != "ab":
        apply(mode)
        for _ in range(3 + steps):
            step()
        torch.cuda.synchronize()
        print(f"{mode}: {3 + steps} steps done")
        return
    names = os.environ.get("AB_SETTINGS", "torch,fused,head_only,loss_only").split(",")
    res = {s: [] for s in names}
    for s in names:
        apply(s)
        for _ in range(3):
            step()
    for r in range(rounds):
        for s in (names if r % 2 == 0 else names[::-1]):
            apply(s)
            step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            res[s].append((time.perf_counter() - t0) / steps * 1e3)
    for s in names:
        v = res[s]
        print(f"{s:10s} min {min(v):8.3f}  median {statistics.median(v):8.3f}  max {max(v):8.3f} ms/step "
              f"(flush included)  rounds {['%.3f' % t for t in v]}")


if __name__ == "__main__":
    main()
