#!/usr/bin/env python
"""Same-process A/B of the node-level train step (static_disp on cfg2: N = 80,656, h = 512, C = 2,
ColumnScaler) with each of the five criteria that bgnn_graph_loss_ex serves: graph_mixed,
graph_max_rel, graph_mae_scaled, graph_mse_scaled, graph_rel_scaled, the kernels (`fused`) against the
torch route (`torch`: the names taken out of losses.FUSED_CRITERIA; the torch segment ops of
GraphMixedError / GraphMaxComponentRelativeError as they were before the kernels, the vectorised torch
fallback of the force-scaled classes). The decoder tail stays on its kernel in both settings.
The protocol is tools/node_head_ab.py's: the settings alternate in one process for R rounds of S
steps, the order reversed every other round, a cache-sized fill before every step, the graph caches
cleared; per setting the fastest, median and slowest round in ms/step, and the verdict of the rule
"fused stays the default only if its slowest round beats the torch route's fastest".

    python tools/graph_loss_ab.py                        # the A/B (AB_ROUNDS, AB_STEPS, AB_LOSSES)
    python tools/graph_loss_ab.py fused|torch graph_mixed   # a few steps of one setting, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/graph_loss_ab.py fused graph_mixed
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "buck-gnn_amd"))
import torch  # noqa: E402

import bgnn  # noqa: E402
from bgnn import losses, synthetic  # noqa: E402

LOSSES = ("graph_mixed", "graph_max_rel", "graph_mae_scaled", "graph_mse_scaled", "graph_rel_scaled")
EVERY = set(LOSSES)


def apply(name):
    losses.FUSED_CRITERIA = set(EVERY) if name == "fused" else set()


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
    norm = bgnn.ColumnScaler([0.1, -0.2], [0.5, 1.5])
    # a buffer larger than the 256 MB Infinity Cache, rewritten before every step: each step starts
    # from the same (cold) cache state whatever ran before it
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

    def step(crit):
        flush.fill_(1)
        bgnn.clear_caches()
        bgnn.train_step(model, batch, opt, crit, norm)

    if mode != "ab":
        apply(mode)
        crit = bgnn.get_loss_function(sys.argv[2] if len(sys.argv) > 2 else "graph_mixed")
        for _ in range(3 + steps):
            step(crit)
        torch.cuda.synchronize()
        print(f"{mode} {sys.argv[2:]}: {3 + steps} steps done")
        return
    names = ("torch", "fused")
    for loss_name in os.environ.get("AB_LOSSES", ",".join(LOSSES)).split(","):
        crit = bgnn.get_loss_function(loss_name)
        res = {s: [] for s in names}
        for s in names:
            apply(s)
            for _ in range(3):
                step(crit)
        for r in range(rounds):
            for s in (names if r % 2 == 0 else names[::-1]):
                apply(s)
                step(crit)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(crit)
                torch.cuda.synchronize()
                res[s].append((time.perf_counter() - t0) / steps * 1e3)
        for s in names:
            v = res[s]
            print(f"{loss_name:17s} {s:6s} min {min(v):8.3f}  median {statistics.median(v):8.3f}  max {max(v):8.3f} "
                  f"ms/step (flush included)  rounds {['%.3f' % t for t in v]}")
        verdict = "fused stays the default" if max(res["fused"]) < min(res["torch"]) else "fused off by default"
        print(f"{loss_name:17s} fused slowest {max(res['fused']):.3f} vs torch fastest {min(res['torch']):.3f}: {verdict}",
              flush=True)


if __name__ == "__main__":
    main()
