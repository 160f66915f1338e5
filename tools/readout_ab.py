#!/usr/bin/env python
"""Train-step time of the super-node and MLP readouts on a cfg3-shaped GraphStore batch: 16
super-node meshes of 71 x 71 (N = 80,672), h = 512, L = 6, GraphSage_addAggr; per pooling_layer one
model, timed through bgnn.train_step with HIP events.

Public API only, so the same file runs on any commit: the A/B of a change to the readout routes is
this tool run on both trees, alternating, in one job (a tree without the routes times the mask /
nonzero / gather readout). Per mode: AB_WARMUP steps, then AB_ROUNDS rounds of AB_STEPS steps, each
step between two events, a cache-sized fill before every step (outside the events); a round's figure
is the median of its steps. Printed per mode: the fastest, median and slowest round in ms/step.
`static_stress` is the node-level head with pooling_layer = supernode_only and GraphRelativeError.

    python tools/readout_ab.py                          # every mode (AB_MODES selects)
    AB_FRESH_BATCH=1 python tools/readout_ab.py         # a new store batch every step, inside the events
"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "buck-gnn_amd"))
import torch  # noqa: E402

import bgnn  # noqa: E402
from bgnn import synthetic  # noqa: E402

MODES = ("mean", "mean_no_super", "supernode_only", "supernode_with_pooling", "mlp_no_super", "mlp", "static_stress")


def main():
    rounds, steps = int(os.environ.get("AB_ROUNDS", "3")), int(os.environ.get("AB_STEPS", "10"))
    warmup = int(os.environ.get("AB_WARMUP", "4"))
    fresh = os.environ.get("AB_FRESH_BATCH", "0") == "1"
    n, graphs, h = int(os.environ.get("AB_MESH", "71")), int(os.environ.get("AB_GRAPHS", "16")), \
        int(os.environ.get("AB_HIDDEN", "512"))
    dev = torch.device("cuda", 0)
    data = [synthetic.make_mesh_graph(n, g, super_node=True) for g in range(graphs)]
    store = bgnn.GraphStore(data, device=dev)
    for i, d in enumerate(data):   # node-level targets: one row per real node
        d.y = torch.randn(d.num_nodes - 1, 3, generator=torch.Generator().manual_seed(100 + i))
    store_nodes = bgnn.GraphStore(data, device=dev)
    ids = list(range(graphs))
    # a buffer larger than the 256 MB Infinity Cache, rewritten before every step
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    for mode in os.environ.get("AB_MODES", ",".join(MODES)).split(","):
        nodes = mode == "static_stress"
        torch.manual_seed(0)
        model = bgnn.BuckGNN(16, 5, hidden_channels=h, num_layers=6, dropout_rate=0.1,
                             pooling_layer="supernode_only" if nodes else mode,
                             prediction_type="static_stress" if nodes else "buckling",
                             model_name=os.environ.get("AB_MODEL", "GraphSage_addAggr")).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-8, fused=True)
        crit = bgnn.GraphRelativeError() if nodes else bgnn.RelativeErrorLoss()
        st = store_nodes if nodes else store
        batch = st.batch(ids)

        def step():
            flush.fill_(1)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            bgnn.train_step(model, st.batch(ids) if fresh else batch, opt, crit)
            t1.record()
            return t0, t1

        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        res = []
        for _ in range(rounds):
            ev = [step() for _ in range(steps)]
            torch.cuda.synchronize()
            res.append(statistics.median(a.elapsed_time(b) for a, b in ev))
        print(f"{mode:24s} min {min(res):8.3f}  median {statistics.median(res):8.3f}  max {max(res):8.3f} ms/step  "
              f"rounds {['%.3f' % t for t in res]}", flush=True)


if __name__ == "__main__":
    main()
