#!/usr/bin/env python
"""Same-process A/B of the node-level eval forward (static_stress on cfg2: N = 80,656, h = 512,
C = 3; GraphSage_addAggr and GraphSage_maxAggr) under three settings:

    f32            the f32-accurate path
    bf16           infer_bf16 alone: bf16 layer loop, f32 hand-over, f32 decoder
    bf16_decoder   infer_bf16 with infer_bf16_decoder: the last layer stores bf16, the decoder
                   reads those rows (fused.node_head_bf16)

The settings alternate for R rounds of S forwards, the order reversed every other round; per
setting the fastest, median and slowest round in ms/forward. Every forward starts after a 512 MB
fill with the graph caches cleared, as tools/node_head_ab.py's steps do (the times include both).
Also printed: the relative L2 difference of each bf16 setting's prediction against f32's.

    python tools/node_infer_ab.py                          # the A/B (AB_ROUNDS, AB_STEPS, AB_MODELS)
    python tools/node_infer_ab.py bf16_decoder             # a few forwards of one setting (AB_MODEL), for
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/node_infer_ab.py bf16_decoder
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "buck-gnn_amd"))
import torch  # noqa: E402

import bgnn  # noqa: E402
from bgnn import synthetic  # noqa: E402
from bgnn.graph import prepare  # noqa: E402

SETTINGS = ("f32", "bf16", "bf16_decoder")


def apply(model, name):
    on = "all" if name != "f32" else False   # ("all" covers the max model; a sum model runs as under True)
    model.infer_bf16, model.infer_bf16_decoder = on, name == "bf16_decoder"


def build(name, dev):
    torch.manual_seed(0)
    model = bgnn.BuckGNN(16, 5, hidden_channels=int(os.environ.get("AB_HIDDEN", "512")), num_layers=6,
                         dropout_rate=0.1, prediction_type="static_stress", model_name=name).to(dev).eval()
    with torch.no_grad():   # running statistics that are not the initial 0 / 1
        for bn in model.batch_norms:
            bn.running_mean.normal_(0.0, 0.1)
            bn.running_var.uniform_(1.0, 1.2)
    return model


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
    rounds, steps = int(os.environ.get("AB_ROUNDS", "6")), int(os.environ.get("AB_STEPS", "40"))
    dev = torch.device("cuda", 0)
    batch = synthetic.make_config_batch(os.environ.get("AB_CONFIG", "cfg2")).to(dev)
    # a buffer larger than the 256 MB Infinity Cache, rewritten before every forward: each forward
    # starts from the same (cold) cache state whatever ran before it
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

    @torch.no_grad()
    def forward(model):
        flush.fill_(1)
        bgnn.clear_caches()
        prepare(batch.edge_index, batch.x.size(0), batch.batch, getattr(batch, "num_graphs", None) or None)
        return model(batch.x, batch.edge_index, batch.edge_attr, batch.batch)[0]

    if mode != "ab":
        model = build(os.environ.get("AB_MODEL", "GraphSage_addAggr"), dev)
        apply(model, mode)
        for _ in range(3 + steps):
            forward(model)
        torch.cuda.synchronize()
        print(f"{model.model_name} {mode}: {3 + steps} forwards done")
        return
    for name in os.environ.get("AB_MODELS", "GraphSage_addAggr,GraphSage_maxAggr").split(","):
        model = build(name, dev)
        res = {s: [] for s in SETTINGS}
        pred = {}
        for s in SETTINGS:
            apply(model, s)
            for _ in range(3):
                pred[s] = forward(model)
        for r in range(rounds):
            for s in (SETTINGS if r % 2 == 0 else SETTINGS[::-1]):
                apply(model, s)
                forward(model)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    forward(model)
                torch.cuda.synchronize()
                res[s].append((time.perf_counter() - t0) / steps * 1e3)
        print(f"{name}  N={batch.x.size(0)}  h={model.hidden_channels}  static_stress  "
              f"{rounds} rounds of {steps} forwards")
        for s in SETTINGS:
            v = res[s]
            print(f"  {s:13s} min {min(v):7.3f}  median {statistics.median(v):7.3f}  max {max(v):7.3f} ms/forward "
                  f"(flush and graph build included)  rounds {['%.3f' % t for t in v]}")
        ref = pred["f32"].double()
        for s in SETTINGS[1:]:
            d = float((pred[s].double() - ref).norm() / ref.norm())
            print(f"  {s:13s} relative L2 difference of the prediction against f32: {d:.3e}")
        b, c = res["bf16"], res["bf16_decoder"]
        print(f"  bf16_decoder slowest {max(c):.3f} vs bf16 fastest {min(b):.3f}: "
              f"{'faster in every round' if max(c) < min(b) else 'no gain outside the spread'}")


if __name__ == "__main__":
    main()
