#!/usr/bin/env python
"""Same-process A/B of the static heads' error metrics: bgnn.losses.stress_errors on
bgnn_graph_metrics (FUSED_STRESS_ERRORS = True) against the torch segment ops (False: the code the
package had before the kernel, unchanged, so it is the baseline).

Cases: the cfg2 batch (16 graphs, N = 80,656) as static_stress (C = 3, threshold 0.2) and as
static_disp (C = 2, threshold 1e-4), and a batch of 128 small graphs (6 x 6 meshes, N = 4,608,
static_stress). Per case two measurements, the settings alternating for R rounds, the order reversed
every other round; per setting the fastest, median and slowest round:
  * call:  one stress_errors call, wall time including its read-back (ms/call over S calls; the
           batch vector's segment index is cached, as in a training loop, where the loss built it);
  * step:  bgnn.train_step(..., metrics=meter) on the h = 512 model, ms/step over S steps. With the
           switch off the meter runs the torch stress_errors after the step, read-back included: the
           reference loop's shape (TRAIN_FINAL.py:271-304). `no_meter` is the step alone.

    python tools/stress_metrics_ab.py                 # the A/B (AB_ROUNDS, AB_STEPS, AB_CASES)
    python tools/stress_metrics_ab.py fused|torch     # some calls of one setting, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/stress_metrics_ab.py fused
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

CASES = {
    # name: (batch maker, prediction type, C)
    "cfg2_stress": (lambda: synthetic.make_config_batch("cfg2"), "static_stress", 3),
    "cfg2_disp": (lambda: synthetic.make_config_batch("cfg2"), "static_disp", 2),
    "small128_stress": (lambda: synthetic.make_batch(6, 128), "static_stress", 3),
}
TRACE_CALLS = 10


def make_case(name, dev):
    maker, kind, C = CASES[name]
    batch = maker().to(dev)
    thr = losses.DEFAULT_THRESHOLD[kind]
    g = torch.Generator().manual_seed(0)
    N = batch.x.size(0)
    # normalised targets of unit scale; the scaler puts the denormalised ones around the threshold
    batch.y = torch.randn(N, C, generator=g).to(dev)
    norm = bgnn.ColumnScaler([0.1 * thr] * C, [3 * thr * (1 + 0.5 * c) for c in range(C)])
    return batch, kind, C, thr, norm


def summary(label, v, unit):
    print(f"{label:34s} min {min(v):8.3f}  median {statistics.median(v):8.3f}  max {max(v):8.3f} {unit}  "
          f"rounds {['%.3f' % t for t in v]}", flush=True)


def ab(settings, rounds, run_one, steps):
    """res[s] = per-round time per unit of run_one(s) (s applied inside), alternating order."""
    res = {s: [] for s in settings}
    for s in settings:
        for _ in range(3):
            run_one(s)
    for r in range(rounds):
        for s in (settings if r % 2 == 0 else settings[::-1]):
            run_one(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run_one(s)
            torch.cuda.synchronize()
            res[s].append((time.perf_counter() - t0) / steps * 1e3)
    return res


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "ab"
    rounds, steps = int(os.environ.get("AB_ROUNDS", "6")), int(os.environ.get("AB_STEPS", "8"))
    dev = torch.device("cuda", 0)
    if mode != "ab":
        batch, kind, C, thr, norm = make_case(os.environ.get("AB_CASES", "cfg2_stress").split(",")[0], dev)
        t = norm.denormalize(batch.y)
        p = t * (1 + 0.1 * torch.randn_like(t))
        losses.FUSED_STRESS_ERRORS = mode == "fused"
        for _ in range(3 + TRACE_CALLS):
            losses.stress_errors(p, t, batch.batch, kind, thr)
        torch.cuda.synchronize()
        print(f"{mode}: {3 + TRACE_CALLS} stress_errors calls done")
        return
    for name in os.environ.get("AB_CASES", ",".join(CASES)).split(","):
        batch, kind, C, thr, norm = make_case(name, dev)
        t = norm.denormalize(batch.y)
        p = t * (1 + 0.1 * torch.randn_like(t))

        def call(s):
            losses.FUSED_STRESS_ERRORS = s == "fused"
            losses.stress_errors(p, t, batch.batch, kind, thr)

        res = ab(["torch", "fused"], rounds, call, steps)
        for s, v in res.items():
            summary(f"{name} call {s}", v, "ms/call")
        torch.manual_seed(0)
        model = bgnn.BuckGNN(16, 5, hidden_channels=int(os.environ.get("AB_HIDDEN", "512")), num_layers=6,
                             dropout_rate=0.1, prediction_type=kind, model_name="GraphSage_addAggr").to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=1e-8, fused=True)
        crit = bgnn.GraphRelativeError()
        meter = losses.StressErrorMeter(kind)
        # a buffer larger than the 256 MB Infinity Cache, rewritten before every step: each step starts
        # from the same (cold) cache state whatever ran before it (tools/node_head_ab.py)
        flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)

        def step(s):
            losses.FUSED_STRESS_ERRORS = s == "fused_meter"
            flush.fill_(1)
            bgnn.clear_caches()
            bgnn.train_step(model, batch, opt, crit, norm, metrics=None if s == "no_meter" else meter)

        res = ab(["torch_meter", "fused_meter", "no_meter"], rounds, step, steps)
        for s, v in res.items():
            summary(f"{name} step {s}", v, "ms/step (flush included)")
        del flush
        losses.FUSED_STRESS_ERRORS = True


if __name__ == "__main__":
    main()
