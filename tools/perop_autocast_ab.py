#!/usr/bin/env python
"""What do bf16 features on the PyG surface buy? A/B in one process at the cfg2 batch (H = 512),
cache flushed before every timed launch, HIP-event times, the median of --rounds launches repeated
--repeats times (the spread is that of the repeat medians):

  kernels  bgnn_spmm_fwd_bf16 / bgnn_spmm_bwd_bf16 (bf16 rows in and out) against bgnn_spmm_fwd /
           bgnn_spmm_bwd (f32) on the same graph, sum and mean, with each kernel's algorithmic
           bytes (every source row read once, every output row written once) as a fraction of 8 TB/s
  step     the per-module train step of GraphSage_addAggr (use_fused = False, bgnn BatchNorm,
           L = 6, Adam): forward + loss + backward + update, without autocast (float32: the code
           this feature leaves unchanged) and under torch.autocast("cuda", dtype=torch.bfloat16)
  loss     20 steps of each from the same weights (dropout 0): the relative difference of the
           last losses

Each part is one invocation (--part), so that a driver can run each under its own time limit.

Usage: python tools/perop_autocast_ab.py --part kernels|step|loss [--rounds 7] [--repeats 3]"""
import argparse
import contextlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "buck-gnn_amd"))

import torch  # noqa: E402

import bgnn  # noqa: E402
from bgnn import _lib, synthetic  # noqa: E402
from bgnn.graph import graph_for  # noqa: E402
from bgnn.nn import use_bgnn_batchnorm  # noqa: E402

H, L = 512, 6


def time_us(f, junk, rounds, warm=2):
    out = []
    for r in range(rounds + warm):
        junk.fill_(1.0)   # flush L2 / Infinity Cache: every launch starts cold
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        if r >= warm:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def medians(f, junk, rounds, repeats):
    meds = [statistics.median(time_us(f, junk, rounds)) for _ in range(max(3, repeats))]
    return {"median": round(statistics.median(meds), 1), "repeats": [round(m, 1) for m in meds],
            "spread": round(max(meds) - min(meds), 1)}


def part_kernels(b, dev, junk, args):
    N = b.num_nodes
    g = graph_for(b.edge_index, N)
    s = torch.cuda.current_stream().cuda_stream
    x = torch.randn(N, H, device=dev)
    xb = x.bfloat16()
    o32, o16 = torch.empty(N, H, device=dev), torch.empty(N, H, device=dev, dtype=torch.bfloat16)
    part = torch.empty(max(g.fwd.plan.n_chunks, g.bwd.plan.n_chunks, 1) * H, device=dev)
    frp = g.fwd.rowptr.data_ptr()
    res = {"N": N, "E": b.num_edges}
    for red, name in ((0, "sum"), (1, "mean")):
        launches = {
            "spmm_fwd_f32": lambda: _lib.call("bgnn_spmm_fwd", g.fwd.ref(), x.data_ptr(), H, H, red, o32.data_ptr(), H,
                                              None, part.data_ptr(), s),
            "spmm_fwd_bf16": lambda: _lib.call("bgnn_spmm_fwd_bf16", g.fwd.ref(), xb.data_ptr(), H, H, red,
                                               o16.data_ptr(), H, 0, part.data_ptr(), s),
            "spmm_bwd_f32": lambda: _lib.call("bgnn_spmm_bwd", g.bwd.ref(), g.perm_t.data_ptr(), frp, x.data_ptr(), H,
                                              H, red, o32.data_ptr(), H, part.data_ptr(), None, 0, s),
            "spmm_bwd_bf16": lambda: _lib.call("bgnn_spmm_bwd_bf16", g.bwd.ref(), frp, xb.data_ptr(), H, H, red,
                                               o16.data_ptr(), H, 0, part.data_ptr(), s),
        }
        out = {}
        for k, f in launches.items():
            t = medians(f, junk, args.rounds, args.repeats)
            nbytes = 2 * N * H * (2 if k.endswith("bf16") else 4)
            t["bytes"] = nbytes
            t["frac_of_8TBs"] = round(nbytes / (t["median"] * 1e-6) / 8e12, 3)
            out[k] = t
            print(f"  {name:4s} {k:14s} median {t['median']:8.1f} us  repeats {t['repeats']}  spread {t['spread']}"
                  f"  {nbytes / 1e6:.0f} MB at {t['frac_of_8TBs']:.2f} of 8 TB/s")
        res[name] = out
    return res


def make_model(dev, dropout):
    torch.manual_seed(0)
    model = bgnn.BuckGNN(16, 5, hidden_channels=H, num_layers=L, pooling_layer="mean", dropout_rate=dropout,
                         model_name="GraphSage_addAggr").to(dev).train()
    model.use_fused = False
    use_bgnn_batchnorm(model)
    return model, torch.optim.Adam(model.parameters(), lr=1e-3)


def stepper(model, opt, b, autocast):
    loss_fn = bgnn.RelativeErrorLoss()
    ctx = (lambda: torch.autocast("cuda", dtype=torch.bfloat16)) if autocast else contextlib.nullcontext

    def step():
        opt.zero_grad(set_to_none=True)
        with ctx():
            pred, _ = model(b.x, b.edge_index, b.edge_attr, b.batch)
            loss = loss_fn(pred.float(), b.y)
        loss.backward()
        opt.step()
        return loss
    return step


def part_step(b, dev, junk, args):
    res = {}
    for autocast in (False, True):
        model, opt = make_model(dev, 0.1)
        key = "step_us_autocast" if autocast else "step_us_f32"
        res[key] = medians(stepper(model, opt, b, autocast), junk, args.rounds, args.repeats)
        print(f"  {key:18s} median {res[key]['median']:9.1f} us  repeats {res[key]['repeats']}  "
              f"spread {res[key]['spread']}")
    return res


def part_loss(b, dev, junk, args):
    last = {}
    for autocast in (False, True):
        model, opt = make_model(dev, 0.0)
        step = stepper(model, opt, b, autocast)
        for _ in range(20):
            loss = step()
        last[autocast] = float(loss.detach())
    res = {"loss20_f32": last[False], "loss20_autocast": last[True],
           "loss20_rel_diff": abs(last[True] - last[False]) / abs(last[False])}
    print(f"  loss after 20 steps: f32 {last[False]:.6f}, autocast {last[True]:.6f}, "
          f"relative difference {res['loss20_rel_diff']:.3e}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "step", "loss"], required=True)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    junk = torch.empty(1 << 28, device=dev)
    b = synthetic.make_config_batch("cfg2").to(dev)
    bgnn.prepare(b.edge_index, b.num_nodes, b.batch, getattr(b, "num_graphs", None) or None)
    print(f"[cfg2] N={b.num_nodes} E={b.num_edges} part={args.part}")
    res = {"kernels": part_kernels, "step": part_step, "loss": part_loss}[args.part](b, dev, junk, args)
    print(json.dumps({args.part: res}))


if __name__ == "__main__":
    main()
