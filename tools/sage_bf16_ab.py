#!/usr/bin/env python
"""What do the launches of the bf16 training mode (BuckGNN.sage_bf16) cost next to the f32-accurate
ones they replace? One process, the cfg2 batch at H = 512, the cache flushed before every timed
launch, HIP-event times, medians of --rounds, repeated --repeats times (the range is that of the
repeat medians):

  aggregation  bgnn_sage_fwd (f32 z) against bgnn_sage_fwd_bf16 (bf16 z), both with the BatchNorm
               sums; the new kernel's algorithmic bytes (z N*2H*2 read, o N*H*4 and nrm N*4 written)
               as a fraction of 8 TB/s
  GEMMs        the layer's three N-row products -- forward z = x [W_l;W_r]^T, dgrad dx = dz [W_l;W_r],
               wgrad dW = dz^T x -- as f16x3 (fused.gemm with the operand maxima given, as the layer
               loop carries them) against bf16 operands (gemm_bf16 with a bf16 z for the forward,
               fused.gemm(bf16=True) for the two gradients). The model's f16x3 forward and dgrad
               additionally take pre-split weight images and the drop-add epilogue; the step times of
               bench.py are the comparison of the two paths, this tool sizes the launches.

Usage: python tools/sage_bf16_ab.py [--rounds 7] [--repeats 3]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "buck-gnn_amd"))

import torch  # noqa: E402

import bgnn  # noqa: E402
from bgnn import _lib, fused, synthetic  # noqa: E402
from bgnn.graph import graph_for  # noqa: E402

H = 512


def time_us(f, junk, rounds, warm=2):
    out = []
    for r in range(rounds + warm):
        junk.fill_(1.0)   # flush L2 / Infinity Cache: every launch starts cold, as inside a step
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        if r >= warm:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    junk = torch.empty(1 << 28, device=dev)
    torch.manual_seed(0)
    b = synthetic.make_config_batch("cfg2").to(dev)
    N, E = b.num_nodes, b.num_edges
    bgnn.prepare(b.edge_index, N, b.batch, getattr(b, "num_graphs", None) or None)
    g = graph_for(b.edge_index, N)
    s = torch.cuda.current_stream().cuda_stream
    x = torch.randn(N, H, device=dev)
    wcat = torch.randn(2 * H, H, device=dev) / H ** 0.5
    wcat_t = wcat.t().contiguous()
    dz = torch.randn(N, 2 * H, device=dev)
    bias = torch.zeros(H, device=dev)
    x_amax, w_amax, dz_amax = fused.absmax(x), fused.absmax(wcat), fused.absmax(dz)
    z = torch.empty(N, 2 * H, device=dev)
    zb = torch.empty(N, 2 * H, device=dev, dtype=torch.bfloat16)
    dx, dw = torch.empty(N, H, device=dev), torch.empty(2 * H, H, device=dev)
    o, nrm = torch.empty(N, H, device=dev), torch.empty(N, device=dev)
    bnp = torch.empty(max(_lib.query("bgnn_sage_fwd_slots", g.fwd.ref()),
                          _lib.query("bgnn_sage_fwd_bf16_slots", g.fwd.ref())), 2, H, device=dev)
    part = torch.empty(max(g.fwd.plan.n_chunks, 1) * H, device=dev)
    launches = {
        "sage_fwd": lambda: _lib.call("bgnn_sage_fwd", g.fwd.ref(), z.data_ptr(), 2 * H, z[:, H:].data_ptr(), 2 * H,
                                      bias.data_ptr(), H, 0, o.data_ptr(), nrm.data_ptr(), bnp.data_ptr(),
                                      part.data_ptr(), None, 0, s),
        "sage_fwd_bf16": lambda: _lib.call("bgnn_sage_fwd_bf16", g.fwd.ref(), zb.data_ptr(), 2 * H, bias.data_ptr(),
                                           H, 0, o.data_ptr(), nrm.data_ptr(), bnp.data_ptr(), part.data_ptr(), s),
        "gemm_fwd_f16x3": lambda: fused.gemm(x, wcat, False, True, out=z, a_amax=x_amax, b_amax=w_amax),
        "gemm_fwd_bf16": lambda: fused.gemm_bf16(x, wcat, False, True, out=zb),
        "gemm_dgrad_f16x3": lambda: fused.gemm(dz, wcat_t, False, True, out=dx, a_amax=dz_amax, b_amax=w_amax),
        "gemm_dgrad_bf16": lambda: fused.gemm(dz, wcat_t, False, True, out=dx, bf16=True),
        "gemm_wgrad_f16x3": lambda: fused.gemm(dz, x, True, False, out=dw, a_amax=dz_amax, b_amax=x_amax),
        "gemm_wgrad_bf16": lambda: fused.gemm(dz, x, True, False, out=dw, bf16=True),
    }
    fused.gemm(x, wcat, False, True, out=z, a_amax=x_amax, b_amax=w_amax)   # z / zb hold finite values
    zb.copy_(z)
    res = {"N": N, "E": E, "H": H, "us": {}}
    for k, f in launches.items():
        meds = [statistics.median(time_us(f, junk, args.rounds)) for _ in range(args.repeats)]
        res["us"][k] = {"median": round(statistics.median(meds), 1), "min": round(min(meds), 1),
                        "max": round(max(meds), 1)}
        print(f"  {k:18s} {res['us'][k]['median']:9.1f} us  (repeat medians {res['us'][k]['min']} .. "
              f"{res['us'][k]['max']})")
    nbytes = N * 2 * H * 2 + N * H * 4 + N * 4
    res["sage_fwd_bf16_bytes"] = nbytes
    res["sage_fwd_bf16_frac_of_8TBs"] = round(nbytes / (res["us"]["sage_fwd_bf16"]["median"] * 1e-6) / 8e12, 3)
    print(f"  sage_fwd_bf16 moves {nbytes / 1e6:.0f} MB at {res['sage_fwd_bf16_frac_of_8TBs']:.2f} of 8 TB/s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
