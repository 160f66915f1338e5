#!/usr/bin/env python
"""What do the launches of the max model's bf16 training mode (BuckGNN.sage_bf16 = "all") cost next
to the f32-accurate ones they replace? One process, the cfg2 batch at H = 512, the cache flushed
before every timed launch, HIP-event times, medians of --rounds, repeated --repeats times (the range
is that of the repeat medians):

  gather        bgnn_spmm_fwd(MAX) with the argmax state (f32 agg) against bgnn_spmm_max_pack_bf16
                (bf16 [agg | x] and the same state); the pack kernel's algorithmic bytes -- x N*H*4
                read once as rows (the gathered re-reads are cache traffic), a N*2H*2 and the state
                N*H written -- as a fraction of 8 TB/s
  forward GEMM  y = [agg | x] [W_l | W_r]^T, K = 2H: f16x3 on the f32 pair read in place (fused.Pair)
                against the mode's two bf16 products on the planes of a, K = H each, stored bf16 as
                the planes of an [N, 2H] y (the sum of both launches); and, for comparison only, one
                bf16 product over K = 2H with one rounding
  row epilogue  normalize + BatchNorm sums: bgnn_sage_fwd on the f32 y over an empty CSR against
                bgnn_sage_fwd_bf16 over the identity CSR, which adds the two bf16 planes of y
  merged dgrad  [dagg | t] = dh [W_l | W_r]: f16x3 against fused.gemm(bf16=True)
  wgrad         [dW_l^T ; dW_r^T] = [agg | x]^T dh: f16x3 on the f32 pair against gemm_bf16 on a
                (storage 1, the layer's form), and with the operands exchanged, [dW_l | dW_r] = dh^T a
                (storage 2)

The model's f16x3 skip layers additionally take the drop-add epilogue; the step times of bench.py
are the comparison of the two paths, this tool sizes the launches.

Usage: python tools/sage_bf16_max_ab.py [--rounds 7] [--repeats 3]"""
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
from bgnn.graph import empty_csr, graph_for, identity_csr  # noqa: E402

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
    ecsr = empty_csr(N, dev)
    icsr = identity_csr(N, dev)
    s = torch.cuda.current_stream().cuda_stream
    both = torch.empty(2, N, H, device=dev)            # agg and x as the f32 layer holds them
    agg, x = both[0], both[1]
    x.copy_(torch.relu(torch.randn(N, H, device=dev)))
    w_l, w_r = torch.randn(H, H, device=dev) / H ** 0.5, torch.randn(H, H, device=dev) / H ** 0.5
    wk = torch.cat([w_l, w_r], 1)                      # [H, 2H]
    wkt = wk.t().contiguous()                          # [W_l^T ; W_r^T], [2H, H]
    wk16 = wk.bfloat16()
    dh = torch.randn(N, H, device=dev)
    bias = torch.zeros(H, device=dev)
    x_amax, w_amax, dh_amax = fused.absmax(x), fused.absmax(wk), fused.absmax(dh)
    arg = torch.empty(_lib.query("bgnn_spmm_max_arg_bytes", N, H, g.fwd.plan.n_heavy), dtype=torch.uint8, device=dev)
    part = torch.empty(max(g.fwd.plan.n_chunks, 1) * H * 2, device=dev)
    a = torch.empty(N, 2 * H, device=dev, dtype=torch.bfloat16)
    y = torch.empty(N, H, device=dev)
    yb2 = torch.empty(N, 2 * H, device=dev, dtype=torch.bfloat16)
    yb = yb2[:, H:]
    dt = torch.empty(N, 2 * H, device=dev)
    dwt, dw = torch.empty(2 * H, H, device=dev), torch.empty(H, 2 * H, device=dev)
    o, nrm = torch.empty(N, H, device=dev), torch.empty(N, device=dev)
    bnp = torch.empty(max(_lib.query("bgnn_sage_fwd_slots", ecsr.ref()),
                          _lib.query("bgnn_sage_fwd_bf16_slots", icsr.ref())), 2, H, device=dev)
    pair = fused.Pair(agg, x)
    launches = {
        "gather_f32": lambda: _lib.call("bgnn_spmm_fwd", g.fwd.ref(), x.data_ptr(), H, H, 2, agg.data_ptr(), H,
                                        arg.data_ptr(), part.data_ptr(), s),
        "gather_pack_bf16": lambda: _lib.call("bgnn_spmm_max_pack_bf16", g.fwd.ref(), x.data_ptr(), H, H,
                                              a.data_ptr(), 2 * H, arg.data_ptr(), part.data_ptr(), s),
        "gemm_fwd_f16x3": lambda: fused.gemm(pair, wk, False, True, out=y, a_amax=x_amax, b_amax=w_amax),
        "gemm_fwd_bf16": lambda: (fused.gemm_bf16(a[:, :H], w_l, False, True, out=yb2[:, :H]),
                                  fused.gemm_bf16(a[:, H:], w_r, False, True, out=yb)),
        "gemm_fwd_bf16_k2h": lambda: fused.gemm_bf16(a, wk16, False, True, out=yb),
        "rows_f32": lambda: _lib.call("bgnn_sage_fwd", ecsr.ref(), y.data_ptr(), H, y.data_ptr(), H, bias.data_ptr(),
                                      H, 0, o.data_ptr(), nrm.data_ptr(), bnp.data_ptr(), None, None, 0, s),
        "rows_bf16": lambda: _lib.call("bgnn_sage_fwd_bf16", icsr.ref(), yb2.data_ptr(), 2 * H, bias.data_ptr(), H, 0,
                                       o.data_ptr(), nrm.data_ptr(), bnp.data_ptr(), None, s),
        "gemm_dgrad_f16x3": lambda: fused.gemm(dh, wkt, False, True, out=dt, a_amax=dh_amax, b_amax=w_amax),
        "gemm_dgrad_bf16": lambda: fused.gemm(dh, wkt, False, True, out=dt, bf16=True),
        "gemm_wgrad_f16x3": lambda: fused.gemm(pair, dh, True, False, out=dwt, a_amax=x_amax, b_amax=dh_amax),
        "gemm_wgrad_bf16": lambda: fused.gemm_bf16(a, dh, True, False, out=dwt),
        "gemm_wgrad_bf16_dh_a": lambda: fused.gemm_bf16(dh, a, True, False, out=dw),
    }
    res = {"N": N, "E": E, "H": H, "us": {}}
    for k, f in launches.items():   # (in order: the gathers fill agg and a before the products read them)
        meds = [statistics.median(time_us(f, junk, args.rounds)) for _ in range(args.repeats)]
        res["us"][k] = {"median": round(statistics.median(meds), 1), "min": round(min(meds), 1),
                        "max": round(max(meds), 1)}
        print(f"  {k:18s} {res['us'][k]['median']:9.1f} us  (repeat medians {res['us'][k]['min']} .. "
              f"{res['us'][k]['max']})")
    assert torch.equal(a[:, :H], agg.bfloat16()) and torch.equal(a[:, H:], x.bfloat16())
    nbytes = N * H * 4 + N * 2 * H * 2 + N * H
    res["pack_bytes"] = nbytes
    res["pack_frac_of_8TBs"] = round(nbytes / (res["us"]["gather_pack_bf16"]["median"] * 1e-6) / 8e12, 3)
    print(f"  gather_pack_bf16 moves {nbytes / 1e6:.0f} MB at {res['pack_frac_of_8TBs']:.2f} of 8 TB/s")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
