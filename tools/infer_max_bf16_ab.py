#!/usr/bin/env python
"""What does the bf16 max inference path (BuckGNN.infer_bf16 = "all") buy? A/B in one process on
the eval forward of GraphSage_maxAggr (h = 512, L = 6) on the cfg2 batch, the method of
tools/infer_bf16_ab.py: cache flushed before every timed launch, HIP-event times, medians of
--rounds, the spread that of --repeats repeat medians.

  forward   the whole eval forward under no_grad, flag off / "all", and the prediction's rel-L2
            between the two paths
  kernels   each launch alone and cold: bgnn_spmm_max_bf16 (no arg) against bgnn_spmm_fwd(MAX)
            without arg on the same values; the K = 2H bf16 GEMM; bgnn_sage_tail_bf16 (bf16 out,
            skip and BatchNorm coefficients). The new kernels' algorithmic bytes as a fraction of
            8 TB/s: gather N*H*2 read + N*H*2 written, tail 2 * N*H*2 read + N*H*2 written.

Usage: python tools/infer_max_bf16_ab.py [--rounds 7] [--repeats 3]"""
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

H, L = 512, 6


def time_us(f, junk, rounds, warm=2):
    out = []
    for r in range(rounds + warm):
        junk.fill_(1.0)   # flush L2 / Infinity Cache: every launch starts cold, as inside a forward
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        torch.cuda.synchronize()
        if r >= warm:
            out.append(e0.elapsed_time(e1) * 1e3)
    return out


def repeat_medians(f, junk, rounds, repeats):
    meds = [statistics.median(time_us(f, junk, rounds)) for _ in range(max(3, repeats))]
    return {"median": round(statistics.median(meds), 1), "repeats": [round(m, 1) for m in meds],
            "spread": round(max(meds) - min(meds), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    junk = torch.empty(1 << 28, device=dev)
    torch.manual_seed(0)
    model = bgnn.BuckGNN(16, 5, hidden_channels=H, num_layers=L, pooling_layer="mean", dropout_rate=0.0,
                         model_name="GraphSage_maxAggr").to(dev).eval()
    b = synthetic.make_config_batch("cfg2").to(dev)
    N, E = b.num_nodes, b.num_edges
    bgnn.prepare(b.edge_index, N, b.batch, getattr(b, "num_graphs", None) or None)

    def fwd():
        with torch.no_grad():
            return model(b.x, b.edge_index, b.edge_attr, b.batch)[0]

    res = {"N": N, "E": E}
    preds = {}
    for flag in (False, "all"):
        model.infer_bf16 = flag
        preds[flag] = fwd().double()
        res["forward_us_all" if flag else "forward_us_off"] = repeat_medians(fwd, junk, args.rounds, args.repeats)
    model.infer_bf16 = False
    res["pred_rel_l2"] = float((preds["all"] - preds[False]).norm() / preds[False].norm())

    # the launches of one layer (layer 1: skip connection, BatchNorm), each alone
    g = graph_for(b.edge_index, N)
    conv, bn = model.sage_blocks_max[1], model.batch_norms[1]
    s = torch.cuda.current_stream().cuda_stream
    buf = torch.randn(N, 2 * H, device=dev).bfloat16()
    xf = buf[:, H:].float().contiguous()
    of = torch.empty(N, H, device=dev)
    y = torch.empty(N, H, device=dev, dtype=torch.bfloat16)
    nxt = torch.empty(N, 2 * H, device=dev, dtype=torch.bfloat16)
    w = fused.infer_weights_max(conv)
    scale, shift = fused.bn_eval_coeffs(bn)
    bias = conv.lin_l.bias.detach()
    n_chunks = g.fwd.plan.n_chunks
    part = torch.empty(max(n_chunks, 1) * H * 2, device=dev)
    launches = {
        "spmm_fwd_max_f32": lambda: _lib.call("bgnn_spmm_fwd", g.fwd.ref(), xf.data_ptr(), H, H, 2, of.data_ptr(), H,
                                              None, part.data_ptr(), s),
        "spmm_max_bf16": lambda: _lib.call("bgnn_spmm_max_bf16", g.fwd.ref(), buf[:, H:].data_ptr(), 2 * H, H,
                                           buf.data_ptr(), 2 * H, None, part.data_ptr(), s),
        "gemm_bf16_k2h": lambda: fused.gemm_bf16(buf, w, False, True, out=y),
        "sage_tail_bf16": lambda: _lib.call("bgnn_sage_tail_bf16", y.data_ptr(), H, bias.data_ptr(),
                                            scale.data_ptr(), shift.data_ptr(), buf[:, H:].data_ptr(), 2 * H, N, H,
                                            nxt[:, H:].data_ptr(), 2 * H, 0, s),
    }
    kern = {k: repeat_medians(f, junk, args.rounds, args.repeats) for k, f in launches.items()}
    # (the same values in: the two gathers must agree exactly)
    launches["spmm_fwd_max_f32"]()
    launches["spmm_max_bf16"]()
    torch.cuda.synchronize()
    res["gathers_equal"] = bool(torch.equal(buf[:, :H].float(), of))
    res["kernels_us"] = kern
    gather_bytes, tail_bytes = 2 * N * H * 2, 3 * N * H * 2
    res["gather_bytes"], res["tail_bytes"] = gather_bytes, tail_bytes
    res["gather_frac_of_8TBs"] = round(gather_bytes / (kern["spmm_max_bf16"]["median"] * 1e-6) / 8e12, 3)
    res["tail_frac_of_8TBs"] = round(tail_bytes / (kern["sage_tail_bf16"]["median"] * 1e-6) / 8e12, 3)

    print(f"[cfg2] N={N} E={E}")
    for k in ("forward_us_off", "forward_us_all"):
        print(f"  {k:16s} median {res[k]['median']:9.1f} us  repeats {res[k]['repeats']}  spread {res[k]['spread']}")
    print(f"  prediction rel-L2 \"all\" vs off: {res['pred_rel_l2']:.3e}")
    for k, v in kern.items():
        print(f"  {k:18s} median {v['median']:8.1f} us  repeats {v['repeats']}  spread {v['spread']}")
    print(f"  gather moves {gather_bytes / 1e6:.0f} MB at {res['gather_frac_of_8TBs']:.2f} of 8 TB/s, the tail "
          f"{tail_bytes / 1e6:.0f} MB at {res['tail_frac_of_8TBs']:.2f}; gathers equal: {res['gathers_equal']}")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
