#!/usr/bin/env python
"""What does the bf16 inference path (BuckGNN.infer_bf16) buy? A/B in one process on the eval
forward of GraphSage_addAggr (h = 512, L = 6), cache flushed between launches, HIP-event times:

  forward    the whole eval forward under no_grad, flag off / on: the median of --rounds forwards,
             repeated --repeats times (the spread is that of the repeat medians), and the
             prediction's rel-L2 between the two paths
  one layer  gemm_f16x3 + sage_fwd + sage_apply (the f32-accurate layer's three launches) against
             gemm_bf16 + sage_infer (bgnn_sage_infer_bf16), each launch timed alone; the new
             kernel's algorithmic bytes (z N*2H*2, x_prev N*H*2, out N*H*2) as a fraction of 8 TB/s.
             (gemm_f16x3 goes through fused.gemm, which finds the operand maxima itself: the model's
             loop carries them and pre-split weights, so the forward times are the comparison of
             the two paths and this line only sizes the f32 GEMM.)

at two shapes: the cfg2 batch, and one cfg2 mesh x 128 (the shape of `bench.py --mode infer`).

Usage: python tools/infer_bf16_ab.py [--rounds 7] [--repeats 3] [--shapes cfg2,infer]"""
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


def make_shape(name):
    if name == "cfg2":
        return synthetic.make_config_batch("cfg2")
    c = synthetic.CONFIGS["cfg2"]
    one = synthetic.make_mesh_graph(c["n"], 0, super_node=c["super_node"])
    return bgnn.Batch.from_data_list([one] * 128)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--shapes", default="cfg2,infer")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    junk = torch.empty(1 << 28, device=dev)
    torch.manual_seed(0)
    model = bgnn.BuckGNN(16, 5, hidden_channels=H, num_layers=L, pooling_layer="mean", dropout_rate=0.0,
                         model_name="GraphSage_addAggr").to(dev).eval()
    result = {}
    for shape in args.shapes.split(","):
        b = make_shape(shape).to(dev)
        N, E = b.num_nodes, b.num_edges
        bgnn.prepare(b.edge_index, N, b.batch, getattr(b, "num_graphs", None) or None)

        def fwd():
            with torch.no_grad():
                return model(b.x, b.edge_index, b.edge_attr, b.batch)[0]

        res = {"N": N, "E": E}
        preds = {}
        for flag in (False, True):
            model.infer_bf16 = flag
            preds[flag] = fwd().double()
            meds = [statistics.median(time_us(fwd, junk, args.rounds)) for _ in range(max(3, args.repeats))]
            res["forward_us_bf16" if flag else "forward_us_f32"] = {
                "median": round(statistics.median(meds), 1), "repeats": [round(m, 1) for m in meds],
                "spread": round(max(meds) - min(meds), 1)}
        model.infer_bf16 = False
        res["pred_rel_l2"] = float((preds[True] - preds[False]).norm() / preds[False].norm())

        # one layer, launch by launch (layer 1: skip connection, BatchNorm)
        g = graph_for(b.edge_index, N)
        conv, bn = model.sage_blocks_add[1], model.batch_norms[1]
        s = torch.cuda.current_stream().cuda_stream
        x = torch.randn(N, H, device=dev)
        xb = x.bfloat16()
        wcat = torch.cat([conv.lin_l.weight, conv.lin_r.weight]).detach()
        wcat_b = fused.infer_weights(conv)
        scale, shift = fused.bn_eval_coeffs(bn)
        z = torch.empty(N, 2 * H, device=dev)
        zb = torch.empty(N, 2 * H, device=dev, dtype=torch.bfloat16)
        o, nrm, x_next = torch.empty(N, H, device=dev), torch.empty(N, device=dev), torch.empty(N, H, device=dev)
        amax = torch.zeros(1, device=dev)
        slots = _lib.query("bgnn_sage_fwd_slots", g.fwd.ref())
        bnp = torch.empty(slots, 2, H, device=dev)
        part = torch.empty(max(g.fwd.plan.n_chunks, 1) * H, device=dev)
        outb = torch.empty(N, H, device=dev, dtype=torch.bfloat16)
        bias = conv.lin_l.bias.detach()
        launches = {
            "gemm_f16x3": lambda: fused.gemm(x, wcat, False, True, out=z),
            "sage_fwd": lambda: _lib.call("bgnn_sage_fwd", g.fwd.ref(), z.data_ptr(), 2 * H, z[:, H:].data_ptr(),
                                          2 * H, bias.data_ptr(), H, 0, o.data_ptr(), nrm.data_ptr(),
                                          bnp.data_ptr(), part.data_ptr(), None, 0, s),
            "sage_apply": lambda: _lib.call("bgnn_sage_apply", o.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                            x.data_ptr(), 1, 0.0, 0, N, H, x_next.data_ptr(), amax.data_ptr(),
                                            None, None, s),
            "gemm_bf16": lambda: fused.gemm_bf16(xb, wcat_b, False, True, out=zb),
            "sage_infer": lambda: _lib.call("bgnn_sage_infer_bf16", g.fwd.ref(), zb.data_ptr(), 2 * H,
                                            bias.data_ptr(), scale.data_ptr(), shift.data_ptr(), xb.data_ptr(), H,
                                            H, 0, outb.data_ptr(), H, 0, part.data_ptr(), s),
        }
        layer = {}
        for k, f in launches.items():
            t = time_us(f, junk, args.rounds)
            layer[k] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
        res["layer_us"] = layer
        nbytes = N * 2 * H * 2 + 2 * N * H * 2
        res["sage_infer_bytes"] = nbytes
        res["sage_infer_frac_of_8TBs"] = round(nbytes / (layer["sage_infer"]["median"] * 1e-6) / 8e12, 3)
        result[shape] = res
        print(f"[{shape}] N={N} E={E}")
        for k in ("forward_us_f32", "forward_us_bf16"):
            print(f"  {k:16s} median {res[k]['median']:9.1f} us  repeats {res[k]['repeats']}  spread {res[k]['spread']}")
        print(f"  prediction rel-L2 bf16 vs f32 path: {res['pred_rel_l2']:.3e}")
        for k, v in layer.items():
            print(f"  {k:12s} {v['median']:9.1f} us  (min {v['min']}, max {v['max']})")
        print(f"  f32 layer {layer['gemm_f16x3']['median'] + layer['sage_fwd']['median'] + layer['sage_apply']['median']:.1f}"
              f" us = gemm + sage_fwd + sage_apply; bf16 layer "
              f"{layer['gemm_bf16']['median'] + layer['sage_infer']['median']:.1f} us; sage_infer moves "
              f"{nbytes / 1e6:.0f} MB at {res['sage_infer_frac_of_8TBs']:.2f} of 8 TB/s")
        del b, x, xb, z, zb, o, x_next, outb
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
