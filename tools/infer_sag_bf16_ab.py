#!/usr/bin/env python
"""What does GraphSAGE_SAG on bf16 rows (BuckGNN.infer_bf16_sag) buy, and what does it change? A/B in
one process on the eval forward of GraphSAGE_SAG (h = 512, L = 6) on the cfg2 batch:

  forward    the whole eval forward under no_grad (host clock around a forward that ends in a device
             synchronise; both paths carry SAGPooling's host reads and the build of the pooled
             graph), cache flushed before each, the f32 path and the bf16 path alternating: --rounds
             rounds each, a round the median of --iters forwards. A speed-up is claimed only when the
             bf16 path's slowest round beats the f32 path's fastest.
  prediction rel-L2 of the bf16 path against the f32 path run at the bf16 path's node selection
             (topk_select answers with the recorded selection), and against the f32 path as it is
  selection  over --sel-batches cfg2 batches (seeds of their own): the share of graphs whose kept
             node set differs between the two paths, and the share of kept nodes that differ

Usage: python tools/infer_sag_bf16_ab.py [--rounds 7] [--iters 9] [--sel-batches 4]
       python tools/infer_sag_bf16_ab.py --trace bf16|f32 [--iters 11]
(--trace: --iters forwards of one path on the cfg2 batch and nothing else, for a kernel trace:
 rocprofv3 --kernel-trace --stats -d OUT -- python tools/infer_sag_bf16_ab.py --trace bf16)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "buck-gnn_amd"))

import torch  # noqa: E402

import bgnn  # noqa: E402
from bgnn import pool, synthetic  # noqa: E402

H, L = 512, 6


def forward(model, b, sag16):
    model.infer_bf16, model.infer_bf16_sag = (True, True) if sag16 else (False, False)
    with torch.no_grad():
        return model(b.x, b.edge_index, b.edge_attr, b.batch)[0]


def forward_ms(model, b, sag16, junk):
    junk.fill_(1.0)   # flush L2 / Infinity Cache: every forward starts cold
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    forward(model, b, sag16)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


class Selection:
    """Records topk_select's answers, or replays a recorded one."""

    def __init__(self):
        self.real = pool.topk_select
        self.seen, self.replay = [], None

    def __call__(self, *a, **k):
        out = self.real(*a, **k) if self.replay is None else self.replay
        self.seen.append(out)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=9)
    ap.add_argument("--sel-batches", type=int, default=4)
    ap.add_argument("--trace", choices=["bf16", "f32"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = bgnn.BuckGNN(16, 5, hidden_channels=H, num_layers=L, pooling_layer="mean", dropout_rate=0.0,
                         model_name="GraphSAGE_SAG").to(dev).eval()
    if args.trace:
        b = synthetic.make_config_batch("cfg2").to(dev)
        bgnn.prepare(b.edge_index, b.num_nodes, b.batch, getattr(b, "num_graphs", None) or None)
        for _ in range(args.iters):
            forward(model, b, args.trace == "bf16")
        torch.cuda.synchronize()
        return
    sel = Selection()
    pool.topk_select = sel
    res = {"H": H, "L": L}

    # predictions and selections
    diff_graphs = graphs = diff_nodes = kept_nodes = 0
    for rank in range(max(1, args.sel_batches)):
        b = synthetic.make_config_batch("cfg2", rank).to(dev)
        bgnn.prepare(b.edge_index, b.num_nodes, b.batch, getattr(b, "num_graphs", None) or None)
        sel.seen.clear()
        p32 = forward(model, b, False).double()
        p16 = forward(model, b, True).double()
        (perm32, _, bo32), picked = sel.seen[0], sel.seen[1]
        sel.replay = picked
        p32_at16 = forward(model, b, False).double()
        sel.replay = None
        k32 = torch.zeros(b.num_nodes, dtype=torch.bool, device=dev)
        k16 = torch.zeros_like(k32)
        k32[perm32], k16[picked[0]] = True, True
        per_graph = torch.zeros(int(b.batch.max()) + 1, device=dev).index_add_(0, b.batch, (k32 != k16).float())
        diff_graphs += int((per_graph > 0).sum())
        graphs += per_graph.numel()
        diff_nodes += int((k16 & ~k32).sum())
        kept_nodes += int(k16.sum())
        if rank == 0:
            res.update(N=b.num_nodes, E=b.num_edges, graphs_per_batch=per_graph.numel(),
                       pred_rel_l2_same_selection=float((p16 - p32_at16).norm() / p32_at16.norm()),
                       pred_rel_l2_own_selections=float((p16 - p32).norm() / p32.norm()))
            b0 = b
    res.update(selection_graphs=graphs, selection_graphs_differ=diff_graphs,
               selection_graphs_differ_share=round(diff_graphs / graphs, 4),
               kept_nodes=kept_nodes, kept_nodes_differ=diff_nodes,
               kept_nodes_differ_share=round(diff_nodes / max(kept_nodes, 1), 6))
    print(f"N={res['N']} E={res['E']} graphs/batch={res['graphs_per_batch']}")
    print(f"  prediction rel-L2, bf16 path vs f32 path at the bf16 path's selection: {res['pred_rel_l2_same_selection']:.3e}")
    print(f"  prediction rel-L2, bf16 path vs f32 path, each at its own selection:   {res['pred_rel_l2_own_selections']:.3e}")
    print(f"  selection: {diff_graphs} of {graphs} graphs differ ({100.0 * diff_graphs / graphs:.1f} %), "
          f"{diff_nodes} of {kept_nodes} kept nodes ({100.0 * diff_nodes / max(kept_nodes, 1):.3f} %)")

    junk = torch.empty(1 << 28, device=dev)
    for sag16 in (False, True, False, True):   # warm-up: code objects, GEMM choices, caches of both paths
        forward_ms(model, b0, sag16, junk)
    rounds = {False: [], True: []}
    for _ in range(args.rounds):
        for sag16 in (False, True):   # alternating
            rounds[sag16].append(statistics.median(forward_ms(model, b0, sag16, junk) for _ in range(args.iters)))
    for sag16, key in ((False, "forward_ms_f32"), (True, "forward_ms_bf16_sag")):
        r = rounds[sag16]
        res[key] = {"median": round(statistics.median(r), 3), "min": round(min(r), 3), "max": round(max(r), 3),
                    "rounds": [round(v, 3) for v in r]}
        print(f"  {key:20s} median {res[key]['median']:7.3f} ms  min {res[key]['min']:7.3f}  max {res[key]['max']:7.3f}"
              f"  rounds {res[key]['rounds']}")
    res["bf16_slowest_beats_f32_fastest"] = res["forward_ms_bf16_sag"]["max"] < res["forward_ms_f32"]["min"]
    print(f"  bf16 path's slowest round < f32 path's fastest round: {res['bf16_slowest_beats_f32_fastest']}")
    model.infer_bf16, model.infer_bf16_sag = False, False
    pool.topk_select = sel.real
    print(json.dumps(res))


if __name__ == "__main__":
    main()
