#!/usr/bin/env python
"""Training-throughput benchmark of buck-gnn's GraphSAGE hot path on MI355X.

Metric (BASELINE.json): graphs/sec of a full train step (fwd + bwd + Adam) of the
6-layer, hidden-512 GraphSage_addAggr BuckGNN on batches of 16 synthetic FE meshes
per GPU (configs[1] = cfg2: 16 non-stiffened 71x71 quad+diagonal meshes with 13.33 %
random virtual edges; N = 80,656 nodes, E = 715,872 directed edges per GPU).

One step = the reference's inner-loop body (TRAIN_FINAL.py:253-298): the next shuffled
16-graph mini-batch gathered on the GPU from a device-resident GraphStore of 256 meshes per
rank (features, edge_index, per-graph CSR; the reference collates it on the host with the
PyG DataLoader, TRAIN_FINAL.py:1298), forward, RelativeErrorLoss on denormalised
eigenvalues, backward, gradient all-reduce (N > 1), Adam. The dataset is resident in HBM
before timing. --data static rebuilds the CSR of one fixed batch from edge_index every step
instead; --data host collates on the host (PCIe-inclusive).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config cfg2|cfg3] [--full] [--dump-outputs DIR]
    torchrun --nproc-per-node N bench.py --gpus N ...      (driver, N > 1)

A plain run sets up, warms up, times the K steps and prints the line. --full adds the measurements
that take runs of their own: `cpu_baseline` (the oracle's train step on the host cores) and the
nested `cfg3` block (the super-node configuration measured after the headline). --dump-outputs DIR
writes what the last timed step left with its caller (the loss, the updated parameters and buffers,
the gradients; the prediction for --mode infer) as DIR/<name>.npy after the timed steps; the inputs
are seeded, so two builds run with the same arguments can be compared output for output.

Rank 0 prints ONE JSON line. `roofline` is the dominant kernel: the SAGE-layer GEMM family
(forward z = x [W_l;W_r]^T, dgrad or wgrad; 18 GEMMs of 84.6 GFLOP each per step) with the
largest time per step, MFMA-bound. Each family is timed under its own key (bgnn/fused.py) so
every averaged launch has the same flops; the folded first layer's K = 128 launches are timed
separately. `roofline_gemm` lists all six shapes and the step total. The GEMM peak is the
ceiling of the algorithm that runs (default f16x3: f16 dense MFMA 2.5 PF / 3 piece products =
833.3 TF f32-equivalent; bf16x6: 2.5 PF / 6 = 416.7 TF; the f32 MFMA peak 157.3 TF is reported
beside it); tools/gemm_launches.py recomputes the same figures from a rocprofv3 kernel trace.
`roofline_hbm` is the fused aggregation kernel (bgnn_sage_fwd: neighbour sum + lin_r term +
bias + L2 normalize + BN statistics), 499.1 MB per launch against 8 TB/s; `roofline_agg_bwd`
the transpose aggregation (333.6 MB). All use HIP events recorded on the launching
stream around each launch inside the timed region; `traffic` is the per-launch fabric traffic
from rocprofv3 PMC passes (profiles/TRAFFIC_FILE, tools/traffic.py).
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "buck-gnn_amd"))

HBM_PEAK_GBS = 8000.0        # MI355X HBM3E spec (MI355X_MICROARCH.md)
FP32_MFMA_PEAK_TFS = 157.3   # MI355X dense fp32 matrix peak (MI355X_MICROARCH.md)
BF16_MFMA_PEAK_TFS = 2500.0  # MI355X dense bf16 matrix peak (MI355X_MICROARCH.md)
X6_PEAK_TFS = BF16_MFMA_PEAK_TFS / 6   # f32-equivalent ceiling of the 6-product bf16 split GEMM
H3_PEAK_TFS = BF16_MFMA_PEAK_TFS / 3   # f32-equivalent ceiling of the 3-product f16 split GEMM (f16 = bf16 rate)
TRAFFIC_FILE = "traffic_r06af.json"   # rocprofv3 PMC passes of this bench (tools/gpu_check.sh TAG pmc)
METRIC = "graphs/sec (fwd+bwd) 6-layer SAGE h=512, ~5k-node meshes, batch 16, 1/2/4/8 GPU"   # BASELINE.json


class HipTimingEvent:
    """A HIP event for the per-launch timers (bgnn.fused.TIMER_EVENT), created with
    hipEventDisableSystemFence: torch.cuda.Event's record ends in a system-scope release (cache
    writeback + invalidate) that idles the GPU ~5 us per event between the timed kernels (rocprofv3
    trace: 5.7 us before and 10.4 us between timed launches, ~0.3 ms per cfg2 step). Same
    record / elapsed_time interface; recorded on torch's current stream (the launching stream).
    The library is the HIP runtime torch already loaded (same soname)."""
    _hip = None

    def __init__(self):
        import ctypes
        import torch
        if HipTimingEvent._hip is None:
            torch.cuda.current_stream()
            hip = ctypes.CDLL("libamdhip64.so.7")
            hip.hipEventCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
            hip.hipEventRecord.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
            hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
            hip.hipEventDestroy.argtypes = [ctypes.c_void_p]
            HipTimingEvent._hip = hip
        self._torch = torch
        self.h = ctypes.c_void_p()
        rc = HipTimingEvent._hip.hipEventCreateWithFlags(ctypes.byref(self.h), 0x20000000)  # DisableSystemFence
        if rc != 0:
            raise RuntimeError(f"hipEventCreateWithFlags failed ({rc})")

    def record(self):
        rc = HipTimingEvent._hip.hipEventRecord(self.h, self._torch.cuda.current_stream().cuda_stream)
        if rc != 0:
            raise RuntimeError(f"hipEventRecord failed ({rc})")

    def elapsed_time(self, end) -> float:
        import ctypes
        ms = ctypes.c_float(0.0)
        rc = HipTimingEvent._hip.hipEventElapsedTime(ctypes.byref(ms), self.h, end.h)
        if rc != 0:
            raise RuntimeError(f"hipEventElapsedTime failed ({rc})")
        return float(ms.value)

    def __del__(self):
        if HipTimingEvent._hip is not None and self.h:
            HipTimingEvent._hip.hipEventDestroy(self.h)


def metric_name(model: str, bsz: int) -> str:
    """BASELINE.json's metric for the SAGE models at batch 16; EA_GNN (configs[4]) is named for
    what it measures."""
    if model.startswith("EA_GNN"):
        return f"graphs/sec (fwd+bwd) 6-block {model} (GraphNetBlock) h=512, ~5k-node meshes, batch {bsz}"
    if bsz == 16:
        return METRIC
    return f"graphs/sec (fwd+bwd) 6-layer SAGE h=512, ~5k-node meshes, batch {bsz}"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cfg2", choices=["cfg2", "cfg3", "cfg5"])
    ap.add_argument("--model", default="GraphSage_addAggr")
    ap.add_argument("--gemm", default="hip", choices=["hip", "torch"])
    ap.add_argument("--path", default="fused", choices=["fused", "per_op"],
                    help="fused (default): bgnn.BuckGNN's fused SAGE layer loop; per_op: the same model with "
                         "use_fused=False, i.e. the module graph the PyG shim gives the reference's unchanged "
                         "Models/BuckGNN.py (bgnn.nn.SAGEConv modules on the hand-written GEMM + fused "
                         "aggregation/normalize, torch BatchNorm/ReLU/Dropout and encoder)")
    ap.add_argument("--bn", default="torch", choices=["torch", "bgnn"],
                    help="per_op path: the BatchNorm1d modules as torch's (default, the reference's modules "
                         "unchanged) or bgnn.nn.BatchNorm1d (install_pyg_shim(batchnorm=True), csrc/bn.hip)")
    ap.add_argument("--mode", default="train", choices=["train", "infer"],
                    help="infer: INFERENCE_TIMER.py:151-270's GNN timing -- one mesh replicated --infer-batch "
                         "times in one batch, eval mode, no_grad forward passes (a separate line, not the "
                         "BASELINE metric)")
    ap.add_argument("--infer-batch", type=int, default=128)
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements that take runs of their own: the CPU baseline (oracle train "
                         "step on the host cores) and the nested cfg3 (super-node) block of the cfg2 line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps write what the last timed step computed (train: loss, updated "
                         "parameters and buffers, gradients; infer: the prediction) as DIR/<name>.npy, float32, "
                         "at most 64 MB in all (a fixed seeded sample of the elements beyond that)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-cfg3", action="store_true",
                    help="with --full: skip the cfg3 (super-node) block the cfg2 line nests after its own "
                         "measurement")
    ap.add_argument("--cpu-steps", type=int, default=2)
    ap.add_argument("--cache-graph", action="store_true", help="reuse the CSR across steps (not the default)")
    ap.add_argument("--data", default="store", choices=["static", "store", "host"],
                    help="store (default): a new shuffled 16-graph batch every step, gathered on the GPU from a "
                         "resident GraphStore of --store-graphs meshes (the training loop's data path); "
                         "static: one resident 16-graph batch, graph structure rebuilt from edge_index every "
                         "step; host: the same batches as store collated on the host (PyG DataLoader path of "
                         "the reference) and copied to the GPU inside the step")
    ap.add_argument("--store-graphs", type=int, default=256)
    ap.add_argument("--epochs", type=int, default=0,
                    help="> 0: the training loop's epoch shape (TRAIN_FINAL.py:246-298 over the DataLoader of "
                         ":1298; BASELINE configs[3]): a dataset of --dataset-graphs meshes sharded by rank "
                         "(each rank builds and keeps only its shard resident in a GraphStore), every epoch a "
                         "shuffled pass over the shard in batches of 16 (drop_last); --steps is then the whole "
                         "timed run (epochs x shard/16)")
    ap.add_argument("--dataset-graphs", type=int, default=0,
                    help="global dataset size for --epochs (default: --store-graphs per rank)")
    ap.add_argument("--timer-every", type=int, default=4,
                    help="record the per-launch roofline events on every N-th timed step (1 = all)")
    ap.add_argument("--torch-events", action="store_true",
                    help="time the launches with torch.cuda.Event (system-fenced records; A/B of HipTimingEvent)")
    ap.add_argument("--lr", type=float, default=None,
                    help="Adam learning rate (default 1e-2, TRAIN_FINAL.py:37; EA_GNN 1e-3: at 1e-2 the h=512 "
                         "EA_GNN diverges in the reference too, tests/test_gpu_ea_train.py)")
    ap.add_argument("--bf16", action="store_true",
                    help="EA_GNN only: bf16 GEMM operands with f32 accumulation (BASELINE configs[4])")
    ap.add_argument("--tune", action="append", default=[], metavar="KNOB=VALUE",
                    help="bgnn_set_tuning(KNOB, VALUE) before the run (A/B profiling; include/bgnn.h BGNN_TUNE_*)")
    ap.add_argument("--py-set", action="append", default=[], metavar="MODULE.ATTR=EXPR",
                    help="set a bgnn module switch before the run (A/B profiling), e.g. bgnn.fused.WSPLIT=False")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_LIMIT_BYTES = 64 << 20   # --dump-outputs: all files together


def dump_outputs(dirname, tensors):
    """Write name -> tensor as dirname/<name>.npy (float64 stays, everything else as float32). Beyond
    DUMP_LIMIT_BYTES in all, every array of more than 4,096 elements keeps the same fraction of its
    elements (flattened), chosen by a fixed seed: the same indices in every run and build."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    arrs = {}
    for name, t in tensors.items():
        if hasattr(t, "detach"):
            t = t.detach().cpu()
            t = (t if t.dtype.is_floating_point and t.element_size() >= 4 else t.float()).numpy()
        a = np.asarray(t)
        arrs[name] = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
    total = sum(a.nbytes for a in arrs.values())
    frac = min(1.0, 0.9 * DUMP_LIMIT_BYTES / max(1, total))
    for name, a in arrs.items():
        if frac < 1.0 and a.size > 4096:
            keep = np.sort(np.random.default_rng(0).choice(a.size, int(a.size * frac), replace=False))
            a = a.reshape(-1)[keep]
        np.save(os.path.join(dirname, name + ".npy"), a)


def _mesh_arrays(job):
    """(worker of make_pool) one synthetic mesh as numpy arrays."""
    from bgnn import synthetic
    n, seed, super_node = job
    d = synthetic.make_mesh_graph(n, seed, super_node=super_node)
    return d.x.numpy(), d.edge_index.numpy(), d.edge_attr.numpy(), d.y.numpy()


def make_pool(n, seeds, super_node):
    """[synthetic.make_mesh_graph(n, s, super_node) for s in seeds]. The random virtual edges are drawn
    pair by pair (85 ms a mesh), so while this process has not touched the GPU yet the meshes are
    generated by forked workers; every mesh depends on its seed alone, the pool is the same."""
    import multiprocessing as mp
    import torch
    import bgnn
    from bgnn import synthetic
    workers = min(16, os.cpu_count() or 1, len(seeds) // 8)
    if workers < 2 or super_node or torch.cuda.is_initialized():
        return [synthetic.make_mesh_graph(n, s, super_node=super_node) for s in seeds]
    with mp.get_context("fork").Pool(workers) as pool:
        parts = pool.map(_mesh_arrays, [(n, s, super_node) for s in seeds], chunksize=4)
    return [bgnn.Data(x=torch.from_numpy(x), edge_index=torch.from_numpy(ei), edge_attr=torch.from_numpy(ea),
                      y=torch.from_numpy(y)) for x, ei, ea, y in parts]


def cpu_baseline(batch, model_state, model_name, steps):
    """The oracle (plain-PyTorch CPU restatement of the reference path) timed on the host cores."""
    import torch
    from oracle.buckgnn_ref import TrainStep

    threads = min(16, os.cpu_count() or 1)
    torch.set_num_threads(threads)
    st = TrainStep(model_state, model_name, lr=1e-2, weight_decay=1e-8, dropout=0.1)
    x, ei, b, y = batch.x.cpu(), batch.edge_index.cpu(), batch.batch.cpu(), batch.y.cpu()
    st(x, ei, b, y)  # warm-up
    t0 = time.perf_counter()
    for _ in range(steps):
        st(x, ei, b, y)
    dt = time.perf_counter() - t0
    g = batch.num_graphs * steps
    return {"value": round(g / dt, 4), "unit": "graphs/s", "cores": threads, "host_cpus": os.cpu_count(),
            "kind": "port",
            "sample": f"{steps} timed train steps (fwd+bwd+Adam, dropout 0.1) of the oracle on the same "
                      f"{batch.num_graphs}-graph batch ({batch.num_nodes} nodes) after 1 warm-up, "
                      f"torch CPU with {threads} threads; {dt:.1f} s"}


def run_infer(args, model, dev, world, rank):
    """INFERENCE_TIMER.py:151-270 (run_time_analysis, GNN part): one graph deep-copied batch_size
    times (:207), one DataLoader batch moved to the device once (:221-225), an untimed forward,
    then total_loop timed forwards under no_grad in eval mode; throughput = batch_size / average
    forward time (:237). The reference times with time.time() around an asynchronous forward; here
    every timed region ends in torch.cuda.synchronize()."""
    import torch
    import bgnn
    from bgnn import fused, synthetic
    c = synthetic.CONFIGS[args.config]
    one = synthetic.make_mesh_graph(c["n"], 1000 * rank, super_node=c["super_node"])
    batch = bgnn.Batch.from_data_list([one] * args.infer_batch).to(dev)
    model.eval()

    def fwd():
        with torch.no_grad():
            return model(batch.x, batch.edge_index, batch.edge_attr, batch.batch)

    for _ in range(max(1, args.warmup)):
        fwd()
    torch.cuda.synchronize()
    fused.TIMER_EVENT = None if args.torch_events else HipTimingEvent
    fused.TIMERS = {}
    if world > 1:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        pred, _ = fwd()
    torch.cuda.synchronize()
    if world > 1:
        torch.distributed.barrier()
    elapsed = time.perf_counter() - t0
    timers, fused.TIMERS = fused.TIMERS, None
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())
    N, E, H = batch.num_nodes, batch.num_edges, 512
    gemm_ev = timers.get("gemm_fwd", [])
    g_ms = sum(a.elapsed_time(b) for a, b in gemm_ev) / len(gemm_ev) if gemm_ev else float("nan")
    g_tfs = 2.0 * N * (2 * H) * H / (g_ms * 1e-3) / 1e12
    agg_ev = timers.get("sage_fwd", [])
    a_ms = sum(a.elapsed_time(b) for a, b in agg_ev) / len(agg_ev) if agg_ev else float("nan")
    a_bytes = 3 * N * H * 4 + 4 * E + 4 * (N + 1) + 4 * N
    out = {
        "metric": "GNN inference throughput (INFERENCE_TIMER.py run_time_analysis)",
        "value": round(args.infer_batch * world * args.steps / elapsed, 3),
        "unit": "graphs/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": f"{args.config} mesh ({c['n']}x{c['n']}"
                               + (" + super node" if c["super_node"] else " + virtual edges")
                               + f") replicated x{args.infer_batch} in one batch, {args.model} h=512 L=6, eval, "
                                 f"no_grad forward per step",
                   "batch": args.infer_batch, "nodes_per_gpu": N, "edges_per_gpu": E, "path": args.path,
                   "parallelism": f"dp{world}"},
        "roofline": {"kernel": "bgnn_gemm_f32 fwd z = x [W_l;W_r]^T (f16x3)", "bound": "mfma",
                     "achieved": round(g_tfs, 2), "peak": H3_PEAK_TFS, "unit": "TFLOP/s",
                     "frac": round(g_tfs / H3_PEAK_TFS, 4), "traffic": None, "avg_launch_ms": round(g_ms, 5),
                     "launches": len(gemm_ev)},
        "roofline_hbm": {"kernel": "bgnn_sage_fwd", "bound": "hbm",
                         "achieved": round(a_bytes / (a_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(a_bytes / (a_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                         "algorithmic_bytes": a_bytes, "avg_launch_ms": round(a_ms, 5), "launches": len(agg_ev)},
        "latency_ms_per_graph": round(elapsed / args.steps / args.infer_batch * 1e3, 5),
        "pred_checksum": float(pred.double().sum()),
    }
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"pred": pred})
    if rank == 0:
        def clean(o):
            if isinstance(o, dict):
                return {k: clean(v) for k, v in o.items()}
            return None if isinstance(o, float) and o != o else o
        print(json.dumps(clean(out)), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def setup_dist(args):
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # BGNN_BENCH_BACKEND=gloo rehearses the N > 1 path on a box with fewer GPUs than ranks
    # (ranks share devices round-robin); the driver's multi-GPU runs use RCCL ("nccl")
    backend = os.environ.get("BGNN_BENCH_BACKEND", "nccl")
    if backend == "gloo":
        local = local % max(1, torch.cuda.device_count())
    if world > 1:
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    return world, rank, torch.device("cuda", local)


def build_model(args, model_name, dev):
    import torch
    import bgnn
    from bgnn import synthetic
    torch.manual_seed(0)
    model = bgnn.BuckGNN(synthetic.NUM_NODE_FEATURES, synthetic.NUM_EDGE_FEATURES, hidden_channels=512,
                         num_layers=6, pooling_layer="mean", prediction_type="buckling", dropout_rate=0.1,
                         model_name=model_name)
    state0 = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.to(dev).train()
    model.use_fused = args.path == "fused"
    if args.path == "per_op" and args.bn == "bgnn":
        bgnn.nn.use_bgnn_batchnorm(model)
    model.ea_bf16 = bool(args.bf16)
    return model, state0


def measure_train(args, config, model_name, dev, world, rank, steps, warmup, heavy_timing=False, dump_dir=None):
    """Build the data (a resident GraphStore of meshes per rank), model and optimizer, run `warmup`
    untimed and `steps` timed train steps (barrier + synchronize on both sides, max over ranks).
    Returns a dict: elapsed (s), timers (bgnn.fused per-launch HIP events), batch (first batch),
    batch_cpu, loss, lr, state0, bsz, steps, heavy (chunk + combine timing of the super rows).
    dump_dir: rank 0 writes the last timed step's loss, parameters, buffers and gradients there."""
    import numpy as np
    import torch
    import torch.distributed as dist

    import bgnn
    from bgnn import _lib, fused, synthetic

    bsz = synthetic.CONFIGS[config]["graphs"]
    batch_cpu = synthetic.make_config_batch(config, rank=rank)
    pool = None
    if args.data != "static":
        # a pool of meshes per rank (made before this process first touches the GPU: make_pool)
        c = synthetic.CONFIGS[config]
        if args.epochs > 0:
            # this rank's shard of a global dataset (graph g seeded by its global id)
            n_global = args.dataset_graphs or args.store_graphs * world
            gids = list(range(rank, n_global, world))
            if len(gids) < bsz:
                raise SystemExit(f"--epochs: the shard of rank {rank} has {len(gids)} graphs, fewer than a batch")
            pool = make_pool(c["n"], gids, c["super_node"])
            per_epoch = len(gids) // bsz
            steps = args.epochs * per_epoch
        else:
            pool = make_pool(c["n"], [1000 * rank + g for g in range(args.store_graphs)], c["super_node"])
    batch = batch_cpu.to(dev)
    model, state0 = build_model(args, model_name, dev)
    is_ea = model_name.startswith("EA_GNN")
    lr = args.lr if args.lr is not None else (1e-3 if is_ea else 1e-2)
    try:
        opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-8, fused=True)
    except (RuntimeError, TypeError):
        opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=1e-8)
    crit = bgnn.RelativeErrorLoss()
    norm = bgnn.EigenvalueScaler(center=1.0, scale=0.5)
    ar = bgnn.GradAllReduce(model) if world > 1 else None

    store = None
    if args.data == "static":
        def step():
            if not args.cache_graph:
                bgnn.clear_caches()
            return bgnn.train_step(model, batch, opt, crit, norm, allreduce=ar)
    else:
        # a different shuffled 16-graph batch of the pool every step
        store = bgnn.GraphStore(pool, dev) if args.data == "store" else None
        rng = np.random.default_rng(rank)
        state = {"order": iter(()), "epoch": -1}

        def next_ids():
            ids = list(itertools.islice(state["order"], bsz))
            if len(ids) < bsz:   # (drop_last: a partial batch starts the next epoch)
                state["epoch"] += 1
                state["order"] = iter(rng.permutation(len(pool)) if args.epochs <= 0
                                      else np.random.default_rng(1234 + state["epoch"]).permutation(len(pool)))
                ids = list(itertools.islice(state["order"], bsz))
            return ids

        def step():
            ids = next_ids()
            if store is not None:
                b = store.batch(ids)
            else:
                b = bgnn.Batch.from_data_list([pool[i] for i in ids]).to(dev, non_blocking=True)
            return bgnn.train_step(model, b, opt, crit, norm, allreduce=ar)

    for _ in range(warmup):
        step()
    if args.epochs > 0 and args.data != "static":   # timed epochs start at an epoch boundary
        state["order"] = iter(())
        state["epoch"] = -1
    torch.cuda.synchronize()
    fused.TIMER_EVENT = None if args.torch_events else HipTimingEvent
    fused.TIMERS = {}
    if heavy_timing:
        _lib.call("bgnn_heavy_timing", 1)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    timers = fused.TIMERS
    every = max(1, args.timer_every)
    t0 = time.perf_counter()
    for i in range(steps):
        # per-launch events on every `every`-th timed step (each event record idles the GPU ~4 us)
        fused.TIMERS = timers if i % every == 0 else None
        loss = step()
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    fused.TIMERS = None
    heavy = None
    if heavy_timing:
        import ctypes
        _lib.call("bgnn_heavy_timing", 0)
        heavy = {}
        for which, name in ((0, "fwd"), (1, "bwd")):
            ms, n = ctypes.c_float(0.0), ctypes.c_int32(0)
            _lib.call("bgnn_heavy_timing_read", which, ctypes.addressof(ms), ctypes.addressof(n))
            heavy[name] = (float(ms.value), int(n.value))
    if args.path == "per_op":   # the per-module SAGEConv launches (bgnn.fused.SageConvFn) under the same keys
        timers = {k[5:]: v for k, v in timers.items() if k.startswith("conv_")}
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    res = {"elapsed": elapsed, "timers": timers, "batch": batch, "batch_cpu": batch_cpu, "loss": float(loss.item()),
           "lr": lr, "state0": state0, "bsz": bsz, "steps": steps, "heavy": heavy,
           "event_steps": len(range(0, steps, every))}
    if dump_dir and rank == 0:
        out = {"loss": loss}
        out.update({"param." + k: v for k, v in model.state_dict().items()})
        out.update({"grad." + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
        dump_outputs(dump_dir, out)
    del model, opt, store
    return res


def roofline_blocks(args, m, model_name):
    """The roofline objects of one measured run (bench line keys roofline, roofline_gemm,
    roofline_hbm, roofline_agg_bwd) from its per-launch HIP events."""
    from bgnn import _lib
    timers, steps = m["timers"], m["event_steps"]   # (the steps whose launches carry events)
    batch = m["batch"]

    def avg_ms(name):
        ev = timers.get(name, [])
        return sum(a.elapsed_time(b) for a, b in ev) / len(ev) if ev else float("nan")

    N, E, H = batch.num_nodes, batch.num_edges, 512
    is_max = "maxAggr" in model_name
    if is_max and "gemm_fwd_max" in timers:   # (the aggregate-first transform: same flops, K = 2H)
        timers.setdefault("gemm_fwd", timers["gemm_fwd_max"])
    # max aggregation (aggregate-first, bgnn/fused.py::_max_transform): bgnn_spmm_fwd(MAX) reads each
    # source row once and writes agg and its argmax; the SAGE row epilogue runs separately
    agg_ms = avg_ms("agg_max" if is_max else "sage_fwd")
    agg_bytes = (3 * N * H * 4 + 4 * E + 4 * (N + 1)) if is_max else 3 * N * H * 4 + 4 * E + 4 * (N + 1) + 4 * N
    agg_gbs = agg_bytes / (agg_ms * 1e-3) / 1e9
    # transpose aggregation (bgnn_spmm_bwd): SURVEY.md §8d's per-layer aggregation bytes
    bwd_ms = avg_ms("spmm_bwd")
    # max: bgnn_spmm_bwd_add(MAXT) reads dagg, its argmax and the addend dh W_r, writes dx
    bwd_bytes = (4 if is_max else 2) * N * H * 4 + 4 * E + 4 * (N + 1)
    bwd_gbs = bwd_bytes / (bwd_ms * 1e-3) / 1e9
    seg_kernel = _lib.query("bgnn_get_tuning", 1)
    from bgnn import graph as _graph
    agg_name = "k_seg_group<2,0,{e},4,8> (row groups of 4, deduplicated source rows)" if (
        seg_kernel == 0 and _graph.GROUP_ROWS == 4) else "k_seg_sweep<2,0,{e},12>"
    traffic = {}
    tpath = os.path.join(ROOT, "profiles", TRAFFIC_FILE)
    is_ea = model_name.startswith("EA_GNN")
    if os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            cfgk = "ea5" if (is_ea and args.bf16 and m["config"] == "cfg5") else m["config"]
            kern = tj.get("configs", {}).get(cfgk, tj["kernels"] if m["config"] == "cfg2" else {})
            traffic = {k: v["bytes_per_launch"] for k, v in kern.items()}
        except (ValueError, OSError, KeyError):
            traffic = {}
    gmode = _lib.query("bgnn_get_tuning", 5) if args.gemm == "hip" else -1
    gemm_peak = {1: X6_PEAK_TFS, 2: H3_PEAK_TFS}.get(gmode, FP32_MFMA_PEAK_TFS)
    gemm_basis = {2: "f16 dense MFMA 2500 TF / 3 f16 products per f32 product",
                  1: "bf16 dense MFMA 2500 TF / 6 bf16 products per f32 product"}.get(gmode, "f32 dense MFMA")
    # The SAGE layer GEMMs, one timer per shape (bgnn/fused.py): every launch averaged under a key
    # has the same flops. K=512 layers: fwd z = x [W_l;W_r]^T, dgrad dx = [dz_l|dh] [W_l;W_r],
    # wgrad d[W_l;W_r] = [dz_l|dh]^T x (each 2*N*2H*H flops); the folded first layer runs the
    # same three products with the encoder width K_in = 128 in place of one H.
    K_in = 128
    fams = {}
    for k, (flop_fn, bytes_fn, kname, tkey, what) in GEMM_FAMILIES.items():
        fams[k] = (flop_fn(N, H, K_in), bytes_fn(N, H, K_in), kname, tkey, what)

    def gemm_block(key):
        """One GEMM family, priced against the bound its arithmetic intensity selects: FLOP per
        algorithmic byte below the ridge (peak FLOP/s / 8 TB/s, 104 FLOP/B for the f16x3 ceiling)
        is HBM-bound (the folded layer's K = 128 products: 57 FLOP/B, What's weak 4 of the round-5
        review), else MFMA-bound; the other figure is given beside it."""
        flop, nbytes, kname, tkey, what = fams[key]
        ms = avg_ms(key)
        n = len(timers.get(key, []))
        tfs = flop / (ms * 1e-3) / 1e12 if n else float("nan")
        gbs = nbytes / (ms * 1e-3) / 1e9 if n else float("nan")
        ridge = gemm_peak * 1e12 / (HBM_PEAK_GBS * 1e9)
        hbm = flop / nbytes < ridge
        blk = {"kernel": f"bgnn_gemm_f32 {what}: {kname}" + (" (f32-accurate f16x3)" if gmode == 2 else ""),
               "bound": "hbm" if hbm else "mfma",
               "achieved": round(gbs, 1) if hbm else round(tfs, 2), "peak": HBM_PEAK_GBS if hbm else gemm_peak,
               "unit": "GB/s" if hbm else "TFLOP/s",
               "frac": round((gbs / HBM_PEAK_GBS) if hbm else (tfs / gemm_peak), 4),
               "traffic": traffic.get(tkey) if tkey else None,
               "peak_basis": "HBM3E 8 TB/s" if hbm else gemm_basis, "algorithmic_flop": flop,
               "algorithmic_bytes": nbytes, "flop_per_byte": round(flop / nbytes, 1), "ridge_flop_per_byte":
               round(ridge, 1), "avg_launch_ms": round(ms, 5), "launches": n,
               "ms_per_step": round(ms * n / steps, 4) if n else float("nan")}
        if hbm:
            blk.update(mfma_achieved=round(tfs, 2), mfma_frac=round(tfs / gemm_peak, 4))
        else:
            blk.update(f32_mfma_peak=FP32_MFMA_PEAK_TFS)
        return blk

    gemm_blocks = {k: gemm_block(k) for k in fams}
    # all SAGE-layer GEMM launches of the step together (K = 512 and folded): summed flops / summed
    # event time against the f16x3 ceiling
    tot_flop = sum(fams[k][0] * gemm_blocks[k]["launches"] for k in fams)
    tot_ms = sum(avg_ms(k) * gemm_blocks[k]["launches"] for k in fams if gemm_blocks[k]["launches"])
    gemm_all_tfs = tot_flop / (tot_ms * 1e-3) / 1e12 if tot_ms else float("nan")
    # `roofline` = the dominant kernel: the GEMM family with the largest time per step
    main_key = max(("gemm_fwd", "gemm_dgrad", "gemm_wgrad"),
                   key=lambda k: (gemm_blocks[k]["launches"] * avg_ms(k)) if gemm_blocks[k]["launches"] else -1)
    return {
        "roofline": dict(gemm_blocks[main_key], family=main_key),
        "roofline_gemm": {
            **{k: {kk: gemm_blocks[k][kk] for kk in ("bound", "achieved", "unit", "frac", "avg_launch_ms", "launches",
                                                     "ms_per_step", "algorithmic_flop", "algorithmic_bytes",
                                                     "kernel")} for k in fams},
            "all_sage_gemms": {"achieved": round(gemm_all_tfs, 2), "frac": round(gemm_all_tfs / gemm_peak, 4),
                               "ms_per_step": round(tot_ms / steps, 4),
                               "tflop_per_step": round(tot_flop / steps / 1e12, 4)},
        },
        "roofline_hbm": {
            "kernel": ("bgnn_spmm_fwd(MAX) with the per-element argmax (aggregate-first max layer)" if is_max else
                       "bgnn_sage_fwd: " + agg_name.format(e=1)
                       + ", SAGE epilogue (+chunk/combine for super nodes)"),
            "bound": "hbm",
            "achieved": round(agg_gbs, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(agg_gbs / HBM_PEAK_GBS, 4),
            "traffic": traffic.get("agg_max" if is_max else "sage_fwd"),
            "algorithmic_bytes": agg_bytes,
            "avg_launch_ms": round(agg_ms, 5),
            "launches": len(timers.get("agg_max" if is_max else "sage_fwd", [])),
        },
        "roofline_agg_bwd": {
            "kernel": ("bgnn_spmm_bwd_add(MAXT): argmax scatter of dagg + the dh W_r addend" if is_max else
                       "bgnn_spmm_bwd (transpose aggregation): " + agg_name.format(e=0)),
            "bound": "hbm",
            "achieved": round(bwd_gbs, 1),
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": round(bwd_gbs / HBM_PEAK_GBS, 4),
            "traffic": traffic.get("spmm_bwd_max" if is_max else "spmm_bwd"),
            "algorithmic_bytes": bwd_bytes,
            "avg_launch_ms": round(bwd_ms, 5),
            "launches": len(timers.get("spmm_bwd", [])),
        },
    }


# family -> (flops(N, H, K_in), algorithmic bytes(N, H, K_in), kernel, traffic key, description); the
# bytes are every operand read once and C written once (fp32), weights included
GEMM_FAMILIES = {
    "gemm_fwd": (lambda N, H, K: 2.0 * N * (2 * H) * H, lambda N, H, K: 4.0 * (N * H + 2 * H * H + N * 2 * H),
                 "k_gemm_x6<1, 0, 1, 256, 256, 4, 2, 0, 4> (weights pre-split once per step, bgnn_gemm_f32_w)",
                 "gemm_fwd_h3", "fwd z = x [W_l;W_r]^T, K = 512 layers (5 per step)"),
    "gemm_dgrad": (lambda N, H, K: 2.0 * N * H * (2 * H),
                   lambda N, H, K: 4.0 * (N * 2 * H + 2 * H * H + N * H) + 4.0 * N * H * 4 / 5,
                   "k_gemm_h3p<128, 256, 2, 4, 4, 8> (skip layers, drop-add epilogue) + "
                   "k_gemm_h3p<128, 256, 2, 4, 4, 0> (last layer): the pipelined pre-split kernel (gemm_h3p.hip); "
                   "weights pre-split once per step (bgnn_gemm_f32_w)", "gemm_dgrad", "dgrad dx = [dz_l|dh] [W_l;W_r], K = 512 layers (5 per step; "
                   "4 read the drop-add source)"),
    "gemm_wgrad": (lambda N, H, K: 2.0 * (2 * H) * H * N, lambda N, H, K: 4.0 * (N * 2 * H + N * H + 2 * H * H),
                   "k_gemm_x6<1, 1, 0, 256, 256, 4, 2, 0> + split-K slab reduce", "gemm_wgrad",
                   "wgrad [dz_l|dh]^T x, K = 512 layers (5 per step)"),
    "gemm_fwd_fold": (lambda N, H, K: 2.0 * N * (2 * H) * K, lambda N, H, K: 4.0 * (N * K + 2 * H * K + N * 2 * H),
                      "k_gemm_x6<1, 0, 1, 256, 256, 4, 2, 0>", None, "folded layer 0 fwd z = h Wf^T, K = 128"),
    "gemm_dgrad_fold": (lambda N, H, K: 2.0 * N * K * (2 * H), lambda N, H, K: 4.0 * (N * 2 * H + 2 * H * K + N * K),
                        "k_gemm_x6<1, 0, 1, 256, 128, 4, 2, 0>", None, "folded layer 0 dgrad dh = dz Wf"),
    "gemm_wgrad_fold": (lambda N, H, K: 2.0 * (2 * H) * K * N, lambda N, H, K: 4.0 * (N * 2 * H + N * K + 2 * H * K),
                        "k_gemm_x6<1, 1, 0, 256, 128, 4, 2, 0>", None, "folded layer 0 wgrad dWf = dz^T h"),
}


def workload_text(args, config, model_name, bsz):
    return (f"{config}: {bsz} synthetic 71x71 quad+diagonal FE meshes per GPU"
            + (" + super node" if config == "cfg3" else " + 13.33% random virtual edges")
            + f", {model_name} h=512 L=6, mean pool, dropout 0.1, Adam"
            + ("; per-op modules (PyG-surface SAGEConv on the bgnn GEMM + fused aggregation/normalize, "
               + ("bgnn BatchNorm1d, " if args.bn == "bgnn" else "torch BatchNorm, ")
               + "torch ReLU/Dropout/encoder)" if args.path == "per_op" else "")
            + (", bf16 GEMM operands" if args.bf16 and model_name.startswith("EA_GNN") else "") + "; "
            + {"static": "CSR rebuilt every step" if not args.cache_graph else "CSR cached across steps",
               "store": f"new shuffled batch every step gathered on the GPU from a resident "
                        f"GraphStore of {args.store_graphs} meshes",
               "host": f"new shuffled batch every step collated on the host from {args.store_graphs} "
                       f"meshes and copied to the GPU (reference DataLoader path)"}[args.data])


def cfg3_block(args, dev, world, rank):
    """BASELINE configs[2] measured in the same process after the headline line:
    16 stiffened meshes with a super node each (in-degree 5,041: VirtualEdgeCreate.py:81-113) per
    GPU, the same model and step; the super rows' 64-edge chunks + combine timed by HIP events."""
    steps = max(5, args.steps // 2)
    m = measure_train(args, "cfg3", args.model, dev, world, rank, steps, min(args.warmup, 3), heavy_timing=True)
    m["config"] = "cfg3"
    blocks = roofline_blocks(args, m, args.model)
    b = m["batch"]
    from bgnn import graph as _graph
    g = _graph.graph_for(b.edge_index, b.num_nodes)
    heavy = m["heavy"] or {}
    sup = {"heavy_rows_per_batch": int(g.fwd.plan.n_heavy), "chunks_per_batch": int(g.fwd.plan.n_chunks),
           "chunk_edges": _graph.DEFAULT_CHUNK}
    for name, key in (("fwd", "agg_fwd"), ("bwd", "spmm_bwd")):
        ms, n = heavy.get(name, (0.0, 0))
        agg = blocks["roofline_hbm" if name == "fwd" else "roofline_agg_bwd"]
        sup[f"chunk_combine_ms_per_launch_{name}"] = round(ms / n, 5) if n else None
        sup[f"chunk_combine_share_of_{key}"] = round(ms / n / agg["avg_launch_ms"], 4) if n else None
        sup[f"chunk_combine_ms_per_step_{name}"] = round(ms / m["steps"], 4) if n else None
    return {"value": round(m["bsz"] * world * m["steps"] / m["elapsed"], 3), "unit": "graphs/s",
            "ms_per_step": round(m["elapsed"] / m["steps"] * 1e3, 4), "steps": m["steps"],
            "workload": workload_text(args, "cfg3", args.model, m["bsz"]),
            "nodes_per_gpu": b.num_nodes, "edges_per_gpu": b.num_edges, "super_rows": sup,
            **blocks, "final_loss": m["loss"]}


def main():
    args = parse()
    import torch
    import torch.distributed as dist

    from bgnn import _lib, fused

    for kv in args.tune:
        k, v = kv.split("=")
        _lib.call("bgnn_set_tuning", int(k), int(v))
    import importlib
    for kv in args.py_set:
        k, v = kv.split("=", 1)
        mod, attr = k.rsplit(".", 1)
        setattr(importlib.import_module(mod), attr, eval(v, {}, {}))
    world, rank, dev = setup_dist(args)
    fused.GEMM_BACKEND = args.gemm
    if args.mode == "infer":
        model, _ = build_model(args, args.model, dev)
        return run_infer(args, model, dev, world, rank)

    m = measure_train(args, args.config, args.model, dev, world, rank, args.steps, args.warmup,
                      dump_dir=args.dump_outputs)
    m["config"] = args.config
    steps, bsz, elapsed = m["steps"], m["bsz"], m["elapsed"]
    batch = m["batch"]
    is_ea = args.model.startswith("EA_GNN")
    blocks = roofline_blocks(args, m, args.model)
    blocks["launch_timing"] = {
        "events": "torch.cuda.Event" if args.torch_events else "hipEventDisableSystemFence (HipTimingEvent)",
        "event_steps": m["event_steps"], "of_timed_steps": steps,
        "note": "per-launch roofline events recorded on every timed step i with i % timer_every == 0 "
                "(inside the timed region, on the launching stream)"}
    graphs = bsz * world * steps
    out = {
        "metric": metric_name(args.model, bsz),
        "value": round(graphs / elapsed, 3),
        "unit": "graphs/s",
        "n_gpus": world,
        "steps": steps,
        "warmup": args.warmup,
        "ms_per_step": round(elapsed / steps * 1e3, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "bf16" if (args.bf16 and is_ea) else "f32",
        "data": "synthetic",
        "config": {
            "workload": workload_text(args, args.config, args.model, bsz),
            "data_path": args.data,
            **({"epochs": args.epochs, "dataset_graphs": args.dataset_graphs or args.store_graphs * world,
                "steps_per_epoch": steps // args.epochs} if args.epochs > 0 else {}),
            "global_batch": bsz * world,
            "nodes_per_gpu": batch.num_nodes,
            "edges_per_gpu": batch.num_edges,
            "hidden": 512,
            "layers": 6,
            "parallelism": f"dp{world}",
            "gemm": args.gemm,
            "path": args.path,
            **({"batchnorm": args.bn} if args.path == "per_op" else {}),
        },
        **blocks,
        "lr": m["lr"],
        "final_loss": m["loss"],
    }
    if is_ea:
        # the SAGE kernels above never run for EA_GNN. Its dominant kernels are the four per-edge
        # K = H products of every GraphNetBlock (Models/BuckGNN.py:552-566 after the transform-first
        # split, bgnn/ea.py): 2*E*H^2 flops each, reading an [E, H] operand and writing an [E, H]
        # result -- 8*E*H bytes in f32 storage, 4*E*H with the bf16 configuration's bf16 edge
        # storage (ea.BF16_STORAGE) -- so at these sizes they are HBM-bound.
        for k in ("roofline_hbm", "roofline_agg_bwd", "roofline_gemm"):
            out.pop(k)
        timers = m["timers"]
        ev = timers.get("ea_edge_fwd", [])
        n_ea = len(ev)
        ea_ms = sum(a.elapsed_time(b) for a, b in ev) / n_ea if n_ea else float("nan")
        from bgnn import ea as ea_mod
        E, H = batch.num_edges, 512
        ea_bytes = (4.0 if (args.bf16 and ea_mod.BF16_STORAGE) else 8.0) * E * H
        ea_flop = 2.0 * E * H * H
        ea_gbs = ea_bytes / (ea_ms * 1e-3) / 1e9
        ea_tfs = ea_flop / (ea_ms * 1e-3) / 1e12
        gmode = _lib.query("bgnn_get_tuning", 5) if args.gemm == "hip" else -1
        ea_peak = BF16_MFMA_PEAK_TFS if args.bf16 else (H3_PEAK_TFS if gmode == 2 else FP32_MFMA_PEAK_TFS)
        traffic = {}
        tpath = os.path.join(ROOT, "profiles", TRAFFIC_FILE)
        if os.path.exists(tpath):
            try:
                tj = json.load(open(tpath))
                traffic = {k: v["bytes_per_launch"] for k, v in tj.get("configs", {}).get("ea5", {}).items()}
            except (ValueError, OSError, KeyError):
                traffic = {}
        out["roofline"] = {
            "kernel": "per-edge GraphNetBlock GEMMs (edge_mlp / phi, K = H = 512; gather-add + ReLU epilogues): "
                      + ("k_gemm_x6 bf16 operands" if args.bf16 else "k_gemm_x6 f16x3"),
            "bound": "hbm", "achieved": round(ea_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(ea_gbs / HBM_PEAK_GBS, 4),
            "traffic": traffic.get("ea_edge_b16") if (args.bf16 and ea_mod.BF16_STORAGE) else None,
            "algorithmic_bytes": ea_bytes,
            "avg_launch_ms": round(ea_ms, 5), "launches": n_ea,
            "ms_per_step": round(ea_ms * n_ea / m["event_steps"], 4) if n_ea else float("nan"),
            "mfma": {"achieved": round(ea_tfs, 2), "peak": ea_peak, "unit": "TFLOP/s",
                     "frac": round(ea_tfs / ea_peak, 4), "algorithmic_flop": ea_flop},
        }
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(m["batch_cpu"], m["state0"], args.model, args.cpu_steps)
    batch_cpu = m.pop("batch_cpu")
    del m, batch, batch_cpu
    # --full: BASELINE configs[2] (super nodes) nested in the same line; the headline stays cfg2
    if (args.full and args.config == "cfg2" and not args.no_cfg3 and not is_ea and args.path == "fused" and args.epochs <= 0
            and args.data == "store"):
        torch.cuda.empty_cache()
        out["cfg3"] = cfg3_block(args, dev, world, rank)
    if rank == 0:
        def clean(o):   # NaN (a kernel the chosen model never launches) -> null: strict JSON
            if isinstance(o, dict):
                return {k: clean(v) for k, v in o.items()}
            return None if isinstance(o, float) and o != o else o
        print(json.dumps(clean(out)), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
