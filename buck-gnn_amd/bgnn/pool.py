"""SAGPooling's node selection and graph coarsening on libbgnn (no CPU fallback).

torch_geometric.nn.SAGPooling, as the reference builds it for GraphSAGE_SAG / EAGNN_SAG
(Models/BuckGNN.py:203-208,231-236; called at :364,502), does [PyG-doc]

    perm   = topk(score, ratio, batch)          # per graph ceil(ratio * n_g) best, descending
    x'     = x[perm] * score[perm]
    edges' = filter_adj(edge_index, perm)        # both ends kept, edge_index order, relabelled
    batch' = batch[perm]

* `topk_select` — bgnn_topk_rank (each node's position in its graph's stable descending
  order) + bgnn_topk_select (scatter of the kept nodes to their output positions, new node
  ids, pooled batch vector). One host sync for the kept-node count (PyG's boolean-mask
  indexing syncs there too).
* `gather_scale` — bgnn_gather_scale / _bwd as an autograd Function (gradients to x and
  to the score, which is how the scoring GNN trains).
* `filter_edges` — bgnn_filter_edges (deterministic stream compaction); one host sync for
  the kept-edge count.
* `sag_score_bf16`, `gather_scale_bf16`, `sag_pool_bf16` — the same step on bfloat16 rows for
  eval-mode inference (BuckGNN.infer_bf16_sag): bgnn_sag_score_bf16 gives the float32 score,
  topk_select and filter_edges run unchanged, bgnn_gather_scale_bf16 writes the kept rows. No
  autograd.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .graph import _stream, require_cuda


def _graph_offsets(batch: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """ptr [B+1] of a non-decreasing `batch` vector and B (one host sync, which also checks
    the order: every PyG Batch has its graphs' nodes contiguous and in graph order)."""
    last, unsorted, first = torch.stack([batch[-1], (batch[1:] < batch[:-1]).any().to(batch.dtype),
                                         batch[0]]).tolist()
    if unsorted:
        raise ValueError("SAGPooling: `batch` must be non-decreasing (graphs contiguous, in order)")
    if first < 0:
        raise ValueError("SAGPooling: negative graph id in `batch`")
    B = int(last) + 1
    ptr = torch.searchsorted(batch, torch.arange(B + 1, dtype=batch.dtype, device=batch.device))
    return ptr, B


def topk_select(score: torch.Tensor, ratio: float, batch: torch.Tensor):
    """(perm [K] int64, new_id [N] int32 (-1 = dropped), batch' [K] int64): PyG's topk with
    ties broken towards the lower node index (a stable descending sort). The order is
    torch.sort(descending=True, stable=True)'s: -0 == +0, and a NaN score (any sign, any payload)
    ranks above +inf, NaNs being equal among themselves (lower node index first). So every slot
    of `perm` is written and names a node of its graph, whatever the scores hold; a NaN score
    is kept first and shows as NaN rows downstream."""
    require_cuda(score, batch, what="topk_select")
    score = score.detach().reshape(-1).contiguous()
    if score.dtype != torch.float32:
        raise TypeError("topk_select: score must be float32")
    # the kernels read `batch` as int64 (an int32 edge_index gives an int32 batch upstream)
    batch = batch.to(torch.long).contiguous()
    N = score.numel()
    dev = score.device
    if batch.numel() != N:
        raise ValueError(f"topk_select: batch has {batch.numel()} entries, score {N}")
    if N == 0:
        e = torch.empty(0, dtype=torch.long, device=dev)
        return e, torch.empty(0, dtype=torch.int32, device=dev), e
    ptr, B = _graph_offsets(batch)
    counts = ptr[1:] - ptr[:-1]
    if ratio >= 1:
        k = counts.new_full((B,), int(ratio)).minimum(counts)
    else:   # PyG: (float(ratio) * num_nodes.to(score.dtype)).ceil()
        k = (float(ratio) * counts.to(score.dtype)).ceil().to(torch.long)
    new_ptr = torch.zeros(B + 1, dtype=torch.long, device=dev)
    torch.cumsum(k, 0, out=new_ptr[1:])
    K = int(new_ptr[-1].item())
    rank = torch.empty(N, dtype=torch.int32, device=dev)
    perm = torch.empty(K, dtype=torch.long, device=dev)
    new_id = torch.empty(N, dtype=torch.int32, device=dev)
    batch_out = torch.empty(K, dtype=torch.long, device=dev)
    s = _stream()
    _lib.call("bgnn_topk_rank", score.data_ptr(), batch.data_ptr(), ptr.data_ptr(), N, rank.data_ptr(), s)
    _lib.call("bgnn_topk_select", rank.data_ptr(), batch.data_ptr(), k.data_ptr(), new_ptr.data_ptr(), N,
              perm.data_ptr(), new_id.data_ptr(), batch_out.data_ptr(), s)
    return perm, new_id, batch_out


class _GatherScale(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, score, perm, new_id):
        N, H = x.shape
        K = perm.numel()
        out = torch.empty(K, H, dtype=x.dtype, device=x.device)
        _lib.call("bgnn_gather_scale", x.data_ptr(), x.stride(0), H, perm.data_ptr(), score.data_ptr(), K,
                  out.data_ptr(), out.stride(0), _stream())
        ctx.save_for_backward(x, score, new_id)
        return out

    @staticmethod
    def backward(ctx, g):
        x, score, new_id = ctx.saved_tensors
        g = g.contiguous()
        N, H = x.shape
        dx = torch.empty_like(x)
        ds = torch.empty_like(score) if ctx.needs_input_grad[1] else None
        _lib.call("bgnn_gather_scale_bwd", g.data_ptr(), g.stride(0), x.data_ptr(), x.stride(0), H,
                  new_id.data_ptr(), score.data_ptr(), N, dx.data_ptr(), dx.stride(0),
                  None if ds is None else ds.data_ptr(), _stream())
        return dx, ds, None, None


def gather_scale(x: torch.Tensor, score: torch.Tensor, perm: torch.Tensor, new_id: torch.Tensor) -> torch.Tensor:
    """x[perm] * score[perm].view(-1, 1) (Models/BuckGNN.py:364,502 via SAGPooling), differentiable
    in x and score."""
    require_cuda(x, score, perm, new_id, what="gather_scale")
    if x.dtype != torch.float32 or x.dim() != 2:
        raise TypeError("gather_scale: x must be a float32 [N, H] tensor")
    x = x.contiguous()
    score = score.reshape(-1).contiguous()
    if score.numel() != x.size(0) or new_id.numel() != x.size(0):
        raise ValueError("gather_scale: score / new_id must have one entry per row of x")
    if new_id.dtype != torch.int32 or perm.dtype != torch.long:
        raise TypeError("gather_scale: new_id must be int32 and perm int64 (topk_select's outputs)")
    if score.dtype != torch.float32:
        raise TypeError("gather_scale: score must be float32")
    return _GatherScale.apply(x, score, perm.contiguous(), new_id.contiguous())


def filter_edges(edge_index: torch.Tensor, new_id: torch.Tensor, num_nodes: int):
    """(edge_index' [2, E'] int64, kept [E'] int64): PyG's filter_adj on device; `kept` holds
    the original positions of the kept edges (edge_attr' = edge_attr[kept])."""
    require_cuda(edge_index, new_id, what="filter_edges")
    if edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise ValueError(f"filter_edges: edge_index must be [2, E], got {tuple(edge_index.shape)}")
    if new_id.dtype != torch.int32 or new_id.numel() != int(num_nodes):
        raise TypeError("filter_edges: new_id must be an int32 vector with one entry per node")
    new_id = new_id.contiguous()
    ei = edge_index.to(torch.long).contiguous()
    E = ei.size(1)
    dev = ei.device
    out = torch.empty(2 * E, dtype=torch.long, device=dev)
    kept = torch.empty(E, dtype=torch.long, device=dev)
    n = torch.empty(1, dtype=torch.long, device=dev)
    ws_bytes = _lib.query("bgnn_filter_edges_ws_bytes", E)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    _lib.call("bgnn_filter_edges", ei.data_ptr(), E, new_id.data_ptr(), int(num_nodes), out.data_ptr(),
              kept.data_ptr(), n.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
    M = int(n.item())
    return out[:2 * M].view(2, M), kept[:M]


def sag_pool(x: torch.Tensor, score: torch.Tensor, ratio: float, edge_index: torch.Tensor,
             edge_attr: Optional[torch.Tensor], batch: torch.Tensor, multiplier: float = 1.0):
    """The selection + coarsening half of SAGPooling.forward given the node scores:
    returns (x', edge_index', edge_attr', batch', perm, score[perm])."""
    perm, new_id, batch_out = topk_select(score, ratio, batch)
    xo = gather_scale(x, score, perm, new_id)
    if multiplier != 1:
        xo = multiplier * xo
    ei, kept = filter_edges(edge_index, new_id, x.size(0))
    ea = edge_attr.index_select(0, kept) if edge_attr is not None else None
    return xo, ei, ea, batch_out, perm, score.reshape(-1)[perm]


# ---------------------------------------------------------------------------
# SAGPooling on bf16 rows (BuckGNN.infer_bf16_sag): eval mode only, no autograd.

def _bf16_rows_checked(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dtype != torch.bfloat16 or x.dim() != 2:
        raise TypeError(f"{what}: x must be a bfloat16 [N, H] tensor")
    H = x.size(1)
    if H % 8 or not 8 <= H <= 512:
        raise ValueError(f"{what}: needs H % 8 == 0 and 8 <= H <= 512 (got {H})")
    # unit column stride, rows of whole 16-byte vectors (a column view of a wider buffer stays a view)
    return x if (x.stride(1) == 1 and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0) else x.contiguous()


def _select_sign(conv, select_weight: torch.Tensor) -> float:
    """sign(select.weight) as a host float, kept on the scorer module per weight version (as
    fused._cached_weights keeps its matrices): one host read when the weight is first seen, written
    in place or replaced, none per call. A zero weight gives NaN, as w / ||w|| does."""
    key = (select_weight._version, select_weight.data_ptr(), str(select_weight.device))
    hit = getattr(conv, "_bgnn_sag_sign", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    if select_weight.numel() != 1:
        raise ValueError("sag_score_bf16: select.weight must have one element (a one-channel scorer)")
    w = float(select_weight.detach().reshape(-1)[0].item())
    sgn = float("nan") if (w == 0 or w != w) else (1.0 if w > 0 else -1.0)
    conv._bgnn_sag_sign = (key, sgn)
    return sgn


def _f32_vector(t: torch.Tensor, n: int, what: str) -> torch.Tensor:
    t = t.detach().reshape(-1)
    if t.dtype != torch.float32 or t.numel() != n:
        raise TypeError(f"sag_score_bf16: {what} must hold {n} float32 value(s)")
    return t.contiguous()


@torch.no_grad()
def sag_score_bf16(x: torch.Tensor, conv, select_weight: torch.Tensor, graph) -> torch.Tensor:
    """SAGPooling's node score on bf16 rows (bgnn_sag_score_bf16, two launches, no host sync):
    tanh(sign(w) * (sum_{j->i} <x_j, W_l> + b_l + <x_i, W_r>)) as float32 [N], for x bfloat16 [N, H],
    `conv` the pooling's one-channel SAGEConv scorer (sum aggregation, its lin_l.weight, lin_l.bias
    and lin_r.weight read as f32 [H] / scalar), `select_weight` the pooling's select.weight w and
    `graph` the bgnn.graph.Graph of the edges. sign(w) is a host float cached per weight version
    (_select_sign): no per-call host read. No autograd."""
    require_cuda(x, select_weight, what="sag_score_bf16")
    x = _bf16_rows_checked(x, "sag_score_bf16")
    N, H = x.shape
    if graph.fwd.n_rows != N:
        raise ValueError(f"sag_score_bf16: the graph has {graph.fwd.n_rows} nodes, x {N} rows")
    w_l = _f32_vector(conv.lin_l.weight, H, "lin_l.weight")
    w_r = _f32_vector(conv.lin_r.weight, H, "lin_r.weight")
    bias = _f32_vector(conv.lin_l.bias, 1, "lin_l.bias") if conv.lin_l.bias is not None else None
    sgn = _select_sign(conv, select_weight)
    score = torch.empty(N, dtype=torch.float32, device=x.device)
    ws = torch.empty(max(N, 1), 2, dtype=torch.float32, device=x.device)
    _lib.call("bgnn_sag_score_bf16", graph.fwd.ref(), x.data_ptr(), x.stride(0), N, H, w_l.data_ptr(),
              w_r.data_ptr(), None if bias is None else bias.data_ptr(), sgn, score.data_ptr(), ws.data_ptr(),
              _stream())
    return score


@torch.no_grad()
def gather_scale_bf16(x: torch.Tensor, score: torch.Tensor, perm: torch.Tensor, multiplier: float = 1.0) -> torch.Tensor:
    """((x[perm] * score[perm].view(-1, 1)) * multiplier) for bfloat16 rows x [N, H], as bfloat16
    [K, H] (bgnn_gather_scale_bf16): both products in f32, each rounded, one bf16 rounding at the
    store. score: float32 [N]; perm: int64 [K] (topk_select's). No autograd."""
    require_cuda(x, score, perm, what="gather_scale_bf16")
    x = _bf16_rows_checked(x, "gather_scale_bf16")
    score = score.detach().reshape(-1).contiguous()
    if score.dtype != torch.float32 or score.numel() != x.size(0):
        raise TypeError("gather_scale_bf16: score must be float32 with one entry per row of x")
    if perm.dtype != torch.long or perm.dim() != 1:
        raise TypeError("gather_scale_bf16: perm must be an int64 vector (topk_select's output)")
    perm = perm.contiguous()
    K, H = perm.numel(), x.size(1)
    out = torch.empty(K, H, dtype=torch.bfloat16, device=x.device)
    _lib.call("bgnn_gather_scale_bf16", x.data_ptr(), x.stride(0), H, perm.data_ptr(), score.data_ptr(), K,
              float(multiplier), out.data_ptr(), out.stride(0), _stream())
    return out


@torch.no_grad()
def sag_pool_bf16(x: torch.Tensor, score: torch.Tensor, ratio: float, edge_index: torch.Tensor,
                  edge_attr: Optional[torch.Tensor], batch: torch.Tensor, multiplier: float = 1.0):
    """sag_pool on bfloat16 rows: topk_select on the float32 score, gather_scale_bf16, filter_edges
    (the same two host syncs). Returns (x' bfloat16, edge_index', edge_attr', batch', perm,
    score[perm]). No autograd."""
    perm, new_id, batch_out = topk_select(score, ratio, batch)
    xo = gather_scale_bf16(x, score, perm, multiplier)
    ei, kept = filter_edges(edge_index, new_id, x.size(0))
    ea = edge_attr.index_select(0, kept) if edge_attr is not None else None
    return xo, ei, ea, batch_out, perm, score.reshape(-1)[perm]
