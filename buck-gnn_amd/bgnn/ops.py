"""Autograd-wrapped segment reductions on libbgnn (no CPU fallback).

* `aggregate(x, graph, reduce)` — SAGEConv's neighbour aggregation
  (PyG semantics: sum over in-edges of target = edge_index[1]; 'add' == 'sum';
  mean divides by the in-degree; max takes the element-wise maximum; empty
  rows are 0 for all three). Used at Models/BuckGNN.py:342,393,434,449,463.
  float32 or bfloat16 features: bf16 sum / mean rows of whole 16-byte vectors run on the bf16
  kernels (csrc/spmm_b16.hip), forward and backward, and bf16 max rows on the bf16 max kernel
  (csrc/spmm_max_b16.hip; its backward is the float32 argmax kernel); every other bf16 case is
  upcast, run on the float32 kernels and rounded once.
* `segment_reduce(src, segments, reduce)` — global_mean_pool
  (Models/BuckGNN.py:274) and torch_scatter.scatter_add / scatter_mean
  (Models/BuckGNN.py:561,605).
"""
from __future__ import annotations

import contextlib

import torch

from . import _lib
from .graph import Graph, SegmentIndex, _stream, require_cuda

REDUCE = {"sum": 0, "add": 0, "mean": 1, "max": 2}


def _check_x(x: torch.Tensor, what: str, bf16: bool = False) -> torch.Tensor:
    require_cuda(x, what=what)
    if x.dtype == torch.bfloat16 and bf16:
        if x.dim() != 2:
            raise ValueError(f"{what}: expected a 2-D [rows, channels] tensor, got {tuple(x.shape)}")
        return x   # (a strided view may run as it is: _b16_rows)
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: only float32{' / bfloat16' if bf16 else ''} features are supported (got {x.dtype})")
    if x.dim() != 2:
        raise ValueError(f"{what}: expected a 2-D [rows, channels] tensor, got {tuple(x.shape)}")
    return x.contiguous()


def _partial(csr, H: int, reduce: int, dev) -> torch.Tensor:
    n = csr.plan.n_chunks
    if n == 0:
        return None
    # MAX keeps an int32 arg plane after the float plane
    return torch.empty(n * H * (2 if reduce == 2 else 1), dtype=torch.float32, device=dev)


def spmm_fwd(csr, x: torch.Tensor, reduce: int, out_rows: int, want_arg: bool = False):
    """AGG over the CSR rows; for MAX with want_arg also the argmax state (a uint8 buffer of
    bgnn_spmm_max_arg_bytes: per-row edge offsets, int32 for heavy rows; max_arg_positions decodes)."""
    H = x.size(1)
    out = torch.empty(out_rows, H, dtype=torch.float32, device=x.device)
    arg = None
    if reduce == 2 and want_arg:
        arg = torch.empty(_lib.query("bgnn_spmm_max_arg_bytes", out_rows, H, csr.plan.n_heavy), dtype=torch.uint8,
                          device=x.device)
    part = _partial(csr, H, reduce, x.device)
    if out_rows > 0 and H > 0:
        _lib.call("bgnn_spmm_fwd", csr.ref(), x.data_ptr(), x.stride(0), H, reduce, out.data_ptr(), out.stride(0),
                  None if arg is None else arg.data_ptr(), None if part is None else part.data_ptr(), _stream())
    return out, arg


def spmm_bwd(csr_t, perm_t, fwd_rowptr, g: torch.Tensor, reduce: int, arg, out_rows: int, amax=None):
    """Transpose aggregation (rows = sources); MAX routes each (target, column) gradient to the
    argmax edge recorded in `arg` (the forward's state; the forward had g.size(0) rows)."""
    g = g.contiguous()
    H = g.size(1)
    gx = torch.empty(out_rows, H, dtype=torch.float32, device=g.device)
    if out_rows > 0 and H > 0:
        if reduce == 2:
            spmm_bwd_max_into(csr_t, perm_t, fwd_rowptr, g, arg, None, gx, amax)
        else:
            spmm_bwd_into(csr_t, perm_t, fwd_rowptr, g, reduce, gx, amax)
    return gx


def _ptr(t):
    return None if t is None else t.data_ptr()


_NO_TIMER = contextlib.nullcontext()


def spmm_bwd_into(csr_t, perm_t, fwd_rowptr, g: torch.Tensor, reduce: int, out: torch.Tensor, amax=None,
                  heavy_done: bool = False, timer=None) -> None:
    """out = A^T g for sum / mean (bgnn_spmm_bwd; rows = sources, MEAN scales by the target's
    in-degree from fwd_rowptr). g is [*, H] float32 with unit column stride and any row stride
    (a half of an interleaved [dz_l | dh] is), out addresses such rows by its data pointer and row
    stride; amax: device scalar that max|out| is folded into; heavy_done: the heavy rows of out
    are already written (range rows); timer: a context manager entered around the launch alone."""
    H = g.size(1)
    part = _partial(csr_t, H, 0, g.device)
    with timer or _NO_TIMER:
        _lib.call("bgnn_spmm_bwd", csr_t.ref(), _ptr(perm_t), _ptr(fwd_rowptr), g.data_ptr(), g.stride(0), H, reduce,
                  out.data_ptr(), out.stride(0), _ptr(part), _ptr(amax), int(heavy_done), _stream())


def spmm_bwd_max_into(csr_t, perm_t, fwd_rowptr, g: torch.Tensor, arg: torch.Tensor, addend, out: torch.Tensor,
                      amax=None, timer=None) -> None:
    """out = A_max^T g (+ addend) (bgnn_spmm_bwd_max): each (target, column) gradient of g (one
    row per target of the forward) goes to the source of the argmax edge recorded in `arg`;
    addend ([rows of out, H] or None) is added row by row. Row strides and timer as in
    spmm_bwd_into."""
    H = g.size(1)
    part = _partial(csr_t, H, 0, g.device)
    with timer or _NO_TIMER:
        _lib.call("bgnn_spmm_bwd_max", csr_t.ref(), perm_t.data_ptr(), fwd_rowptr.data_ptr(), g.size(0), g.data_ptr(),
                  g.stride(0), H, arg.data_ptr(), _ptr(addend), addend.stride(0) if addend is not None else 0,
                  out.data_ptr(), out.stride(0), _ptr(part), _ptr(amax), _stream())


def max_arg_positions(csr, arg: torch.Tensor, rows: int, H: int) -> torch.Tensor:
    """Decode spmm_fwd's MAX argmax state into int64 CSR positions [rows, H] (-1 for empty rows):
    test / inspection helper (torch ops on the device)."""
    from .graph import Plan  # noqa: F401  (documentation: heavy rows come from csr.plan)
    n = rows * H
    hoff = (n + 255) // 256 * 256
    aoff = hoff + (rows * 4 + 255) // 256 * 256
    a8 = arg[:n].view(rows, H).long()
    rp = csr.rowptr.long()
    deg = rp[1:] - rp[:-1]
    pos = rp[:-1].view(-1, 1) + a8
    nh = csr.plan.n_heavy
    if nh > 0:
        heavy_of = arg[hoff:hoff + rows * 4].view(torch.int32)
        ah = arg[aoff:aoff + nh * H * 4].view(torch.int32).view(nh, H).long()
        hr = csr.plan.heavy_row[:nh].long()
        pos[hr] = rp[hr].view(-1, 1) + ah[heavy_of[hr].long()]
    return torch.where(deg.view(-1, 1) > 0, pos, torch.full_like(pos, -1))


def _b16_width(H: int) -> bool:
    """Row widths of the bf16 aggregation kernels: whole 16-byte vectors, at most one per lane."""
    return H % 8 == 0 and 8 <= H <= 512


def _b16_rows(t: torch.Tensor) -> bool:
    """Whether the bf16 kernels can read t where it lies: unit column stride, rows a multiple of
    8 elements apart and a 16-byte aligned base (a column slice z[:, :H] of a wider tensor is)."""
    return (t.stride(1) == 1 and t.stride(0) % 8 == 0 and t.stride(0) >= t.size(1) and t.data_ptr() % 16 == 0)


def spmm_fwd_bf16(csr, x: torch.Tensor, reduce: int, out_rows: int, out_f32: bool = False) -> torch.Tensor:
    """sum / mean over the CSR rows of bf16 source rows (bgnn_spmm_fwd_bf16): f32 accumulation, the
    result stored once as bf16, or f32 with out_f32. x: bf16 [*, H] that satisfies _b16_rows."""
    H = x.size(1)
    out = torch.empty(out_rows, H, dtype=torch.float32 if out_f32 else torch.bfloat16, device=x.device)
    part = _partial(csr, H, 0, x.device)
    if out_rows > 0:
        _lib.call("bgnn_spmm_fwd_bf16", csr.ref(), x.data_ptr(), x.stride(0), H, reduce, out.data_ptr(),
                  out.stride(0), int(out_f32), None if part is None else part.data_ptr(), _stream())
    return out


def spmm_bwd_bf16(csr_t, fwd_rowptr, g: torch.Tensor, reduce: int, out_rows: int, out_f32: bool = False):
    """The transpose of spmm_fwd_bf16 over bf16 gradient rows (bgnn_spmm_bwd_bf16; rows = sources)."""
    H = g.size(1)
    gx = torch.empty(out_rows, H, dtype=torch.float32 if out_f32 else torch.bfloat16, device=g.device)
    part = _partial(csr_t, H, 0, g.device)
    if out_rows > 0:
        _lib.call("bgnn_spmm_bwd_bf16", csr_t.ref(), None if fwd_rowptr is None else fwd_rowptr.data_ptr(),
                  g.data_ptr(), g.stride(0), H, reduce, gx.data_ptr(), gx.stride(0), int(out_f32),
                  None if part is None else part.data_ptr(), _stream())
    return gx


def spmm_max_bf16(csr, x: torch.Tensor, out_rows: int, want_arg: bool = False, out: torch.Tensor = None):
    """max over the CSR rows of bf16 source rows (bgnn_spmm_max_bf16): exact, the values and ties of
    spmm_fwd(MAX) on the upcast x. x: bf16 [*, H] that satisfies _b16_rows; out: a bf16 [out_rows, H]
    destination that does too (a column plane of a wider buffer), or None for a new one. Returns
    (out, arg): with want_arg the argmax state spmm_fwd(MAX) would have written (spmm_bwd reads it,
    max_arg_positions decodes it)."""
    H = x.size(1)
    if out is None:
        out = torch.empty(out_rows, H, dtype=torch.bfloat16, device=x.device)
    arg = None
    if want_arg:
        arg = torch.empty(_lib.query("bgnn_spmm_max_arg_bytes", out_rows, H, csr.plan.n_heavy), dtype=torch.uint8,
                          device=x.device)
    part = _partial(csr, H, 2 if want_arg else 0, x.device)
    if out_rows > 0:
        _lib.call("bgnn_spmm_max_bf16", csr.ref(), x.data_ptr(), x.stride(0), H, out.data_ptr(), out.stride(0),
                  None if arg is None else arg.data_ptr(), None if part is None else part.data_ptr(), _stream())
    return out, arg


def spmm_max_pack_bf16(csr, x: torch.Tensor, out_rows: int, out: torch.Tensor = None):
    """The max layer's bf16 GEMM operand from f32 rows in one pass (bgnn_spmm_max_pack_bf16):
    a = [bf16(max over the CSR rows of x) | bf16(x)], the maximum and its argmax taken on the f32
    values -- spmm_fwd(MAX)'s values rounded once, and its argmax state bit for bit. x: f32
    [out_rows, H] with unit column stride, rows a multiple of 4 elements apart and a 16-byte aligned
    base; out: a bf16 [out_rows, >= 2H] destination that satisfies _b16_rows (columns from 2H on
    are left alone), or None for a new [out_rows, 2H]. Returns (a, arg): arg is the state spmm_bwd
    reads and max_arg_positions decodes."""
    require_cuda(x, what="spmm_max_pack_bf16")
    H = x.size(1)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1 or x.size(0) != out_rows:
        raise ValueError("spmm_max_pack_bf16: x must be float32 [out_rows, H] with unit column stride")
    if out is None:
        out = torch.empty(out_rows, 2 * H, dtype=torch.bfloat16, device=x.device)
    elif (out.dtype != torch.bfloat16 or out.dim() != 2 or out.size(0) != out_rows or out.size(1) < 2 * H
          or out.stride(1) != 1 or out.device != x.device):
        raise ValueError("spmm_max_pack_bf16: out must be bfloat16 [out_rows, >= 2H] with unit column stride")
    arg = torch.empty(_lib.query("bgnn_spmm_max_arg_bytes", out_rows, H, csr.plan.n_heavy), dtype=torch.uint8,
                      device=x.device)
    part = _partial(csr, H, 2, x.device)
    if out_rows > 0:
        _lib.call("bgnn_spmm_max_pack_bf16", csr.ref(), x.data_ptr(), x.stride(0), H, out.data_ptr(), out.stride(0),
                  arg.data_ptr(), None if part is None else part.data_ptr(), _stream())
    return out, arg


class _AggregateMaxBf16(torch.autograd.Function):
    """max aggregation of bf16 rows on the bf16 kernel, output bf16 or its exact f32 widening. The
    backward is the f32 route's: the gradient upcast to f32, bgnn_spmm_bwd_max on the saved argmax
    state, the result rounded to bf16 once."""

    @staticmethod
    def forward(ctx, x, graph: Graph, out_f32: bool):
        out, arg = spmm_max_bf16(graph.fwd, x, graph.num_nodes, want_arg=x.requires_grad)
        ctx.graph = graph
        ctx.save_for_backward(arg if arg is not None else torch.empty(0, device=x.device))
        return out.float() if out_f32 else out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        graph = ctx.graph
        gx = spmm_bwd(graph.bwd, graph.perm_t, graph.fwd.rowptr, g.float(), 2, arg, graph.num_nodes)
        return gx.to(torch.bfloat16), None, None


class _AggregateBf16(torch.autograd.Function):
    """sum / mean aggregation of bf16 rows on the bf16 kernels, output bf16 or f32; the backward
    gathers the incoming gradient as bf16 (a f32 gradient is rounded once) and returns bf16."""

    @staticmethod
    def forward(ctx, x, graph: Graph, reduce: int, out_f32: bool):
        ctx.graph = graph
        ctx.reduce = reduce
        return spmm_fwd_bf16(graph.fwd, x, reduce, graph.num_nodes, out_f32)

    @staticmethod
    def backward(ctx, g):
        graph = ctx.graph
        if g.dtype != torch.bfloat16:
            g = g.to(torch.bfloat16)
        if not _b16_rows(g):
            g = g.contiguous()
        return spmm_bwd_bf16(graph.bwd, graph.fwd.rowptr, g, ctx.reduce, graph.num_nodes), None, None, None


class _Aggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, graph: Graph, reduce: int):
        out, arg = spmm_fwd(graph.fwd, x, reduce, graph.num_nodes, want_arg=x.requires_grad)
        ctx.graph = graph
        ctx.reduce = reduce
        ctx.save_for_backward(arg if arg is not None else torch.empty(0, device=x.device))
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        graph = ctx.graph
        gx = spmm_bwd(graph.bwd, graph.perm_t, graph.fwd.rowptr, g, ctx.reduce,
                      arg if ctx.reduce == 2 else None, graph.num_nodes)
        return gx, None, None


def aggregate(x: torch.Tensor, graph: Graph, reduce: str = "sum", out_dtype=None) -> torch.Tensor:
    """out[i] = AGG_{j: (j -> i) in E} x[j]  (PyG SAGEConv aggregation), in x's dtype.
    bfloat16 x: out_dtype=torch.float32 keeps the f32 accumulator's value instead of rounding it to
    bf16. sum / mean over rows the bf16 kernels can read in place (_b16_width, _b16_rows: a column
    slice of a wider tensor included) run on them, forward and backward; max over such rows runs
    its forward on the bf16 max kernel (exact: the maximum of bf16 values is one of them; values,
    ties and the argmax state are the float32 kernel's) and its backward on the float32 argmax
    kernel, rounded once. Every other case -- other widths or layouts -- is upcast, run on the
    float32 kernels and rounded once."""
    x = _check_x(x, "aggregate", bf16=True)
    if x.size(0) != graph.num_nodes:
        raise ValueError(f"aggregate: x has {x.size(0)} rows, graph has {graph.num_nodes} nodes")
    if out_dtype not in (None, x.dtype, torch.float32):
        raise TypeError(f"aggregate: out_dtype must be the input's dtype or float32 (got {out_dtype})")
    r = REDUCE[reduce]
    if x.dtype == torch.float32:
        return _Aggregate.apply(x, graph, r)
    out_f32 = out_dtype == torch.float32
    if _b16_width(x.size(1)) and _b16_rows(x):
        if r == 2:
            return _AggregateMaxBf16.apply(x, graph, out_f32)
        return _AggregateBf16.apply(x, graph, r, out_f32)
    out = _Aggregate.apply(x.float().contiguous(), graph, r)
    return out if out_f32 else out.to(torch.bfloat16)


class _SegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, seg: SegmentIndex, reduce: int):
        out, arg = spmm_fwd(seg.fwd, src, reduce, seg.num_rows, want_arg=src.requires_grad)
        ctx.seg = seg
        ctx.reduce = reduce
        ctx.save_for_backward(arg if arg is not None else torch.empty(0, device=src.device))
        return out

    @staticmethod
    def backward(ctx, g):
        seg = ctx.seg
        r = ctx.reduce
        if r == 2:
            (arg,) = ctx.saved_tensors
            # position i receives g[seg(i), c] where arg[seg(i), c] is i's slot in the forward CSR.
            slot = torch.empty(seg.n, dtype=torch.int32, device=g.device)
            slot[seg.fwd.col[:seg.n].long()] = torch.arange(seg.n, dtype=torch.int32, device=g.device)
            return spmm_bwd(seg.bwd, slot, seg.fwd.rowptr, g, 2, arg, seg.n), None, None
        # sum / mean: every position receives its segment's gradient row (a broadcast;
        # one HBM write of the output, no gather structure needed)
        g = g.contiguous()
        if r == 1:
            cnt = seg.fwd.degree().clamp_min(1).to(g.dtype)
            g = g / cnt.unsqueeze(1)
        return g.index_select(0, seg.index), None, None


class _SegmentReduceBf16(torch.autograd.Function):
    """sum / mean over segments of a bf16 [n, H] source into f32 [R, H] (bgnn_segment_sum_bf16);
    backward: every position receives its segment's (scaled) gradient row, in bf16."""

    @staticmethod
    def forward(ctx, src, seg: SegmentIndex, mean: bool):
        H = src.size(1)
        out = torch.empty(seg.num_rows, H, dtype=torch.float32, device=src.device)
        _lib.call("bgnn_segment_sum_bf16", seg.fwd.rowptr.data_ptr(), seg.fwd.col.data_ptr(), seg.num_rows,
                  src.data_ptr(), src.stride(0), H, int(mean), out.data_ptr(), out.stride(0), _stream())
        ctx.seg, ctx.mean = seg, mean
        return out

    @staticmethod
    def backward(ctx, g):
        seg = ctx.seg
        g = g.contiguous()
        H = g.size(1)
        if g.dtype == torch.float32 and g.is_cuda and H % 8 == 0 and H <= 512 and g.data_ptr() % 16 == 0:
            # one pass: scale, bf16 rounding and the broadcast to every position (bgnn_segment_bcast_bf16)
            out = torch.empty(seg.n, H, dtype=torch.bfloat16, device=g.device)
            _lib.call("bgnn_segment_bcast_bf16", seg.fwd.rowptr.data_ptr(), seg.fwd.col.data_ptr(), seg.num_rows,
                      g.data_ptr(), g.stride(0), H, int(ctx.mean), out.data_ptr(), out.stride(0), _stream())
            return out, None, None
        if ctx.mean:
            g = g / seg.fwd.degree().clamp_min(1).to(g.dtype).unsqueeze(1)
        return g.to(torch.bfloat16).index_select(0, seg.index), None, None


def segment_reduce(src: torch.Tensor, seg: SegmentIndex, reduce: str = "sum") -> torch.Tensor:
    if src.dtype == torch.bfloat16 and reduce in ("sum", "add", "mean"):
        require_cuda(src, what="segment_reduce")
        src = src.contiguous()
        if src.dim() != 2 or src.size(0) != seg.n or src.size(1) % 8 or src.size(1) > 512:
            raise ValueError("segment_reduce(bf16): need [n, H] with H % 8 == 0, H <= 512")
        return _SegmentReduceBf16.apply(src, seg, reduce == "mean")
    if src.dtype == torch.bfloat16 and reduce == "max":
        # exact through the float32 kernel: the maximum of bf16 values is one of them
        return segment_reduce(src.float(), seg, reduce).to(torch.bfloat16)
    src = _check_x(src, "segment_reduce")
    if src.size(0) != seg.n:
        raise ValueError(f"segment_reduce: src has {src.size(0)} rows, index has {seg.n} entries")
    return _SegmentReduce.apply(src, seg, REDUCE[reduce])
