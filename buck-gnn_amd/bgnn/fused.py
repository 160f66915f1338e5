"""Fused GraphSAGE layer for the BuckGNN layer loop (Models/BuckGNN.py:430-444).

One autograd node per layer computes, for train or eval mode,

    x_next = Dropout_p( ReLU( BN( normalize( SAGEConv(x_prev, edge_index) ) ) ) + [skip] x_prev )

with SAGEConv(aggr in {add, sum, mean}, normalize=True) evaluated transform-first:

    z   = x_prev · [W_l ; W_r]^T                 one fp32 MFMA GEMM, stored as planes
                                                  z_l [N, H] and z_r [N, H]
    h_i = AGG_{j->i} z_l[j] + z_r[i] + b_l        (= lin_l(AGG x) + lin_r(x): AGG is linear)
    o_i = h_i / max(||h_i||, 1e-12)               fused into the aggregation kernel,
                                                  which also emits BatchNorm partial sums

The backward mirrors it: BN statistics of dL/dx_next, a row-wise kernel for the
BN + normalize backward giving dh, the transpose aggregation dz_l = A^T dh, and
two GEMMs  dx = [dz_l | dh] · [W_l ; W_r]  and  d[W_l ; W_r] = [dz_l | dh]^T · x_prev.
"""
from __future__ import annotations

import torch

from . import _lib
from .graph import Graph, _stream, require_cuda
from .ops import _ptr, spmm_bwd_into, spmm_bwd_max_into

# "hip" = bgnn_gemm_f32 (hand-written f32 MFMA); "torch" = torch.mm (rocBLAS/hipBLASLt),
# kept only for A/B measurement. Both run on the GPU.
GEMM_BACKEND = "hip"

# z = [z_l | z_r] and dz = [dz_l | dh] are stored either interleaved ([N, 2H], row i holds
# both halves) or as two dense [N, H] planes (needs H % PLANE_TILE == 0, the GEMM tile width).
# Measured on MI355X (cfg2, tools/tune_agg.py + tools/ab_step.py): the forward aggregation is
# 5% faster on interleaved z (z_l[i], z_r[i] in one DRAM page), the transpose aggregation 4%
# faster on dz planes, but the plane-operand GEMMs lose more than that: whole step 18.83 ms
# interleaved vs 18.92 (dz planes) / 19.12 (z planes) / 19.23 (both).
PLANE_TILE = 128
Z_PLANES = False
DZ_PLANES = False
# folded input transform: the weight-by-weight products (Wf = Wcat W_in, its gradients; no node
# dimension, <= 0.3 GFLOP each) in the grouped native launches of csrc/fold.hip
# (bgnn_fold_weights_fwd / _bwd: one or two launches per direction instead of ~7, bit-identical
# to the bgnn_gemm chain, which stays as the fallback for shapes the planner does not put on the
# 128 x 128 f16x3 tile; A/B switch)
FOLD_NATIVE = True
# skip layers' dgrad adds the dropout-masked incoming gradient in its epilogue
# (bgnn_gemm_f32_dropadd) instead of reading a skip gradient bgnn_sage_bwd_rows wrote
DGRAD_DROPADD = True

# bf16-stored Linear backward (EA_GNN's bf16 configuration): ReLU mask + f32 bias-gradient sums
# in one bgnn pass (bgnn_linear_bwd_prep_bf16) instead of torch threshold_backward + sum (A/B switch)
BF16_PREP = True
# [W_l;W_r] of all layers packed by a multi-tensor copy into a persistent buffer (not torch.cat)
PERSISTENT_WPACK = True
# max aggregation: the two input-gradient products as one GEMM [dh W_l | dh W_r (+ drop(g))] and
# the two weight gradients as one [agg | x]^T dh (A/B switch)
MAX_MERGED = True
# forward / input-gradient GEMMs of the K = H layers take [W_l;W_r] (and its transpose) as images
# pre-split once per step (bgnn_gemm_wsplit), staged by LDS-DMA in the GEMM (bgnn_gemm_f32_w);
# bit-identical to the register-staged path (A/B switch)
WSPLIT = True

# Optional per-launch timing (bench.py): name -> list of (start, end) HIP events recorded
# on the launching stream around the named launch.
TIMERS = None
# event factory for TIMERS (None: torch.cuda.Event(enable_timing=True)); bench.py installs HIP events
# created with hipEventDisableSystemFence: a default event's record does a system-scope release (cache
# writeback + invalidate) that leaves the GPU idle ~5 us per event between the timed kernels
TIMER_EVENT = None


class _timed:
    __slots__ = ("name", "ev")

    def __init__(self, name):
        self.name = name
        self.ev = None

    def __enter__(self):
        if TIMERS is not None and self.name is not None:   # (a launcher called without a timer key)
            mk = TIMER_EVENT or (lambda: torch.cuda.Event(enable_timing=True))
            self.ev = (mk(), mk())
            self.ev[0].record()
        return self

    def __exit__(self, *exc):
        if self.ev is not None:
            self.ev[1].record()
            TIMERS.setdefault(self.name, []).append(self.ev)
        return False


class Planes:
    """A row-major matrix [rows, P*blk] stored as P contiguous [rows, blk] planes (tensor t of
    shape [P, rows, blk]). Used for z = [z_l | z_r] and dz = [dz_l | dh], whose halves the
    aggregation kernels read as separate dense arrays."""
    __slots__ = ("t",)

    def __init__(self, t: torch.Tensor):
        if t.dim() != 3 or not t.is_contiguous():
            raise ValueError("Planes: need a contiguous [P, rows, blk] tensor")
        self.t = t

    def size(self, d):
        return self.t.size(1) if d == 0 else self.t.size(0) * self.t.size(2)

    def dense(self) -> torch.Tensor:
        return self.t.permute(1, 0, 2).reshape(self.size(0), self.size(1))


class Pair:
    """The row-wise concatenation [a | b] of two [rows, blk] fp32 matrices with the same row
    stride, read in place as one GEMM A operand (the plane-split addressing of the bgnn GEMM:
    plane 1 lives (b - a) elements after plane 0). The aggregate-first max-aggregation layer
    multiplies [AGG x | x] by [W_l | W_r]^T this way without building the concatenation."""
    __slots__ = ("a", "b")

    def __init__(self, a: torch.Tensor, b: torch.Tensor):
        if (a.dim() != 2 or a.shape != b.shape or a.stride() != b.stride() or a.stride(1) != 1
                or a.dtype != torch.float32 or b.dtype != torch.float32 or a.device != b.device):
            raise ValueError("Pair: need two fp32 [rows, blk] matrices of one shape and row stride")
        self.a, self.b = a, b

    def size(self, d):
        return self.a.size(0) if d == 0 else 2 * self.a.size(1)

    def dense(self) -> torch.Tensor:
        return torch.cat([self.a, self.b], 1)


def _operand(x):
    """(ptr, ld, blk, pstride) of a dense tensor, Planes or Pair operand."""
    if isinstance(x, Planes):
        P, R, blk = x.t.shape
        return x.t.data_ptr(), blk, (blk if P > 1 else 0), R * blk
    if isinstance(x, Pair):
        diff = x.b.data_ptr() - x.a.data_ptr()
        if diff % 16:   # (the GEMM's float4 loads test plane 0's alignment only)
            raise ValueError("Pair: the two halves must be 16-byte aligned relative to each other")
        return x.a.data_ptr(), x.a.stride(0), x.a.size(1), diff // 4
    if x.stride(1) != 1:
        raise ValueError("gemm: operands must have unit column stride")
    return x.data_ptr(), x.stride(0), 0, 0


def _saved(t, dev):
    """t, or an empty placeholder for None (save_for_backward takes tensors only)."""
    return t if t is not None else torch.empty(0, device=dev)


def _workspace(nbytes: int, dev):
    """A kernel's scratch of nbytes bytes (None for 0)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None


def gemm_workspace(M: int, N: int, K: int, trans_a, trans_b, prec: int, dev):
    """(ws, ws_bytes): the split-K scratch of an M x N x K bgnn GEMM (prec 0: f32-accurate,
    1: bf16 operands), which every GEMM entry point takes as its last two arguments."""
    ws_bytes = _lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, int(trans_a), int(trans_b), prec)
    return _workspace(ws_bytes, dev), ws_bytes


def reduce_partials(part: torch.Tensor, slots: int, C: int, out0: torch.Tensor, out1: torch.Tensor = None):
    """Column sums over the slots of a row pass's [slots, 2, C] partials: plane 0 into out0 and,
    where given, plane 1 into out1 (bgnn_reduce_partials)."""
    _lib.call("bgnn_reduce_partials", part.data_ptr(), slots, C, out0.data_ptr(), _ptr(out1), 0, _stream())


def absmax(x: torch.Tensor, out: torch.Tensor = None, accumulate: bool = False) -> torch.Tensor:
    """max |x| of a row-major fp32 matrix (unit column stride) into a 1-element device tensor
    (bgnn_absmax_f32; accumulate folds into out's current value)."""
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
        accumulate = False
    x2 = x.reshape(x.size(0), -1) if x.dim() != 2 else x
    _lib.call("bgnn_absmax_f32", x2.data_ptr(), x2.size(0), x2.size(1), x2.stride(0), out.data_ptr(),
              int(accumulate), _stream())
    return out


def gemm(a, b: torch.Tensor, trans_a: bool, trans_b: bool, out=None, beta: float = 0.0, alpha: float = 1.0,
         bias: torch.Tensor = None, relu: bool = False, a_amax: torch.Tensor = None,
         b_amax: torch.Tensor = None, c_amax: torch.Tensor = None, bf16: bool = False):
    """C = act(alpha * op(a) @ op(b) + beta * C + bias) (fp32, row-major operands, unit column
    stride). `a` and `out` may be Planes. a_amax / b_amax: optional device scalars holding
    max|a| / max|b| (the f16x3 operand scales; computed inside when absent); c_amax: optional
    device scalar that max |C| is folded into (bgnn_gemm_f32_scaled). bf16: round both operands
    to bf16 (one MFMA product, f32 accumulation and output) instead of the f32-accurate split."""
    M = a.size(1) if trans_a else a.size(0)
    K = a.size(0) if trans_a else a.size(1)
    N = b.size(0) if trans_b else b.size(1)
    Kb = b.size(1) if trans_b else b.size(0)
    if K != Kb:
        raise ValueError(f"gemm: inner dims differ ({K} vs {Kb})")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=b.device)
        beta = 0.0
    if out.size(0) != M or out.size(1) != N:
        raise ValueError(f"gemm: out is {out.size(0)}x{out.size(1)}, expected {M}x{N}")
    if GEMM_BACKEND == "torch":
        ad = a.dense() if isinstance(a, (Planes, Pair)) else a
        od = out.dense() if isinstance(out, Planes) else out
        ra = ad.t() if trans_a else ad
        rb = b.t() if trans_b else b
        if beta == 0.0:
            torch.mm(ra, rb, out=od)
            if alpha != 1.0:
                od.mul_(alpha)
        else:
            od.mul_(beta).addmm_(ra, rb, alpha=alpha)
        if bias is not None:
            od.add_(bias)
        if relu:
            od.relu_()
        if isinstance(out, Planes):
            out.t.copy_(od.view(M, out.t.size(0), out.t.size(2)).permute(1, 0, 2))
        return out
    pa, lda, a_blk, a_ps = _operand(a)
    pb, ldb, _, _ = _operand(b)
    pc, ldc, c_blk, c_ps = _operand(out)
    prec = 1 if bf16 else 0
    ws, ws_bytes = gemm_workspace(M, N, K, trans_a, trans_b, prec, b.device)
    _lib.call("bgnn_gemm_f32_scaled", int(trans_a), int(trans_b), M, N, K, float(alpha), pa, lda, a_blk, a_ps,
              pb, ldb, float(beta), pc, ldc, c_blk, c_ps, _ptr(bias), int(relu),
              _ptr(a_amax), _ptr(b_amax), _ptr(c_amax), prec, _ptr(ws), ws_bytes, _stream())
    return out


_BF16_BUILT = {(0, 1): (0, 1, 3, 4, 5, 7), (1, 0): (0, 1, 2, 3)}
# bf16-stored A times an f32 weight (A B^T, K % 64 == 0): round the weight to bf16 once (torch's
# round-to-nearest-even, the rounding the GEMM applies in-tile) so that both operands are bf16 and
# the LDS-DMA bf16 kernel (gemm_b16.hip, bit-identical) takes the product. False: the
# register-staged kernel reads the f32 weight (A/B).
B16_WEIGHTS = True


def b16_weight(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """w (the B^T operand of a K-contiguous product with a) as bf16 when a is stored bf16 and
    the LDS-DMA bf16 kernel applies; else w unchanged."""
    if B16_WEIGHTS and a.dtype == torch.bfloat16 and w.dtype == torch.float32 and w.size(1) % 64 == 0:
        return w.to(torch.bfloat16)
    return w


def gemm_bf16(a: torch.Tensor, b: torch.Tensor, trans_a: bool, trans_b: bool, out=None, out_bf16: bool = False,
              bias: torch.Tensor = None, relu: bool = False):
    """C = act(op(a) @ op(b) + bias) on the bf16-operand GEMM (one bf16 MFMA product, f32
    accumulation) with each of a / b / C stored as float32 or bfloat16 (bgnn_gemm_bf16): the bf16
    configuration of EA_GNN keeps its per-edge activations in bf16 (half the HBM bytes)."""
    for t in (a, b):
        if t.dtype not in (torch.float32, torch.bfloat16) or t.stride(1) != 1:
            raise ValueError("gemm_bf16: operands must be float32 / bfloat16 with unit column stride")
    M = a.size(1) if trans_a else a.size(0)
    K = a.size(0) if trans_a else a.size(1)
    N = b.size(0) if trans_b else b.size(1)
    if (b.size(1) if trans_b else b.size(0)) != K:
        raise ValueError("gemm_bf16: inner dims differ")
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=b.device)
    if not trans_a and trans_b:
        b = b16_weight(a, b)
    storage = ((1 if a.dtype == torch.bfloat16 else 0) | (2 if b.dtype == torch.bfloat16 else 0)
               | (4 if out.dtype == torch.bfloat16 else 0))
    if storage not in _BF16_BUILT.get((int(trans_a), int(trans_b)), (0,)):
        raise ValueError(f"gemm_bf16: storage {storage} with trans_a={trans_a}, trans_b={trans_b} is not built")
    ws, ws_bytes = gemm_workspace(M, N, K, trans_a, trans_b, 1, b.device)
    _lib.call("bgnn_gemm_bf16", int(trans_a), int(trans_b), M, N, K, 1.0, a.data_ptr(), a.stride(0), b.data_ptr(),
              b.stride(0), 0.0, out.data_ptr(), out.stride(0), _ptr(bias), int(relu), storage, _ptr(ws), ws_bytes,
              _stream())
    return out


class LinearBf16Fn(torch.autograd.Function):
    """y = act(x W^T + b) with bf16 operands and bf16 storage of x and / or y (EA_GNN's bf16
    configuration: per-edge activations in bf16, like torch autocast's bf16 Linear). Backward:
    ReLU mask and bias gradient (f32 sum) in torch, dgrad / wgrad on bgnn_gemm_bf16 (dx in x's
    dtype, dW f32)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu: bool, out_bf16: bool):
        x = x.contiguous()
        y = gemm_bf16(x, weight.contiguous(), False, True, out_bf16=out_bf16, bias=bias, relu=relu)
        ctx.relu, ctx.has_bias = relu, bias is not None
        ctx.save_for_backward(x, weight, _saved(y if relu else None, x.device))
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, y = ctx.saved_tensors
        if g.dtype == torch.bfloat16 and BF16_PREP:
            g, db = relu_bias_grad_bf16(g, y if ctx.relu else None, ctx.has_bias)
        else:
            g = g.contiguous()
            if ctx.relu:
                g = torch.ops.aten.threshold_backward(g, y, 0.0)
            db = torch.sum(g, 0, dtype=torch.float32) if ctx.has_bias else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = gemm_bf16(g, weight.t().contiguous(), False, True, out_bf16=x.dtype == torch.bfloat16)
        dw = gemm_bf16(g, x, True, False)
        return dx, dw, db, None, None


def linear_bf16(x, weight, bias=None, relu=False, out_bf16=True):
    return LinearBf16Fn.apply(x, weight, bias, relu, out_bf16)


def mlp_bf16(seq: torch.nn.Sequential, x: torch.Tensor, out_bf16: bool = True):
    """An nn.Sequential of Linear/ReLU with bf16 operands, every activation stored in bf16
    (out_bf16: also the last one), each ReLU fused into the preceding Linear's epilogue."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, torch.nn.Linear):
            fuse = i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU)
            last = i + (2 if fuse else 1) >= len(mods)
            x = linear_bf16(x, m.weight, m.bias, fuse, out_bf16 or not last)
            i += 2 if fuse else 1
        else:
            x = m(x)
            i += 1
    return x


def relu_bias_grad_bf16(g: torch.Tensor, y=None, bias: bool = True):
    """(g', db) for the backward of act(x W^T + b) with bf16 g (and bf16 ReLU output y): g' = g
    masked by y > 0 (bf16; g itself when y is None), db = f32 column sums of g' (None when bias is
    False). One pass over g (bgnn_linear_bwd_prep_bf16) instead of torch's threshold_backward plus
    a float32 sum, each of which torch splits in two launches at E x 512 bf16 (> 2^31 bytes)."""
    g = g.contiguous()
    C = g.size(1)
    ok = (C % 8 == 0 and 8 <= C <= 2048 and 256 % (C // 8) == 0 and g.data_ptr() % 16 == 0
          and (y is None or (y.dtype == torch.bfloat16 and y.is_contiguous() and y.data_ptr() % 16 == 0)))
    if not ok:
        if y is not None:
            g = torch.ops.aten.threshold_backward(g, y, 0.0)
        return g, (torch.sum(g, 0, dtype=torch.float32) if bias else None)
    if y is None and not bias:
        return g, None
    gm = torch.empty_like(g) if y is not None else g
    slots = _lib.query("bgnn_linear_bwd_prep_slots")
    part = torch.empty(slots, 2, C, dtype=torch.float32, device=g.device)
    _lib.call("bgnn_linear_bwd_prep_bf16", g.data_ptr(), _ptr(y), g.size(0), C,
              gm.data_ptr() if y is not None else None, part.data_ptr(), _stream())
    db = None
    if bias:
        db = torch.empty(C, dtype=torch.float32, device=g.device)
        reduce_partials(part, slots, C, db)
    return gm, db


def relu_bias_grad(g: torch.Tensor, y=None, bias: bool = True):
    """(g', db, max|g'|) for the backward of act(x W^T + b): g' = g masked by y > 0 (y = the ReLU
    output; None = no ReLU), db = column sums of g' (None when bias is False). One pass over g
    (bgnn_linear_bwd_prep: mask, bias-gradient partials and max|g'|) where the width allows,
    else torch threshold_backward + sum + a max pass."""
    g = g.contiguous()
    C = g.size(1)
    if C % 4 == 0 and 4 <= C <= 1024 and 256 % (C // 4) == 0:
        gm = torch.empty_like(g) if y is not None else g
        slots = _lib.query("bgnn_linear_bwd_prep_slots")
        part = torch.empty(slots, 2, C, dtype=torch.float32, device=g.device)
        g_amax = torch.zeros(1, dtype=torch.float32, device=g.device)
        _lib.call("bgnn_linear_bwd_prep", g.data_ptr(), _ptr(y), g.size(0), C,
                  gm.data_ptr() if y is not None else None, part.data_ptr(), g_amax.data_ptr(), _stream())
        db = None
        if bias:
            db = torch.empty(C, dtype=torch.float32, device=g.device)
            reduce_partials(part, slots, C, db)
        return gm, db, g_amax
    if y is not None:
        g = torch.ops.aten.threshold_backward(g, y, 0.0)   # ReLU mask in one pass
    return g, (g.sum(0) if bias else None), absmax(g)


class LinearFn(torch.autograd.Function):
    """(y, max|y|) with y = act(x W^T + b) on the bgnn GEMM (bias + ReLU fused in the epilogue,
    max|y| folded in there too: the next Linear's operand scale); backward: dgrad and wgrad
    GEMMs on the same kernel, sharing one max|g| pass (Models/BuckGNN.py:67-74 encoder)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu: bool, x_amax, bf16: bool = False, amax=None):
        x = x.contiguous()
        if amax is None:   # [max|W|, max|y|], zeroed (callers batch these: one fill per MLP)
            amax = torch.zeros(2, dtype=torch.float32, device=x.device)
        w_amax, y_amax = amax[0:1], amax[1:2]
        if not bf16:   # (bf16 operands need no scales)
            absmax(weight, w_amax, accumulate=True)
            if x_amax is None:
                x_amax = absmax(x)
        y = gemm(x, weight.contiguous(), trans_a=False, trans_b=True, bias=bias, relu=relu,
                 a_amax=None if bf16 else x_amax, b_amax=None if bf16 else w_amax,
                 c_amax=None if bf16 else y_amax, bf16=bf16)
        ctx.relu = relu
        ctx.bf16 = bf16
        ctx.has_bias = bias is not None
        ctx.save_for_backward(x, weight, _saved(y if relu else None, x.device), _saved(x_amax, x.device), w_amax)
        ctx.mark_non_differentiable(y_amax)
        ctx.set_materialize_grads(False)   # no zero-filled gradient for y_amax
        return y, y_amax

    @staticmethod
    def backward(ctx, g, _g_amax):
        if g is None:
            return None, None, None, None, None, None, None
        x, weight, y, x_amax, w_amax = ctx.saved_tensors
        bf16 = ctx.bf16
        g, db, g_amax = relu_bias_grad(g, y if ctx.relu else None, ctx.has_bias)
        if bf16:
            g_amax = None
        w_amax = None if bf16 else w_amax
        x_amax = None if bf16 else x_amax
        dx = None
        if ctx.needs_input_grad[0]:
            # (W transposed once so the dgrad reads its B operand K-contiguous)
            dx = gemm(g, weight.t().contiguous(), trans_a=False, trans_b=True, a_amax=g_amax, b_amax=w_amax,
                      bf16=bf16)
        dw = gemm(g, x, trans_a=True, trans_b=False, a_amax=g_amax, b_amax=x_amax, bf16=bf16)
        return dx, dw, db, None, None, None, None


def linear(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor = None, relu: bool = False,
           x_amax: torch.Tensor = None, return_amax: bool = False, bf16: bool = False, amax_buf=None):
    """act(x W^T + b) on the bgnn GEMM; bf16: bf16 operands, f32 accumulation and output.
    amax_buf: optional zeroed 2-float device scratch for [max|W|, max|y|]."""
    y, y_amax = LinearFn.apply(x, weight, bias, relu, x_amax, bf16, amax_buf)
    return (y, y_amax) if return_amax else y


# the node encoder's leading Linear(16,64).ReLU.Linear(64,128).ReLU as one VALU kernel
# (bgnn_mlp2_fwd / _bwd) instead of two GEMM launches with their operand-max passes:
# fwd 57 us, bwd 108 us + 11 us slot sums on cfg2; the step 9.94 -> 9.82 ms (tools/ab_step.py);
# round 4: conflict-free W2^T load, backward at 512 threads: fwd 54 us, bwd 94 us (bit-identical)
FUSED_MLP2 = True


class _Mlp2Fn(torch.autograd.Function):
    """(h, max|h|) with h = ReLU(ReLU(x W1^T + b1) W2^T + b2) on bgnn_mlp2_fwd; backward: the
    four weight / bias gradients from bgnn_mlp2_bwd (x gets none: node features are data)."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2):
        N, F = x.shape
        D1, D2 = W1.size(0), W2.size(0)
        h = torch.empty(N, D2, dtype=torch.float32, device=x.device)
        amax = torch.zeros(1, dtype=torch.float32, device=x.device)
        _lib.call("bgnn_mlp2_fwd", x.data_ptr(), N, F, D1, D2, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                  b2.data_ptr(), h.data_ptr(), amax.data_ptr(), _stream())
        ctx.save_for_backward(x, W1, b1, W2, h)
        ctx.mark_non_differentiable(amax)
        ctx.set_materialize_grads(False)
        return h, amax

    @staticmethod
    def backward(ctx, dh, _g_amax):
        if dh is None:
            return None, None, None, None, None
        x, W1, b1, W2, h = ctx.saved_tensors
        dh = dh.contiguous()
        N, F = x.shape
        D1, D2 = W1.size(0), W2.size(0)
        dW1, db1 = torch.empty_like(W1), torch.empty_like(b1)
        dW2 = torch.empty_like(W2)
        db2 = torch.empty(D2, dtype=torch.float32, device=x.device)
        ws_bytes = _lib.query("bgnn_mlp2_bwd_ws_bytes", N)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
        _lib.call("bgnn_mlp2_bwd", x.data_ptr(), N, F, D1, D2, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                  h.data_ptr(), dh.data_ptr(), dW1.data_ptr(), db1.data_ptr(), dW2.data_ptr(), db2.data_ptr(),
                  ws.data_ptr(), ws_bytes, _stream())
        return None, dW1, db1, dW2, db2


class SmallMLPFn(torch.autograd.Function):
    """An nn.Sequential of Linear (+ ReLU) layers on a few rows (the decoder on the pooled
    [graphs, H] features, Models/BuckGNN.py:94-100) with one bgnn_small_linear_fwd launch per layer
    (bias and ReLU inside) and one bgnn_small_linear_bwd per layer backward (ReLU mask, dW, db and
    dx together) instead of a library GEMM, a ReLU kernel, bias reductions and ReLU-mask kernels
    per layer. Inputs: x, then (W, b, relu) per layer flattened as weights / biases."""

    @staticmethod
    def forward(ctx, x, relus, *params):
        x = x.contiguous()
        B = x.size(0)
        s = _stream()
        acts = [x]
        for i, relu in enumerate(relus):
            W, b = params[2 * i], params[2 * i + 1]
            N, K = W.shape
            y = torch.empty(B, N, dtype=torch.float32, device=x.device)
            _lib.call("bgnn_small_linear_fwd", acts[-1].data_ptr(), B, K, W.data_ptr(), _ptr(b), N, int(relu),
                      y.data_ptr(), s)
            acts.append(y)
        ctx.relus = relus
        ctx.has_bias = [params[2 * i + 1] is not None for i in range(len(relus))]
        ctx.save_for_backward(*acts, *[params[2 * i] for i in range(len(relus))])
        return acts[-1]

    @staticmethod
    def backward(ctx, g):
        L = len(ctx.relus)
        saved = ctx.saved_tensors
        acts, Ws = saved[:L + 1], saved[L + 1:]
        s = _stream()
        g = g.contiguous()
        B = g.size(0)
        grads = [None] * (2 * L)
        gx = None
        for i in reversed(range(L)):
            W = Ws[i]
            N, K = W.shape
            dW = torch.empty_like(W)
            db = torch.empty(N, dtype=torch.float32, device=W.device) if ctx.has_bias[i] else None
            need_dx = i > 0 or ctx.needs_input_grad[0]
            dx = torch.empty(B, K, dtype=torch.float32, device=W.device) if need_dx else None
            _lib.call("bgnn_small_linear_bwd", g.data_ptr(), acts[i + 1].data_ptr() if ctx.relus[i] else None,
                      acts[i].data_ptr(), B, K, W.data_ptr(), N, _ptr(dx), dW.data_ptr(), _ptr(db), s)
            grads[2 * i], grads[2 * i + 1] = dW, db
            g = dx
            gx = dx
        return (gx, None, *grads)


# the decoder on the pooled features as bgnn_small_linear layers (SmallMLPFn) when it qualifies
SMALL_MLP = True
SMALL_MLP_MAX_ROWS = 256


def small_mlp(seq: torch.nn.Sequential, x: torch.Tensor):
    """seq(x) through SmallMLPFn when seq is Linear (ReLU) ... Linear with f32 weights, x on the
    GPU with at most SMALL_MLP_MAX_ROWS rows and every in_features a multiple of 4; else None."""
    if not (SMALL_MLP and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
            and 0 < x.size(0) <= SMALL_MLP_MAX_ROWS):
        return None
    mods = list(seq)
    relus, params = [], []
    i = 0
    while i < len(mods):
        m = mods[i]
        if not (isinstance(m, torch.nn.Linear) and m.weight.dtype == torch.float32 and m.in_features % 4 == 0
                and m.weight.is_contiguous()):
            return None
        relu = i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU)
        relus.append(relu)
        params += [m.weight, m.bias]
        i += 2 if relu else 1
    return SmallMLPFn.apply(x, tuple(relus), *params)


class _Head2Fn(torch.autograd.Function):
    """y = ReLU(x W1^T + b1) W2^T + b2 on bgnn_head2_fwd (the node-level decoder's tail, one launch,
    the hidden activation never stored); backward: dx and the four weight / bias gradients from
    bgnn_head2_bwd, which recomputes the hidden layer from x (deterministic slot sums)."""

    @staticmethod
    def forward(ctx, x, W1, b1, W2, b2):
        N, D0 = x.shape
        D1, C = W1.size(0), W2.size(0)
        y = torch.empty(N, C, dtype=torch.float32, device=x.device)
        _lib.call("bgnn_head2_fwd", x.data_ptr(), N, D0, D1, C, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                  b2.data_ptr(), y.data_ptr(), _stream())
        ctx.save_for_backward(x, W1, b1, W2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, W1, b1, W2 = ctx.saved_tensors
        dy = dy.contiguous()
        N, D0 = x.shape
        D1, C = W1.size(0), W2.size(0)
        dx = torch.empty_like(x)
        dW1, db1, dW2 = torch.empty_like(W1), torch.empty_like(b1), torch.empty_like(W2)
        db2 = torch.empty(C, dtype=torch.float32, device=x.device)
        ws_bytes = _lib.query("bgnn_head2_bwd_ws_bytes", N, D0, C)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
        _lib.call("bgnn_head2_bwd", x.data_ptr(), N, D0, D1, C, W1.data_ptr(), b1.data_ptr(), W2.data_ptr(),
                  dy.data_ptr(), dx.data_ptr(), dW1.data_ptr(), db1.data_ptr(), dW2.data_ptr(), db2.data_ptr(),
                  ws.data_ptr(), ws_bytes, _stream())
        return dx, dW1, db1, dW2, db2


# the node-level decoder (prediction_type static_disp / static_stress / mode_shape) through
# bgnn_head2 (node_head) instead of the torch modules
FUSED_NODE_HEAD = True


def _head_linears(seq):
    """The Linears of a node-level decoder that bgnn_head2 covers: seq is Linear.ReLU.Linear or
    Linear.ReLU.Linear.ReLU.Linear with f32 contiguous GPU weights and biases, consecutive widths
    agree and the last two Linears have a built shape (bgnn_head2_supported); else None."""
    if not isinstance(seq, torch.nn.Sequential):
        return None
    mods = list(seq)
    want = (torch.nn.Linear, torch.nn.ReLU) * (len(mods) // 2) + (torch.nn.Linear,)
    if len(mods) not in (3, 5) or not all(type(m) is t for m, t in zip(mods, want)):
        return None
    lins = mods[0::2]
    if not all(m.weight.dtype == torch.float32 and m.weight.is_cuda and m.weight.is_contiguous() and m.bias is not None
               and m.bias.is_contiguous() for m in lins):
        return None
    if any(a.out_features != b.in_features for a, b in zip(lins, lins[1:])):
        return None
    l1, l2 = lins[-2:]
    if not _lib.query("bgnn_head2_supported", l1.in_features, l1.out_features, l2.out_features):
        return None
    return lins


def node_head(seq: torch.nn.Sequential, x: torch.Tensor):
    """seq(x) for the node-level decoder: Linear(D0,64).ReLU.Linear(64,C) as one bgnn_head2 kernel
    (h <= 128: the whole decoder), with a leading Linear.ReLU on the bgnn GEMM in front (h >= 256:
    Linear(h,128).ReLU, bias and ReLU in the epilogue). None when seq is not of that form with f32
    contiguous weights and biases, the shapes are not built (bgnn_head2_supported), or x is not a
    float32 [N >= 1, in_features] GPU tensor."""
    if not (FUSED_NODE_HEAD and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.size(0) > 0):
        return None
    lins = _head_linears(seq)
    if lins is None or x.size(1) != lins[0].in_features:
        return None
    l1, l2 = lins[-2:]
    if len(lins) == 3:
        if lins[0].in_features % 4:
            return None
        x = linear(x, lins[0].weight, lins[0].bias, relu=True)
    x = x.contiguous()
    if x.data_ptr() % 16:
        return None
    return _Head2Fn.apply(x, l1.weight, l1.bias, l2.weight, l2.bias)


def head_front_weight(lin: torch.nn.Linear) -> torch.Tensor:
    """The weight of the decoder's front Linear as node_head_bf16's GEMM reads it: rounded to bf16
    once per weight version and kept on the module (as _cached_weights keeps a layer's), where the
    bf16-weight kernel applies (b16_weight); else the f32 weight itself."""
    w = lin.weight
    if not (B16_WEIGHTS and w.size(1) % 64 == 0):
        return w.detach()
    key = (w._version, w.data_ptr(), str(w.device))
    hit = getattr(lin, "_bgnn_head_w16", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        w16 = w.detach().to(torch.bfloat16).contiguous()
    lin._bgnn_head_w16 = (key, w16)
    return w16


def node_head_bf16_accepts(seq) -> bool:
    """Whether node_head_bf16 takes the decoder seq for bf16 rows of seq[0].in_features columns (the
    conditions on seq alone: known before the rows exist)."""
    lins = _head_linears(seq) if FUSED_NODE_HEAD else None
    return lins is not None and lins[0].in_features % 8 == 0


@torch.no_grad()
def node_head_bf16(seq: torch.nn.Sequential, x: torch.Tensor):
    """node_head on bfloat16 rows (eval-mode inference, no autograd): the tail is
    bgnn_head2_fwd_bf16, which widens the bf16 rows exactly and then computes as bgnn_head2_fwd. With
    two Linears (h = 64 or 128) it reads x in place, strided rows included; with three (h >= 256)
    the front Linear.ReLU runs on gemm_bf16 -- bf16 A, the weight rounded to bf16 once
    (head_front_weight), bias and ReLU in the epilogue, a bf16 [N, 128] output -- and the tail
    reads that. Returns f32 [N, C]; None when seq is not node_head's form, or x is not a bfloat16
    [N >= 1, in_features] GPU tensor with unit column stride and 16-byte aligned rows."""
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 2 and x.size(0) > 0 and x.stride(1) == 1
            and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0):
        return None
    if not node_head_bf16_accepts(seq):
        return None
    lins = _head_linears(seq)
    if x.size(1) != lins[0].in_features:
        return None
    l1, l2 = lins[-2:]
    if len(lins) == 3:
        with _timed("head_front_bf16"):
            x = gemm_bf16(x, head_front_weight(lins[0]), trans_a=False, trans_b=True, out_bf16=True,
                          bias=lins[0].bias, relu=True)
    N = x.size(0)
    y = torch.empty(N, l2.out_features, dtype=torch.float32, device=x.device)
    with _timed("head2_bf16"):
        _lib.call("bgnn_head2_fwd_bf16", x.data_ptr(), x.stride(0), N, l1.in_features, l1.out_features,
                  l2.out_features, l1.weight.data_ptr(), l1.bias.data_ptr(), l2.weight.data_ptr(),
                  l2.bias.data_ptr(), y.data_ptr(), _stream())
    return y


def _mlp2_prefix(mods, x: torch.Tensor) -> bool:
    """Whether mods starts with Linear . ReLU . Linear . ReLU that bgnn_mlp2 covers for x."""
    if not FUSED_MLP2 or len(mods) < 4 or x.requires_grad or x.dtype != torch.float32 or x.dim() != 2:
        return False
    l1, r1, l2, r2 = mods[:4]
    if not (isinstance(l1, torch.nn.Linear) and isinstance(l2, torch.nn.Linear) and isinstance(r1, torch.nn.ReLU)
            and isinstance(r2, torch.nn.ReLU) and l1.bias is not None and l2.bias is not None):
        return False
    if l2.in_features != l1.out_features or x.size(1) != l1.in_features:
        return False
    return bool(_lib.query("bgnn_mlp2_supported", l1.in_features, l1.out_features, l2.out_features))


def _require_f32(x: torch.Tensor, what: str) -> None:
    """The f32-accurate fused path reads float32 rows; its custom functions ignore autocast, so a
    bf16 activation can only come from the caller (handing it to the kernels would read past the
    end of its buffer)."""
    if x.dtype != torch.float32:
        raise TypeError(f"{what}: the fused path takes float32 activations (got {x.dtype}); bf16 features run on "
                        "the per-module path (bgnn.nn.SAGEConv)")


def mlp(seq: torch.nn.Sequential, x: torch.Tensor, return_amax: bool = False, bf16: bool = False):
    """Run an nn.Sequential of Linear/ReLU through bgnn GEMMs, fusing each ReLU into the
    preceding Linear's epilogue (same parameters, same result as seq(x)); a leading
    Linear(16,64).ReLU.Linear(64,128).ReLU runs as one bgnn_mlp2 kernel. With return_amax,
    also returns max|output| (device scalar) when the last module is a Linear or that kernel's
    ReLU, else None."""
    _require_f32(x, "mlp")
    mods = list(seq)
    i = 0
    amax = None
    if not bf16 and _mlp2_prefix(mods, x):
        x, amax = _Mlp2Fn.apply(x.contiguous(), mods[0].weight, mods[0].bias, mods[2].weight, mods[2].bias)
        if len(mods) == 4:
            return (x, amax) if return_amax else x
        mods = mods[4:]
    n_lin = sum(isinstance(m, torch.nn.Linear) for m in mods)
    bufs = torch.zeros(n_lin, 2, dtype=torch.float32, device=x.device)   # one fill for the whole MLP
    k = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, torch.nn.Linear):
            fuse = i + 1 < len(mods) and isinstance(mods[i + 1], torch.nn.ReLU)
            x, amax = linear(x, m.weight, m.bias, fuse, x_amax=amax, return_amax=True, bf16=bf16, amax_buf=bufs[k])
            k += 1
            i += 2 if fuse else 1
        else:
            x = m(x)
            amax = None
            i += 1
    return (x, amax) if return_amax else x


class RangeRows:
    """Range-row plumbing of one fused sum / mean layer (csrc/ranges.hip; Csr.ensure_ranges): the
    super nodes of a stiffened batch (VirtualEdgeCreate.py:81-113) aggregate their graph's whole
    contiguous real-node range, so
      forward   the previous layer's bgnn_sage_apply also writes the range sums S of x_next as R
                extra rows after it ([N + R, H], x_full); this layer's GEMM runs on all N + R rows,
                and z_l's extra rows (S W_l^T = the summed z_l rows) are the range rows' aggregates
                (bgnn_sage_fwd heavy_agg) -- no chunk pass over the real rows;
      backward  bgnn_sage_bwd_rows also sums dh over each transposed range row's targets, and
                bgnn_range_sums_finish writes those dz_l rows (bgnn_spmm_bwd heavy_done).
    x_full / x_amax: the input's [N + R, H] buffer and a device scalar >= its max |.| (the GEMM's A
    scale), or None; out: write the range sums of x_next into `out_amax`'s layer buffer, appended
    to `holder`; bwd: the backward takes the range path."""
    __slots__ = ("x_full", "x_amax", "out", "out_amax", "bwd", "holder")

    def __init__(self, x_full=None, x_amax=None, out=False, out_amax=None, bwd=True):
        self.x_full, self.x_amax, self.out, self.out_amax, self.bwd = x_full, x_amax, out, out_amax, bwd
        self.holder = []


# range rows (RangeRows) for stiffened batches; False: the chunk + combine path for every heavy row
RANGE_ROWS = True


class LayerConfig:
    __slots__ = ("reduce", "bn", "training", "momentum", "eps", "skip", "p", "seed", "famax", "rng", "bf16")

    def __init__(self, reduce: int, bn: bool, training: bool, momentum: float, eps: float, skip: bool,
                 p: float, seed: int, *, dropout: bool = None, famax=None, rng=None, bf16: bool = False):
        self.reduce = reduce
        self.bn = bn
        # `training` selects the BatchNorm batch statistics (a module that tracks no running
        # statistics uses them in eval mode too); `dropout` (default: training) whether the
        # dropout is active, which follows the module's mode alone
        self.training = training
        self.momentum = momentum
        self.eps = eps
        self.skip = skip
        self.p = p if (training if dropout is None else dropout) else 0.0
        self.seed = seed
        # folded layer: 5 zeroed device slots for the maxima of the weight-product operands
        # (max|Wcat|, max|W_in|, max|b_in|, max|dWf|, max|dbf|), so those small f16x3 GEMMs need no
        # max pass (and no zero fill) of their own
        self.famax = famax
        self.rng = rng      # RangeRows (range rows of a stiffened batch) or None
        # layer with autocast's rounding points (sage_layer bf16=True): bf16 operands in the N-row
        # products, z (max: [agg | x] and y) stored bf16, everything else f32
        self.bf16 = bf16


_E_ARG = 1001   # BGNN_E_ARG (include/bgnn.h)


def _glue_fwd(o, bn_part, slots, x_prev, gamma, beta, running_mean, running_var, cfg: LayerConfig, next_amax,
              graph: Graph = None, pool=None, need_x: bool = True):
    """The layer glue after the normalised SAGE output o (Models/BuckGNN.py:436-444): BatchNorm
    finalize (train: batch statistics from the aggregation's partial sums, running stats updated;
    eval: running stats), then x_next = drop(relu(o * scale + shift) + skip * x_prev) with
    max|x_next| folded into next_amax. Returns (x_next, (scale, shift, mean, invstd), pooled) (None
    coefficients without BN). pool (a SegmentIndex): the mean pool of x_next per segment comes out of
    the same pass (pooled; None when the layer took the plain apply, and the caller pools x_next),
    and with need_x False x_next is then neither written nor returned (None).

    The BatchNorm partials here are the UNSHIFTED f32 per-block sums of o and o^2 from the
    aggregation epilogue, reduced in fp64 (the per-module BatchNorm1d shifts by the first row,
    bgnn_bn_finalize_shifted, because its input can have |mean| >> std). o is L2-normalised per row,
    so sum_c E[o_c^2] = 1 and each channel's E[o_c^2] <= 1: the E[o^2] - E[o]^2 cancellation costs
    at most the f32 rounding of a block's ~80-row sum, <= 80 * 2^-24 * E[o_c^2] <= 5e-6 * E[o_c^2]
    (typically 1e-8 at h = 512, E[o_c^2] ~ 1/512), next to BatchNorm's eps = 1e-5 in var + eps.
    The shift would need o's first row before the kernel that produces it; the full-size tests
    bound the running statistics against fp64 at rtol 1e-5 (tests/test_gpu_fullsize.py)."""
    N, H = o.shape
    dev = o.device
    s = _stream()
    scale = shift = mean = invstd = None
    if cfg.bn:
        scale = torch.empty(H, dtype=torch.float32, device=dev)
        shift = torch.empty(H, dtype=torch.float32, device=dev)
        mean = torch.empty(H, dtype=torch.float32, device=dev)
        invstd = torch.empty(H, dtype=torch.float32, device=dev)
        if cfg.training:
            _lib.call("bgnn_bn_finalize", bn_part.data_ptr(), slots, H, N, _ptr(gamma), _ptr(beta), cfg.eps,
                      cfg.momentum, _ptr(running_mean), _ptr(running_var), mean.data_ptr(), invstd.data_ptr(),
                      scale.data_ptr(), shift.data_ptr(), s)
        else:
            _lib.call("bgnn_bn_eval_coeffs", H, _ptr(gamma), _ptr(beta), cfg.eps, running_mean.data_ptr(),
                      running_var.data_ptr(), scale.data_ptr(), shift.data_ptr(), s)
            mean.copy_(running_mean)
            invstd.copy_(torch.rsqrt(running_var + cfg.eps))
    rng = cfg.rng
    if rng is not None and rng.out:
        # x_next and the next layer's range sums S in one [N + R, H] buffer (RangeRows)
        R = graph.fwd.plan.n_heavy
        full = torch.empty(N + R, H, dtype=torch.float32, device=dev)
        x_next = full[:N]
        rp = torch.empty(_lib.query("bgnn_range_partial_bytes", N, H) // 4, dtype=torch.float32, device=dev)
        _lib.call("bgnn_sage_apply", o.data_ptr(), _ptr(scale), _ptr(shift), x_prev.data_ptr(), int(cfg.skip),
                  float(cfg.p), cfg.seed, N, H, x_next.data_ptr(), next_amax.data_ptr(), graph.fwd.ranges.data_ptr(),
                  rp.data_ptr(), s)
        _lib.call("bgnn_range_sums_finish", rp.data_ptr(), N, H, graph.fwd.ref(), 0, full[N:].data_ptr(), H,
                  next_amax.data_ptr(), rng.out_amax.data_ptr(), s)
        rng.holder.append(full)
        return x_next, (scale, shift, mean, invstd), None
    if pool is not None and N > 0 and pool.n == N:
        # the segment pool of x_next summed by the apply pass itself (bgnn_sage_apply_pool): x_next
        # is not read back, and not written at all when nothing else reads it (need_x False)
        x_next = torch.empty(N, H, dtype=torch.float32, device=dev) if need_x else None
        pooled = torch.empty(pool.num_rows, H, dtype=torch.float32, device=dev)
        nch = pool.fwd.plan.n_chunks
        part = torch.empty(nch * H, dtype=torch.float32, device=dev) if nch else None
        try:
            _lib.call("bgnn_sage_apply_pool", o.data_ptr(), _ptr(scale), _ptr(shift), x_prev.data_ptr(),
                      int(cfg.skip), float(cfg.p), cfg.seed, N, H, _ptr(x_next),
                      next_amax.data_ptr() if need_x else None,   # (the scale of a GEMM that reads x_next)
                      pool.fwd.ref(), 1, _ptr(part), pooled.data_ptr(), s)
            return x_next, (scale, shift, mean, invstd), pooled
        except _lib.BgnnError as e:
            if e.code != _E_ARG:   # an unsupported shape takes the two-kernel path below
                raise
    x_next = torch.empty(N, H, dtype=torch.float32, device=dev)
    _lib.call("bgnn_sage_apply", o.data_ptr(), _ptr(scale), _ptr(shift), x_prev.data_ptr(), int(cfg.skip),
              float(cfg.p), cfg.seed, N, H, x_next.data_ptr(), next_amax.data_ptr(), None, None, s)
    return x_next, (scale, shift, mean, invstd), None


def _glue_bwd_stats(g, o, scale, shift, mean, invstd, cfg: LayerConfig, g_rows=None):
    """BatchNorm backward statistics of the layer glue (bgnn_sage_bwd_stats + one slot reduce):
    (dgamma, dbeta, sum_g2, sum_g2xhat) -- all None without BN; eval mode uses zero sums.
    g_rows (int64 [N] or None): row r's gradient is row g_rows[r] of g (the pooled gradient)."""
    if not cfg.bn:
        return None, None, None, None
    N, H = o.shape
    dev = o.device
    rs = _lib.query("bgnn_rows_slots", N)
    part2 = torch.empty(rs, 2, H, dtype=torch.float32, device=dev)
    _lib.call("bgnn_sage_bwd_stats", g.data_ptr(), _ptr(g_rows), o.data_ptr(), scale.data_ptr(), shift.data_ptr(),
              mean.data_ptr(), invstd.data_ptr(), float(cfg.p), cfg.seed, N, H, part2.data_ptr(), _stream())
    sums = torch.empty(2, H, dtype=torch.float32, device=dev)
    reduce_partials(part2, rs, H, sums[0], sums[1])
    dbeta, dgamma = sums[0], sums[1]
    if cfg.training:
        return dgamma, dbeta, sums[0], sums[1]
    z = torch.zeros(H, dtype=torch.float32, device=dev)
    return dgamma, dbeta, z, z


def _fold_native_ok(famax, wcat, w_in, b_in) -> bool:
    """The folded layer's weight products take the grouped native launches (FOLD_NATIVE): the hip
    backend with its fold_amax slots, row-major operands, and a shape whose five products the GEMM
    planner puts on the tile csrc/fold.hip regroups."""
    return bool(FOLD_NATIVE and GEMM_BACKEND == "hip" and famax is not None and famax.is_contiguous()
                and famax.numel() >= 5 and wcat.stride(1) == 1 and w_in.stride(1) == 1 and b_in.is_contiguous()
                and _lib.query("bgnn_fold_weights_supported", wcat.size(1), w_in.size(1)))


def _fold_fwd(wcat, w_in, b_in, famax, w_amax):
    """The folded layer 0's weight chain: the encoder's last Linear folded into the transform
    (x = h W_in^T + b_in never materialised), z = x [W_l;W_r]^T = h Wf^T + bf with
    Wf = [W_l;W_r] W_in [2H, K_in] and bf = [W_l;W_r] b_in; max|Wf| is folded into w_amax.
    famax: LayerConfig.famax (slots 0..2: max|Wcat|, max|W_in|, max|b_in|) or None.
    Returns (wf, bf, wf_t): wf_t = Wf^T (the dgrad operand) from the native launch
    (bgnn_fold_weights_fwd), None from the bgnn_gemm chain."""
    H, K_in = w_in.shape
    dev = wcat.device
    if _fold_native_ok(famax, wcat, w_in, b_in):   # (folds max|Wf| in itself)
        wf = torch.empty(2 * H, K_in, dtype=torch.float32, device=dev)
        bf = torch.empty(2 * H, dtype=torch.float32, device=dev)
        wf_t = torch.empty(K_in, 2 * H, dtype=torch.float32, device=dev)
        _lib.call("bgnn_fold_weights_fwd", H, K_in, wcat.data_ptr(), wcat.stride(0), w_in.data_ptr(),
                  w_in.stride(0), b_in.data_ptr(), famax.data_ptr(), wf.data_ptr(), K_in, bf.data_ptr(),
                  wf_t.data_ptr(), 2 * H, w_amax.data_ptr(), _stream())
        return wf, bf, wf_t
    fa = (None, None, None)
    if famax is not None:   # the same maxima the GEMMs would compute, without their fills
        fa = (famax[0:1], famax[1:2], famax[2:3])
        absmax(wcat, fa[0], accumulate=True)
        absmax(w_in, fa[1], accumulate=True)
        absmax(b_in.view(1, -1), fa[2], accumulate=True)
    wf = gemm(wcat, w_in.contiguous(), trans_a=False, trans_b=False, a_amax=fa[0], b_amax=fa[1])
    # (bgnn GEMM, not torch.mv: rocBLAS's GEMV moved the BN-amplified gradients of the
    # Shared variant 50x further from fp64, tests/test_gpu_fold.py)
    bf = gemm(wcat, b_in.contiguous().view(H, 1), trans_a=False, trans_b=False, a_amax=fa[0],
              b_amax=fa[2]).view(-1)
    absmax(wf, w_amax, accumulate=True)
    return wf, bf, None


def _fold_bwd(dwf, db2, wcat, w_in, b_in, famax):
    """Backward of _fold_fwd from dWf = dz^T h [2H, K_in] (max|dWf| in famax[3]) and dbf = db2
    viewed flat ([Σ dz_l ; Σ dh]): dWcat = dWf W_in^T + dbf b_in^T (= dz^T x) [2H, H],
    dW_in = Wcat^T dWf [H, K_in], db_in = Wcat^T dbf [H], on bgnn_fold_weights_bwd or the
    bgnn_gemm chain. Returns (dWcat, dW_in, db_in)."""
    H, K_in = w_in.shape
    dev = dwf.device
    dbf = db2.view(-1)
    if _fold_native_ok(famax, wcat, w_in, b_in) and dwf.stride(1) == 1:   # (folds max|dbf| in itself)
        dw = torch.empty(2 * H, H, dtype=torch.float32, device=dev)
        dw_in = torch.empty(H, K_in, dtype=torch.float32, device=dev)
        db_in = torch.empty(H, dtype=torch.float32, device=dev)
        ws_bytes = _lib.query("bgnn_fold_weights_ws_bytes", H, K_in)
        ws = _workspace(ws_bytes, dev)
        _lib.call("bgnn_fold_weights_bwd", H, K_in, dwf.data_ptr(), dwf.stride(0), dbf.data_ptr(),
                  wcat.data_ptr(), wcat.stride(0), w_in.data_ptr(), w_in.stride(0), b_in.data_ptr(),
                  famax.data_ptr(), dw.data_ptr(), H, dw_in.data_ptr(), K_in, db_in.data_ptr(), _ptr(ws),
                  ws_bytes, _stream())
        return dw, dw_in, db_in
    a_wcat = a_win = a_dwf = a_dbf = None
    if famax is not None:
        a_wcat, a_win, a_dwf, a_dbf = famax[0:1], famax[1:2], famax[3:4], famax[4:5]
        absmax(db2, a_dbf, accumulate=True)
    dw = gemm(dwf, w_in.contiguous(), trans_a=False, trans_b=True, a_amax=a_dwf, b_amax=a_win)
    dw.add_(torch.outer(dbf, b_in))
    dw_in = gemm(wcat, dwf, trans_a=True, trans_b=False, a_amax=a_wcat, b_amax=a_dwf)
    db_in = gemm(wcat, dbf.view(-1, 1), trans_a=True, trans_b=False, a_amax=a_wcat, b_amax=a_dbf).view(-1)
    return dw, dw_in, db_in


def _gemm_w(a, img, bn: int, N: int, a_amax, b_amax, g=None, ldg: int = 0, p: float = 0.0, seed: int = 0,
            timer: str = None):
    """C = a W^T [M, N] with W given as its pre-split image (WPrep img_f / img_d with column tile
    bn; bgnn_gemm_f32_w, bit-identical to gemm on the f32 W); g (ld ldg): drop_p(g) added in the
    epilogue, as _gemm_dropadd does. timer: the TIMERS key of the launch (the launchers that take
    one bracket the launch alone, not their allocations and queries)."""
    M, K = a.shape
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    with _timed(timer):
        _lib.call("bgnn_gemm_f32_w", M, N, K, a.data_ptr(), a.stride(0), img.data_ptr(), bn, out.data_ptr(), N, None,
                  0, a_amax.data_ptr(), b_amax.data_ptr(), None, _ptr(g), ldg, float(p), seed, _stream())
    return out


def _gemm_dropadd(a, bt, a_amax, b_amax, g, p: float, seed: int, timer: str = None):
    """C = a bt^T + drop_p(g) [M, N]: the skip connection's incoming gradient g added through the
    layer's counter-based dropout mask in the GEMM epilogue (bgnn_gemm_f32_dropadd)."""
    M, K = a.shape
    N = bt.size(0)
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    ws, ws_bytes = gemm_workspace(M, N, K, 0, 1, 0, a.device)
    with _timed(timer):
        _lib.call("bgnn_gemm_f32_dropadd", 0, 1, M, N, K, a.data_ptr(), a.stride(0), bt.data_ptr(), bt.stride(0),
                  out.data_ptr(), out.stride(0), a_amax.data_ptr(), b_amax.data_ptr(), g.data_ptr(), g.stride(0),
                  float(p), seed, _ptr(ws), ws_bytes, _stream())
    return out


def _sage_rows_fwd(csr, zl, zr, bias, H: int, reduce: int, bn_stats: bool = True, heavy_agg=None,
                   timer: str = None):
    """The SAGE row epilogue over csr: o_i = normalize(AGG_{j->i} z_l[j] + z_r[i] + bias), its row
    norms and the per-slot BatchNorm partial sums of o.
    f32 (bgnn_sage_fwd): zl / zr address the [*, H] halves of z by data pointer and row stride (an
    interleaved z itself serves as zl); bias a tensor; heavy_agg: the heavy rows' aggregates
    ([n_heavy, *] rows, RangeRows) instead of their chunk pass.
    bf16 (bgnn_sage_fwd_bf16; zl a bfloat16 [*, 2H] = [z_l | z_r], zr None): bias may be None, and
    the partial sums are written only with bn_stats (the f32 kernel always writes them).
    Returns (o, nrm, bn_part, slots)."""
    N = csr.n_rows
    dev = zl.device
    b16 = zl.dtype == torch.bfloat16
    o = torch.empty(N, H, dtype=torch.float32, device=dev)
    nrm = torch.empty(N, dtype=torch.float32, device=dev)
    slots = _lib.query("bgnn_sage_fwd_bf16_slots" if b16 else "bgnn_sage_fwd_slots", csr.ref())
    bn_part = torch.empty(slots, 2, H, dtype=torch.float32, device=dev)
    part = torch.empty(csr.plan.n_chunks * H, dtype=torch.float32, device=dev) if csr.plan.n_chunks else None
    with _timed(timer):
        if b16:
            _lib.call("bgnn_sage_fwd_bf16", csr.ref(), zl.data_ptr(), zl.stride(0), _ptr(bias), H, reduce,
                      o.data_ptr(), nrm.data_ptr(), bn_part.data_ptr() if bn_stats else None, _ptr(part), _stream())
        else:
            _lib.call("bgnn_sage_fwd", csr.ref(), zl.data_ptr(), zl.stride(0), zr.data_ptr(), zr.stride(0),
                      bias.data_ptr(), H, reduce, o.data_ptr(), nrm.data_ptr(), bn_part.data_ptr(), _ptr(part),
                      _ptr(heavy_agg), heavy_agg.stride(0) if heavy_agg is not None else 0, _stream())
    return o, nrm, bn_part, slots


def _sage_rows_bwd(g, g_rows, o, nrm, gamma, coeffs, sums, cfg: LayerConfig, dh, dz_amax, gskip=None,
                   graph: Graph = None, folded: bool = False, range_dzl=None):
    """The backward row pass (bgnn_sage_bwd_rows): dropout, skip, ReLU, BatchNorm and normalize
    backward of every row, dh written into `dh` ([N, H], any row stride), max|dh| folded into
    dz_amax; gskip ([N, H] or None): also write the skip gradient drop(g) there.
    coeffs = (scale, shift, mean, invstd) and sums = (sum_g2, sum_g2xhat) from the forward glue and
    _glue_bwd_stats (ignored without BatchNorm); g_rows: see _glue_bwd_stats.
    folded (needs graph): the pass also sums dz_l = A^T dh per column from the in-degrees.
    range_dzl (needs graph; RangeRows): the pass sums dh over each transposed range row's targets
    and bgnn_range_sums_finish writes those dz_l rows into range_dzl.
    Returns db2: [1, H] = Σ dh (db_l), or folded [2, H] = [Σ dz_l ; Σ dh], which flat is dbf."""
    N, H = o.shape
    dev = o.device
    s = _stream()
    scale, shift, mean, invstd = coeffs if cfg.bn else (None,) * 4
    rs = _lib.query("bgnn_rows_slots", N)
    part_db = torch.empty(rs, 2, H, dtype=torch.float32, device=dev)
    bw = graph.bwd if range_dzl is not None else None
    rp = (torch.empty(_lib.query("bgnn_range_partial_bytes", N, H) // 4, dtype=torch.float32, device=dev)
          if bw is not None else None)
    _lib.call("bgnn_sage_bwd_rows", g.data_ptr(), _ptr(g_rows), o.data_ptr(), nrm.data_ptr(), _ptr(scale),
              _ptr(shift), _ptr(gamma) if (cfg.bn and gamma.numel()) else None, _ptr(mean), _ptr(invstd),
              _ptr(sums[0]), _ptr(sums[1]), float(cfg.p), cfg.seed, int(gskip is not None), N, H, dh.data_ptr(),
              dh.stride(0), _ptr(gskip), part_db.data_ptr(), dz_amax.data_ptr(),
              graph.fwd.rowptr.data_ptr() if folded else None, (2 if cfg.reduce == 1 else 1) if folded else 0,
              _ptr(bw.ranges) if bw is not None else None,
              graph.fwd.rowptr.data_ptr() if (bw is not None and cfg.reduce == 1) else None, _ptr(rp), s)
    if bw is not None:   # the super nodes' dz_l rows (and their max |.| into dz_amax)
        _lib.call("bgnn_range_sums_finish", rp.data_ptr(), N, H, bw.ref(), 1, range_dzl.data_ptr(),
                  range_dzl.stride(0), None, dz_amax.data_ptr(), s)
    db2 = torch.empty(2 if folded else 1, H, dtype=torch.float32, device=dev)
    reduce_partials(part_db, rs, H, db2[-1], db2[0] if folded else None)
    return db2


def _pool_grad(g, g_pool, seg, skip: bool):
    """The gradient of a layer whose mean pool was an output (SageLayerFn pool): (g, g_rows) with
    the pooled gradient / count (bgnn.ops._SegmentReduce.backward) either read through the batch
    vector (g_rows: row r's gradient is row g_rows[r] of g) or, where x_next has a gradient of its
    own or the skip reads g by row, broadcast and added."""
    if g_pool is None:
        return g, None
    # one launch with the bits of g_pool / seg.fwd.degree().clamp_min(1).to(float32).unsqueeze(1)
    gpc = g_pool.contiguous()
    gp = torch.empty_like(gpc)
    _lib.call("bgnn_pool_grad_scale", gpc.data_ptr(), seg.fwd.rowptr.data_ptr(), gpc.size(0), gpc.size(1),
              gp.data_ptr(), _stream())
    if g is None and not skip:
        return gp, seg.index
    gb = gp.index_select(0, seg.index)
    return (gb if g is None else g + gb), None


def _sage_transform(x_prev, x_amax, wmat, bf, w_amax, cfg: LayerConfig, img, folded: bool):
    """Step 1 of the layer, z = x_prev wmat^T (+ bf): returns (zl, zr, heavy_agg) as
    _sage_rows_fwd takes them. The layout of z is decided here: bf16 [N, 2H] (cfg.bf16), two dense
    [N, H] planes (Z_PLANES), else interleaved [M, 2H] -- with range rows (RangeRows) x_prev is the
    head of an [N + R, H] buffer whose last R rows are the range sums of x_prev, the GEMM runs on
    all M = N + R rows and z_l's extra rows are the range rows' aggregates (heavy_agg).
    img: the layer's WPrep with a pre-split [W_l;W_r] image, or None."""
    N = x_prev.size(0)
    H = wmat.size(0) // 2
    # (the folded layer's transform has K = K_in, not H: timed under its own name so the
    # bench's flops per launch are right for every launch it averages)
    name = "gemm_fwd_fold" if folded else "gemm_fwd"
    if cfg.bf16:   # operands rounded to bf16 in-tile, z stored bf16 (bgnn_gemm_bf16 storage 4)
        with _timed(name):
            return gemm_bf16(x_prev, wmat, trans_a=False, trans_b=True, out_bf16=True), None, None
    if Z_PLANES and H % PLANE_TILE == 0 and not folded:
        z = torch.empty(2, N, H, dtype=torch.float32, device=x_prev.device)
        with _timed(name):
            gemm(x_prev, wmat, trans_a=False, trans_b=True, out=Planes(z), a_amax=x_amax, b_amax=w_amax)
        return z[0], z[1], None
    rng = cfg.rng
    xa, a_amax = x_prev, x_amax
    full = rng is not None and rng.x_full is not None and not folded
    if full:
        if rng.x_full.data_ptr() != x_prev.data_ptr():
            raise RuntimeError("sage_layer: RangeRows.x_full must start at x_prev")
        xa, a_amax = rng.x_full, rng.x_amax
    pre = img is not None and not folded and _lib.query("bgnn_gemm_w_tile", xa.size(0), 2 * H, H) == img.bn_f
    with _timed(name):
        if pre:
            z = _gemm_w(xa, img.img_f, img.bn_f, 2 * H, a_amax, w_amax)
        else:
            z = gemm(xa, wmat, trans_a=False, trans_b=True, bias=bf, a_amax=a_amax, b_amax=w_amax)
    return z, z[:, H:], (z[N:] if full else None)   # (z addresses its left half as it is)


def _sage_dgrad(dz, wcat_t, dz_amax, w_amax, g, cfg: LayerConfig, dropadd: bool, gskip, img):
    """dx = dz [W_l;W_r] plus the skip gradient: drop(g) added in the GEMM's epilogue (dropadd), or
    accumulated onto the gskip the row pass wrote. wcat_t = [W_l;W_r]^T, so that the GEMM reads its
    B operand K-contiguous; img: the layer's WPrep with a pre-split image of it, or None."""
    N, H = dz.size(0), wcat_t.size(0)
    pre = (img is not None and (dropadd or gskip is None)
           and _lib.query("bgnn_gemm_w_tile", N, H, 2 * H) == img.bn_d)
    if pre:
        return _gemm_w(dz, img.img_d, img.bn_d, H, dz_amax, w_amax, g if dropadd else None, H,
                       cfg.p if dropadd else 0.0, cfg.seed if dropadd else 0, timer="gemm_dgrad")
    if dropadd:
        return _gemm_dropadd(dz, wcat_t, dz_amax, w_amax, g, cfg.p, cfg.seed, timer="gemm_dgrad")
    with _timed("gemm_dgrad"):
        return gemm(dz, wcat_t, trans_a=False, trans_b=True, out=gskip, beta=1.0, a_amax=dz_amax, b_amax=w_amax,
                    bf16=cfg.bf16)


class SageLayerFn(torch.autograd.Function):
    """Outputs (x_next, max|x_next|): the second output (non-differentiable) is the f16x3 GEMM
    operand scale of the next layer, folded in by bgnn_sage_apply at no extra pass.
    wprep: the layer's WPrep (prepare_weights) or None.
    pool (a SegmentIndex, the batch vector's segments): a third output, the mean pool of x_next
    per segment (global_mean_pool, Models/BuckGNN.py:246-249; the same segment kernel as
    bgnn.ops.segment_reduce). Its gradient reaches the backward row passes as the pooled
    gradient / count read through the batch vector (g_rows), not as a materialised [N, H]
    broadcast (the pool's index_select) read twice -- the same g values, so the same bits."""

    @staticmethod
    def forward(ctx, x_prev, x_amax, w_l, b_l, w_r, gamma, beta, running_mean, running_var, graph: Graph,
                cfg: LayerConfig, amax=None, w_in=None, b_in=None, wprep=None, pool=None, need_x: bool = True):
        dev = x_prev.device
        x_prev = x_prev.contiguous()
        H = w_l.size(0)
        folded = w_in is not None
        if folded and cfg.skip:
            raise ValueError("sage_layer: a folded input transform needs a layer without skip")
        # operand maxima: [0] = max|W|, [1] = max|x_next| (this layer's output), [2] = max|dz|
        # (zeroed; the layer loop passes one slice of a single per-step fill)
        if amax is None:
            amax = torch.zeros(3, dtype=torch.float32, device=dev)
        w_amax, next_amax, dz_amax = amax[0:1], amax[1:2], amax[2:3]
        # [W_l;W_r] [2H, H]: from prepare_weights (all layers in a few launches; the amax slot then
        # already holds max|W|) or built here. A folded layer (K = K_in) transforms by Wf instead.
        wcat = wprep.wcat if wprep is not None else torch.cat([w_l, w_r], 0).contiguous()
        wmat, bf, wf_t = wcat, None, None
        if folded:
            wmat, bf, wf_t = _fold_fwd(wcat, w_in, b_in, cfg.famax, w_amax)
        elif wprep is None and not cfg.bf16:
            absmax(wcat, w_amax, accumulate=True)
        if x_amax is None:   # (the bf16 products take no operand scale: a placeholder for the saved list)
            x_amax = torch.empty(0, dtype=torch.float32, device=dev) if cfg.bf16 else absmax(x_prev)
        # transform, rows, glue
        zl, zr, hagg = _sage_transform(x_prev, x_amax, wmat, bf, w_amax, cfg,
                                       wprep if (wprep is not None and wprep.img_f is not None) else None, folded)
        # (bf16: batch statistics only where _glue_fwd reads them)
        o, nrm, bn_part, slots = _sage_rows_fwd(graph.fwd, zl, zr, b_l, H, cfg.reduce, cfg.bn and cfg.training, hagg,
                                                timer="sage_fwd")
        del zl, zr, hagg
        x_next, coeffs, pooled = _glue_fwd(o, bn_part, slots, x_prev, gamma, beta, running_mean, running_var, cfg,
                                           next_amax, graph, pool, need_x)
        ctx.graph = graph
        ctx.cfg = cfg
        ctx.wcat_t = wprep.wcat_t if wprep is not None else None
        ctx.img_d = wprep if (wprep is not None and wprep.img_d is not None and not folded) else None
        ctx.set_materialize_grads(False)   # the amax output never gets a gradient: no zero fill for it
        ctx.fold = (w_in, b_in, wmat, wf_t) if folded else None
        ctx.save_for_backward(x_prev, o, nrm, wcat, _saved(gamma, dev), *(_saved(c, dev) for c in coeffs),
                              x_amax, w_amax, dz_amax)
        ctx.mark_non_differentiable(next_amax)
        ctx.pool = pool
        if pool is not None:
            if pooled is None:   # (the plain apply ran: range sums on this layer, or an unsupported shape)
                from .ops import spmm_fwd
                pooled, _ = spmm_fwd(pool.fwd, x_next, 1, pool.num_rows)
            return (x_next if need_x else None), next_amax, pooled
        return x_next, next_amax

    @staticmethod
    def backward(ctx, g, _g_amax, g_pool=None):
        cfg: LayerConfig = ctx.cfg
        g, g_rows = _pool_grad(g, g_pool, ctx.pool, cfg.skip)
        if g is None:   # (materialize_grads off: the layer output did not reach the loss)
            return (None,) * 17
        x_prev, o, nrm, wcat, gamma, scale, shift, mean, invstd, x_amax, w_amax, dz_amax = ctx.saved_tensors
        graph: Graph = ctx.graph
        folded = ctx.fold is not None
        g = g.contiguous()
        N, H = o.shape
        dev = o.device
        b16 = cfg.bf16   # the N-row dgrad / wgrad on bf16 operands; the row passes and A^T stay f32
        # dz = [dz_l | dh] and what its layout allows: two dense [N, H] planes take the plain GEMMs
        # only; interleaved f32 rows also the drop-add epilogue (skip layers: the dgrad adds drop(g)
        # itself, so the row pass writes no [N, H] skip gradient), the range rows (RangeRows: the
        # transposed range rows' dz_l rows summed by the row pass) and the pre-split weight image
        # (the bf16 products have none of the three: their skip gradient takes the gskip route)
        if DZ_PLANES and H % PLANE_TILE == 0 and not b16:
            dzt = torch.empty(2, N, H, dtype=torch.float32, device=dev)
            dz, dzl, dh = Planes(dzt), dzt[0], dzt[1]
            dropadd, ranges, img_d = False, False, None
        else:
            dz = torch.empty(N, 2 * H, dtype=torch.float32, device=dev)
            dzl, dh = dz, dz[:, H:]   # (dz addresses its left half as it is)
            dropadd = (cfg.skip and DGRAD_DROPADD and GEMM_BACKEND == "hip" and not b16 and H % 4 == 0
                       and _lib.query("bgnn_get_tuning", 5) == 2)
            ranges = cfg.rng is not None and cfg.rng.bwd and graph.bwd.ranges is not None
            img_d = None if b16 else ctx.img_d
        gskip = torch.empty(N, H, dtype=torch.float32, device=dev) if (cfg.skip and not dropadd) else None
        # stats, rows, transpose aggregation dz_l = A^T dh (MEAN scales by the target's in-degree)
        dgamma, dbeta, sum_g2, sum_g2xhat = _glue_bwd_stats(g, o, scale, shift, mean, invstd, cfg, g_rows)
        db2 = _sage_rows_bwd(g, g_rows, o, nrm, gamma, (scale, shift, mean, invstd), (sum_g2, sum_g2xhat), cfg, dh,
                             dz_amax, gskip, graph, folded, dzl if ranges else None)
        spmm_bwd_into(graph.bwd, graph.perm_t, graph.fwd.rowptr, dh, cfg.reduce, dzl, dz_amax, heavy_done=ranges,
                      timer=_timed("spmm_bwd"))
        has_affine = cfg.bn and gamma.numel() > 0
        dgamma, dbeta = (dgamma, dbeta) if has_affine else (None, None)
        if folded:
            # x = h W_in^T + b_in folded in: dh = dz Wf; dWf = dz^T h; dbf = column sums of dz (db2)
            w_in, b_in, wf, wf_t = ctx.fold
            with _timed("gemm_dgrad_fold"):
                dx = gemm(dz, wf_t if wf_t is not None else wf.t().contiguous(), trans_a=False, trans_b=True,
                          a_amax=dz_amax, b_amax=w_amax)
            with _timed("gemm_wgrad_fold"):
                dwf = gemm(dz, x_prev, trans_a=True, trans_b=False, a_amax=dz_amax, b_amax=x_amax,
                           c_amax=None if cfg.famax is None else cfg.famax[3:4])           # [2H, K_in]
            dw, dw_in, db_in = _fold_bwd(dwf, db2, wcat, w_in, b_in, cfg.famax)
            return (dx, None, dw[:H], db2[-1], dw[H:], dgamma, dbeta, None, None, None, None, None, dw_in, db_in,
                    None, None, None)
        # dgrad dx = dz · Wcat (+ skip gradient), wgrad dWcat = dz^T · x_prev [2H, H]
        wcat_t = ctx.wcat_t if ctx.wcat_t is not None else wcat.t().contiguous()
        dx = _sage_dgrad(dz, wcat_t, dz_amax, w_amax, g, cfg, dropadd, gskip, img_d)
        with _timed("gemm_wgrad"):
            dw = gemm(dz, x_prev, trans_a=True, trans_b=False, a_amax=dz_amax, b_amax=x_amax, bf16=b16)
        return (dx, None, dw[:H], db2[-1], dw[H:], dgamma, dbeta, None, None, None, None, None, None, None, None,
                None, None)


def _max_transform(x, w_l, w_r, graph: Graph, x_amax, w_amax, name: str):
    """Aggregate-first SAGEConv(aggr='max') transform (max is not linear, so the transform-first
    algebra of the sum / mean layers does not apply):
        agg = max_{j->i} x_j                 bgnn_spmm_fwd(MAX) with the per-element CSR argmax
        y   = [agg | x] [W_l | W_r]^T        one f16x3 GEMM, K = 2 C_in, [agg | x] read in place
    max|[agg | x]| = max|x| (every agg element is an x element or 0), so x's maximum scales A.
    Returns (y, agg, arg)."""
    from .ops import spmm_fwd
    N, C = x.shape
    with _timed("agg_max"):
        agg, arg = spmm_fwd(graph.fwd, x, 2, N, want_arg=True)
    wk = torch.cat([w_l, w_r], 1)                                    # [H, 2C]
    in_place = C % 32 == 0 and (x.data_ptr() - agg.data_ptr()) % 16 == 0
    a = Pair(agg, x) if in_place else torch.cat([agg, x], 1)
    with _timed(name):
        y = gemm(a, wk, trans_a=False, trans_b=True, a_amax=x_amax, b_amax=w_amax)
    return y, agg, arg


def _max_rows_fwd(y, b_l, H: int):
    """o = normalize(y + b_l), its row norms and the BatchNorm partial sums of o: bgnn_sage_fwd
    over a CSR without entries (graph.empty_csr), i.e. the SAGE row epilogue alone (the same
    arithmetic as the fused sum / mean layers' epilogue)."""
    from .graph import empty_csr
    bias = b_l if b_l is not None else torch.zeros(H, dtype=torch.float32, device=y.device)
    return _sage_rows_fwd(empty_csr(y.size(0), y.device), y, y, bias, H, 0)


def _max_transform_bf16(x, w_l, w_r, graph: Graph, name: str):
    """_max_transform with autocast's rounding points (sage_layer bf16=True, reduce 2):
        a = [bf16(agg) | bf16(x)]            bgnn_spmm_max_pack_bf16: the maximum and its argmax on the
                                             f32 rows (the state _max_transform's gather would write),
                                             rounded only where it is stored
        y = [bf16(agg) W_l^T | bf16(x) W_r^T]   two bf16 MFMA products, K = C_in, each stored as bf16
    The two terms are rounded apart, as autocast's two Linears round them (lin_l(agg) and lin_r(x) are
    bf16 tensors before they are added): one product over K = 2 C_in with one rounding has a smaller
    error of its own but another one than autocast's, and the prediction -- a few numbers behind a
    mean pool -- then lands anywhere from 0.2 to 3 times autocast's distance from fp64 (DESIGN.md
    section 3h). y is the [N, 2H] bf16 z of bgnn_sage_fwd_bf16, which adds its planes in f32 over
    the identity CSR (_max_rows_fwd_bf16).
    Returns (y, a, arg)."""
    from .ops import spmm_max_pack_bf16
    N = x.size(0)
    H, C = w_l.shape
    with _timed("agg_max"):
        a, arg = spmm_max_pack_bf16(graph.fwd, x, N)
    y = torch.empty(N, 2 * H, dtype=torch.bfloat16, device=x.device)
    with _timed(name):
        gemm_bf16(a[:, :C], w_l, trans_a=False, trans_b=True, out=y[:, :H])
        gemm_bf16(a[:, C:], w_r, trans_a=False, trans_b=True, out=y[:, H:])
    return y, a, arg


def _max_rows_fwd_bf16(y, b_l, H: int, bn_stats: bool):
    """_max_rows_fwd on the bf16 y = [y_l | y_r] of _max_transform_bf16: bgnn_sage_fwd_bf16 (sum)
    over the identity CSR, h_i = (y_l[i] + y_r[i]) + b in f32 (bn_stats: the BatchNorm partial
    sums, only where _glue_fwd reads them)."""
    from .graph import identity_csr
    N = y.size(0)
    if y.dtype != torch.bfloat16 or tuple(y.shape) != (N, 2 * H) or not y.is_contiguous():
        raise ValueError("_max_rows_fwd_bf16: y must be a contiguous [N, 2H] bfloat16 tensor")
    return _sage_rows_fwd(identity_csr(N, y.device), y, None, b_l, H, 0, bn_stats)


def _max_scatter(dagg, t, arg, graph: Graph):
    """dx = A_max^T dagg + t (bgnn_spmm_bwd_max, f32: the gradient of each (target, column) goes to
    its argmax edge's source, CSR-first on ties)."""
    dx = torch.empty(dagg.size(0), dagg.size(1), dtype=torch.float32, device=dagg.device)
    spmm_bwd_max_into(graph.bwd, graph.perm_t, graph.fwd.rowptr, dagg, arg, t, dx, timer=_timed("spmm_bwd"))
    return dx


def _max_backward_bf16(dh, wcat_t, a, arg, graph: Graph, gskip, need_dx: bool):
    """_max_backward with bf16 operands in the N-row products (f32 accumulation and results):
        [dagg | t] = dh [W_l | W_r]          one product; a skip layer takes two, dagg on its own and
                                             t accumulated into gskip = drop(g) (beta = 1)
        dx = A_max^T dagg + t                _max_scatter, on the f32 argmax
        [dW_l^T ; dW_r^T] = a^T dh           a = bf16 [agg | x], as the forward product read it
    wcat_t = [W_l ; W_r]^T ([C, 2H])."""
    H = dh.size(1)
    C = a.size(1) // 2
    dx = None
    if need_dx:
        with _timed("gemm_dgrad"):
            if gskip is None:
                wkt = torch.cat([wcat_t[:, :H], wcat_t[:, H:]], 0)      # [W_l^T ; W_r^T], [2C, H]
                dt = gemm(dh, wkt, trans_a=False, trans_b=True, bf16=True)
                dagg, t = dt[:, :C], dt[:, C:]
            else:
                dagg = gemm(dh, wcat_t[:, :H], trans_a=False, trans_b=True, bf16=True)
                t = gemm(dh, wcat_t[:, H:], trans_a=False, trans_b=True, out=gskip, beta=1.0, bf16=True)
        dx = _max_scatter(dagg, t, arg, graph)
    with _timed("gemm_wgrad"):
        dwt = gemm_bf16(a, dh, trans_a=True, trans_b=False)              # [2C, H]
    return dx, dwt[:C].t(), dwt[C:].t()


def _max_backward(dh, dz_amax, wcat_t, x, agg, arg, graph: Graph, x_amax, w_amax, addend_beta_src,
                  need_dx: bool, p: float = 0.0, seed: int = 0):
    """Backward of y = [agg | x] [W_l | W_r]^T with agg = max-aggregate(x), given dh = dL/dy:
        dagg = dh W_l, then dx = A_max^T dagg + (dh W_r [+ drop(g)])   (_max_scatter)
        dW_l = dh^T agg,  dW_r = dh^T x
    wcat_t = [W_l ; W_r]^T ([C, 2H]); addend_beta_src: the skip connection's incoming gradient g
    (added through its dropout mask in the dW_r product's epilogue) or None."""
    N, H = dh.shape
    C = x.size(1)
    g = addend_beta_src
    dx = None
    hip16 = GEMM_BACKEND == "hip" and _lib.query("bgnn_get_tuning", 5) == 2
    if need_dx and MAX_MERGED and hip16 and C % 256 == 0:
        # one GEMM [dagg | t] = dh [W_l | W_r] (B^T = [W_l^T ; W_r^T], [2C, H]), the skip layers'
        # drop(g) added to the t columns only (bgnn_gemm_f32_dropadd_cols): one launch at N = 2C
        # instead of two at N = C
        wkt = torch.cat([wcat_t[:, :H], wcat_t[:, H:]], 0)          # [W_l^T ; W_r^T]
        with _timed("gemm_dgrad"):
            if g is not None:
                dt = torch.empty(N, 2 * C, dtype=torch.float32, device=dh.device)
                ws, ws_bytes = gemm_workspace(N, 2 * C, H, 0, 1, 0, dh.device)
                _lib.call("bgnn_gemm_f32_dropadd_cols", N, 2 * C, H, dh.data_ptr(), dh.stride(0), wkt.data_ptr(), H,
                          dt.data_ptr(), 2 * C, dz_amax.data_ptr(), w_amax.data_ptr(), g.data_ptr(), g.stride(0), C,
                          float(p), seed, _ptr(ws), ws_bytes, _stream())
            else:
                dt = gemm(dh, wkt, trans_a=False, trans_b=True, a_amax=dz_amax, b_amax=w_amax)
        dx = _max_scatter(dt[:, :C], dt[:, C:], arg, graph)
        del dt
    elif need_dx:
        wl_t, wr_t = wcat_t[:, :H], wcat_t[:, H:]                    # W_l^T, W_r^T: [C, H], ld 2H
        with _timed("gemm_dgrad"):
            dagg = gemm(dh, wl_t, trans_a=False, trans_b=True, a_amax=dz_amax, b_amax=w_amax)
            if g is not None and hip16:
                t = _gemm_dropadd(dh, wr_t, dz_amax, w_amax, g, p, seed)
            else:
                t = gemm(dh, wr_t, trans_a=False, trans_b=True, a_amax=dz_amax, b_amax=w_amax)
                if g is not None:   # (torch GEMM backend / other GEMM modes: an explicit add)
                    t.add_(_dropped(g, p, seed))
        dx = _max_scatter(dagg, t, arg, graph)
    with _timed("gemm_wgrad"):
        if (MAX_MERGED and GEMM_BACKEND == "hip" and C % 256 == 0 and agg.shape == x.shape
                and agg.stride() == x.stride() and (x.data_ptr() - agg.data_ptr()) % 16 == 0):
            # [dW_l^T ; dW_r^T] = [agg | x]^T dh in one GEMM ([agg | x] read in place as two planes
            # of the M dimension; max|[agg | x]| = max|x|)
            dwt = gemm(Pair(agg, x), dh, trans_a=True, trans_b=False, a_amax=x_amax, b_amax=dz_amax)   # [2C, H]
            dw_l, dw_r = dwt[:C].t(), dwt[C:].t()
        else:
            dw_l = gemm(dh, agg, trans_a=True, trans_b=False, a_amax=dz_amax, b_amax=x_amax)
            dw_r = gemm(dh, x, trans_a=True, trans_b=False, a_amax=dz_amax, b_amax=x_amax)
    return dx, dw_l, dw_r


def _dropped(g, p: float, seed: int):
    """drop(g) with the layer's counter-based mask (bgnn_add_dropout with a zero addend): the skip
    gradient for the GEMM modes without the drop-add epilogue."""
    out = torch.empty_like(g)
    _lib.call("bgnn_add_dropout", g.data_ptr(), None, g.numel(), float(p), seed, out.data_ptr(), _stream())
    return out


class SageMaxLayerFn(torch.autograd.Function):
    """The fused layer of GraphSage_maxAggr (Models/BuckGNN.py:165-180,459-471): SAGEConv(aggr='max',
    normalize=True) -> BatchNorm -> ReLU -> skip -> Dropout, aggregate-first (_max_transform), then
    the same row epilogue and glue kernels as the sum / mean layers. Outputs (x_next, max|x_next|).
    wprep: the layer's WPrep (prepare_weights) or None."""

    @staticmethod
    def forward(ctx, x_prev, x_amax, w_l, b_l, w_r, gamma, beta, running_mean, running_var, graph: Graph,
                cfg: LayerConfig, amax=None, wprep=None):
        dev = x_prev.device
        x_prev = x_prev.contiguous()
        H = w_l.size(0)
        if amax is None:
            amax = torch.zeros(3, dtype=torch.float32, device=dev)
        w_amax, next_amax, dz_amax = amax[0:1], amax[1:2], amax[2:3]
        if wprep is not None:   # (prepare_weights has folded max|[W_l;W_r]| into the slot)
            wcat_t = wprep.wcat_t
        else:
            wcat_t = torch.cat([w_l, w_r], 0).t().contiguous()
            if not cfg.bf16:
                absmax(wcat_t, w_amax, accumulate=True)
        # transform, rows, glue
        if cfg.bf16:
            # autocast's rounding points: the bf16 products take no operand scale (a placeholder for
            # the saved list); `agg` is a = bf16 [agg | x], which also stands in for x_prev in the
            # weight gradient
            if x_amax is None:
                x_amax = torch.empty(0, dtype=torch.float32, device=dev)
            y, agg, arg = _max_transform_bf16(x_prev, w_l, w_r, graph, "gemm_fwd_max")
        else:
            if x_amax is None:
                x_amax = absmax(x_prev)
            y, agg, arg = _max_transform(x_prev, w_l, w_r, graph, x_amax, w_amax, "gemm_fwd_max")
        with _timed("sage_fwd"):
            o, nrm, bn_part, slots = (_max_rows_fwd_bf16(y, b_l, H, cfg.bn and cfg.training) if cfg.bf16
                                      else _max_rows_fwd(y, b_l, H))
        del y
        x_next, coeffs, _ = _glue_fwd(o, bn_part, slots, x_prev, gamma, beta, running_mean, running_var, cfg,
                                      next_amax)
        ctx.graph = graph
        ctx.cfg = cfg
        ctx.set_materialize_grads(False)
        # (bf16: a replaces both agg and x_prev in the products; the skip reads g, not x_prev)
        ctx.save_for_backward(_saved(None if cfg.bf16 else x_prev, dev), agg, arg, o, nrm, wcat_t, _saved(gamma, dev),
                              *(_saved(c, dev) for c in coeffs), x_amax, w_amax, dz_amax)
        ctx.mark_non_differentiable(next_amax)
        return x_next, next_amax

    @staticmethod
    def backward(ctx, g, _g_amax):
        if g is None:
            return (None,) * 13
        (x_prev, agg, arg, o, nrm, wcat_t, gamma, scale, shift, mean, invstd, x_amax, w_amax,
         dz_amax) = ctx.saved_tensors
        cfg: LayerConfig = ctx.cfg
        g = g.contiguous()
        N, H = o.shape
        dev = o.device
        dh = torch.empty(N, H, dtype=torch.float32, device=dev)
        # bf16: the products have no drop-add epilogue, so a skip layer's drop(g) is written by the
        # row pass (gskip) and the dh W_r product accumulates into it
        need_dx = ctx.needs_input_grad[0]
        gskip = (torch.empty(N, H, dtype=torch.float32, device=dev) if (cfg.bf16 and cfg.skip and need_dx)
                 else None)
        # stats, rows, then dgrad + transpose aggregation + wgrad
        dgamma, dbeta, sum_g2, sum_g2xhat = _glue_bwd_stats(g, o, scale, shift, mean, invstd, cfg)
        db2 = _sage_rows_bwd(g, None, o, nrm, gamma, (scale, shift, mean, invstd), (sum_g2, sum_g2xhat), cfg, dh,
                             dz_amax, gskip)
        if cfg.bf16:
            dx, dw_l, dw_r = _max_backward_bf16(dh, wcat_t, agg, arg, ctx.graph, gskip, need_dx)
        else:
            dx, dw_l, dw_r = _max_backward(dh, dz_amax, wcat_t, x_prev, agg, arg, ctx.graph, x_amax, w_amax,
                                           g if cfg.skip else None, need_dx, cfg.p, cfg.seed)
        has_affine = cfg.bn and gamma.numel() > 0
        return (dx, None, dw_l, db2[-1], dw_r, dgamma if has_affine else None, dbeta if has_affine else None,
                None, None, None, None, None, None)


def _weight_pack(pairs, L: int, H: int):
    """[L, 2H, H] / [L, H, 2H] buffers holding one layer loop's [W_l;W_r] (and its transpose),
    filled by one multi-tensor copy and one transpose on every call (~20 us of GPU time per
    step; a fresh torch.cat of the 2L weights each step blocked the host ~0.4 ms,
    tools/host_profile.py). Every call packs into NEW buffers, never into ones a live autograd
    graph may have saved, so a second forward before the first backward (two micro-batches, an
    eval forward in between) keeps the first graph's operands intact. (Round 4 reused the pack
    while the weights' data pointers and autograd versions were unchanged; round-4 ADVICE: a
    freed model's addresses can be handed to a new model with equal versions, and writes through
    p.data bump no version, so a reused pack could be stale. Refilling costs nothing measurable.)"""
    dev = pairs[0][0].device
    W = torch.empty(L, 2 * H, H, dtype=torch.float32, device=dev)
    Wt = torch.empty(L, H, 2 * H, dtype=torch.float32, device=dev)
    torch._foreach_copy_([W[i, k * H:(k + 1) * H] for i in range(L) for k in (0, 1)], [t for pr in pairs for t in pr])
    Wt.copy_(W.transpose(1, 2))
    return W, Wt


class WPrep:
    """One layer's prepared weight operands (prepare_weights): [W_l;W_r] [2H, H], its transpose
    [H, 2H] (dgrad B operand), and optionally their pre-split images (fwd: img_f with column tile
    bn_f; dgrad: img_d, bn_d) for bgnn_gemm_f32_w."""
    __slots__ = ("wcat", "wcat_t", "img_f", "bn_f", "img_d", "bn_d")

    def __init__(self, wcat, wcat_t, img_f=None, bn_f=0, img_d=None, bn_d=0):
        self.wcat, self.wcat_t = wcat, wcat_t
        self.img_f, self.bn_f, self.img_d, self.bn_d = img_f, bn_f, img_d, bn_d


def _wsplit_run(W, i, j, amax_bufs, M):
    """Pre-split images of W[i:j] ([n, N, K] fp32 contiguous, the B^T operands of C = A W^T with
    M rows) in one launch, each scaled by its layer's max|W| (amax_bufs[k, 0]); (images, bn) or
    (None, 0) when the shape has no pre-split path."""
    _, N, K = W.shape
    bn = _lib.query("bgnn_gemm_w_tile", M, N, K)
    if bn == 0:
        return None, 0
    nb = _lib.query("bgnn_gemm_wsplit_bytes", N, K)
    img = torch.empty(j - i, nb, dtype=torch.uint8, device=W.device)
    _lib.call("bgnn_gemm_wsplit", W[i].data_ptr(), j - i, W.stride(0), N, K, W.stride(1), amax_bufs[i].data_ptr(),
              amax_bufs.stride(0), img.data_ptr(), nb, bn, _stream())
    return img, bn


def _runs(flags):
    """(i, j) of every maximal run flags[i:j] of consecutive true values."""
    i, L = 0, len(flags)
    while i < L:
        j = i
        while j < L and flags[j]:
            j += 1
        if j > i:
            yield i, j
        i = j + 1


def prepare_weights(pairs, amax_bufs: torch.Tensor, fill_amax, n_rows: int = 0):
    """[W_l;W_r] and its transpose for every layer of a loop in a few launches (one multi-tensor
    copy into a fresh pack, one transpose, one max|W| launch per run of layers that take it)
    instead of three launches per layer. pairs: [(w_l, w_r)] per layer; amax_bufs: the loop's
    zeroed [L, 3] operand-max slots, whose slot 0 receives max|[W_l;W_r]| for the layers where
    fill_amax[i] (a folded layer scales by max|Wf| instead). n_rows > 0: also the pre-split images
    for GEMMs of n_rows rows (WSPLIT). Returns a WPrep per layer (views of [L, ...] buffers)."""
    L = len(pairs)
    H = pairs[0][0].size(0)
    with torch.no_grad():   # operands only: the layers return the weight gradients themselves
        if PERSISTENT_WPACK and all(a.dtype == torch.float32 and b.dtype == torch.float32 and a.is_contiguous()
                                    and b.is_contiguous() and a.shape == (H, H) and b.shape == (H, H)
                                    for a, b in pairs):
            W, Wt = _weight_pack(pairs, L, H)
        else:
            W = torch.cat([t for pr in pairs for t in pr], 0).view(L, 2 * H, H)
            Wt = W.transpose(1, 2).contiguous()
        # max|W| per layer with bgnn_absmax (torch's dim=(1, 2) max-reduction took 128 us here),
        # one launch per run of consecutive layers that take it (the folded first layer does not)
        for i, j in _runs(fill_amax):
            if amax_bufs.is_contiguous() and H % 4 == 0:
                _lib.call("bgnn_absmax_items_f32", W[i].data_ptr(), j - i, 2 * H * H, 2 * H, H, H,
                          amax_bufs[i].data_ptr(), amax_bufs.stride(0), _stream())
            else:
                for k in range(i, j):
                    absmax(W[k], amax_bufs[k, 0:1], accumulate=True)
        out = [WPrep(W[i], Wt[i]) for i in range(L)]
        # pre-split images (after the maxima they are scaled by): the layers that scale by
        # max|[W_l;W_r]| (not a folded layer, whose transform is a per-step weight product)
        if (WSPLIT and n_rows > 0 and GEMM_BACKEND == "hip" and not Z_PLANES and not DZ_PLANES
                and amax_bufs.is_contiguous() and _lib.query("bgnn_get_tuning", 5) == 2):
            for i, j in _runs(fill_amax):
                img_f, bn_f = _wsplit_run(W, i, j, amax_bufs, n_rows)
                img_d, bn_d = _wsplit_run(Wt, i, j, amax_bufs, n_rows)
                for k in range(i, j):
                    o = out[k]
                    if img_f is not None:
                        o.img_f, o.bn_f = img_f[k - i], bn_f
                    if img_d is not None:
                        o.img_d, o.bn_d = img_d[k - i], bn_d
    return out


def sage_layer(x_prev: torch.Tensor, w_l: torch.Tensor, b_l: torch.Tensor, w_r: torch.Tensor,
               bn_module, graph: Graph, reduce: int, skip: bool, p: float, training: bool,
               seed: int, x_amax: torch.Tensor = None, return_amax: bool = False, amax_buf=None,
               w_in: torch.Tensor = None, b_in: torch.Tensor = None, wprep=None, count_batch: bool = True,
               fold_amax: torch.Tensor = None, rng: RangeRows = None, pool=None, need_x: bool = True,
               bf16: bool = False):
    """Run one fused layer. `bn_module` is a torch.nn.BatchNorm1d (or None for no BN).
    x_amax: optional device scalar >= max|x_prev| (the previous layer's second output), which
    spares the GEMM a pass over x_prev; return_amax: also return max|x_next|.
    w_in / b_in: fold a preceding Linear into this layer (x_prev is then that Linear's INPUT h,
    and the layer computes on x = h W_in^T + b_in without materialising x); only for a layer
    without skip connection (the reference's first SAGE layer after the node encoder).
    rng: the range-row plumbing of a stiffened batch (RangeRows; sum / mean only).
    pool: a SegmentIndex (sum / mean only): also return the mean pool of x_next per segment as the
    last element (SageLayerFn). need_x=False (with pool): the caller reads only the pool, so x_next
    is returned as None and, where the pooling apply pass runs, never written (nor is max|x_next|
    folded into the amax output then: it scales a GEMM that would read x_next).
    bf16 (H % 8 == 0): autocast's rounding points -- the operands of the layer's N-row
    products (transform, dgrad, wgrad) are rounded to bf16 and z = x [W_l;W_r]^T is stored as bf16
    (bgnn_gemm_bf16, bgnn_sage_fwd_bf16); accumulators, bias, normalize, BatchNorm, ReLU, skip,
    dropout, the stored x / o / dh and every gradient stay f32. Range rows, pre-split weight images
    and the operand maxima are not used then (rng is ignored), and w_in / b_in are refused.
    bf16 with reduce 2 (max): the layer stays aggregate-first -- the maximum and its argmax come from
    the f32 rows (bgnn_spmm_max_pack_bf16), [agg | x] and the two terms of y = agg W_l^T + x W_r^T are
    stored as bf16, the dgrad / wgrad products take bf16 operands (SageMaxLayerFn, _max_transform_bf16)."""
    require_cuda(x_prev, w_l, b_l, w_r, what="sage_layer")
    _require_f32(x_prev, "sage_layer")
    H = w_l.size(0)
    if w_in is None and x_prev.size(1) != H:
        raise ValueError(f"sage_layer: x has {x_prev.size(1)} features, the layer {H}")
    if H % 4 or H > 512:
        raise ValueError(f"sage_layer: fused path needs H % 4 == 0 and H <= 512 (got {H})")
    if reduce not in (0, 1, 2):
        raise ValueError("sage_layer: reduce must be 0 (sum), 1 (mean) or 2 (max)")
    if reduce == 2 and w_in is not None:
        raise ValueError("sage_layer: max aggregation needs its input rows (no folded input transform)")
    if reduce == 2 and pool is not None:
        raise ValueError("sage_layer: the fused mean pool is for sum / mean layers")
    if bf16 and H % 8:
        raise ValueError(f"sage_layer: bf16 needs H % 8 == 0 (got H {H})")
    if bf16 and w_in is not None:
        raise ValueError("sage_layer: bf16 takes no folded input transform (w_in): the folded Linear would join "
                         "the layer's bf16 product")
    bn = bn_module
    stats, momentum, eps = training, 0.0, 0.0
    if bn is not None:
        # the BatchNorm statistics follow `training or not track_running_stats`; dropout follows
        # `training` alone (LayerConfig dropout=)
        stats = training or not bn.track_running_stats
        momentum = bn.momentum
        if training and bn.track_running_stats:
            if count_batch:
                bn.num_batches_tracked.add_(1)
            if momentum is None:   # cumulative average (torch: 1 / num_batches_tracked after the increment;
                # with count_batch=False the caller has already incremented the counter)
                momentum = 1.0 / float(bn.num_batches_tracked.item())
        momentum = float(momentum or 0.0) if bn.track_running_stats else 0.0
        eps = float(bn.eps)
    cfg = LayerConfig(reduce, bn is not None, stats, momentum, eps, skip, p, seed, dropout=training,
                      famax=fold_amax if w_in is not None else None,
                      rng=rng if (reduce != 2 and not bf16) else None, bf16=bool(bf16))
    bn_args = (bn.weight, bn.bias, bn.running_mean, bn.running_var) if bn is not None else (None,) * 4
    if reduce == 2:
        out = SageMaxLayerFn.apply(x_prev, x_amax, w_l, b_l, w_r, *bn_args, graph, cfg, amax_buf, wprep)
    else:
        out = SageLayerFn.apply(x_prev, x_amax, w_l, b_l, w_r, *bn_args, graph, cfg, amax_buf, w_in, b_in, wprep,
                                pool, need_x)
    if pool is not None:
        return out if return_amax else (out[0], out[2])
    return out if return_amax else out[0]


class SageConvFn(torch.autograd.Function):
    """One SAGEConv(normalize=True, aggr in {add, sum, mean, max}) module on the hand-written path:
    the per-module form of SageLayerFn without the layer glue, for the PyG call surface
    (bgnn.nn.SAGEConv, i.e. the reference's unchanged Models/BuckGNN.py:434 under the shim,
    whose BatchNorm / ReLU / skip / Dropout stay torch modules).

        z = x [W_l;W_r]^T                 f16x3 MFMA GEMM (bgnn_gemm_f32_scaled)
        o = normalize(AGG z_l + z_r + b)  bgnn_sage_fwd (aggregation + bias + L2 normalize)

    backward: bgnn_l2norm_bwd (dh, bias-gradient partials, max|dh|), the transpose aggregation
    dz_l = A^T dh (bgnn_spmm_bwd) and the dgrad / wgrad GEMMs on [dz_l | dh].
    aggr='max' runs aggregate-first (_max_transform / _max_rows_fwd / _max_backward)."""

    @staticmethod
    def forward(ctx, x, w_l, b_l, w_r, graph: Graph, reduce: int):
        dev = x.device
        x = x.contiguous()
        N = x.size(0)
        H = w_l.size(0)
        wcat = torch.cat([w_l, w_r], 0).contiguous()            # [2H, C_in]
        amax = torch.zeros(2, dtype=torch.float32, device=dev)   # max|W|, max|x|
        w_amax, x_amax = amax[0:1], amax[1:2]
        absmax(wcat, w_amax, accumulate=True)
        absmax(x, x_amax, accumulate=True)
        ctx.graph = graph
        ctx.reduce = reduce
        ctx.has_bias = b_l is not None
        if reduce == 2:   # aggregate-first (max is not linear): SageMaxLayerFn's transform + row epilogue
            y, agg, arg = _max_transform(x, w_l, w_r, graph, x_amax, w_amax, "conv_gemm_fwd")
            with _timed("conv_sage_fwd"):
                o, nrm, _, _ = _max_rows_fwd(y, b_l, H)
            ctx.save_for_backward(x, o, nrm, wcat, x_amax, w_amax, agg, arg)
            return o
        with _timed("conv_gemm_fwd"):
            z = gemm(x, wcat, trans_a=False, trans_b=True, a_amax=x_amax, b_amax=w_amax)   # [N, 2H]
        bias = b_l if b_l is not None else torch.zeros(H, dtype=torch.float32, device=dev)
        # (the BN sums are unused here)
        o, nrm, _, _ = _sage_rows_fwd(graph.fwd, z, z[:, H:], bias, H, reduce, timer="conv_sage_fwd")
        ctx.save_for_backward(x, o, nrm, wcat, x_amax, w_amax)
        return o

    @staticmethod
    def backward(ctx, g):
        x, o, nrm, wcat, x_amax, w_amax = ctx.saved_tensors[:6]
        graph: Graph = ctx.graph
        g = g.contiguous()
        N, H = o.shape
        dev = o.device
        s = _stream()
        mx = ctx.reduce == 2
        # max aggregation: dh alone ([N, H]); sum / mean: dz = [dz_l | dh] for the K = 2H GEMMs
        dz = torch.empty(N, H if mx else 2 * H, dtype=torch.float32, device=dev)
        dh = dz if mx else dz[:, H:]
        rs = _lib.query("bgnn_rows_slots", N)
        part_db = torch.empty(rs, 2, H, dtype=torch.float32, device=dev)
        dz_amax = torch.zeros(1, dtype=torch.float32, device=dev)   # max|dz| (fresh: re-entrant backward)
        _lib.call("bgnn_l2norm_bwd", g.data_ptr(), o.data_ptr(), nrm.data_ptr(), N, H, dh.data_ptr(), dh.stride(0),
                  part_db.data_ptr(), dz_amax.data_ptr(), s)
        db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = torch.empty(H, dtype=torch.float32, device=dev)
            reduce_partials(part_db, rs, H, db)
        if mx:
            agg, arg = ctx.saved_tensors[6:]
            dx, dw_l, dw_r = _max_backward(dh, dz_amax, wcat.t().contiguous(), x, agg, arg, graph, x_amax, w_amax,
                                           None, ctx.needs_input_grad[0])
            return dx, dw_l, db, dw_r, None, None
        spmm_bwd_into(graph.bwd, graph.perm_t, graph.fwd.rowptr, dh, ctx.reduce, dz, dz_amax,
                      timer=_timed("conv_spmm_bwd"))
        dx = None
        if ctx.needs_input_grad[0]:
            with _timed("conv_gemm_dgrad"):
                dx = gemm(dz, wcat.t().contiguous(), trans_a=False, trans_b=True, a_amax=dz_amax, b_amax=w_amax)
        dw = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[3]:
            with _timed("conv_gemm_wgrad"):
                dw = gemm(dz, x, trans_a=True, trans_b=False, a_amax=dz_amax, b_amax=x_amax)   # [2H, C_in]
        return (dx, None if dw is None else dw[:H], db, None if dw is None else dw[H:], None, None)


def sage_conv(x: torch.Tensor, w_l: torch.Tensor, b_l, w_r: torch.Tensor, graph: Graph, reduce: int):
    """normalize(lin_l(AGG x) + lin_r(x)) of one SAGEConv module on the hand-written path
    (SageConvFn); reduce 0 = sum/add, 1 = mean, 2 = max (aggregate-first)."""
    require_cuda(x, w_l, w_r, what="sage_conv")
    _require_f32(x, "sage_conv")
    return SageConvFn.apply(x, w_l, b_l, w_r, graph, reduce)


# ---------------------------------------------------------------------------
# bf16 inference layer (BuckGNN.infer_bf16): eval mode only, no autograd.

def _cached_weights(conv, attr: str, dim: int) -> torch.Tensor:
    """cat([W_l, W_r], dim) of a SAGEConv as one contiguous bf16 matrix, built once per weight
    version and kept on the module under `attr`: rebuilt when either weight is written in place
    (`_version`) or replaced (storage / device)."""
    w_l, w_r = conv.lin_l.weight, conv.lin_r.weight
    key = (w_l._version, w_r._version, w_l.data_ptr(), w_r.data_ptr(), str(w_l.device))
    hit = getattr(conv, attr, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        wcat = torch.cat([w_l.detach(), w_r.detach()], dim).to(torch.bfloat16).contiguous()
    setattr(conv, attr, (key, wcat))
    return wcat


def _bf16_rows(t: torch.Tensor) -> torch.Tensor:
    """t as bf16 rows with unit column stride and an 8-element-aligned row stride (an f32 t is
    rounded once)."""
    t = t if t.dtype == torch.bfloat16 else t.to(torch.bfloat16)
    return t.contiguous() if (t.stride(1) != 1 or t.stride(0) % 8) else t


def infer_weights(conv) -> torch.Tensor:
    """[W_l ; W_r] of a SAGEConv as one bf16 [2H, H] matrix (the B^T operand of the layer's
    GEMM), cached per weight version on the module (_cached_weights)."""
    return _cached_weights(conv, "_bgnn_infer_wcat", 0)


def bn_eval_coeffs(bn):
    """(scale, shift) of an eval-mode BatchNorm1d from its running statistics
    (bgnn_bn_eval_coeffs): BN(o) = o * scale + shift."""
    H = bn.num_features
    dev = bn.running_mean.device
    scale = torch.empty(H, dtype=torch.float32, device=dev)
    shift = torch.empty(H, dtype=torch.float32, device=dev)
    _lib.call("bgnn_bn_eval_coeffs", H, _ptr(bn.weight), _ptr(bn.bias), float(bn.eps), bn.running_mean.data_ptr(),
              bn.running_var.data_ptr(), scale.data_ptr(), shift.data_ptr(), _stream())
    return scale, shift


@torch.no_grad()
def sage_infer_layer(x: torch.Tensor, w_cat: torch.Tensor, bias, bn_coeffs, graph: Graph, reduce: int,
                     x_prev=None, out_f32: bool = False) -> torch.Tensor:
    """One eval-mode GraphSAGE layer on bf16 rows, two launches:
        z = x [W_l ; W_r]^T                       bf16 in, bf16 out, one MFMA product (gemm_bf16)
        y = ReLU(BN(normalize(AGG z_l + z_r + b))) (+ x_prev)     bgnn_sage_infer_bf16
    x: [N, H] bfloat16 (a float32 x, the encoder's output, is rounded to bf16 once); w_cat: bf16
    [2H, H] (infer_weights); bias: f32 [H] or None; bn_coeffs: (scale, shift) f32 [H] or None;
    reduce: 0 sum, 1 mean; x_prev: the skip input [N, H] or None. Returns y [N, H] as bfloat16, or
    float32 with out_f32 (the last layer). No autograd."""
    require_cuda(x, w_cat, bias, x_prev, what="sage_infer_layer")
    N, H = x.size(0), w_cat.size(1)
    if w_cat.dtype != torch.bfloat16 or w_cat.size(0) != 2 * H or x.size(1) != H:
        raise ValueError("sage_infer_layer: w_cat must be bfloat16 [2H, H] and x [N, H]")
    if H % 8 or H > 512:
        raise ValueError(f"sage_infer_layer: needs H % 8 == 0 and H <= 512 (got {H})")
    if reduce not in (0, 1):
        raise ValueError("sage_infer_layer: reduce must be 0 (sum) or 1 (mean)")
    dev = x.device
    xb = _bf16_rows(x)
    with _timed("infer_gemm"):
        z = gemm_bf16(xb, w_cat, trans_a=False, trans_b=True, out_bf16=True)
    xp = _bf16_rows(x_prev) if x_prev is not None else None
    scale, shift = bn_coeffs if bn_coeffs is not None else (None, None)
    out = torch.empty(N, H, dtype=torch.float32 if out_f32 else torch.bfloat16, device=dev)
    n_chunks = graph.fwd.plan.n_chunks
    part = torch.empty(n_chunks * H, dtype=torch.float32, device=dev) if n_chunks else None
    with _timed("sage_infer"):
        _lib.call("bgnn_sage_infer_bf16", graph.fwd.ref(), z.data_ptr(), z.stride(0), _ptr(bias), _ptr(scale),
                  _ptr(shift), _ptr(xp), xp.stride(0) if xp is not None else 0, H, reduce, out.data_ptr(),
                  out.stride(0), int(out_f32), _ptr(part), _stream())
    return out


# ---------------------------------------------------------------------------
# bf16 max-aggregation inference layer (BuckGNN.infer_bf16 = "all"): max is not linear, so the layer
# aggregates first and transforms [agg | x] in one GEMM of K = 2H.

def infer_weights_max(conv) -> torch.Tensor:
    """[W_l | W_r] of a SAGEConv as one bf16 [H, 2H] matrix (the B^T operand of the max layer's
    GEMM over [agg | x]), cached as infer_weights is, under an attribute of its own."""
    return _cached_weights(conv, "_bgnn_infer_wcat_max", 1)


@torch.no_grad()
def sage_infer_max_layer(buf: torch.Tensor, w: torch.Tensor, bias, bn_coeffs, graph: Graph, x_prev_plane,
                         out: torch.Tensor, out_f32: bool = False, y: torch.Tensor = None) -> torch.Tensor:
    """One eval-mode max-aggregation GraphSAGE layer on bf16 rows, three launches:
        agg = max_{j->i} x[j]                     into plane 0 of buf = [agg | x]   bgnn_spmm_max_bf16
        y   = buf [W_l | W_r]^T                   bf16 in, bf16 out, K = 2H          (gemm_bf16)
        out = ReLU(BN(normalize(y + b))) (+ x_prev)                                 bgnn_sage_tail_bf16
    buf: bf16 [N, 2H] whose plane 1 (columns [H, 2H)) holds the layer input x; w: bf16 [H, 2H]
    (infer_weights_max); bias: f32 [H] or None; bn_coeffs: (scale, shift) f32 [H] or None;
    x_prev_plane: the skip input, a bf16 [N, H] view (plane 1 of buf), or None; out: where the
    result goes -- plane 1 of the next layer's buffer (bf16), or a contiguous f32 [N, H] with
    out_f32 (the last layer); y: a bf16 [N, H] scratch to reuse across layers (None: a new one).
    Returns out. No autograd."""
    from .ops import spmm_max_bf16

    require_cuda(buf, w, bias, x_prev_plane, out, what="sage_infer_max_layer")
    N, H = buf.size(0), w.size(0)
    if (buf.dtype != torch.bfloat16 or w.dtype != torch.bfloat16 or buf.dim() != 2 or buf.size(1) != 2 * H
            or w.size(1) != 2 * H or not buf.is_contiguous()):
        raise ValueError("sage_infer_max_layer: buf must be a contiguous bfloat16 [N, 2H] and w bfloat16 [H, 2H]")
    if H % 8 or H > 512:
        raise ValueError(f"sage_infer_max_layer: needs H % 8 == 0 and H <= 512 (got {H})")
    if out.dtype != (torch.float32 if out_f32 else torch.bfloat16) or tuple(out.shape) != (N, H) or out.stride(1) != 1:
        raise ValueError("sage_infer_max_layer: out must be [N, H] with unit column stride, f32 with out_f32 "
                         "and bfloat16 without")
    if x_prev_plane is not None and (x_prev_plane.dtype != torch.bfloat16 or tuple(x_prev_plane.shape) != (N, H)
                                     or x_prev_plane.stride(1) != 1):
        raise ValueError("sage_infer_max_layer: x_prev_plane must be a bfloat16 [N, H] view")
    if y is None:
        y = torch.empty(N, H, dtype=torch.bfloat16, device=buf.device)
    with _timed("infer_max_agg"):
        spmm_max_bf16(graph.fwd, buf[:, H:], N, False, out=buf[:, :H])
    with _timed("infer_max_gemm"):
        gemm_bf16(buf, w, trans_a=False, trans_b=True, out=y)
    scale, shift = bn_coeffs if bn_coeffs is not None else (None, None)
    with _timed("infer_max_tail"):
        _lib.call("bgnn_sage_tail_bf16", y.data_ptr(), y.stride(0), _ptr(bias), _ptr(scale), _ptr(shift),
                  _ptr(x_prev_plane), x_prev_plane.stride(0) if x_prev_plane is not None else 0, N, H,
                  out.data_ptr(), out.stride(0), int(out_f32), _stream())
    return out
