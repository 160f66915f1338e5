// The rest of the reference's criterion(pred, target, batch, x) family on the batch vector's segment
// CSR (Utils/Losses.py:303-359, 403-443, 509-695), loss and d loss / d pred together; the contract of
// each kind is in include/bgnn.h. Kinds 0..2 are graph_loss.hip's (same element code,
// graph_loss_elem.h) with a device-side multiplier m = mult * *mult_dev; kind 3 (ratio of sums) runs a
// sums pass, a gradient pass that re-adds the graph's block sums in order, and the finish; kind 4
// (mixed) runs kind 1's pass for the MAE term, then one workgroup of 1024 per graph selects the two
// order statistics of torch.quantile (graph_select.h) and adds their gradient at (at most) two
// elements; kind 5 (max component) runs one workgroup per graph. Sums in double by fixed trees, no
// floating-point atomics (the select's are integer LDS atomics): bit-identical from run to run.
// bgnn_force_scale: max(sum over rows of ||x[r, c0 : c0 + nc]||_2, min_scale) on the device.
#include "graph_loss_elem.h"
#include "graph_select.h"

namespace bgnn {

namespace {

constexpr double kRatioEps = 1e-8;   // ScaledGraphRELoss.compute_relative_error's constant

// the entry point's arguments as the kernels take them; part / part_t / gv: the workspace's [B S] block
// sums, [B S] second sums of kind 3 and [B] per-graph values of kinds 4 and 5
struct LossExArgs {
    const float *pred, *target, *scale, *center, *mult_dev;
    const int32_t *rowptr, *col;
    double *part, *part_t, *gv;
    float *loss, *dpred;
    int C, B, kind;
    float eps, mult, q;
    // the effective multiplier m = mult * *mult_dev
    __device__ __forceinline__ double m() const { return mult_dev ? (double)mult * (double)*mult_dev : (double)mult; }
    __device__ __forceinline__ float sc(int c) const { return scale ? scale[c] : 1.f; }
};

// ---- kinds 0..2, and the MAE term of kind 4 (kind 1 at the weight 0.8 m): block (g, s)
__global__ __launch_bounds__(256) void k_graph_loss_ex_mean(const LossExArgs a) {
    __shared__ double red[256];
    graph_loss_block(a.pred, a.target, a.C, a.rowptr, a.col, a.B, a.kind == 4 ? 1 : a.kind, a.eps,
                     a.kind == 4 ? a.m() * 0.8 : a.m(), a.scale, a.center, a.part, a.dpred, red, blockIdx.x, gridDim.y,
                     blockIdx.y);
}

// ---- kind 3: block (g, s) sums |p' - t'| and |t'| over its segment-block
__global__ __launch_bounds__(256) void k_graph_loss_ratio_sums(const LossExArgs a) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const int S = gridDim.y, s = blockIdx.y, g = blockIdx.x;
    double ad = 0.0, tt = 0.0;
    seg_block_walk(a.col, a.rowptr[g], a.rowptr[g + 1], a.C, S, s, t, [&](int64_t i, int c) {
        const float tv = denorm_of(a.target[i], c, a.scale, a.center);
        ad += (double)fabsf(__fsub_rn(denorm_of(a.pred[i], c, a.scale, a.center), tv));
        tt += (double)fabsf(tv);
    });
    red[t] = ad;
    tree_sum256(red, t);
    if (t == 0) a.part[(int64_t)g * S + s] = red[0];
    __syncthreads();
    red[t] = tt;
    tree_sum256(red, t);
    if (t == 0) a.part_t[(int64_t)g * S + s] = red[0];
}

// T_g: the graph's S block sums in order (the same order in the gradient and in the finish)
__device__ __forceinline__ double sum_in_order(const double* __restrict__ part, int g, int S) {
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += part[(int64_t)g * S + s];
    return sum;
}

// kind 3: dpred = m / B * sign(p' - t') * scale[c] / (T_g + 1e-8)
__global__ __launch_bounds__(256) void k_graph_loss_ratio_grad(const LossExArgs a) {
    const int S = gridDim.y, s = blockIdx.y, g = blockIdx.x;
    const double w = a.m() / (double)a.B / (sum_in_order(a.part_t, g, S) + kRatioEps);
    seg_block_walk(a.col, a.rowptr[g], a.rowptr[g + 1], a.C, S, s, threadIdx.x, [&](int64_t i, int c) {
        const float dir = __fsub_rn(denorm_of(a.pred[i], c, a.scale, a.center),
                                    denorm_of(a.target[i], c, a.scale, a.center));
        a.dpred[i] = (float)(sign0(dir) * w * (double)a.sc(c));
    });
}

// ---- kind 4: one workgroup per graph selects Q_q of r over the graph's n_g C elements into qv[g]
// and adds the quantile term's gradient into dpred (the dense pass has written it: stream order)
__global__ __launch_bounds__(kQT) void k_graph_loss_quantile(const LossExArgs a) {
    const float *pred = a.pred, *target = a.target;
    const int32_t *rowptr = a.rowptr, *col = a.col;
    double* qv = a.gv;
    float* dpred = a.dpred;
    const int C = a.C;
    const float eps = a.eps;
    __shared__ SelectShared sh;
    __shared__ uint32_t s_first[2];
    const int t = threadIdx.x;
    const int g = blockIdx.x;
    const int64_t r0 = rowptr[g], r1 = rowptr[g + 1];
    if (r1 <= r0) {   // a graph id without rows: no quantile is defined
        if (t == 0) qv[g] = __builtin_nan("");
        return;
    }
    const int64_t n = (r1 - r0) * C;   // (n <= N C < 2^31: the entry's check)
    QuantileRank rk = quantile_rank(a.q, n);
    if (rk.k_lo >= n - 1) {   // (q = 1; past 2^24 elements the f32 rank can round above n - 1)
        rk.k_lo = n - 1;
        rk.need_hi = false;
    }
    const Denorm dn{a.scale, a.center};
    // f(bits of r, flat index) for each of this thread's elements; every pass recomputes them
    auto walk_at = [&](auto&& f) {
        for (int64_t r = r0 + t; r < r1; r += kQT) {
            const int64_t i0 = (int64_t)col[r] * C;
            for (int c = 0; c < C; ++c) {
                const float tv = dn(target[i0 + c], c);
                f(select_bits(rel_diff_eps(abs_diff_of(tv, dn(pred[i0 + c], c)), tv, eps)), (uint32_t)(i0 + c));
            }
        }
    };
    auto walk = [&](auto&& f) { walk_at([&](uint32_t b, uint32_t) { f(b); }); };
    const Selected sel = radix_select(sh, walk, (uint32_t)rk.k_lo, rk.need_hi);
    const bool grad = dpred != nullptr && !sel.has_nan;   // (a NaN among the elements: the loss is NaN)
    if (t == 0) s_first[0] = s_first[1] = 0xFFFFFFFFu;
    __syncthreads();
    if (grad) {
        // of the elements that hold a selected value, the one at the smallest flat index
        walk_at([&](uint32_t b, uint32_t i) {
            if (b == sel.lo_bits) atomicMin(&s_first[0], i);
            if (b == sel.hi_bits) atomicMin(&s_first[1], i);
        });
    }
    __syncthreads();
    if (t != 0) return;
    const float lo = __uint_as_float(sel.lo_bits), hi = __uint_as_float(sel.hi_bits);
    qv[g] = (double)(sel.has_nan ? __uint_as_float(kNanBits) : rk.need_hi ? lerp_f32(lo, hi, rk.w) : lo);
    if (!grad) return;
    const double coef = 0.2 * a.m() / (double)a.B;
    auto add = [&](uint32_t i, float weight) {
        if (i == 0xFFFFFFFFu) return;   // (no element held the value: cannot happen for finite elements)
        const int c = (int)(i % (uint32_t)C);
        const float tv = dn(target[i], c);
        const float dir = __fsub_rn(dn(pred[i], c), tv);
        const double d = coef * (double)weight * sign0(dir) * (double)a.sc(c) / (double)__fadd_rn(fabsf(tv), eps);
        dpred[i] = (float)((double)dpred[i] + d);
    };
    if (!rk.need_hi || sel.hi_bits == sel.lo_bits) {
        add(s_first[0], 1.f);
    } else {
        add(s_first[0], __fsub_rn(1.f, rk.w));
        add(s_first[1], rk.w);
    }
}

// ---- kind 5: one workgroup per graph; gv[g] = sum_c of the relative error at the row of the largest
// |t'_c|; dpred: zero over the graph's rows, then the C selected elements
__global__ __launch_bounds__(kMT) void k_graph_loss_maxc(const LossExArgs a) {
    const float *pred = a.pred, *target = a.target;
    const int32_t *rowptr = a.rowptr, *col = a.col;
    double* gv = a.gv;
    float* dpred = a.dpred;
    const int C = a.C;
    const float eps = a.eps;
    __shared__ float shf[kMW];
    __shared__ int shr[kMW];
    __shared__ double term[8];
    const int t = threadIdx.x;
    const int g = blockIdx.x;
    const int64_t r0 = rowptr[g], r1 = rowptr[g + 1];
    if (r1 <= r0) {   // a graph id without rows: no maximum is defined
        if (t == 0) gv[g] = __builtin_nan("");
        return;
    }
    const Denorm dn{a.scale, a.center};
    // (fixed trip counts with a c < C guard: the per-column state stays in registers)
    float bv[8];
    int br[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        bv[c] = -1.f;
        br[c] = INT_MAX;
    }
    for (int64_t r = r0 + t; r < r1; r += kMT) {
        const int row = col[r];
        const int64_t i0 = (int64_t)row * C;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            if (c < C) {
                arg_better(bv[c], br[c], fabsf(dn(target[i0 + c], c)), row);
                if (dpred) dpred[i0 + c] = 0.f;
            }
        }
    }
    int best = INT_MAX;   // thread c keeps column c's row
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c < C) {
            const int b = block_argmax(bv[c], br[c], shf, shr);
            if (t == c) best = b;
        }
    }
    __syncthreads();   // the zeros are written before the selected elements
    if (t < C) {
        if (best == INT_MAX) {   // no row won: every candidate was NaN (targets are to be finite)
            term[t] = __builtin_nan("");
        } else {
            const int64_t i = (int64_t)best * C + t;
            const float tv = dn(target[i], t);
            const float dir = __fsub_rn(dn(pred[i], t), tv);
            const float den = __fadd_rn(fabsf(tv), eps);
            term[t] = (double)__fdiv_rn(fabsf(dir), den);
            if (dpred)
                dpred[i] = (float)(a.m() / ((double)a.B * (double)C) * sign0(dir) * (double)a.sc(t) / (double)den);
        }
    }
    __syncthreads();
    if (t == 0) {
        double sum = 0.0;
        for (int c = 0; c < C; ++c) sum += term[c];
        gv[g] = sum;
    }
}

// ---- the finish, one workgroup: the per-graph values in a fixed order, then a fixed tree
__global__ __launch_bounds__(256) void k_graph_loss_ex_finish(const LossExArgs a, int S) {
    __shared__ double red[256];
    const double *part = a.part, *part_t = a.part_t, *gv = a.gv;
    const int32_t* rowptr = a.rowptr;
    const int B = a.B, C = a.C, kind = a.kind;
    const double m = a.m();
    if (kind <= 2) {
        graph_loss_finish_block(part, S, B, C, rowptr, m, a.loss, red);
        return;
    }
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int g = t; g < B; g += 256) {
        if (kind == 3) {
            acc += sum_in_order(part, g, S) / (sum_in_order(part_t, g, S) + kRatioEps);
        } else if (kind == 4) {   // (no rows: 0 / 0 = NaN)
            const double mae = sum_in_order(part, g, S) / ((double)(rowptr[g + 1] - rowptr[g]) * (double)C);
            acc += 0.2 * gv[g] + 0.8 * mae;
        } else {
            acc += gv[g] / (double)C;
        }
    }
    red[t] = acc;
    tree_sum256(red, t);
    if (t == 0) *a.loss = (float)(red[0] / (double)B * m);
}

// ---- bgnn_force_scale: block b sums the f32 row norms of its rows (grid-stride) in double
__global__ __launch_bounds__(256) void k_force_scale_sums(const float* __restrict__ x, int64_t N, int64_t ldx, int c0,
                                                          int nc, int flag_col, double* __restrict__ part) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + t; r < N; r += (int64_t)gridDim.x * 256) {
        const float* xr = x + r * ldx;
        if (flag_col >= 0 && xr[flag_col] != 0.f) continue;
        acc += (double)row_norm([&](int c) { return xr[c0 + c]; }, nc);
    }
    red[t] = acc;
    tree_sum256(red, t);
    if (t == 0) part[blockIdx.x] = red[0];
}

// one workgroup: the G block sums (G <= 256) by the fixed tree, rounded once; max(total, min_scale)
// as Python's max(total, min_scale): a NaN total stays NaN
__global__ __launch_bounds__(256) void k_force_scale_finish(const double* __restrict__ part, int G, float min_scale,
                                                            float* __restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    red[t] = t < G ? part[t] : 0.0;
    tree_sum256(red, t);
    if (t == 0) {
        const float total = (float)red[0];
        *out = min_scale > total ? min_scale : total;
    }
}

inline int force_blocks(int64_t N) {
    const int64_t G = (N + 255) / 256;
    return (int)(G < 1 ? 1 : (G > 256 ? 256 : G));
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

// [B S] block sums, [B S] the second sums of kind 3, [B] the per-graph values of kinds 4 and 5
extern "C" size_t bgnn_graph_loss_ex_ws_bytes(int64_t N, int32_t C, int64_t B) {
    return (B > 0 && N > 0 && C > 0) ? (size_t)B * (2 * (size_t)loss_segments(N, C, B) + 1) * sizeof(double) : 0;
}

extern "C" int bgnn_graph_loss_ex(const float* pred, const float* target, int64_t N, int32_t C, const int32_t* rowptr,
                                  const int32_t* col, int64_t B, int32_t kind, float eps, float mult,
                                  const float* scale, const float* center, float q, const float* mult_dev, float* loss,
                                  float* dpred, void* ws, size_t ws_bytes, void* stream) {
    BGNN_REQUIRE(kind >= 0 && kind <= 5,
                 "graph_loss_ex: kind %d unknown (0 relative, 1 MAE, 2 squares, 3 ratio of sums, 4 mixed, 5 max "
                 "component)", kind);
    BGNN_REQUIRE(C >= 1 && C <= 8, "graph_loss_ex: C=%d unsupported (1..8)", C);
    // flat indices row * C + c and the select's ranks are 32-bit
    BGNN_REQUIRE(N >= 1 && N * (int64_t)C <= INT32_MAX && B >= 1 && B <= INT32_MAX,
                 "graph_loss_ex: N C and B must be in [1, 2^31)");
    BGNN_REQUIRE(kind != 4 || (q >= 0.f && q <= 1.f), "graph_loss_ex: q=%g outside [0, 1]", (double)q);
    BGNN_REQUIRE(pred && target && rowptr && col && loss, "graph_loss_ex: null pointer");
    BGNN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= bgnn_graph_loss_ex_ws_bytes(N, C, B),
                 "graph_loss_ex: workspace too small or not 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const int S = loss_segments(N, C, B);
    double* part = static_cast<double*>(ws);
    LossExArgs a{};
    a.pred = pred, a.target = target, a.scale = scale, a.center = center, a.mult_dev = mult_dev;
    a.rowptr = rowptr, a.col = col;
    a.part = part, a.part_t = part + (size_t)B * S, a.gv = part + 2 * (size_t)B * S;
    a.loss = loss, a.dpred = dpred;
    a.C = (int)C, a.B = (int)B, a.kind = (int)kind;
    a.eps = eps, a.mult = mult, a.q = q;
    const dim3 seg_grid((unsigned)B, S), graph_grid((unsigned)B);
    if (kind <= 2 || kind == 4) {
        hipLaunchKernelGGL(k_graph_loss_ex_mean, seg_grid, dim3(256), 0, s, a);
        BGNN_CHECK_LAUNCH();
        if (kind == 4) {
            hipLaunchKernelGGL(k_graph_loss_quantile, graph_grid, dim3(kQT), 0, s, a);
            BGNN_CHECK_LAUNCH();
        }
    } else if (kind == 3) {
        hipLaunchKernelGGL(k_graph_loss_ratio_sums, seg_grid, dim3(256), 0, s, a);
        BGNN_CHECK_LAUNCH();
        if (dpred) {
            hipLaunchKernelGGL(k_graph_loss_ratio_grad, seg_grid, dim3(256), 0, s, a);
            BGNN_CHECK_LAUNCH();
        }
    } else {
        hipLaunchKernelGGL(k_graph_loss_maxc, graph_grid, dim3(kMT), 0, s, a);
        BGNN_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(k_graph_loss_ex_finish, dim3(1), dim3(256), 0, s, a, S);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

extern "C" size_t bgnn_force_scale_ws_bytes(int64_t N) {
    return N > 0 ? (size_t)force_blocks(N) * sizeof(double) : 0;
}

extern "C" int bgnn_force_scale(const float* x, int64_t N, int64_t ldx, int32_t c0, int32_t nc, int32_t flag_col,
                                float min_scale, float* out, void* ws, size_t ws_bytes, void* stream) {
    BGNN_REQUIRE(N >= 1 && N <= INT32_MAX, "force_scale: N must be in [1, 2^31)");
    BGNN_REQUIRE(nc >= 1 && nc <= 8 && c0 >= 0 && (int64_t)c0 + nc <= ldx,
                 "force_scale: columns [%d, %d + %d) must be 1..8 columns within the row stride %lld", c0, c0, nc,
                 (long long)ldx);
    BGNN_REQUIRE(flag_col < ldx, "force_scale: flag column %d outside the row stride %lld (negative: none)", flag_col,
                 (long long)ldx);
    BGNN_REQUIRE(x && out, "force_scale: null pointer");
    BGNN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= bgnn_force_scale_ws_bytes(N),
                 "force_scale: workspace too small or not 8-byte aligned");
    hipStream_t s = as_stream(stream);
    const int G = force_blocks(N);
    double* part = static_cast<double*>(ws);
    hipLaunchKernelGGL(k_force_scale_sums, dim3(G), dim3(256), 0, s, x, N, ldx, (int)c0, (int)nc,
                       flag_col < 0 ? -1 : (int)flag_col, part);
    BGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_force_scale_finish, dim3(1), dim3(256), 0, s, part, G, min_scale, out);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}
