// The element term and the (graph, segment-block) walk of the per-graph losses, shared by
// graph_loss.hip (bgnn_graph_loss) and graph_loss_ex.hip (bgnn_graph_loss_ex): one definition, so
// kinds 0..2 give the same bits through either entry point.
// Every product, sum, difference and quotient of the element term is rounded on its own
// (__fmul_rn and friends: no contraction whatever the file's flags), as torch's f32 expressions.
#pragma once

#include "common.h"

namespace bgnn {

// block tree sum over 256 doubles, fixed order; the result in red[0]
__device__ __forceinline__ void tree_sum256(double* red, int t) {
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
}

// segment-blocks per graph: about 2048 elements each at the mean graph size, at most 64
inline int loss_segments(int64_t N, int32_t C, int64_t B) {
    const int64_t per = (N * C + B - 1) / B;
    const int64_t S = (per + 2047) / 2048;
    return (int)(S < 1 ? 1 : (S > 64 ? 64 : S));
}

// Segment-block s of S of the graph whose rows are col[r0 .. r1): elements [s * chunk, (s + 1) * chunk)
// of the graph's n_g C elements (chunk = the count split S ways, rounded up), 256 threads;
// f(i, c) with i the flat index row * C + c.
template <class F>
__device__ __forceinline__ void seg_block_walk(const int32_t* __restrict__ col, int64_t r0, int64_t r1, int C, int S,
                                               int s, int t, F&& f) {
    const int64_t cnt = (r1 - r0) * C;
    const int64_t chunk = (cnt + S - 1) / S;
    const int64_t e0 = s * chunk, e1 = min(cnt, e0 + chunk);
    for (int64_t e = e0 + t; e < e1; e += 256) {
        const int64_t r = e / C;
        const int c = (int)(e - r * C);
        f((int64_t)col[r0 + r] * C + c, c);
    }
}

// p' = v * scale[c] + center[c] (NULL: identity), product and sum rounded
__device__ __forceinline__ float denorm_of(float v, int c, const float* __restrict__ scale,
                                           const float* __restrict__ center) {
    if (scale) v = __fmul_rn(v, scale[c]);
    if (center) v = __fadd_rn(v, center[c]);
    return v;
}

// sign with sign(0) = sign(NaN) = 0: torch's abs backward (grad * sgn(x)), as k_rel_error_loss
__device__ __forceinline__ double sign0(float dir) { return dir > 0.f ? 1.0 : (dir < 0.f ? -1.0 : 0.0); }

// One element of kinds 0 / 1 / 2: f = |p' - t'| / (|t'| + eps), |p' - t'|, |p'^2 - t'^2|; dir: what the
// absolute value is taken of; d f / d pred = sign(dir) * fac * sc / den (the chain through
// p' = pred * scale + center adds the factor sc = scale[c])
struct LossTerm {
    float f, dir, den, fac, sc;
};

__device__ __forceinline__ LossTerm loss_term(int kind, float p, float q, int c, float eps,
                                              const float* __restrict__ scale, const float* __restrict__ center) {
    LossTerm e;
    e.sc = scale ? scale[c] : 1.f;
    p = denorm_of(p, c, scale, center);
    q = denorm_of(q, c, scale, center);
    e.den = 1.f;
    e.fac = 1.f;
    if (kind == 2) {
        e.dir = __fsub_rn(__fmul_rn(p, p), __fmul_rn(q, q));
        e.f = fabsf(e.dir);
        e.fac = 2.f * p;
    } else {
        e.dir = __fsub_rn(p, q);
        e.f = fabsf(e.dir);
        if (kind == 0) {
            e.den = __fadd_rn(fabsf(q), eps);
            e.f = __fdiv_rn(e.f, e.den);
        }
    }
    return e;
}

// w: d loss / d f of the element
__device__ __forceinline__ float loss_term_grad(const LossTerm& e, double w) {
    return (float)(sign0(e.dir) * w * (double)e.fac * (double)e.sc / (double)e.den);
}

// Workgroup (g, s) of the per-graph-mean losses (kinds 0..2): the sum of f over segment-block s of
// graph g goes to part[g * S + s]; dpred (NULL: skipped) gets mult / (B n_g C) * d f / d pred.
__device__ __forceinline__ void graph_loss_block(const float* __restrict__ pred, const float* __restrict__ target,
                                                 int C, const int32_t* __restrict__ rowptr,
                                                 const int32_t* __restrict__ col, int B, int kind, float eps,
                                                 double mult, const float* __restrict__ scale,
                                                 const float* __restrict__ center, double* __restrict__ part,
                                                 float* __restrict__ dpred, double* red, int g, int S, int s) {
    const int t = threadIdx.x;
    const int64_t r0 = rowptr[g], r1 = rowptr[g + 1];
    // d loss / d f of this graph's elements: mult / (B n_g C)
    const double w = mult / ((double)B * (double)((r1 - r0) * C));
    double acc = 0.0;
    seg_block_walk(col, r0, r1, C, S, s, t, [&](int64_t i, int c) {
        const LossTerm e = loss_term(kind, pred[i], target[i], c, eps, scale, center);
        acc += (double)e.f;
        if (dpred) dpred[i] = loss_term_grad(e, w);
    });
    red[t] = acc;
    tree_sum256(red, t);
    if (t == 0) part[(int64_t)g * S + s] = red[0];
}

// One workgroup: per graph the S segment-block sums in order, over n_g C (no rows: 0 / 0 = NaN, as
// the torch path); the per-graph means by a fixed tree
__device__ __forceinline__ void graph_loss_finish_block(const double* __restrict__ part, int S, int B, int C,
                                                        const int32_t* __restrict__ rowptr, double mult,
                                                        float* __restrict__ loss, double* red) {
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int g = t; g < B; g += 256) {
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += part[(int64_t)g * S + s];
        acc += sum / ((double)(rowptr[g + 1] - rowptr[g]) * (double)C);
    }
    red[t] = acc;
    tree_sum256(red, t);
    if (t == 0) *loss = (float)(red[0] / (double)B * mult);
}

}  // namespace bgnn
