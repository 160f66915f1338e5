// Per-graph reductions shared by graph_metrics.hip (bgnn_graph_metrics) and graph_loss_ex.hip
// (bgnn_graph_loss_ex): the fixed-order block reductions, the first-argmax reduction, the element
// terms in f32 with torch's roundings, and the radix select of a graph's order statistics (described
// at the head of graph_metrics.hip).
// Ties in the select's gradient (graph_loss_ex.hip, kind 4): torch.quantile sends the gradient to
// whichever of several equal elements its sort put at the selected rank, which torch does not
// specify. Here the whole weight of a selected value goes to the element that holds it at the
// smallest flat index row * C + c; when ranks lo and lo + 1 hold the same value, it gets weight 1.
#pragma once

#include "common.h"

#include <limits.h>

namespace bgnn {

constexpr int kMT = 256;                       // threads per workgroup (sums)
constexpr int kQT = 1024;                      // threads per workgroup (selects: 41 VGPRs, walks are latency-bound)
constexpr int kMW = kMT / kWave;               // waves per workgroup
constexpr uint32_t kNanBits = 0x7FC00000u;     // every NaN sorts as this pattern (above +inf)

// ---- block reductions over kMT threads, fixed order, result on every thread. `sh` is scratch of
// kMW entries.
__device__ __forceinline__ double block_sum(double v, double* sh) {
    for (int m = kWave >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    __syncthreads();   // (the scratch of the call before is read by now)
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    double s = sh[0];
    for (int w = 1; w < kMW; ++w) s += sh[w];
    return s;
}

// (value, row) of the largest value; ties to the smallest row. Values are finite and >= 0.
__device__ __forceinline__ void arg_better(float& v, int& r, float v2, int r2) {
    if (v2 > v || (v2 == v && r2 < r)) {
        v = v2;
        r = r2;
    }
}

__device__ __forceinline__ int block_argmax(float v, int r, float* shv, int* shr) {
    for (int m = kWave >> 1; m > 0; m >>= 1) {
        const float v2 = __shfl_xor(v, m, kWave);
        const int r2 = __shfl_xor(r, m, kWave);
        arg_better(v, r, v2, r2);
    }
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) {
        shv[threadIdx.x / kWave] = v;
        shr[threadIdx.x / kWave] = r;
    }
    __syncthreads();
    float bv = shv[0];
    int br = shr[0];
    for (int w = 1; w < kMW; ++w) arg_better(bv, br, shv[w], shr[w]);
    return br;
}

// ---- the element terms, f32 with torch's roundings
struct Denorm {
    const float* scale;
    const float* center;
    __device__ __forceinline__ float operator()(float v, int c) const {
        if (scale) v = __fmul_rn(v, scale[c]);
        if (center) v = __fadd_rn(v, center[c]);
        return v;
    }
};

__device__ __forceinline__ float abs_diff_of(float t, float p) { return fabsf(__fsub_rn(t, p)); }
__device__ __forceinline__ float rel_diff_eps(float a, float t, float eps) {
    return __fdiv_rn(a, __fadd_rn(fabsf(t), eps));
}
__device__ __forceinline__ float rel_diff_of(float a, float t) { return rel_diff_eps(a, t, 1e-8f); }

// sqrt(sum_c v_c^2): squares and sums rounded one by one in column order, the root correctly rounded
// (v(c): the row's value in column c; no per-thread arrays, a runtime C would put them in scratch)
template <class F>
__device__ __forceinline__ float row_norm(F&& v, int C) {
    const float v0 = v(0);
    float acc = __fmul_rn(v0, v0);
    for (int c = 1; c < C; ++c) {
        const float vc = v(c);
        acc = __fadd_rn(acc, __fmul_rn(vc, vc));
    }
    return sqrtf(acc);   // correctly rounded (hipcc's default; __fsqrt_rn is the 1-ulp native root here)
}

// the bit pattern an element is selected by
__device__ __forceinline__ uint32_t select_bits(float v) { return v != v ? kNanBits : __float_as_uint(v); }

// torch.quantile's linear interpolation, restated in f32 with explicit roundings. Both branches
// have d / da = 1 - w and d / db = w.
__device__ __forceinline__ float lerp_f32(float a, float b, float w) {
    const float d = __fsub_rn(b, a);
    return w < 0.5f ? __fadd_rn(a, __fmul_rn(w, d)) : __fsub_rn(b, __fmul_rn(d, __fsub_rn(1.f, w)));
}

// torch.quantile's rank among n elements: rank = q * (n - 1) in f32, the two neighbours lo and
// lo + 1 (need_hi: the upper one exists and differs), weight = rank - floor
struct QuantileRank {
    int64_t k_lo;
    bool need_hi;
    float w;
};

__device__ __forceinline__ QuantileRank quantile_rank(float q, int64_t n) {
    const float rank = __fmul_rn(q, (float)(n - 1));
    const float below = floorf(rank);
    QuantileRank r;
    r.k_lo = (int64_t)below;
    r.need_hi = (int64_t)ceilf(rank) > r.k_lo;
    r.w = __fsub_rn(rank, below);
    return r;
}

// LDS of one select
struct SelectShared {
    uint32_t hist[256];
    uint32_t scan[256];
    uint32_t prefix, k, eq, min, nan;
};

struct Selected {
    uint32_t lo_bits, hi_bits;   // the values of rank k_lo and (need_hi) k_lo + 1; hi_bits = lo_bits otherwise
    bool has_nan;                // a NaN among the elements (torch.quantile then gives NaN)
};

// The select, by a workgroup of kQT threads, every thread of which must call it; the result on
// every thread. walk(f): calls f(bits) for each of this thread's elements of the set (the threads'
// shares partition the set; every call walks the same elements). k_lo < the set's size < 2^31.
template <class Walk>
__device__ __forceinline__ Selected radix_select(SelectShared& sh, Walk&& walk, uint32_t k_lo, bool need_hi) {
    const int t = threadIdx.x;
    if (t == 0) {
        sh.prefix = 0;
        sh.k = k_lo;
        sh.nan = 0;
        sh.min = 0xFFFFFFFFu;
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (t < 256) sh.hist[t] = 0;
        __syncthreads();
        const uint32_t prefix = sh.prefix;
        const uint32_t mask = shift == 24 ? 0u : 0xFFFFFFFFu << (shift + 8);
        walk([&](uint32_t b) {
            if (shift == 24 && b == kNanBits) sh.nan = 1;   // (same value from every writer)
            if ((b & mask) == prefix) atomicAdd(&sh.hist[(b >> shift) & 255u], 1u);
        });
        __syncthreads();
        // inclusive scan of the 256 bins by the first 256 threads (Hillis-Steele, two buffers folded
        // into one with barriers; every thread takes the barriers)
        const bool bin = t < 256;
        const uint32_t v = bin ? sh.hist[t] : 0u;
        if (bin) sh.scan[t] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t add = (bin && t >= d) ? sh.scan[t - d] : 0u;
            __syncthreads();
            if (bin) sh.scan[t] += add;
            __syncthreads();
        }
        const uint32_t incl = bin ? sh.scan[t] : 0u, excl = incl - v, k = sh.k;
        __syncthreads();
        if (bin && k >= excl && k < incl) {   // exactly one bin holds rank k
            sh.prefix = prefix | ((uint32_t)t << shift);
            sh.k = k - excl;
            sh.eq = v;
        }
        __syncthreads();
    }
    Selected r;
    r.lo_bits = sh.prefix;
    r.hi_bits = r.lo_bits;
    if (need_hi && sh.k + 1 >= sh.eq) {   // rank lo + 1 lies past the copies of the value: the next larger one
        const uint32_t lo_bits = r.lo_bits;
        walk([&](uint32_t b) {
            if (b > lo_bits) atomicMin(&sh.min, b);
        });
        __syncthreads();
        r.hi_bits = sh.min;
    }
    r.has_nan = sh.nan != 0;
    return r;
}

}  // namespace bgnn
