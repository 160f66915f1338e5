// The per-graph error metrics of the static heads (Dataset_Preparation/Metrics.py:25-191,
// stress_errors for static_stress / static_disp) as one table out[B, BGNN_GRAPH_METRICS_COLS] of
// doubles, column order in include/bgnn.h.
//
// Two launches. k_graph_metrics_sums, one workgroup per graph, walks the graph's rows through the
// batch vector's segment CSR (any row order) twice: the first walk takes every sum, the region
// counts, the largest |error| and the first row of the largest |target| per tracked component; the
// second walk takes sum (|error| - mean)^2 for the unbiased standard deviation. k_graph_quantiles, one
// workgroup per (graph, quantile), finds the two order statistics torch.quantile interpolates
// between by a most-significant-digit-first radix select over the elements' bit patterns (all
// candidates are >= 0 or NaN, so the patterns order as unsigned integers, NaN canonicalised above
// +inf): four 8-bit passes with a 256-bin integer histogram in LDS give the value of rank lo; rank
// lo + 1 is the same value when the bin holds more of it, else the smallest larger element (one
// more pass, an integer minimum). The elements are recomputed from pred / target in every pass
// (L2-resident); nothing is staged, so a graph's size has no upper limit. The select, the block
// reductions and the element terms live in graph_select.h, shared with graph_loss_ex.hip.
//
// Arithmetic: every element term in f32 with torch's roundings (each product, sum, difference and
// quotient rounded, no contraction); every sum in double, per thread in walk order, then lanes and
// waves by a fixed butterfly; no floating-point atomics (the histogram and the minimum are integer
// LDS atomics, which are order-independent). The table is bit-identical from run to run.
#include "graph_select.h"

namespace bgnn {

namespace {

__device__ __forceinline__ long long block_sum_i(long long v, long long* sh) {
    for (int m = kWave >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    long long s = sh[0];
    for (int w = 1; w < kMW; ++w) s += sh[w];
    return s;
}

// max that keeps a NaN once seen (torch's amax propagates NaN)
__device__ __forceinline__ float nan_max(float m, float a) { return (a > m || a != a) ? a : m; }

__device__ __forceinline__ float block_nan_max(float v, float* sh) {
    for (int m = kWave >> 1; m > 0; m >>= 1) v = nan_max(v, __shfl_xor(v, m, kWave));
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = v;
    __syncthreads();
    float s = sh[0];
    for (int w = 1; w < kMW; ++w) s = nan_max(s, sh[w]);
    return s;
}

struct RegionSums {
    double rel = 0.0, abs = 0.0, tabs = 0.0, sq = 0.0;
    long long n = 0;
    __device__ __forceinline__ void add(float a, float r, float t, float p) {
        rel += (double)r;
        abs += (double)a;
        tabs += (double)fabsf(t);
        sq += (double)__fsub_rn(__fmul_rn(t, t), __fmul_rn(p, p));
        n += 1;
    }
};

// the five columns mape / re / rmse / mae of a region from its sums (p90 comes from the select);
// a region without elements: zeros
__device__ __forceinline__ void write_region(double* o, const RegionSums& s) {
    if (s.n == 0) {
        o[0] = o[1] = o[2] = o[3] = 0.0;
        return;
    }
    const double n = (double)s.n;
    o[0] = s.rel / n * 100.0;
    o[1] = s.abs / s.tabs * 100.0;
    o[2] = sqrt(s.sq / n);   // NaN where the mean of t^2 - p^2 is negative, as the reference
    o[3] = s.abs / n;
}

// column offsets (include/bgnn.h)
constexpr int kColMax = 0, kColHigh = 9, kColLow = 14, kColAll = 19, kColMse = 23, kColP90 = 24, kColMaxMae = 25,
              kColStd = 26, kColP90Abs = 27, kColNHigh = 28, kColNLow = 29;
constexpr int kCols = BGNN_GRAPH_METRICS_COLS;
static_assert(kCols == 30, "column layout");

__global__ __launch_bounds__(kMT) void k_graph_metrics_sums(const float* __restrict__ pred,
                                                            const float* __restrict__ target, int C,
                                                            const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ col, int mode, float threshold,
                                                            const float* __restrict__ scale,
                                                            const float* __restrict__ center,
                                                            double* __restrict__ out) {
    __shared__ double shd[kMW];
    __shared__ long long shi[kMW];
    __shared__ float shf[kMW];
    __shared__ int shr[kMW];
    const int t = threadIdx.x;
    const int g = blockIdx.x;
    const int64_t r0 = rowptr[g], r1 = rowptr[g + 1];
    double* o = out + (int64_t)g * kCols;
    if (r1 <= r0) {   // a graph id without rows: no metric is defined
        for (int k = t; k < kCols; k += kMT) o[k] = k < kColNHigh ? __builtin_nan("") : 0.0;
        return;
    }
    const Denorm dn{scale, center};
    RegionSums hi, lo, all;
    float mx = -INFINITY;
    float bv[3] = {-1.f, -1.f, -1.f};
    int br[3] = {INT_MAX, INT_MAX, INT_MAX};
    for (int64_t r = r0 + t; r < r1; r += kMT) {
        const int row = col[r];
        const float* pp = pred + (int64_t)row * C;
        const float* tp = target + (int64_t)row * C;
        bool row_hi = false;
        if (mode == 1) {
            const float mag = row_norm([&](int c) { return dn(tp[c], c); }, C);
            row_hi = mag >= threshold;
            arg_better(bv[0], br[0], mag, row);
            arg_better(bv[1], br[1], fabsf(dn(tp[0], 0)), row);
            arg_better(bv[2], br[2], fabsf(dn(tp[1], 1)), row);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) arg_better(bv[c], br[c], fabsf(dn(tp[c], c)), row);
        }
        for (int c = 0; c < C; ++c) {
            const float tv = dn(tp[c], c), pv = dn(pp[c], c);
            const float a = abs_diff_of(tv, pv);
            const float rl = rel_diff_of(a, tv);
            const bool h = mode == 1 ? row_hi : fabsf(tv) >= threshold;
            if (h) hi.add(a, rl, tv, pv);
            else lo.add(a, rl, tv, pv);
            all.add(a, rl, tv, pv);
            mx = nan_max(mx, a);
        }
    }
    auto reduce = [&](RegionSums& s) {
        s.rel = block_sum(s.rel, shd);
        s.abs = block_sum(s.abs, shd);
        s.tabs = block_sum(s.tabs, shd);
        s.sq = block_sum(s.sq, shd);
        s.n = block_sum_i(s.n, shi);
    };
    reduce(hi);
    reduce(lo);
    reduce(all);
    mx = block_nan_max(mx, shf);
    int best[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) best[k] = block_argmax(bv[k], br[k], shf, shr);
    // second walk: the unbiased variance of |error| about its mean, in double
    const double mean = all.abs / (double)all.n;
    double var = 0.0;
    for (int64_t r = r0 + t; r < r1; r += kMT) {
        const int row = col[r];
        for (int c = 0; c < C; ++c) {
            const float a = abs_diff_of(dn(target[(int64_t)row * C + c], c), dn(pred[(int64_t)row * C + c], c));
            const double d = (double)a - mean;
            var += d * d;
        }
    }
    var = block_sum(var, shd);
    if (t != 0) return;
    // the values at the maxima: val, mae, rel (x 100 in f32, as the torch expression)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (best[k] == INT_MAX) {   // no row won: every candidate was NaN (targets are to be finite)
            o[kColMax + 3 * k + 0] = o[kColMax + 3 * k + 1] = o[kColMax + 3 * k + 2] = __builtin_nan("");
            continue;
        }
        const float* tp = target + (int64_t)best[k] * C;
        const float* pp = pred + (int64_t)best[k] * C;
        float val, err;
        if (mode == 1 && k == 0) {
            val = row_norm([&](int c) { return dn(tp[c], c); }, C);
            err = row_norm([&](int c) { return abs_diff_of(dn(tp[c], c), dn(pp[c], c)); }, C);
        } else {
            const int c = mode == 1 ? k - 1 : k;
            val = fabsf(dn(tp[c], c));
            err = abs_diff_of(dn(tp[c], c), dn(pp[c], c));
        }
        o[kColMax + 3 * k + 0] = (double)val;
        o[kColMax + 3 * k + 1] = (double)err;
        o[kColMax + 3 * k + 2] = (double)__fmul_rn(__fdiv_rn(err, __fadd_rn(val, 1e-8f)), 100.f);
    }
    write_region(o + kColHigh, hi);
    write_region(o + kColLow, lo);
    write_region(o + kColAll, all);
    o[kColMse] = all.sq / (double)all.n;
    o[kColMaxMae] = (double)mx;
    o[kColStd] = sqrt(var / (double)(all.n - 1));   // one element: 0 / 0 = NaN, as torch.std
    o[kColNHigh] = (double)hi.n;
    o[kColNLow] = (double)lo.n;
}

// block (g, which): which 0 / 1 / 2: the relative error over the high region / the low region / all
// elements, 3: the absolute error over all elements. Element counts come from the sums kernel's
// count columns. Writes (x 100 for the relative ones) into the p90 columns.
__global__ __launch_bounds__(kQT) void k_graph_quantiles(const float* __restrict__ pred,
                                                         const float* __restrict__ target, int C,
                                                         const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col, int mode, float threshold,
                                                         float q, const float* __restrict__ scale,
                                                         const float* __restrict__ center, double* __restrict__ out) {
    __shared__ SelectShared sh;
    const int t = threadIdx.x;
    const int g = blockIdx.x, which = blockIdx.y;
    const int64_t r0 = rowptr[g], r1 = rowptr[g + 1];
    if (r1 <= r0) return;   // (the sums kernel wrote the NaN row)
    double* o = out + (int64_t)g * kCols;
    const int ocol = which == 0 ? kColHigh + 4 : which == 1 ? kColLow + 4 : which == 2 ? kColP90 : kColP90Abs;
    const int64_t n = which == 0 ? (int64_t)o[kColNHigh] : which == 1 ? (int64_t)o[kColNLow] : (r1 - r0) * C;
    if (n == 0) {
        if (t == 0) o[ocol] = 0.0;
        return;
    }
    const QuantileRank rk = quantile_rank(q, n);   // (k_lo < n <= N C < 2^31: the entry's check)
    const Denorm dn{scale, center};

    // Walks the graph's elements of this block's set: f(bits) for each. Every pass recomputes them.
    auto walk = [&](auto&& f) {
        for (int64_t r = r0 + t; r < r1; r += kQT) {
            const int row = col[r];
            const float* tp = target + (int64_t)row * C;
            const float* pp = pred + (int64_t)row * C;
            bool row_hi = false;
            if (mode == 1 && which < 2) row_hi = row_norm([&](int c) { return dn(tp[c], c); }, C) >= threshold;
            for (int c = 0; c < C; ++c) {
                const float tv = dn(tp[c], c);
                if (which < 2) {
                    const bool h = mode == 1 ? row_hi : fabsf(tv) >= threshold;
                    if (h != (which == 0)) continue;
                }
                const float a = abs_diff_of(tv, dn(pp[c], c));
                const float v = which == 3 ? a : rel_diff_of(a, tv);
                f(select_bits(v));
            }
        }
    };

    const Selected sel = radix_select(sh, walk, (uint32_t)rk.k_lo, rk.need_hi);
    if (t == 0) {
        float res;
        if (sel.has_nan) res = __uint_as_float(kNanBits);   // torch.quantile: any NaN in the set gives NaN
        else res = rk.need_hi ? lerp_f32(__uint_as_float(sel.lo_bits), __uint_as_float(sel.hi_bits), rk.w)
                              : __uint_as_float(sel.lo_bits);
        o[ocol] = which == 3 ? (double)res : (double)res * 100.0;
    }
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_graph_metrics_ws_bytes(int64_t N, int32_t C, int64_t B) {
    // nothing is staged today; one aligned word so that callers always pass a real buffer
    return (B > 0 && N > 0 && C > 0) ? 8 : 0;
}

extern "C" int bgnn_graph_metrics(const float* pred, const float* target, int64_t N, int32_t C, const int32_t* rowptr,
                                  const int32_t* col, int64_t B, int32_t mode, float threshold, const float* scale,
                                  const float* center, void* out_, void* ws, size_t ws_bytes, void* stream) {
    double* out = static_cast<double*>(out_);
    BGNN_REQUIRE(mode == 0 || mode == 1, "graph_metrics: mode %d unknown (0 static_stress, 1 static_disp)", mode);
    BGNN_REQUIRE(C >= 1 && C <= 8, "graph_metrics: C=%d unsupported (1..8)", C);
    BGNN_REQUIRE(C >= (mode == 0 ? 3 : 2), "graph_metrics: mode %d needs C >= %d, got %d", mode, mode == 0 ? 3 : 2, C);
    // a graph's element count n <= N C must fit the select's 32-bit ranks
    BGNN_REQUIRE(N >= 1 && N * (int64_t)C <= INT32_MAX && B >= 1 && B <= INT32_MAX,
                 "graph_metrics: N C and B must be in [1, 2^31)");
    BGNN_REQUIRE(pred && target && rowptr && col && out, "graph_metrics: null pointer");
    BGNN_REQUIRE(((uintptr_t)out & 7) == 0, "graph_metrics: out must be 8-byte aligned");
    BGNN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= bgnn_graph_metrics_ws_bytes(N, C, B),
                 "graph_metrics: workspace too small or not 8-byte aligned");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_graph_metrics_sums, dim3((unsigned)B), dim3(kMT), 0, s, pred, target, (int)C, rowptr, col,
                       (int)mode, threshold, scale, center, out);
    BGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_graph_quantiles, dim3((unsigned)B, 4), dim3(kQT), 0, s, pred, target, (int)C, rowptr, col,
                       (int)mode, threshold, 0.9f, scale, center, out);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}
