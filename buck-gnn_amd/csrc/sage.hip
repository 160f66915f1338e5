// The f32 GraphSAGE layer loop around the aggregation (Models/BuckGNN.py:430-444):
//   forward   x_next = Dropout(ReLU(BatchNorm1d(o)) + skip * x_prev): k_sage_apply (flat),
//             k_sage_apply_rows (row-blocked, with the range partials of x_next) and
//             k_sage_apply_pool (with the segment pool of x_next), over one element body
//             (apply_vec) and one argument struct filled and validated in one place (apply_args);
//   backward  of BatchNorm(train) and of SAGEConv's L2 normalize: the column sums
//             (k_sage_bwd_stats), then one wave per row (k_sage_bwd_rows; bgnn_l2norm_bwd is its
//             RELU = false form), launched from one place (launch_bwd_rows);
//   slots     every per-block partial [n_slots, 2, H] of these passes, of bn.hip and of the Linear
//             backward prep (mlp.hip) is summed by k_reduce_slots, in f64 and in a fixed order, so
//             results do not depend on scheduling; its BatchNorm form ends in bn_finalize.
//
// All kernels stream [N, H] fp32 rows with 16-B (float4) accesses.
#include <type_traits>

#include "common.h"
#include "ranges.h"
#include "seg_common.h"

namespace bgnn {

// ---------------------------------------------------------------------------
// What k_reduce_slots does with a channel's two slot sums. MODE 0 (SlotSums): out0 / out1 (either
// may be NULL) = the sums, or += with accumulate. MODE 1 (BnParams): bn_finalize.
struct SlotSums {
    float* out0;
    float* out1;
    int accumulate;
};

struct BnParams {
    int64_t count;         // rows behind the sums
    const float* kshift;   // NULL, or the per-channel shift k the sums were taken about
    const float* gamma;    // NULL: 1
    const float* beta;     // NULL: 0
    float eps, momentum;
    float* rmean;          // running statistics, updated when both are set and momentum > 0
    float* rvar;
    float* mean;
    float* invstd;
    float* scale;
    float* shift;
};

// BatchNorm1d finalize of channel c (train mode, torch semantics), in f64 from s0 = sum (x - k) and
// s1 = sum (x - k)^2 over `count` rows (k = kshift[c], or 0 without kshift):
//   mean = k + s0 / n,  var = max(s1 / n - (s0 / n)^2, 0)  (biased: the normalisation's),
//   invstd = 1 / sqrt(var + eps),  scale = gamma invstd,  shift = beta - mean scale,
//   running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with the
//   unbiased var n / (n - 1) (var itself when n = 1).
// (Every input is read before the first store: the struct's pointers carry no __restrict__.)
__device__ __forceinline__ void bn_finalize(const BnParams& P, int c, double s0, double s1) {
    const double k = P.kshift ? (double)P.kshift[c] : 0.0;
    const float g = P.gamma ? P.gamma[c] : 1.f;
    const float b = P.beta ? P.beta[c] : 0.f;
    const bool running = P.rmean && P.rvar && P.momentum > 0.f;
    const double rm = running ? (double)P.rmean[c] : 0.0, rv = running ? (double)P.rvar[c] : 0.0;
    const double n = (double)P.count;
    const double mu0 = s0 / n;
    double var = s1 / n - mu0 * mu0;
    if (var < 0.0) var = 0.0;
    const double mu = P.kshift ? k + mu0 : mu0;
    const double is = 1.0 / sqrt(var + (double)P.eps);
    P.mean[c] = (float)mu;
    P.invstd[c] = (float)is;
    P.scale[c] = (float)((double)g * is);
    P.shift[c] = (float)((double)b - mu * (double)g * is);
    if (running) {
        const double unb = P.count > 1 ? var * n / (n - 1.0) : var;
        P.rmean[c] = (float)((1.0 - P.momentum) * rm + P.momentum * mu);
        P.rvar[c] = (float)((1.0 - P.momentum) * rv + P.momentum * unb);
    }
}

// The reduction of [n_slots, 2, H] partial slots, one launch: a block owns 8 channels, its 256
// threads are 8 channels x 32 slot phases; each thread sums its slots ph, ph + 32, ... of both
// halves in f64 (eight loads in flight), then a fixed f64 tree over the 32 phases.
template <int MODE>
__global__ __launch_bounds__(256) void k_reduce_slots(const float* __restrict__ part, int n_slots, int H,
                                                      std::conditional_t<MODE == 0, SlotSums, BnParams> A) {
    constexpr int CPB = 8, NPH = 256 / CPB;   // channels per block, slot phases
    __shared__ double red[2][NPH][CPB];
    const int cl = threadIdx.x % CPB, ph = threadIdx.x / CPB;
    const int c = blockIdx.x * CPB + cl;
    const int64_t W = 2 * (int64_t)H;
    double s0 = 0.0, s1 = 0.0;
    if (c < H) {
        int sl = ph;
        for (; sl + 7 * NPH < n_slots; sl += 8 * NPH) {
            float a[8], b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                a[u] = part[(int64_t)(sl + u * NPH) * W + c];
                b[u] = part[(int64_t)(sl + u * NPH) * W + H + c];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s0 += (double)a[u];
                s1 += (double)b[u];
            }
        }
        for (; sl < n_slots; sl += NPH) {
            s0 += (double)part[(int64_t)sl * W + c];
            s1 += (double)part[(int64_t)sl * W + H + c];
        }
    }
    red[0][ph][cl] = s0;
    red[1][ph][cl] = s1;
    __syncthreads();
    for (int o = NPH / 2; o > 0; o >>= 1) {
        if (ph < o) {
            red[0][ph][cl] += red[0][ph + o][cl];
            red[1][ph][cl] += red[1][ph + o][cl];
        }
        __syncthreads();
    }
    if (ph != 0 || c >= H) return;
    s0 = red[0][0][cl];
    s1 = red[1][0][cl];
    if constexpr (MODE == 0) {
        if (A.out0) A.out0[c] = A.accumulate ? A.out0[c] + (float)s0 : (float)s0;
        if (A.out1) A.out1[c] = A.accumulate ? A.out1[c] + (float)s1 : (float)s1;
    } else {
        bn_finalize(A, c, s0, s1);
    }
}

template <int MODE>
int reduce_slots(const float* part, int n_slots, int H, const std::conditional_t<MODE == 0, SlotSums, BnParams>& A,
                 void* stream) {
    hipLaunchKernelGGL(k_reduce_slots<MODE>, dim3((H + 7) / 8), dim3(256), 0, as_stream(stream), part, n_slots, H, A);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

__global__ void k_bn_eval(int H, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                          const float* __restrict__ rmean, const float* __restrict__ rvar,
                          float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= H) return;
    const double is = 1.0 / sqrt((double)rvar[c] + (double)eps);
    const double g = gamma ? gamma[c] : 1.0;
    const double b = beta ? beta[c] : 0.0;
    scale[c] = (float)(g * is);
    shift[c] = (float)(b - (double)rmean[c] * g * is);
}

// ---------------------------------------------------------------------------
// The arguments the three forms of the apply pass share (filled by apply_args).
struct ApplyArgs {
    const float* o;
    const float* scale;   // NULL (with shift): no BatchNorm
    const float* shift;
    const float* xprev;
    uint32_t thr;         // dropout (common.h Dropout)
    float inv_keep;
    uint64_t seed;
    int32_t H, nt;        // nt: non-temporal x_next stores
    float* xn;
    uint32_t* amax;       // NULL, or where max |x_next| is folded
    int32_t skip;
};

// The element expression of x_next for one float4: y = o on entry, x_next on return;
// drop(relu(o*scale+shift) + skip*x_prev), i = the float4's index row * H/4 + c4 (the dropout hash's
// counter). One function for k_sage_apply, k_sage_apply_rows and k_sage_apply_pool: this file is
// compiled with the default contraction (o*scale+shift is an FMA), and all three must round alike.
__device__ __forceinline__ void x_next4(float (&y)[4], bool bn, const float4& sc, const float4& sh, bool skip,
                                        const float4& p, uint32_t thr, float inv_keep, uint64_t seed, uint64_t i) {
    if (bn) {
        y[0] = y[0] * sc.x + sh.x; y[1] = y[1] * sc.y + sh.y;
        y[2] = y[2] * sc.z + sh.z; y[3] = y[3] * sc.w + sh.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = fmaxf(y[k], 0.f);
    if (skip) {
        y[0] += p.x; y[1] += p.y; y[2] += p.z; y[3] += p.w;
    }
    if (thr) {
        const uint32_t keep = keep_bits4(seed, i, thr);
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = ((keep >> k) & 1u) ? y[k] * inv_keep : 0.f;
    }
}

// One float4 of the apply pass once its inputs are loaded (ov = o's float4 i, p = x_prev's when
// skip): y = x_next4; a kept vector is stored (when `store`) and |y| folded into the running max m.
__device__ __forceinline__ void apply_vec(const ApplyArgs& A, bool skip, const float4& ov, const float4& p,
                                          const float4& sc, const float4& sh, int64_t i, bool keep, bool store,
                                          float (&y)[4], uint32_t& m) {
    y[0] = ov.x; y[1] = ov.y; y[2] = ov.z; y[3] = ov.w;
    x_next4(y, A.scale != nullptr, sc, sh, skip, p, A.thr, A.inv_keep, A.seed, (uint64_t)i);
    if (!keep) return;
    if (store) store4(A.xn + 4 * i, y[0], y[1], y[2], y[3], A.nt);
#pragma unroll
    for (int k = 0; k < 4; ++k) m = max(m, __float_as_uint(y[k]) & 0x7fffffffu);
}

// x_prev's float4 i of a skip layer, zeros otherwise
__device__ __forceinline__ float4 load_xprev(const ApplyArgs& A, int64_t i) {
    return A.skip ? reinterpret_cast<const float4*>(A.xprev)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// x_next = drop(relu(o*scale+shift) + skip*x_prev). Grid-stride over the n4 = n_rows H / 4 float4s.
__global__ __launch_bounds__(256) void k_sage_apply(ApplyArgs A, int64_t n4, int rev) {
    const int H4 = A.H / 4;
    uint32_t m = 0;
    // rev = 1 (grid a multiple of 8): block b sweeps the eighth (b & 7) of the rows from its last
    // element down, so each eighth starts on the rows the aggregation (which sweeps the same
    // eighths upward, one per XCD) wrote last and are still in the Infinity Cache. Element-wise:
    // the result does not depend on the order.
    int64_t lo = 0, hi = n4, i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, st = (int64_t)gridDim.x * blockDim.x;
    if (rev) {
        const int64_t nr = n4 / H4, x = blockIdx.x & 7;
        lo = (nr * x / 8) * H4;
        hi = (nr * (x + 1) / 8) * H4;
        i0 = (int64_t)(blockIdx.x >> 3) * blockDim.x + threadIdx.x;
        st = (int64_t)(gridDim.x >> 3) * blockDim.x;
    }
    for (int64_t q = i0; q < hi - lo; q += st) {
        const int64_t i = rev ? hi - 1 - q : q;
        const float4 ov = reinterpret_cast<const float4*>(A.o)[i];   // (issued ahead of the 64-bit i % H4)
        const int c = (int)(i % H4) * 4;
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (A.scale) {
            sc = *reinterpret_cast<const float4*>(A.scale + c);
            sh = *reinterpret_cast<const float4*>(A.shift + c);
        }
        float y[4];
        apply_vec(A, A.skip != 0, ov, load_xprev(A, i), sc, sh, i, true, true, y, m);
    }
    if (A.amax) block_amax(A.amax, m);
}

// Row-blocked form of k_sage_apply with the range partials of x_next (bgnn_sage_apply given a
// `ranges` buffer; ranges.hip): block lb owns rows [lb rpb, (lb+1) rpb) of the bgnn_rows_slots
// partition, one wave per row (two rows in flight). The element-wise arithmetic, the dropout mask
// index and the store are k_sage_apply's, so x_next has the same bits. Like k_sage_apply's `rev`
// sweep, each XCD takes its share of the row blocks from the last one down and each block its rows
// from the last one down, so the first rows read are the ones the aggregation on that XCD wrote last
// (still in the Infinity Cache). Each wave adds its rows' x_next into its own LDS sum per range
// slot (BlockRanges; the slot is wave-uniform, so no register array is indexed); the 4 waves' sums
// are added in wave order into rpart[lb][slot][H] (every slot written, 0 when unused).
template <int NV>
__global__ __launch_bounds__(256) void k_sage_apply_rows(ApplyArgs A, int64_t n_rows, int64_t rpb,
                                                         const int32_t* __restrict__ ranges,
                                                         float* __restrict__ rpart) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lb = xcd_remap_rev(blockIdx.x, gridDim.x);
    const int64_t r0 = (int64_t)lb * rpb;
    const int64_t r1 = min(n_rows, r0 + rpb);
    const int H = A.H, H4 = H / 4;
    BlockRanges br;
    br.load(ranges, r0, r1);
    __shared__ float4 racc[4][kRangeSlots][128];
    int c4[NV];
    bool cok[NV];
    float4 sc[NV], sh[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        c4[v] = lane + 64 * v;
        cok[v] = c4[v] < H4;
        const int c = cok[v] ? 4 * c4[v] : 0;
        sc[v] = A.scale ? *reinterpret_cast<const float4*>(A.scale + c) : make_float4(1.f, 1.f, 1.f, 1.f);
        sh[v] = A.shift ? *reinterpret_cast<const float4*>(A.shift + c) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < kRangeSlots; ++q)
            if (cok[v]) racc[wave][q][c4[v]] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    uint32_t m = 0;
    auto row = [&](int64_t r) {
        const int sl = br.slot(r);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (!cok[v]) continue;
            const int64_t i = r * H4 + c4[v];
            const float4 ov = reinterpret_cast<const float4*>(A.o)[i];
            float y[4];
            apply_vec(A, A.skip != 0, ov, load_xprev(A, i), sc[v], sh[v], i, true, true, y, m);
            if (sl >= 0) {
                float4 t = racc[wave][sl][c4[v]];
                t.x += y[0]; t.y += y[1]; t.z += y[2]; t.w += y[3];
                racc[wave][sl][c4[v]] = t;
            }
        }
    };
    int64_t r = r1 - 1 - wave;
    for (; r - 4 >= r0; r -= 8) {
        row(r);
        row(r - 4);
    }
    if (r >= r0) row(r);
    if (A.amax) block_amax(A.amax, m);
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(rpart + (int64_t)lb * kRangeSlots * H);
    for (int c = threadIdx.x; c < kRangeSlots * H4; c += 256) {
        const int q = c / H4, cc = c % H4;
        const float4 a0 = racc[0][q][cc], a1 = racc[1][q][cc], a2 = racc[2][q][cc], a3 = racc[3][q][cc];
        dst[c] = make_float4((a0.x + a1.x) + (a2.x + a3.x), (a0.y + a1.y) + (a2.y + a3.y),
                             (a0.z + a1.z) + (a2.z + a3.z), (a0.w + a1.w) + (a2.w + a3.w));
    }
}

// ---------------------------------------------------------------------------
// k_sage_apply with the segment pool of x_next (bgnn_sage_apply_pool): the gather of spmm.hip's
// k_seg_chunk / k_seg_light over the pooling CSR, whose "source row" col[e] is formed from o on the
// fly (x_next4) instead of being read from a stored x_next. A wave owns one work item and one
// column tile of 64 float4s; the `ct` tiles of an item (2 at H = 512) sit in one block, so a block
// holds 4 / ct items. (Measured on the cfg2 pool, 1,264 chunks of 64 rows, H = 512: 41.7 us per
// launch without amax against the 69 + 33 + 5 us of k_sage_apply, k_seg_chunk and the empty
// light-row sweep it replaces. max |x_next| goes through block_amax, one atomic per block: with one
// per wave, 2,528 atomics on one address, the launch took 58 us whatever the load schedule -- a
// whole row per wave, or the next batch's loads issued ahead, measured the same -- and 17 us less
// without them; the dropout hash costs 5 us of the rest.)
// Items [0, n_chunks) are the chunks of the heavy segments (-> partial[c, :], finished by
// k_seg_combine), items [n_chunks, n_chunks + n_light) the segments themselves, of which the light
// ones (deg <= chunk) are finished here: sum, then * inv_deg for MEAN, as spmm.hip's store_plain.
// The rows of a range are loaded 8 at a time (gather_range's batching: a load schedule only) and
// added one by one in CSR order with a rounded add (__fadd_rn: no contraction with the dropout
// scale), so the sums have the bits of bgnn_spmm_fwd over the stored rows. x_next (optional) is
// stored on the way: every row lies in exactly one segment.
struct ApplyPoolArgs : ApplyArgs {   // (skip is the kernel's template argument; xn may be NULL)
    const int32_t* rowptr;
    const int32_t* col;
    const int32_t* heavy_row;
    const int32_t* heavy_chunk0;
    const int32_t* chunk_heavy;
    int32_t n_chunks, chunk, mean;
    int32_t ct;        // column tiles per block (1, 2 or 4)
    int64_t n_light;   // segments swept for light rows: n_seg, or 0 when every segment is heavy
    float* partial;    // [n_chunks, H]
    float* out;        // [n_seg, H]
};

// One batch of the gather: up to 8 rows of the range in flight (slots >= nvalid re-read the first
// row and are not added or stored), then x_next of each row and the adds, in order.
template <bool SKIP>
__device__ __forceinline__ void apply_pool_batch(const ApplyPoolArgs& A, float (&acc)[4], uint32_t& m, int32_t e,
                                                 int32_t nvalid, int c4, bool cok, const float4& sc,
                                                 const float4& sh) {
    constexpr int U = 8;
    const int H4 = A.H / 4;
    int64_t i[U];
#pragma unroll
    for (int u = 0; u < U; ++u) i[u] = (int64_t)A.col[e + (u < nvalid ? u : 0)] * H4 + c4;
    float4 ov[U], pv[SKIP ? U : 1];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        ov[u] = reinterpret_cast<const float4*>(A.o)[i[u]];
        if constexpr (SKIP) pv[u] = reinterpret_cast<const float4*>(A.xprev)[i[u]];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const bool ok = cok && u < nvalid;
        float y[4];
        apply_vec(A, SKIP, ov[u], SKIP ? pv[u] : make_float4(0.f, 0.f, 0.f, 0.f), sc, sh, i[u], ok, A.xn != nullptr, y,
                  m);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], ok ? y[k] : 0.f);
    }
}

template <bool SKIP>
__global__ __launch_bounds__(256) void k_sage_apply_pool(ApplyPoolArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int H4 = A.H / 4;
    const int tile = blockIdx.y * A.ct + wave % A.ct;
    const int64_t w = (int64_t)blockIdx.x * (4 / A.ct) + wave / A.ct;
    // (a wave without work -- a tile past the row, an item past the last, a heavy segment's own item
    // -- keeps an empty range and stays for block_amax's barrier)
    bool live = tile * 64 < H4;   // (wave-uniform)
    int32_t beg = 0, end = 0;
    int64_t seg = -1;
    if (live && w < A.n_chunks) {
        const int32_t h = A.chunk_heavy[w];
        const int32_t r = A.heavy_row[h];
        const int32_t k = (int32_t)(w - A.heavy_chunk0[h]);
        beg = A.rowptr[r] + k * A.chunk;
        end = min(beg + A.chunk, A.rowptr[r + 1]);
    } else if (live) {
        seg = w - A.n_chunks;
        live = seg < A.n_light;
        if (live) {
            beg = A.rowptr[seg];
            end = A.rowptr[seg + 1];
            if (end - beg > A.chunk) {   // heavy segment: its chunks above + k_seg_combine
                live = false;
                end = beg;
            }
        }
    }
    const bool cok = tile * 64 + lane < H4;
    const int c4 = cok ? tile * 64 + lane : 0;   // (lanes past the row read column 0 and keep nothing)
    const float4 sc = A.scale ? *reinterpret_cast<const float4*>(A.scale + 4 * c4) : make_float4(1.f, 1.f, 1.f, 1.f);
    const float4 sh = A.shift ? *reinterpret_cast<const float4*>(A.shift + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t m = 0;
    int32_t e = beg;
    for (; e + 8 <= end; e += 8) apply_pool_batch<SKIP>(A, acc, m, e, 8, c4, cok, sc, sh);
    if (e < end) apply_pool_batch<SKIP>(A, acc, m, e, end - e, c4, cok, sc, sh);
    if (A.amax) block_amax(A.amax, m);   // one atomic per block: same-address atomics serialise in L2
    if (!live || !cok) return;
    const float s = (seg >= 0 && A.mean) ? inv_deg(end - beg) : 1.f;
    float* dst = seg >= 0 ? A.out + seg * A.H : A.partial + w * A.H;
    *reinterpret_cast<float4*>(dst + 4 * c4) = make_float4(acc[0] * s, acc[1] * s, acc[2] * s, acc[3] * s);
}

// gp = g / max(count, 1) per segment row (bgnn_pool_grad_scale): IEEE division
__global__ __launch_bounds__(256) void k_pool_grad_scale(const float* __restrict__ g, const int32_t* __restrict__ rowptr,
                                                         int64_t n, int H, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t s = i / H;
    const int32_t d = rowptr[s + 1] - rowptr[s];
    out[i] = __fdiv_rn(g[i], (float)(d > 0 ? d : 1));
}

// Backward pass 1: partial sums over rows of g2 and g2*xhat per channel.
// Thread layout: H4 = H/4 threads per row, 256/H4 rows per step.
__global__ __launch_bounds__(256) void k_sage_bwd_stats(const float* __restrict__ g,
                                                        const int64_t* __restrict__ g_rows,
                                                        const float* __restrict__ o,
                                                        const float* __restrict__ scale,
                                                        const float* __restrict__ shift,
                                                        const float* __restrict__ mean,
                                                        const float* __restrict__ invstd, uint32_t thr,
                                                        float inv_keep, uint64_t seed, int64_t n_rows, int H,
                                                        int64_t rows_per_block, float* __restrict__ part) {
    const int H4 = H / 4;
    const int rpi = 256 / H4;                 // rows per iteration
    const int t = threadIdx.x;
    const int c4 = t % H4, ph = t / H4;
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t r0 = (int64_t)lb * rows_per_block;
    const int64_t r1 = min(n_rows, r0 + rows_per_block);
    float s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    const int c = c4 * 4;
    if (ph < rpi) {
        const float4 sc = *reinterpret_cast<const float4*>(scale + c);
        const float4 sh = *reinterpret_cast<const float4*>(shift + c);
        const float4 mu = *reinterpret_cast<const float4*>(mean + c);
        const float4 is = *reinterpret_cast<const float4*>(invstd + c);
        const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
        const float muv[4] = {mu.x, mu.y, mu.z, mu.w}, isv[4] = {is.x, is.y, is.z, is.w};
        for (int64_t r = r0 + ph; r < r1; r += rpi) {
            const int64_t i4 = r * H4 + c4;
            const float4 gv = reinterpret_cast<const float4*>(g)[(g_rows ? g_rows[r] : r) * H4 + c4];
            const float4 ov = reinterpret_cast<const float4*>(o)[i4];
            float gg[4] = {gv.x, gv.y, gv.z, gv.w}, oo[4] = {ov.x, ov.y, ov.z, ov.w};
            uint32_t m = 0xF;
            if (thr) m = keep_bits4(seed, (uint64_t)i4, thr);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float g1 = ((m >> k) & 1u) ? gg[k] * (thr ? inv_keep : 1.f) : 0.f;
                const float yp = oo[k] * scv[k] + shv[k];
                const float g2 = yp > 0.f ? g1 : 0.f;
                const float xh = (oo[k] - muv[k]) * isv[k];
                s0[k] += g2;
                s1[k] += g2 * xh;
            }
        }
    }
    block_col_partials(s0, s1, H, part + (int64_t)lb * 2 * H);   // (over the row phases: rpi <= 2 at H = 512)
}

// Backward pass 2: one wave per row (H <= 512, NV float4 per lane). RELU = false: the layer
// is the bare SAGEConv(normalize=True) of the per-op path (g is dL/do; no ReLU mask, no BN,
// no dropout), i.e. only the L2-normalize backward.
// The parameters stay positional, spread from BwdRowsArgs in one place (launch_bwd_rows): the
// pointers of an argument struct passed by value carry no __restrict__, and without it the
// wave-uniform loads in the row loop (g_rows[r], nrm[r], the rowptr pairs) are no longer scalar
// loads but vector loads whose s_waitcnt vmcnt(0) also waits for the row prefetched one ahead.
template <int NV, bool RELU = true, bool RANGES = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_sage_bwd_rows(
    const float* __restrict__ g, const int64_t* __restrict__ g_rows, const float* __restrict__ o,
    const float* __restrict__ nrm, const float* __restrict__ scale, const float* __restrict__ shift, const float* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ invstd, const float* __restrict__ sum_g2,
    const float* __restrict__ sum_g2xhat, uint32_t thr, float inv_keep, uint64_t seed, int skip,
    int64_t n_rows, int H, int64_t rows_per_block, float* __restrict__ dh, int64_t lddh,
    float* __restrict__ gskip, float* __restrict__ part, uint32_t* __restrict__ amax, int nt,
    const int32_t* __restrict__ w_rowptr, int w_mode, int rev, const int32_t* __restrict__ ranges,
    const int32_t* __restrict__ rw_rowptr, float* __restrict__ rpart) {
    const int lane = threadIdx.x & 63;
    uint32_t tmax = 0;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lb = xcd_remap(blockIdx.x, gridDim.x);
    const int64_t r0 = (int64_t)lb * rows_per_block;
    const int64_t r1 = min(n_rows, r0 + rows_per_block);
    const int H4 = H / 4;
    const bool bn = (mean != nullptr);
    const float invn = 1.f / (float)(n_rows > 0 ? n_rows : 1);
    int cpos[NV];
    bool cok[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        cpos[v] = (lane + 64 * v) * 4;
        cok[v] = cpos[v] < H;
    }
    // per-channel constants in LDS (read back per row as float4), not VGPRs: 56 registers
    // fewer keep 4 waves per SIMD with two rows in flight per wave.
    // cst[0..6][c] = scale, shift, kA, kB, kC, mean, invstd with
    // do = gamma*invstd/N * (N*g2 - sum_g2 - xhat*sum_g2xhat) = kA g2 - kB - xhat kC
    __shared__ __attribute__((aligned(16))) float cst[7][512];
    for (int c = threadIdx.x; c < H; c += 256) {
        cst[0][c] = scale ? scale[c] : 1.f;
        cst[1][c] = shift ? shift[c] : 0.f;
        if (bn) {
            const float gi = (gamma ? gamma[c] : 1.f) * invstd[c];
            cst[2][c] = gi;
            cst[3][c] = gi * sum_g2[c] * invn;
            cst[4][c] = gi * sum_g2xhat[c] * invn;
            cst[5][c] = mean[c];
            cst[6][c] = invstd[c];
        } else {
            cst[2][c] = 1.f; cst[3][c] = 0.f; cst[4][c] = 0.f; cst[5][c] = 0.f; cst[6][c] = 0.f;
        }
    }
    __syncthreads();
    float db[NV][4], dw[NV][4];   // sums of dh and of w_r * dh (w_mode: row weights from w_rowptr)
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int k = 0; k < 4; ++k) db[v][k] = dw[v][k] = 0.f;
    // end-of-block reductions; RANGES: first each wave's own sums of rw * dh per range slot
    // (ranges.h; the transposed aggregation of range rows: a super node's dz_l row; rw = 1 or
    // 1 / max(deg_fwd, 1)), kept in LDS rather than registers (the slot is wave-uniform; a register
    // array per slot would cost this kernel a wave per SIMD)
    __shared__ __attribute__((aligned(16))) float red[4][RANGES ? kRangeSlots : 2][512];
    BlockRanges br;
    if constexpr (RANGES) {
        br.load(ranges, r0, r1);
#pragma unroll
        for (int q = 0; q < kRangeSlots; ++q)
#pragma unroll
            for (int v = 0; v < NV; ++v)
                if (cok[v]) *reinterpret_cast<float4*>(&red[wave][q][cpos[v]]) = make_float4(0.f, 0.f, 0.f, 0.f);
    }

    // the next row's g and o rows are loaded one row ahead (two rows in flight per wave: the
    // kernel is latency-bound on these loads, not bandwidth-bound); same rows, same order
    float4 gn[NV], on[NV];
    auto fetch = [&](int64_t rr) {
        const int64_t gr = g_rows ? g_rows[rr] : rr;   // (g_rows: row rr's gradient is row g_rows[rr] of g)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const int64_t i4 = rr * H4 + (cok[v] ? (cpos[v] >> 2) : 0);
            gn[v] = reinterpret_cast<const float4*>(g)[gr * H4 + (cok[v] ? (cpos[v] >> 2) : 0)];
            on[v] = reinterpret_cast<const float4*>(o)[i4];
        }
    };
    // rev = 1: the block's rows are walked from its last row down (wave w takes r1-1-w, r1-5-w, ...),
    // so the first rows read are the ones bgnn_sage_bwd_stats read last over the same block ranges
    // and that are still in the Infinity Cache. Only the summation order of the dh partials changes.
    const int64_t nr = r1 - r0 - wave;
    const int64_t cnt = nr > 0 ? (nr + 3) / 4 : 0;
    const int64_t rfirst = rev ? r1 - 1 - wave : r0 + wave;
    const int64_t rstep = rev ? -4 : 4;
    if (cnt > 0) fetch(rfirst);
    for (int64_t j = 0; j < cnt; ++j) {
        const int64_t r = rfirst + j * rstep;
        float ov[NV][4], dov[NV][4], g1v[NV][4];
        float4 gc[NV], oc[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) { gc[v] = gn[v]; oc[v] = on[v]; }
        if (j + 1 < cnt) fetch(r + rstep);
        float dot = 0.f;
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (!cok[v]) {
#pragma unroll
                for (int k = 0; k < 4; ++k) ov[v][k] = dov[v][k] = g1v[v][k] = 0.f;
                continue;
            }
            const int64_t i4 = r * H4 + (cpos[v] >> 2);
            const float4 gv = gc[v];
            const float4 o4 = oc[v];
            const float gg[4] = {gv.x, gv.y, gv.z, gv.w};
            ov[v][0] = o4.x; ov[v][1] = o4.y; ov[v][2] = o4.z; ov[v][3] = o4.w;
            uint32_t m = 0xF;
            if (thr) m = keep_bits4(seed, (uint64_t)i4, thr);
            float cv[7][4];
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const float4 t4 = *reinterpret_cast<const float4*>(&cst[q][cpos[v]]);
                cv[q][0] = t4.x; cv[q][1] = t4.y; cv[q][2] = t4.z; cv[q][3] = t4.w;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float g1 = ((m >> k) & 1u) ? gg[k] * (thr ? inv_keep : 1.f) : 0.f;
                g1v[v][k] = g1;
                const float yp = ov[v][k] * cv[0][k] + cv[1][k];
                const float g2 = (!RELU || yp > 0.f) ? g1 : 0.f;
                float d;
                if (bn) {
                    const float xh = (ov[v][k] - cv[5][k]) * cv[6][k];
                    d = cv[2][k] * g2 - cv[3][k] - xh * cv[4][k];
                } else {
                    d = g2;
                }
                dov[v][k] = d;
                dot += ov[v][k] * d;
            }
        }
        dot = group_sum(dot, kWave);
        const float n = nrm[r];
        const bool through = n >= 1e-12f;
        const float rn = through ? 1.f / n : 1e12f;
        float wr = 0.f;
        if (w_mode) {
            const int32_t d = w_rowptr[r + 1] - w_rowptr[r];
            wr = (w_mode == 1) ? (float)d : (d > 0 ? 1.f : 0.f);
        }
        int sl = -1;
        float rw = 1.f;
        if constexpr (RANGES) {
            sl = br.slot(r);
            if (rw_rowptr) {   // (spmm.hip inv_deg: the MEAN transposed weight)
                const int32_t d = rw_rowptr[r + 1] - rw_rowptr[r];
                rw = __frcp_rn((float)(d > 0 ? d : 1));
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (!cok[v]) continue;
            float out[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                out[k] = through ? (dov[v][k] - ov[v][k] * dot) * rn : dov[v][k] * rn;
                db[v][k] += out[k];
                dw[v][k] = fmaf(wr, out[k], dw[v][k]);
                tmax = max(tmax, __float_as_uint(out[k]) & 0x7fffffffu);
            }
            if constexpr (RANGES) {
                if (sl >= 0) {
                    float4* a = reinterpret_cast<float4*>(&red[wave][sl][cpos[v]]);
                    float4 t = *a;
                    t.x += rw_rowptr ? __fmul_rn(out[0], rw) : out[0];
                    t.y += rw_rowptr ? __fmul_rn(out[1], rw) : out[1];
                    t.z += rw_rowptr ? __fmul_rn(out[2], rw) : out[2];
                    t.w += rw_rowptr ? __fmul_rn(out[3], rw) : out[3];
                    *a = t;
                }
            }
            store4(dh + r * lddh + cpos[v], out[0], out[1], out[2], out[3], nt);
            if (skip)
                store4(gskip + r * H + cpos[v], g1v[v][0], g1v[v][1], g1v[v][2], g1v[v][3], nt);
        }
    }
    if (amax) block_amax(amax, tmax);
    if constexpr (RANGES) {   // the range slots first; then the same LDS for db / dw
        __syncthreads();
        float* rd = rpart + (int64_t)lb * kRangeSlots * H;
        for (int c = threadIdx.x; c < kRangeSlots * H; c += 256) {
            const int q = c / H, cc = c % H;
            rd[c] = wave_tree(red, q, cc);
        }
        __syncthreads();
    }
#pragma unroll
    for (int v = 0; v < NV; ++v)
        if (cok[v])
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                red[wave][0][cpos[v] + k] = db[v][k];
                red[wave][1][cpos[v] + k] = dw[v][k];
            }
    __syncthreads();
    float* dst = part + (int64_t)lb * 2 * H;
    for (int c = threadIdx.x; c < H; c += 256) {
        dst[c] = wave_tree(red, 0, c);
        dst[H + c] = wave_tree(red, 1, c);
    }
}

static int g_rows_nt = 0;
void set_rows_nt(int on) { g_rows_nt = on ? 1 : 0; }
int rows_nt() { return g_rows_nt; }
static int g_rows_rev = 1;   // bit 0 on: bwd_rows 107.5 -> 92.9 us in the cfg2 step (profiles/r03_ab_rows_rev.txt)
void set_rows_rev(int on) { g_rows_rev = on & 15; }
int rows_rev() { return g_rows_rev; }

// The checks and the arguments that bgnn_sage_apply and bgnn_sage_apply_pool share; `name` is the
// entry point's, the prefix of its messages. need_xn: x_next must be set (the pool form may drop it).
static int apply_args(ApplyArgs& A, const char* name, const float* o, const float* scale, const float* shift,
                      const float* x_prev, int32_t skip, float p, uint64_t seed, int64_t n_rows, int32_t H,
                      float* x_next, float* amax, bool need_xn) {
    BGNN_REQUIRE(H > 0 && H % 4 == 0, "%s: H must be a multiple of 4", name);
    BGNN_REQUIRE(n_rows >= 0, "%s: negative n_rows", name);
    BGNN_REQUIRE(n_rows == 0 || (o && (x_next || !need_xn)), "%s: null o%s", name, need_xn ? " / x_next" : "");
    BGNN_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout p must be in [0, 1)", name);
    BGNN_REQUIRE((scale == nullptr) == (shift == nullptr), "%s: scale/shift must both be set or NULL", name);
    BGNN_REQUIRE(!skip || x_prev, "%s: skip requires x_prev", name);
    BGNN_REQUIRE(aligned16(o) && aligned16(x_next) && (!x_prev || aligned16(x_prev)) &&
                     (!scale || (aligned16(scale) && aligned16(shift))),
                 "%s: pointers must be 16-byte aligned", name);
    const Dropout d = dropout_of(p);
    A.o = o; A.scale = scale; A.shift = shift; A.xprev = x_prev;
    A.thr = d.thr;
    A.inv_keep = d.inv_keep;
    A.seed = seed;
    A.H = H;
    A.nt = rows_nt();
    A.xn = x_next;
    A.amax = reinterpret_cast<uint32_t*>(amax);
    A.skip = skip;
    return BGNN_OK;
}

// bgnn_sage_bwd_rows' arguments as its two callers fill them (include/bgnn.h; part = partial_db,
// rw_rowptr / rpart = range_w_rowptr / range_partial). Zero: no BatchNorm, no dropout (inv_keep
// unread), no skip, no row weights, no ranges.
struct BwdRowsArgs {
    const float* g;
    const int64_t* g_rows;
    const float* o;
    const float* nrm;
    const float* scale;
    const float* shift;
    const float* gamma;
    const float* mean;
    const float* invstd;
    const float* sum_g2;
    const float* sum_g2xhat;
    Dropout drop;
    uint64_t seed;
    int32_t skip;
    int64_t n_rows;
    int32_t H;
    float* dh;
    int64_t lddh;
    float* gskip;
    float* part;
    float* amax;
    const int32_t* w_rowptr;
    int32_t w_mode;
    const int32_t* ranges;
    const int32_t* rw_rowptr;
    float* rpart;
};

// The launch of k_sage_bwd_rows (bgnn_sage_bwd_rows; relu = false: bgnn_l2norm_bwd, which has no
// ranges): the row partition, the store policy and the sweep direction, and the instantiation.
static int launch_bwd_rows(const BwdRowsArgs& A, bool relu, void* stream) {
    int64_t rpb = 0;
    const int64_t blocks = rows_grid(A.n_rows, 4, &rpb);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), A.g, A.g_rows, A.o, A.nrm,
                           A.scale, A.shift, A.gamma, A.mean, A.invstd, A.sum_g2, A.sum_g2xhat, A.drop.thr,
                           A.drop.inv_keep, A.seed, A.skip, A.n_rows, A.H, rpb, A.dh, A.lddh, A.gskip, A.part,
                           reinterpret_cast<uint32_t*>(A.amax), rows_nt(), A.w_rowptr, A.w_mode, rows_rev() & 1, A.ranges,
                           A.rw_rowptr, A.rpart);
    };
    const bool wide = A.H > 256;   // two float4 per lane
    if (!relu) wide ? launch(k_sage_bwd_rows<2, false>) : launch(k_sage_bwd_rows<1, false>);
    else if (A.ranges) wide ? launch(k_sage_bwd_rows<2, true, true>) : launch(k_sage_bwd_rows<1, true, true>);
    else wide ? launch(k_sage_bwd_rows<2>) : launch(k_sage_bwd_rows<1>);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_reduce_partials(const float* partial, int32_t n_slots, int32_t H, float* out0, float* out1,
                                    int32_t accumulate, void* stream) {
    BGNN_REQUIRE(partial && H > 0 && n_slots >= 0, "reduce_partials: bad args");
    return reduce_slots<0>(partial, n_slots, H, SlotSums{out0, out1, accumulate}, stream);
}

extern "C" int bgnn_bn_finalize(const float* bn_partial, int32_t n_slots, int32_t H, int64_t count,
                                const float* gamma, const float* beta, float eps, float momentum,
                                float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                                float* shift, void* stream) {
    BGNN_REQUIRE(bn_partial && H > 0 && count > 0 && mean && invstd && scale && shift, "bn_finalize: bad args");
    return reduce_slots<1>(bn_partial, n_slots, H,
                           BnParams{count, nullptr, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd,
                                    scale, shift},
                           stream);
}

extern "C" int bgnn_bn_finalize_shifted(const float* bn_partial, int32_t n_slots, int32_t H, int64_t count,
                                        const float* kshift, const float* gamma, const float* beta, float eps,
                                        float momentum, float* running_mean, float* running_var, float* mean,
                                        float* invstd, float* scale, float* shift, void* stream) {
    BGNN_REQUIRE(bn_partial && kshift && H > 0 && count > 0 && mean && invstd && scale && shift,
                 "bn_finalize_shifted: bad args");
    return reduce_slots<1>(bn_partial, n_slots, H,
                           BnParams{count, kshift, gamma, beta, eps, momentum, running_mean, running_var, mean, invstd,
                                    scale, shift},
                           stream);
}

extern "C" int bgnn_bn_eval_coeffs(int32_t H, const float* gamma, const float* beta, float eps,
                                   const float* running_mean, const float* running_var, float* scale, float* shift,
                                   void* stream) {
    BGNN_REQUIRE(H > 0 && running_mean && running_var && scale && shift, "bn_eval_coeffs: bad args");
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_bn_eval, dim3((H + 255) / 256), dim3(256), 0, s, H, gamma, beta, eps, running_mean,
                       running_var, scale, shift);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

extern "C" int bgnn_sage_apply(const float* o, const float* scale, const float* shift, const float* x_prev,
                               int32_t skip, float p, uint64_t seed, int64_t n_rows, int32_t H, float* x_next,
                               float* amax, const int32_t* ranges, float* range_partial, void* stream) {
    ApplyArgs A{};
    if (const int e = apply_args(A, "sage_apply", o, scale, shift, x_prev, skip, p, seed, n_rows, H, x_next, amax, true))
        return e;
    BGNN_REQUIRE(!ranges || (range_partial && aligned16(range_partial) && H <= 512),
                 "sage_apply: ranges need a 16-B aligned range_partial and H <= 512");
    if (n_rows == 0) return BGNN_OK;
    hipStream_t s = as_stream(stream);
    if (ranges) {   // row-blocked form with the range partials (the same x_next)
        int64_t rpb = 0;
        const int64_t blocks = rows_slots_of(n_rows, &rpb);
        hipLaunchKernelGGL(H > 256 ? k_sage_apply_rows<2> : k_sage_apply_rows<1>, dim3((unsigned)blocks), dim3(256), 0, s,
                           A, n_rows, rpb, ranges, range_partial);
    } else {
        const int64_t n4 = n_rows * (H / 4);
        int64_t blocks = (n4 + 255) / 256;
        if (blocks > 4096) blocks = 4096;
        const int rev = (rows_rev() & 2) ? 1 : 0;
        if (rev) blocks = (blocks + 7) / 8 * 8;
        hipLaunchKernelGGL(k_sage_apply, dim3((unsigned)blocks), dim3(256), 0, s, A, n4, rev);
    }
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

extern "C" int bgnn_sage_apply_pool(const float* o, const float* scale, const float* shift, const float* x_prev,
                                    int32_t skip, float p, uint64_t seed, int64_t n_rows, int32_t H, float* x_next,
                                    float* amax, const bgnn_csr_t* pool, int32_t reduce, float* partial,
                                    float* pooled, void* stream) {
    ApplyPoolArgs A{};
    if (const int e =
            apply_args(A, "sage_apply_pool", o, scale, shift, x_prev, skip, p, seed, n_rows, H, x_next, amax, false))
        return e;
    BGNN_REQUIRE(pool && pool->rowptr, "sage_apply_pool: null pool csr");
    BGNN_REQUIRE(reduce == BGNN_REDUCE_SUM || reduce == BGNN_REDUCE_MEAN, "sage_apply_pool: reduce must be sum/mean");
    BGNN_REQUIRE(pool->n_rows >= 0, "sage_apply_pool: negative segment count");
    BGNN_REQUIRE(pool->nnz == n_rows, "sage_apply_pool: the pool must list each of the n_rows rows once (nnz = %lld)",
                 (long long)pool->nnz);
    BGNN_REQUIRE(n_rows == 0 || pool->col, "sage_apply_pool: null col");
    BGNN_REQUIRE(pool->n_rows == 0 || pooled, "sage_apply_pool: null pooled");
    BGNN_REQUIRE(pool->n_chunks <= 0 ||
                     (partial && pool->chunk > 0 && pool->heavy_row && pool->heavy_chunk0 && pool->chunk_heavy),
                 "sage_apply_pool: heavy segments need partial and the CSR's chunk plan");
    BGNN_REQUIRE(aligned16(partial) && aligned16(pooled), "sage_apply_pool: partial / pooled must be 16-byte aligned");
    if (n_rows == 0) return BGNN_OK;
    hipStream_t s = as_stream(stream);
    A.rowptr = pool->rowptr; A.col = pool->col;
    A.heavy_row = pool->heavy_row; A.heavy_chunk0 = pool->heavy_chunk0; A.chunk_heavy = pool->chunk_heavy;
    A.n_chunks = pool->n_chunks > 0 ? pool->n_chunks : 0;
    A.chunk = (A.n_chunks > 0 && pool->chunk > 0) ? pool->chunk : 0x7fffffff;   // no chunk plan: every segment light
    A.mean = reduce == BGNN_REDUCE_MEAN;
    // no light-row items when the plan says every segment is heavy (a batch of large graphs)
    A.n_light = (A.n_chunks > 0 && pool->n_heavy == pool->n_rows) ? 0 : pool->n_rows;
    A.partial = partial;
    A.out = pooled;
    const int64_t items = A.n_chunks + A.n_light;
    const int tiles = (H / 4 + 63) / 64;
    A.ct = tiles <= 2 ? tiles : 4;   // (a divisor of the block's 4 waves; a tile past the row leaves at once)
    const int ipb = 4 / A.ct;        // items per block
    const dim3 grid((unsigned)((items + ipb - 1) / ipb), (unsigned)((tiles + A.ct - 1) / A.ct));
    hipLaunchKernelGGL(skip ? k_sage_apply_pool<true> : k_sage_apply_pool<false>, grid, dim3(256), 0, s, A);
    BGNN_CHECK_LAUNCH();
    if (A.n_chunks > 0) return seg_combine_plain(pool, H, reduce, partial, pooled, s);
    return BGNN_OK;
}

extern "C" int bgnn_pool_grad_scale(const float* g, const int32_t* rowptr, int64_t segments, int32_t H, float* out,
                                    void* stream) {
    BGNN_REQUIRE(segments >= 0 && H > 0, "pool_grad_scale: bad sizes");
    BGNN_REQUIRE(segments == 0 || (g && rowptr && out), "pool_grad_scale: null pointer");
    if (segments == 0) return BGNN_OK;
    const int64_t n = segments * H;
    hipLaunchKernelGGL(k_pool_grad_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), g, rowptr,
                       n, H, out);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

extern "C" int32_t bgnn_rows_slots(int64_t n_rows) {
    int64_t rpb = 0;
    return (int32_t)rows_grid(n_rows, 4, &rpb);
}

extern "C" int bgnn_sage_bwd_stats(const float* g, const int64_t* g_rows, const float* o, const float* scale,
                                   const float* shift,
                                   const float* mean, const float* invstd, float p, uint64_t seed, int64_t n_rows,
                                   int32_t H, float* partial2, void* stream) {
    BGNN_REQUIRE(H > 0 && H % 4 == 0 && H <= 1024, "sage_bwd_stats: H=%d unsupported", H);
    BGNN_REQUIRE(n_rows >= 0, "sage_bwd_stats: negative n_rows");
    BGNN_REQUIRE(g && o && scale && shift && mean && invstd && partial2, "sage_bwd_stats: null pointer");
    BGNN_REQUIRE(aligned16(g) && aligned16(o) && aligned16(scale) && aligned16(shift) && aligned16(mean) &&
                     aligned16(invstd) && aligned16(partial2),
                 "sage_bwd_stats: pointers must be 16-byte aligned");
    hipStream_t s = as_stream(stream);
    int64_t rpb = 0;
    const int64_t blocks = rows_grid(n_rows, 4, &rpb);
    const Dropout d = dropout_of(p);
    hipLaunchKernelGGL(k_sage_bwd_stats, dim3((unsigned)blocks), dim3(256), 0, s, g, g_rows, o, scale, shift, mean, invstd,
                       d.thr, d.inv_keep, seed, n_rows, H, rpb, partial2);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

extern "C" int bgnn_sage_bwd_rows(const float* g, const int64_t* g_rows, const float* o, const float* nrm,
                                  const float* scale,
                                  const float* shift, const float* gamma, const float* mean, const float* invstd,
                                  const float* sum_g2, const float* sum_g2xhat, float p, uint64_t seed,
                                  int32_t skip, int64_t n_rows, int32_t H, float* dh, int64_t lddh, float* gskip,
                                  float* partial_db, float* amax, const int32_t* w_rowptr, int32_t w_mode,
                                  const int32_t* ranges, const int32_t* range_w_rowptr, float* range_partial,
                                  void* stream) {
    BGNN_REQUIRE(H > 0 && H % 4 == 0 && H <= 512, "sage_bwd_rows: H=%d unsupported", H);
    BGNN_REQUIRE(n_rows >= 0, "sage_bwd_rows: negative n_rows");
    BGNN_REQUIRE(g && o && nrm && dh && partial_db, "sage_bwd_rows: null pointer");
    BGNN_REQUIRE(w_mode >= 0 && w_mode <= 2 && (w_mode == 0 || w_rowptr), "sage_bwd_rows: bad row weights");
    BGNN_REQUIRE(lddh >= H && lddh % 4 == 0, "sage_bwd_rows: bad lddh");
    BGNN_REQUIRE(!skip || gskip, "sage_bwd_rows: skip requires gskip");
    BGNN_REQUIRE(!mean || (invstd && sum_g2 && sum_g2xhat), "sage_bwd_rows: BN stats incomplete");
    BGNN_REQUIRE(aligned16(g) && aligned16(o) && aligned16(dh) && (!gskip || aligned16(gskip)) && aligned16(partial_db),
                 "sage_bwd_rows: pointers must be 16-byte aligned");
    BGNN_REQUIRE(!ranges || (range_partial && aligned16(range_partial)), "sage_bwd_rows: ranges need range_partial");
    BwdRowsArgs A{};
    A.g = g; A.g_rows = g_rows; A.o = o; A.nrm = nrm;
    A.scale = scale; A.shift = shift; A.gamma = gamma; A.mean = mean; A.invstd = invstd;
    A.sum_g2 = sum_g2; A.sum_g2xhat = sum_g2xhat;
    A.drop = dropout_of(p); A.seed = seed; A.skip = skip;
    A.n_rows = n_rows; A.H = H;
    A.dh = dh; A.lddh = lddh; A.gskip = gskip;
    A.part = partial_db; A.amax = amax;
    A.w_rowptr = w_rowptr; A.w_mode = w_mode;
    A.ranges = ranges; A.rw_rowptr = range_w_rowptr; A.rpart = range_partial;
    return launch_bwd_rows(A, true, stream);
}

// The L2-normalize backward of SAGEConv(normalize=True) on its own (bgnn.nn.SAGEConv's fused
// per-module path, Models/BuckGNN.py:434 under the PyG shim): dh = (g - o <o, g>) / ||h|| per
// row (rows with ||h|| < 1e-12 get g * 1e12: F.normalize's clamped denominator), written at dh (row stride lddh), per-block column sums of dh into partial_db (the bias
// gradient, bgnn_reduce_partials layout) and max |dh| folded into *amax.
extern "C" int bgnn_l2norm_bwd(const float* g, const float* o, const float* nrm, int64_t n_rows, int32_t H,
                               float* dh, int64_t lddh, float* partial_db, float* amax, void* stream) {
    BGNN_REQUIRE(H > 0 && H % 4 == 0 && H <= 512, "l2norm_bwd: H=%d unsupported", H);
    BGNN_REQUIRE(n_rows >= 0, "l2norm_bwd: negative n_rows");
    BGNN_REQUIRE(g && o && nrm && dh && partial_db && amax, "l2norm_bwd: null pointer");
    BGNN_REQUIRE(lddh >= H && lddh % 4 == 0, "l2norm_bwd: bad lddh");
    BGNN_REQUIRE(aligned16(g) && aligned16(o) && aligned16(dh) && aligned16(partial_db),
                 "l2norm_bwd: pointers must be 16-byte aligned");
    BwdRowsArgs A{};
    A.g = g; A.o = o; A.nrm = nrm;
    A.drop.inv_keep = 1.f;
    A.n_rows = n_rows; A.H = H;
    A.dh = dh; A.lddh = lddh;
    A.part = partial_db; A.amax = amax;
    return launch_bwd_rows(A, false, stream);
}
