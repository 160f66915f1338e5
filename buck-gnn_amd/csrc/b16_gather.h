// The gather skeleton of the bf16 aggregation kernels (sage_infer.hip, spmm_b16.hip,
// spmm_max_b16.hip), written once: the 16-byte loads and the 8-column store, the arguments every
// kernel reads (GatherArgs), the row-group walker (walk_groups), the per-row edge gather
// (gather_edges), the heavy-chunk body (chunk_body), the 16-wave combine of f32 chunk partials
// (combine_chunks) and the host side (argument checks, CSR fill, group eligibility, launch
// sequence; the grid, grid8, is seg_common.h's). A file supplies its argument struct (derived from GatherArgs), a policy, an epilogue
// and thin __global__ wrappers.
//
// Mapping: a lane owns 8 consecutive columns (one 16-byte load of bf16), so a 512-column row is one
// vector per lane and 8 lines of 128 B instead of the f32 kernels' 16.
//
// A policy P says what a gathered element does to an accumulator, one float at a time:
//   P::kWeighted                  a per-key weight travels with the key (computed once per key,
//                                 beside the key prefetch, distributed by readlane with it)
//   P::init()                     the accumulator's initial value (0, or -inf)
//   p.weight(j)                   [kWeighted] the weight of source row j
//   P::prepare(f, w)              a source element, prepared once per key (walk_groups)
//   P::absorb(a, f)               the accumulator after a prepared element
//   P::absorb_weighted(a, f, w)   [kWeighted] gather_edges: one key feeds one row there, so
//                                 prepare and absorb are one step
//   P::wins(f, a)                 [argmax] whether absorb replaces a by f
// They are functions of values on purpose: with an absorb that took a row's 8 accumulators by
// reference the compiler turned walk_groups' mask-bit branches into selects in the 4-row kernels
// (260 to 400 more instructions, one wave per SIMD fewer). Everything here is forced inline and
// every accumulator index is an unrolled constant, so the accumulators stay in registers; the three
// files are compiled with different flags, which is why nothing here is instantiated outside the
// file that uses it.
#pragma once

#include "common.h"
#include "seg_common.h"

namespace bgnn {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }

// stream-once rows (z_r, y, x_prev): non-temporal, so they do not displace gathered rows
__device__ __forceinline__ uint4 ld16_nt(const uint16_t* p) {
    const u32x4_t q = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
    return make_uint4(q[0], q[1], q[2], q[3]);
}

// 8 columns of a result row, stored once, non-temporal: rounded to bf16 (one 16-byte store) ...
__device__ __forceinline__ void store8_bf16_nt(uint16_t* p, const float (&y)[8]) {
    const u32x4_t v = {bf16_pack2(y[0], y[1]), bf16_pack2(y[2], y[3]), bf16_pack2(y[4], y[5]),
                       bf16_pack2(y[6], y[7])};
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4_t*>(p));
}

// ... or as f32 (two)
__device__ __forceinline__ void store8_f32_nt(float* p, const float (&y)[8]) {
    const f32x4_t v0 = {y[0], y[1], y[2], y[3]}, v1 = {y[4], y[5], y[6], y[7]};
    __builtin_nontemporal_store(v0, reinterpret_cast<f32x4_t*>(p));
    __builtin_nontemporal_store(v1, reinterpret_cast<f32x4_t*>(p + 4));
}

// columns [c, c + 8) of the row that starts at element `row` of out, which holds f32 (out_f32) or bf16
__device__ __forceinline__ void store8_nt(void* out, int64_t row, int c, int32_t out_f32, const float (&y)[8]) {
    if (out_f32) store8_f32_nt(static_cast<float*>(out) + row + c, y);
    else store8_bf16_nt(static_cast<uint16_t*>(out) + row + c, y);
}

// What every bf16 aggregation kernel reads: the CSR with its heavy-row plan and row-group plan, the
// bf16 source rows and the heavy chunks' f32 partials.
struct GatherArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const int32_t* heavy_row;
    const int32_t* heavy_chunk0;
    const int32_t* chunk_heavy;
    int64_t n_rows;
    int32_t n_heavy, n_chunks, chunk, H;
    const uint16_t* x;      int64_t ldx;    // bf16 source rows
    float* partial;                         // [n_chunks, H]
    const int32_t* gsrc;
    const uint8_t* gmask;
    const int32_t* gcnt;
    const int32_t* grow;
    int64_t n_groups;
};

// a lane's first column (0 outside H) and whether it lies inside H
__device__ __forceinline__ int lane_col8(int lane, int32_t H, bool& ok) {
    ok = lane * 8 < H;
    return ok ? lane * 8 : 0;
}

template <class T, int N>
__device__ __forceinline__ void fill(T (&a)[N], T v) {
#pragma unroll
    for (int q = 0; q < N; ++q) a[q] = v;
}

// ---------------------------------------------------------------------------
// Light rows on the row-group plan: k_seg_group's structure (spmm.hip: XCD sweep over the groups,
// keys and masks distributed by readlane, a wave-uniform branch per mask bit) with a 16-byte bf16
// gather. R rows per wave, U keys per gather batch. Called by all 4 waves of a 256-thread block.
// The epilogue runs once per group, epi(r0, rows, rp, chunk, a, cs, ok): lane t <= R of rp holds
// rowptr[r0 + t]; rows t >= `rows` and rows of degree > chunk (heavy: chunk + combine) are not the
// group's to store.
template <int R, int U, class P, class Epi>
__device__ __forceinline__ void walk_groups(const GatherArgs& A, const P& pol, const Epi& epi) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Sweep sw = sweep_rows(A.n_groups, wave);
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    const int32_t chunk = A.chunk;

    for (int t0 = 0; t0 < sw.T; t0 += 64) {
        const int ng = min(64, sw.T - t0);
        // heads of the next 64 groups of this wave: first row, row count, first CSR position
        // and key count
        int32_t hr = 0, hn = 0, hb = 0, hc = 0;
        if (lane < ng) {
            const int64_t gl = sw.first + (int64_t)sw.W * (t0 + lane);
            if (A.grow) {
                hr = A.grow[gl];
                hn = A.grow[gl + 1] - hr;
            } else {
                hr = (int32_t)(gl * R);
                hn = (int32_t)min((int64_t)R, A.n_rows - hr);
            }
            hb = A.rowptr[hr];
            hc = A.gcnt[gl];
        }
        // prefetch of a group: its rows' rowptr (lane t <= R), its first 64 keys and their weights
        int32_t rp_n, sl_n;
        uint32_t ml_n;
        float wl_n = 1.f;
        {
            const int64_t r0 = __builtin_amdgcn_readlane(hr, 0);
            rp_n = lane <= R ? A.rowptr[min(r0 + lane, A.n_rows)] : 0;
            const int32_t b = __builtin_amdgcn_readlane(hb, 0), c = __builtin_amdgcn_readlane(hc, 0);
            sl_n = lane < c ? A.gsrc[b + lane] : 0;
            ml_n = lane < c ? (uint32_t)A.gmask[b + lane] : 0u;
            if constexpr (P::kWeighted) wl_n = lane < c ? pol.weight(sl_n) : 0.f;
        }
        for (int k = 0; k < ng; ++k) {
            const int64_t r0 = __builtin_amdgcn_readlane(hr, k);
            const int rows = __builtin_amdgcn_readlane(hn, k);
            const int32_t base = __builtin_amdgcn_readlane(hb, k), cnt = __builtin_amdgcn_readlane(hc, k);
            const int32_t rp = rp_n, sl0 = sl_n;
            const uint32_t ml0 = ml_n;
            const float wl0 = wl_n;
            if (k + 1 < ng) {   // one group ahead, before this group's gather
                const int64_t r1 = __builtin_amdgcn_readlane(hr, k + 1);
                rp_n = lane <= R ? A.rowptr[min(r1 + lane, A.n_rows)] : 0;
                const int32_t b = __builtin_amdgcn_readlane(hb, k + 1), c = __builtin_amdgcn_readlane(hc, k + 1);
                sl_n = lane < c ? A.gsrc[b + lane] : 0;
                ml_n = lane < c ? (uint32_t)A.gmask[b + lane] : 0u;
                if constexpr (P::kWeighted) wl_n = lane < c ? pol.weight(sl_n) : 0.f;
            }
            float a[R][8];
#pragma unroll
            for (int t = 0; t < R; ++t) fill(a[t], P::init());
            for (int32_t eb = 0; eb < cnt; eb += 64) {
                const int n = min(64, cnt - eb);
                int32_t sl = sl0;
                uint32_t ml = ml0;
                float wl = wl0;
                if (eb > 0) {
                    sl = lane < n ? A.gsrc[base + eb + lane] : 0;
                    ml = lane < n ? (uint32_t)A.gmask[base + eb + lane] : 0u;
                    if constexpr (P::kWeighted) wl = lane < n ? pol.weight(sl) : 0.f;
                }
                for (int u0 = 0; u0 < n; u0 += U) {
                    int32_t j[U];
                    uint32_t m[U];
                    float w[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const bool in = u0 + u < n;
                        const int kk = in ? u0 + u : u0;   // masked slots re-read the first row (L1 hit)
                        j[u] = __builtin_amdgcn_readlane(sl, kk);
                        m[u] = in ? (uint32_t)__builtin_amdgcn_readlane((int)ml, kk) : 0u;
                        w[u] = P::kWeighted ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl), kk)) : 1.f;
                    }
                    uint4 val[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) val[u] = ld16(A.x + (int64_t)j[u] * A.ldx + cs);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        float f[8];
                        bf16x8_unpack(val[u], f);
#pragma unroll
                        for (int q = 0; q < 8; ++q) f[q] = P::prepare(f[q], w[u]);   // once per key
#pragma unroll
                        for (int t = 0; t < R; ++t) {
                            // the mask bit is wave-uniform (j[u], m[u] come from readlane): absorb
                            // only where the key is used, by a scalar branch
                            if (__builtin_amdgcn_readfirstlane((int)((m[u] >> t) & 1u))) {
#pragma unroll
                                for (int q = 0; q < 8; ++q) a[t][q] = P::absorb(a[t][q], f[q]);
                            }
                        }
                    }
                }
            }
            epi(r0, rows, rp, chunk, a, cs, ok);
        }
    }
}

// (a, g) absorb the source rows col[beg .. end), in CSR order, 8 rows per gather batch
// (wave-uniform indices). ARG: g[8] tracks the CSR position of each column's winner.
template <bool ARG = false, class P>
__device__ __forceinline__ void gather_edges(const GatherArgs& A, const P& pol, int32_t beg, int32_t end, int cs,
                                             float (&a)[8], int32_t* g = nullptr) {
    for (int32_t e0 = beg; e0 < end; e0 += 8) {
        const int n = min(8, end - e0);
        uint4 val[8];
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int32_t j = A.col[e0 + (u < n ? u : 0)];   // masked slots re-read the first row
            val[u] = ld16(A.x + (int64_t)j * A.ldx + cs);
            if constexpr (P::kWeighted) w[u] = pol.weight(j);
            else w[u] = 1.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (u < n) {
                float f[8];
                bf16x8_unpack(val[u], f);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if constexpr (ARG) {
                        const bool better = P::wins(f[q], a[q]);
                        a[q] = better ? f[q] : a[q];
                        g[q] = better ? e0 + u : g[q];
                    } else if constexpr (P::kWeighted) {
                        a[q] = P::absorb_weighted(a[q], f[q], w[u]);
                    } else {
                        a[q] = P::absorb(a[q], f[q]);
                    }
                }
            }
        }
    }
}

// Heavy chunks: one wave per chunk -> partial[c, :] (f32), and with ARG the winners' CSR positions
// -> partial_arg[c, :]. Called by all 4 waves of a 256-thread block (4 chunks).
template <bool ARG, class P>
__device__ __forceinline__ void chunk_body(const GatherArgs& A, const P& pol, int32_t* partial_arg) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * 4 + wave;
    if (c >= A.n_chunks) return;
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    const int32_t h = A.chunk_heavy[c];
    const int32_t r = A.heavy_row[h];
    const int32_t k = (int32_t)(c - A.heavy_chunk0[h]);
    const int32_t beg = A.rowptr[r] + k * A.chunk;
    const int32_t end = min(beg + A.chunk, A.rowptr[r + 1]);
    float a[8];
    int32_t g[8];
    fill(a, P::init());
    fill(g, -1);
    gather_edges<ARG>(A, pol, beg, end, cs, a, g);
    if (!ok) return;
    float4* p = reinterpret_cast<float4*>(A.partial + c * A.H + cs);
    p[0] = make_float4(a[0], a[1], a[2], a[3]);
    p[1] = make_float4(a[4], a[5], a[6], a[7]);
    if constexpr (ARG) {
        int4* pg = reinterpret_cast<int4*>(partial_arg + c * A.H + cs);
        pg[0] = make_int4(g[0], g[1], g[2], g[3]);
        pg[1] = make_int4(g[4], g[5], g[6], g[7]);
    }
}

// Sum of heavy row h's chunk partials, by a block of 16 waves: each wave sums a contiguous run of
// the row's chunks in chunk order, wave 0 adds the 16 run sums in order (a fixed tree). True on
// wave 0, whose lanes inside H then hold the row's sum in a; the other waves are done. Wave 0's loop
// over the run sums is unrolled by 5, not fully: with all 15 steps' LDS reads in flight the block's
// 128-VGPR budget (__launch_bounds__(1024)) overflowed into scratch in k_b16_combine.
// (kCombineWaves: seg_common.h)
__device__ __forceinline__ bool combine_chunks(const GatherArgs& A, int h, int cs, bool ok, float (&a)[8]) {
    constexpr int W = kCombineWaves;
    __shared__ __attribute__((aligned(16))) float red[W][512];
    const int wave = threadIdx.x >> 6;
    const int32_t c0 = A.heavy_chunk0[h], c1 = A.heavy_chunk0[h + 1];
    const int32_t per = (c1 - c0 + W - 1) / W;
    const int32_t qa = min(c1, c0 + wave * per), qb = min(c1, qa + per);
    fill(a, 0.f);
    if (ok) {
        for (int32_t c = qa; c < qb; ++c) {
            const float4* p = reinterpret_cast<const float4*>(A.partial + (int64_t)c * A.H + cs);
            const float4 p0 = p[0], p1 = p[1];
            a[0] += p0.x; a[1] += p0.y; a[2] += p0.z; a[3] += p0.w;
            a[4] += p1.x; a[5] += p1.y; a[6] += p1.z; a[7] += p1.w;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) red[wave][cs + q] = a[q];
    }
    __syncthreads();
    if (wave != 0) return false;
    if (ok) {
#pragma unroll 5
        for (int w = 1; w < W; ++w) {   // a holds wave 0's run sum
            const float4* p = reinterpret_cast<const float4*>(&red[w][cs]);
            const float4 p0 = p[0], p1 = p[1];
            a[0] += p0.x; a[1] += p0.y; a[2] += p0.z; a[3] += p0.w;
            a[4] += p1.x; a[5] += p1.y; a[6] += p1.z; a[7] += p1.w;
        }
    }
    return true;
}

// ---------------------------------------------------------------------------
// Host side.

#define BGNN_TRY(expr)                                                              \
    do {                                                                            \
        const int _rc = (expr);                                                     \
        if (_rc != BGNN_OK) return _rc;                                             \
    } while (0)

// The argument checks the entry points share, in the order they run (an entry point puts the checks
// only it has between them). name: the entry point; xn / on: its source / result operand names;
// need: its bound on H in words.
inline int check_operands(const char* name, const char* xn, const char* on, const char* need, const bgnn_csr_t* csr,
                          const void* x, const void* out, int32_t H, int32_t reduce) {
    BGNN_REQUIRE(csr && csr->rowptr, "%s: null csr", name);
    BGNN_REQUIRE(x && out, "%s: null %s / %s", name, xn, on);
    BGNN_REQUIRE(H > 0 && H % 8 == 0 && H <= 512, "%s: H=%d unsupported (need H%%8==0, %s)", name, H, need);
    BGNN_REQUIRE(reduce == BGNN_REDUCE_SUM || reduce == BGNN_REDUCE_MEAN, "%s: reduce must be sum/mean (got %d)",
                 name, reduce);
    return BGNN_OK;
}

// a leading dimension of rows of H columns, 16-byte aligned: a multiple of `mult` elements
inline int check_ld(const char* name, const char* ldn, int64_t ld, int32_t H, int mult) {
    BGNN_REQUIRE(ld >= H && ld % mult == 0, "%s: %s must be >= H and a multiple of %d", name, ldn, mult);
    return BGNN_OK;
}

inline int check_heavy_plan(const char* name, const bgnn_csr_t* csr, const float* partial) {
    BGNN_REQUIRE(csr->n_chunks == 0 || partial, "%s: partial scratch required for heavy rows", name);
    BGNN_REQUIRE(csr->n_chunks == 0 || (csr->heavy_row && csr->heavy_chunk0 && csr->chunk_heavy && csr->chunk > 0 &&
                                        csr->n_heavy > 0),
                 "%s: heavy rows need the CSR's chunk plan", name);
    return BGNN_OK;
}

// The alignment check (ops: the operands in words; extra: x_prev / arg, or NULL) and the fields of
// A that come from the CSR and the source. *go = 1: launch; 0 with BGNN_OK: no rows, nothing to
// launch.
inline int check_aligned_and_fill(const char* name, const char* ops, const bgnn_csr_t* csr, const void* x,
                                  int64_t ldx, int32_t H, const void* out, const void* extra, float* partial,
                                  GatherArgs& A, int* go) {
    *go = 0;
    BGNN_REQUIRE(aligned16(x) && aligned16(out) && (!extra || aligned16(extra)) && (!partial || aligned16(partial)),
                 "%s: %s must be 16-byte aligned", name, ops);
    if (csr->n_rows <= 0) return BGNN_OK;
    BGNN_REQUIRE(csr->col || csr->nnz == 0, "%s: null col", name);
    A.rowptr = csr->rowptr;
    A.col = csr->col;
    A.heavy_row = csr->heavy_row;
    A.heavy_chunk0 = csr->heavy_chunk0;
    A.chunk_heavy = csr->chunk_heavy;
    A.n_rows = csr->n_rows;
    A.n_heavy = csr->n_heavy;
    A.n_chunks = csr->n_chunks;
    A.chunk = csr->chunk > 0 ? csr->chunk : 0x7fffffff;
    A.H = H;
    A.x = static_cast<const uint16_t*>(x);
    A.ldx = ldx;
    A.partial = partial;
    *go = 1;
    return BGNN_OK;
}

// Whether the light rows can run on the CSR's row-group plan -- every light row's keys must fit
// the 8-bit masks and one key vector -- and if so, the plan's fields of A.
inline bool use_group_plan(const bgnn_csr_t* csr, GatherArgs& A) {
    if (!(csr->gsrc && csr->gmask && csr->gcnt && (csr->group_rows == 4 || csr->group_rows == 8) && A.chunk <= 64))
        return false;
    A.gsrc = csr->gsrc;
    A.gmask = csr->gmask;
    A.gcnt = csr->gcnt;
    A.grow = csr->grow;
    A.n_groups = csr->grow ? csr->n_groups : (csr->n_rows + csr->group_rows - 1) / csr->group_rows;
    return true;
}

// The kernels of one aggregation: light rows on the row-group plan (groups of 8 and of 4 rows;
// NULL: never) or one row per wave, heavy chunks, and the heavy rows' combine with its block size.
template <class Args>
struct GatherKernels {
    void (*group8)(Args);
    void (*group4)(Args);
    void (*row)(Args);
    void (*chunk)(Args);
    void (*combine)(Args);
    unsigned combine_threads;
};

// Light rows, then the heavy rows' chunks, then their combine.
template <class Args>
int launch_gather(const bgnn_csr_t* csr, Args& A, const GatherKernels<Args>& K, void* stream) {
    hipStream_t s = as_stream(stream);
    if (K.group8 && use_group_plan(csr, A)) {
        const dim3 gr((unsigned)grid8(A.n_groups, 1024));   // 4 blocks of 4 waves per CU
        hipLaunchKernelGGL(csr->group_rows == 8 ? K.group8 : K.group4, gr, dim3(256), 0, s, A);
    } else {
        hipLaunchKernelGGL(K.row, dim3((unsigned)grid8(A.n_rows, 2048)), dim3(256), 0, s, A);
    }
    BGNN_CHECK_LAUNCH();
    if (A.n_chunks > 0) {
        hipLaunchKernelGGL(K.chunk, dim3((unsigned)((A.n_chunks + 3) / 4)), dim3(256), 0, s, A);
        BGNN_CHECK_LAUNCH();
        hipLaunchKernelGGL(K.combine, dim3((unsigned)A.n_heavy), dim3(K.combine_threads), 0, s, A);
        BGNN_CHECK_LAUNCH();
    }
    return BGNN_OK;
}

}  // namespace bgnn
