// Neighbour aggregation of bf16 rows with a plain store epilogue, and its transpose
// (bgnn_spmm_fwd_bf16 / bgnn_spmm_bwd_bf16): the gather of sage_infer.hip without the layer tail.
//   forward : out[r] = s_r * sum_{e in row r} x[col[e]]          s_r = 1, or 1 / max(deg r, 1) (MEAN)
//   backward: gx[j]  = sum_{q in rowT j} w(t_q) * g[t_q]         w(t) = 1, or 1 / max(deg_fwd t, 1)
// bf16 rows in, f32 accumulation, one rounding at the store (bf16, or f32 with out_f32).
//
// Mapping: a lane owns 8 consecutive columns (one 16-byte load of bf16): a 512-column source row is
// 8 lines of 128 B instead of the f32 kernels' 16. Light rows (deg <= chunk) run on the CSR's
// row-group plan as k_infer_group does (XCD sweep over the groups, keys and masks distributed by
// readlane, a wave-uniform branch per mask bit); the transposed MEAN's weight of a key is computed
// once per key, beside the key prefetch, and travels by readlane with it. A CSR without a plan takes
// one row per wave. Heavy rows are reduced per chunk into f32 partials and combined in chunk order
// by one block per row. No atomics: every row's summation order is fixed by the plan, so results
// are bit-identical run to run.
#include "common.h"
#include "seg_common.h"

namespace bgnn {

namespace {

struct B16Args {
    const int32_t* rowptr;
    const int32_t* col;
    const int32_t* heavy_row;
    const int32_t* heavy_chunk0;
    const int32_t* chunk_heavy;
    int64_t n_rows;
    int32_t n_heavy, n_chunks, chunk, H;
    const uint16_t* x;      int64_t ldx;    // bf16 source rows
    const int32_t* wrp;                     // weighted (transposed MEAN): the forward rowptr
    void* out;              int64_t ldo;
    int32_t out_f32, mean;                  // mean: scale row r by 1 / max(deg r, 1) (forward MEAN)
    float* partial;                         // [n_chunks, H]
    const int32_t* gsrc;
    const uint8_t* gmask;
    const int32_t* gcnt;
    const int32_t* grow;
    int64_t n_groups;
};

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }

// weight of source row t of the transposed MEAN: 1 / max(forward in-degree of t, 1)
__device__ __forceinline__ float key_weight(const int32_t* wrp, int32_t t) {
    return inv_deg(wrp[t + 1] - wrp[t]);
}

template <bool WT>
__device__ __forceinline__ void acc8(float (&a)[8], const uint4 v, float w) {
    float f[8];
    bf16x8_unpack(v, f);
#pragma unroll
    for (int q = 0; q < 8; ++q) a[q] = WT ? fmaf(w, f[q], a[q]) : a[q] + f[q];
}

// Row r's result, held by the lanes with ok: scaled (forward MEAN) and stored once, non-temporal.
__device__ __forceinline__ void store_row(const B16Args& A, int64_t r, int32_t deg, const float (&a)[8], int c) {
    const float sc = A.mean ? inv_deg(deg) : 1.f;
    float y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = __fmul_rn(a[q], sc);
    if (A.out_f32) {
        float* p = static_cast<float*>(A.out) + r * A.ldo + c;
        const f32x4_t v0 = {y[0], y[1], y[2], y[3]}, v1 = {y[4], y[5], y[6], y[7]};
        __builtin_nontemporal_store(v0, reinterpret_cast<f32x4_t*>(p));
        __builtin_nontemporal_store(v1, reinterpret_cast<f32x4_t*>(p + 4));
    } else {
        uint16_t* p = static_cast<uint16_t*>(A.out) + r * A.ldo + c;
        const u32x4_t v = {bf16_pack2(y[0], y[1]), bf16_pack2(y[2], y[3]), bf16_pack2(y[4], y[5]),
                           bf16_pack2(y[6], y[7])};
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4_t*>(p));
    }
}

// a += (w *) the rows col[beg .. end), in CSR order, 8 rows per gather batch (wave-uniform indices)
template <bool WT>
__device__ __forceinline__ void gather_edges(const B16Args& A, int32_t beg, int32_t end, int cs, float (&a)[8]) {
    for (int32_t e0 = beg; e0 < end; e0 += 8) {
        const int n = min(8, end - e0);
        uint4 val[8];
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int32_t j = A.col[e0 + (u < n ? u : 0)];   // masked slots re-read the first row
            val[u] = ld16(A.x + (int64_t)j * A.ldx + cs);
            w[u] = WT ? key_weight(A.wrp, j) : 1.f;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (u < n) acc8<WT>(a, val[u], w[u]);
        }
    }
}

// ---------------------------------------------------------------------------
// Light rows on the row-group plan: k_infer_group's structure (sage_infer.hip) with the plain store
// as the epilogue. R rows per wave, U keys per gather batch.
template <int R, int U, bool WT>
__global__ __launch_bounds__(256) void k_b16_group(B16Args A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Sweep sw = sweep_rows(A.n_groups, wave);
    int cpos[1];
    bool cok[1];
    lane_cols<8, 1, 64>(0, lane, A.H, cpos, cok);
    const bool ok = cok[0];
    const int cs = ok ? cpos[0] : 0;
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
            if (WT) wl_n = lane < c ? key_weight(A.wrp, sl_n) : 0.f;
        }
        for (int k = 0; k < ng; ++k) {
            const int64_t r0 = __builtin_amdgcn_readlane(hr, k);
            const int rows = __builtin_amdgcn_readlane(hn, k);
            const int32_t base = __builtin_amdgcn_readlane(hb, k), cnt = __builtin_amdgcn_readlane(hc, k);
            const int32_t rp = rp_n, sl0 = sl_n;
            const uint32_t ml0 = ml_n;
            const float wl0 = wl_n;
            if (k + 1 < ng) {
                const int64_t r1 = __builtin_amdgcn_readlane(hr, k + 1);
                rp_n = lane <= R ? A.rowptr[min(r1 + lane, A.n_rows)] : 0;
                const int32_t b = __builtin_amdgcn_readlane(hb, k + 1), c = __builtin_amdgcn_readlane(hc, k + 1);
                sl_n = lane < c ? A.gsrc[b + lane] : 0;
                ml_n = lane < c ? (uint32_t)A.gmask[b + lane] : 0u;
                if (WT) wl_n = lane < c ? key_weight(A.wrp, sl_n) : 0.f;
            }
            float a[R][8];
#pragma unroll
            for (int t = 0; t < R; ++t)
#pragma unroll
                for (int q = 0; q < 8; ++q) a[t][q] = 0.f;
            for (int32_t eb = 0; eb < cnt; eb += 64) {
                const int n = min(64, cnt - eb);
                int32_t sl = sl0;
                uint32_t ml = ml0;
                float wl = wl0;
                if (eb > 0) {
                    sl = lane < n ? A.gsrc[base + eb + lane] : 0;
                    ml = lane < n ? (uint32_t)A.gmask[base + eb + lane] : 0u;
                    if (WT) wl = lane < n ? key_weight(A.wrp, sl) : 0.f;
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
                        w[u] = WT ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wl), kk)) : 1.f;
                    }
                    uint4 val[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) val[u] = ld16(A.x + (int64_t)j[u] * A.ldx + cs);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        float f[8];
                        bf16x8_unpack(val[u], f);
                        if (WT) {
#pragma unroll
                            for (int q = 0; q < 8; ++q) f[q] = __fmul_rn(w[u], f[q]);   // once per key
                        }
#pragma unroll
                        for (int t = 0; t < R; ++t) {
                            // the mask bit is wave-uniform (j[u], m[u] come from readlane): add only
                            // where the key is used, by a scalar branch
                            if (__builtin_amdgcn_readfirstlane((int)((m[u] >> t) & 1u))) {
#pragma unroll
                                for (int q = 0; q < 8; ++q) a[t][q] += f[q];
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const int32_t rb = __builtin_amdgcn_readlane(rp, t);
                const int32_t deg = __builtin_amdgcn_readlane(rp, t + 1) - rb;
                if (t >= rows || deg > chunk) continue;   // heavy row: chunk + combine
                if (ok) store_row(A, r0 + t, deg, a[t], cs);
            }
        }
    }
}

// Light rows without a row-group plan: one row per wave, CSR order.
template <bool WT>
__global__ __launch_bounds__(256) void k_b16_row(B16Args A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool ok = lane * 8 < A.H;
    const int cs = ok ? lane * 8 : 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < A.n_rows; r += (int64_t)gridDim.x * 4) {
        const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
        if (end - beg > A.chunk) continue;   // heavy row: chunk + combine
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        gather_edges<WT>(A, beg, end, cs, a);
        if (ok) store_row(A, r, end - beg, a, cs);
    }
}

// Heavy chunks: one wave per chunk -> partial[c, :] (f32). 256 threads (4 chunks).
template <bool WT>
__global__ __launch_bounds__(256) void k_b16_chunk(B16Args A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * 4 + wave;
    if (c >= A.n_chunks) return;
    const bool ok = lane * 8 < A.H;
    const int cs = ok ? lane * 8 : 0;
    const int32_t h = A.chunk_heavy[c];
    const int32_t r = A.heavy_row[h];
    const int32_t k = (int32_t)(c - A.heavy_chunk0[h]);
    const int32_t beg = A.rowptr[r] + k * A.chunk;
    const int32_t end = min(beg + A.chunk, A.rowptr[r + 1]);
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    gather_edges<WT>(A, beg, end, cs, a);
    if (!ok) return;
    float4* p = reinterpret_cast<float4*>(A.partial + c * A.H + cs);
    p[0] = make_float4(a[0], a[1], a[2], a[3]);
    p[1] = make_float4(a[4], a[5], a[6], a[7]);
}

// Combine heavy rows: one block per heavy row. The block's 16 waves sum 16 contiguous runs of the
// row's chunk partials, each in chunk order; wave 0 adds the 16 run sums in order and stores.
constexpr int kCombineWaves = 16;
__global__ __launch_bounds__(1024) void k_b16_combine(B16Args A) {
    constexpr int W = kCombineWaves;
    __shared__ __attribute__((aligned(16))) float red[W][512];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int h = blockIdx.x;
    if (h >= A.n_heavy) return;   // uniform over the block
    const bool ok = lane * 8 < A.H;
    const int cs = ok ? lane * 8 : 0;
    const int64_t r = A.heavy_row[h];
    const int32_t deg = A.rowptr[r + 1] - A.rowptr[r];
    const int32_t c0 = A.heavy_chunk0[h], c1 = A.heavy_chunk0[h + 1];
    const int32_t per = (c1 - c0 + W - 1) / W;
    const int32_t qa = min(c1, c0 + wave * per), qb = min(c1, qa + per);
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
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
    if (wave != 0 || !ok) return;
    for (int w = 1; w < W; ++w) {   // a holds wave 0's run sum
        const float4* p = reinterpret_cast<const float4*>(&red[w][cs]);
        const float4 p0 = p[0], p1 = p[1];
        a[0] += p0.x; a[1] += p0.y; a[2] += p0.z; a[3] += p0.w;
        a[4] += p1.x; a[5] += p1.y; a[6] += p1.z; a[7] += p1.w;
    }
    store_row(A, r, deg, a, cs);
}

inline int64_t grid8(int64_t waves_wanted, int64_t cap) {
    int64_t blocks = (waves_wanted + 3) / 4;   // at most one row / group per wave
    if (blocks > cap) blocks = cap;
    blocks = (blocks + 7) / 8 * 8;
    return blocks < 8 ? 8 : blocks;
}

template <bool WT>
int launch(const bgnn_csr_t* csr, B16Args& A, void* stream) {
    // the row-group plan needs every light row's keys to fit the 8-bit masks and one key vector
    const bool group = csr->gsrc && csr->gmask && csr->gcnt && (csr->group_rows == 4 || csr->group_rows == 8) &&
                       A.chunk <= 64;
    hipStream_t s = as_stream(stream);
    if (group) {
        A.gsrc = csr->gsrc;
        A.gmask = csr->gmask;
        A.gcnt = csr->gcnt;
        A.grow = csr->grow;
        A.n_groups = csr->grow ? csr->n_groups : (csr->n_rows + csr->group_rows - 1) / csr->group_rows;
        const dim3 gr((unsigned)grid8(A.n_groups, 1024));   // 4 blocks of 4 waves per CU
        if (csr->group_rows == 8) hipLaunchKernelGGL((k_b16_group<8, 4, WT>), gr, dim3(256), 0, s, A);
        else hipLaunchKernelGGL((k_b16_group<4, 8, WT>), gr, dim3(256), 0, s, A);
    } else {
        hipLaunchKernelGGL(k_b16_row<WT>, dim3((unsigned)grid8(A.n_rows, 2048)), dim3(256), 0, s, A);
    }
    BGNN_CHECK_LAUNCH();
    if (A.n_chunks > 0) {
        hipLaunchKernelGGL(k_b16_chunk<WT>, dim3((unsigned)((A.n_chunks + 3) / 4)), dim3(256), 0, s, A);
        BGNN_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_b16_combine, dim3((unsigned)A.n_heavy), dim3(64 * kCombineWaves), 0, s, A);
        BGNN_CHECK_LAUNCH();
    }
    return BGNN_OK;
}

// The checks both entry points share (name: the entry point; xn / on / ldon: its operand names) and
// the launch arguments. *go = 1: launch; 0 with BGNN_OK: no rows, nothing to launch.
int check_and_fill(const char* name, const char* xn, const char* on, const char* ldon, const bgnn_csr_t* csr,
                   const void* x, int64_t ldx, int32_t H, int32_t reduce, void* out, int64_t ldo, int32_t out_f32,
                   float* partial, B16Args& A, int* go) {
    *go = 0;
    BGNN_REQUIRE(csr && csr->rowptr, "%s: null csr", name);
    BGNN_REQUIRE(x && out, "%s: null %s / %s", name, xn, on);
    BGNN_REQUIRE(H > 0 && H % 8 == 0 && H <= 512, "%s: H=%d unsupported (need H%%8==0, H<=512)", name, H);
    BGNN_REQUIRE(reduce == BGNN_REDUCE_SUM || reduce == BGNN_REDUCE_MEAN, "%s: reduce must be sum/mean (got %d)",
                 name, reduce);
    BGNN_REQUIRE(ldx >= H && ldx % 8 == 0, "%s: ld%s must be >= H and a multiple of 8", name, xn);
    BGNN_REQUIRE(ldo >= H && ldo % (out_f32 ? 4 : 8) == 0, "%s: %s must be >= H and a multiple of %d", name, ldon,
                 out_f32 ? 4 : 8);
    BGNN_REQUIRE(csr->n_chunks == 0 || partial, "%s: partial scratch required for heavy rows", name);
    BGNN_REQUIRE(csr->n_chunks == 0 || (csr->heavy_row && csr->heavy_chunk0 && csr->chunk_heavy && csr->chunk > 0 &&
                                        csr->n_heavy > 0),
                 "%s: heavy rows need the CSR's chunk plan", name);
    BGNN_REQUIRE(aligned16(x) && aligned16(out) && (!partial || aligned16(partial)),
                 "%s: %s / %s / partial must be 16-byte aligned", name, xn, on);
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
    A.out = out;
    A.ldo = ldo;
    A.out_f32 = out_f32 ? 1 : 0;
    A.partial = partial;
    *go = 1;
    return BGNN_OK;
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_spmm_fwd_bf16(const bgnn_csr_t* csr, const void* x, int64_t ldx, int32_t H, int32_t reduce,
                                  void* out, int64_t ldo, int32_t out_f32, float* partial, void* stream) {
    B16Args A{};
    int go = 0;
    const int rc = check_and_fill("spmm_fwd_bf16", "x", "out", "ldo", csr, x, ldx, H, reduce, out, ldo, out_f32, partial, A, &go);
    if (rc != BGNN_OK || !go) return rc;
    A.mean = reduce == BGNN_REDUCE_MEAN;
    return launch<false>(csr, A, stream);
}

extern "C" int bgnn_spmm_bwd_bf16(const bgnn_csr_t* csr_t, const int32_t* fwd_rowptr, const void* g, int64_t ldg,
                                  int32_t H, int32_t reduce, void* gx, int64_t ldgx, int32_t out_f32,
                                  float* partial, void* stream) {
    B16Args A{};
    int go = 0;
    const int rc = check_and_fill("spmm_bwd_bf16", "g", "gx", "ldgx", csr_t, g, ldg, H, reduce, gx, ldgx, out_f32, partial, A,
                                  &go);
    if (rc != BGNN_OK) return rc;
    BGNN_REQUIRE(reduce != BGNN_REDUCE_MEAN || fwd_rowptr, "spmm_bwd_bf16: MEAN needs fwd_rowptr");
    if (!go) return BGNN_OK;
    A.mean = 0;
    if (reduce == BGNN_REDUCE_MEAN) {
        A.wrp = fwd_rowptr;
        return launch<true>(csr_t, A, stream);
    }
    return launch<false>(csr_t, A, stream);
}
