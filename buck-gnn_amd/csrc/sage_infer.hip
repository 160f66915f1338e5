// Eval-mode GraphSAGE layer on bf16 rows (bgnn_sage_infer_bf16): the neighbour aggregation of
// bf16 z_l rows with the whole layer tail in its epilogue,
//   h = s_i * sum_e z_l[col[e]] + z_r[i] + b;  o = h / max(||h||, 1e-12);
//   y = ReLU(o * scale + shift) (+ x_prev[i]),
// everything in f32 with one rounding at the store (bf16, or f32 for the last layer). BatchNorm
// is in eval mode, so scale / shift are known before the layer starts (bgnn_bn_eval_coeffs) and
// the f32 o [N, H] round trip between bgnn_sage_fwd and bgnn_sage_apply disappears.
//
// Mapping: a lane owns 8 consecutive columns (one 16-byte load of bf16), so a 512-column row is one
// vector per lane and 8 lines of 128 B instead of the f32 kernel's 16. Light rows (deg <= chunk)
// run on the CSR's row-group plan exactly as k_seg_group does (spmm.hip: XCD sweep over the
// groups, keys and masks distributed by readlane, a wave-uniform branch per mask bit); a CSR
// without a plan takes one row per wave. Heavy rows (super nodes) are reduced per chunk into f32
// partials and combined in chunk order by a block that then runs the same tail. No atomics; the
// summation order of every row is fixed by the plan, so results are deterministic run to run.
#include "common.h"
#include "seg_common.h"
#include "sage_tail.h"

namespace bgnn {

namespace {

// (the tail's operands -- H, bias, scale, shift, xprev, out, mean -- are TailArgs, sage_tail.h)
struct InferArgs : TailArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const int32_t* heavy_row;
    const int32_t* heavy_chunk0;
    const int32_t* chunk_heavy;
    int64_t n_rows;
    int32_t n_heavy, n_chunks, chunk;
    const uint16_t* z;      int64_t ldz;    // bf16 [N, 2H]: z_l = cols [0, H), z_r = cols [H, 2H)
    float* partial;                         // [n_chunks, H]
    const int32_t* gsrc;
    const uint8_t* gmask;
    const int32_t* gcnt;
    const int32_t* grow;
    int64_t n_groups;
};

// a += the z_l rows col[beg .. end), in CSR order, 8 rows per gather batch (wave-uniform indices)
__device__ __forceinline__ void gather_edges(const InferArgs& A, int32_t beg, int32_t end, int cs, float (&a)[8]) {
    for (int32_t e0 = beg; e0 < end; e0 += 8) {
        const int n = min(8, end - e0);
        uint4 val[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int32_t j = A.col[e0 + (u < n ? u : 0)];   // masked slots re-read the first row
            val[u] = ld16(A.z + (int64_t)j * A.ldz + cs);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (u < n) {
                float f[8];
                bf16x8_unpack(val[u], f);
#pragma unroll
                for (int q = 0; q < 8; ++q) a[q] += f[q];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Light rows on the row-group plan: k_seg_group's structure (spmm.hip) with a 16-byte bf16 gather
// and the layer tail as the epilogue. R rows per wave, U keys per gather batch.
template <int R, int U>
__global__ __launch_bounds__(256) void k_infer_group(InferArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const Sweep sw = sweep_rows(A.n_groups, wave);
    int cpos[1];
    bool cok[1];
    lane_cols<8, 1, 64>(0, lane, A.H, cpos, cok);
    const bool ok = cok[0];
    const int cs = ok ? cpos[0] : 0;
    __shared__ __attribute__((aligned(16))) Coef C;
    stage_coef(A, C);
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
        // prefetch of a group: its rows' rowptr (lane t <= R) and its first 64 keys
        int32_t rp_n, sl_n;
        uint32_t ml_n;
        {
            const int64_t r0 = __builtin_amdgcn_readlane(hr, 0);
            rp_n = lane <= R ? A.rowptr[min(r0 + lane, A.n_rows)] : 0;
            const int32_t b = __builtin_amdgcn_readlane(hb, 0), c = __builtin_amdgcn_readlane(hc, 0);
            sl_n = lane < c ? A.gsrc[b + lane] : 0;
            ml_n = lane < c ? (uint32_t)A.gmask[b + lane] : 0u;
        }
        for (int k = 0; k < ng; ++k) {
            const int64_t r0 = __builtin_amdgcn_readlane(hr, k);
            const int rows = __builtin_amdgcn_readlane(hn, k);
            const int32_t base = __builtin_amdgcn_readlane(hb, k), cnt = __builtin_amdgcn_readlane(hc, k);
            const int32_t rp = rp_n, sl0 = sl_n;
            const uint32_t ml0 = ml_n;
            if (k + 1 < ng) {
                const int64_t r1 = __builtin_amdgcn_readlane(hr, k + 1);
                rp_n = lane <= R ? A.rowptr[min(r1 + lane, A.n_rows)] : 0;
                const int32_t b = __builtin_amdgcn_readlane(hb, k + 1), c = __builtin_amdgcn_readlane(hc, k + 1);
                sl_n = lane < c ? A.gsrc[b + lane] : 0;
                ml_n = lane < c ? (uint32_t)A.gmask[b + lane] : 0u;
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
                if (eb > 0) {
                    sl = lane < n ? A.gsrc[base + eb + lane] : 0;
                    ml = lane < n ? (uint32_t)A.gmask[base + eb + lane] : 0u;
                }
                for (int u0 = 0; u0 < n; u0 += U) {
                    int32_t j[U];
                    uint32_t m[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const bool in = u0 + u < n;
                        const int kk = in ? u0 + u : u0;   // masked slots re-read the first row (L1 hit)
                        j[u] = __builtin_amdgcn_readlane(sl, kk);
                        m[u] = in ? (uint32_t)__builtin_amdgcn_readlane((int)ml, kk) : 0u;
                    }
                    uint4 val[U];
#pragma unroll
                    for (int u = 0; u < U; ++u) val[u] = ld16(A.z + (int64_t)j[u] * A.ldz + cs);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        float f[8];
                        bf16x8_unpack(val[u], f);
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
            // the rows' own stream-once loads (z_r, x_prev), all issued before the first tail
            uint4 zq[R], xq[R];
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const int64_t r = r0 + (t < rows ? t : 0);
                zq[t] = ld16_nt(A.z + r * A.ldz + A.H + cs);
                xq[t] = A.xprev ? ld16_nt(A.xprev + r * A.ldx + cs) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const int32_t rb = __builtin_amdgcn_readlane(rp, t);
                const int32_t deg = __builtin_amdgcn_readlane(rp, t + 1) - rb;
                if (t >= rows || deg > chunk) continue;   // heavy row: chunk + combine
                infer_tail(A, C, r0 + t, deg, a[t], zq[t], xq[t], cs, ok);
            }
        }
    }
}

// Light rows without a row-group plan: one row per wave, CSR order.
__global__ __launch_bounds__(256) void k_infer_row(InferArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool ok = lane * 8 < A.H;
    const int cs = ok ? lane * 8 : 0;
    __shared__ __attribute__((aligned(16))) Coef C;
    stage_coef(A, C);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < A.n_rows; r += (int64_t)gridDim.x * 4) {
        const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
        if (end - beg > A.chunk) continue;   // heavy row: chunk + combine
        const uint4 zq = ld16_nt(A.z + r * A.ldz + A.H + cs);
        const uint4 xq = A.xprev ? ld16_nt(A.xprev + r * A.ldx + cs) : make_uint4(0, 0, 0, 0);
        float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        gather_edges(A, beg, end, cs, a);
        infer_tail(A, C, r, end - beg, a, zq, xq, cs, ok);
    }
}

// Heavy chunks: one wave per chunk -> partial[c, :] (f32). 256 threads (4 chunks).
__global__ __launch_bounds__(256) void k_infer_chunk(InferArgs A) {
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
    gather_edges(A, beg, end, cs, a);
    if (!ok) return;
    float4* p = reinterpret_cast<float4*>(A.partial + c * A.H + cs);
    p[0] = make_float4(a[0], a[1], a[2], a[3]);
    p[1] = make_float4(a[4], a[5], a[6], a[7]);
}

// Combine heavy rows: one block per heavy row. The block's 16 waves sum 16 contiguous runs of the
// row's chunk partials, wave 0 adds the 16 run sums in order (a fixed tree) and runs the tail.
constexpr int kInferCombineWaves = 16;
__global__ __launch_bounds__(1024) void k_infer_combine(InferArgs A) {
    constexpr int W = kInferCombineWaves;
    __shared__ __attribute__((aligned(16))) float red[W][512];
    __shared__ __attribute__((aligned(16))) Coef C;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int h = blockIdx.x;
    if (h >= A.n_heavy) return;   // uniform over the block
    stage_coef(A, C);
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
    if (wave != 0) return;
    if (ok) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            float t = red[0][cs + q];
#pragma unroll
            for (int w = 1; w < W; ++w) t += red[w][cs + q];
            a[q] = t;
        }
    }
    const uint4 zq = ld16_nt(A.z + r * A.ldz + A.H + cs);
    const uint4 xq = A.xprev ? ld16_nt(A.xprev + r * A.ldx + cs) : make_uint4(0, 0, 0, 0);
    infer_tail(A, C, r, deg, a, zq, xq, cs, ok);
}

inline int64_t grid8(int64_t waves_wanted, int64_t cap) {
    int64_t blocks = (waves_wanted + 3) / 4;   // at most one row / group per wave
    if (blocks > cap) blocks = cap;
    blocks = (blocks + 7) / 8 * 8;
    return blocks < 8 ? 8 : blocks;
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_sage_infer_bf16(const bgnn_csr_t* csr, const void* z, int64_t ldz, const float* bias,
                                    const float* scale, const float* shift, const void* x_prev, int64_t ldx,
                                    int32_t H, int32_t reduce, void* out, int64_t ldo, int32_t out_f32,
                                    float* partial, void* stream) {
    BGNN_REQUIRE(csr && csr->rowptr, "sage_infer_bf16: null csr");
    BGNN_REQUIRE(z && out, "sage_infer_bf16: null z / out");
    BGNN_REQUIRE(H > 0 && H % 8 == 0 && H <= 512, "sage_infer_bf16: H=%d unsupported (need H%%8==0, H<=512)", H);
    BGNN_REQUIRE(reduce == BGNN_REDUCE_SUM || reduce == BGNN_REDUCE_MEAN,
                 "sage_infer_bf16: reduce must be sum/mean (got %d)", reduce);
    BGNN_REQUIRE(ldz >= 2 * (int64_t)H && ldz % 8 == 0, "sage_infer_bf16: ldz must be >= 2H and a multiple of 8");
    BGNN_REQUIRE(!x_prev || (ldx >= H && ldx % 8 == 0), "sage_infer_bf16: ldx must be >= H and a multiple of 8");
    BGNN_REQUIRE(ldo >= H && ldo % (out_f32 ? 4 : 8) == 0,
                 "sage_infer_bf16: ldo must be >= H and a multiple of %d", out_f32 ? 4 : 8);
    BGNN_REQUIRE((scale == nullptr) == (shift == nullptr), "sage_infer_bf16: scale and shift go together");
    BGNN_REQUIRE(csr->n_chunks == 0 || partial, "sage_infer_bf16: partial scratch required for heavy rows");
    BGNN_REQUIRE(csr->n_chunks == 0 || (csr->heavy_row && csr->heavy_chunk0 && csr->chunk_heavy && csr->chunk > 0 &&
                                        csr->n_heavy > 0),
                 "sage_infer_bf16: heavy rows need the CSR's chunk plan");
    BGNN_REQUIRE(aligned16(z) && aligned16(out) && (!x_prev || aligned16(x_prev)) && (!partial || aligned16(partial)),
                 "sage_infer_bf16: z / x_prev / out / partial must be 16-byte aligned");
    if (csr->n_rows <= 0) return BGNN_OK;
    BGNN_REQUIRE(csr->col || csr->nnz == 0, "sage_infer_bf16: null col");

    InferArgs A{};
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
    A.z = static_cast<const uint16_t*>(z);
    A.ldz = ldz;
    A.bias = bias;
    A.scale = scale;
    A.shift = shift;
    A.xprev = static_cast<const uint16_t*>(x_prev);
    A.ldx = ldx;
    A.out = out;
    A.ldo = ldo;
    A.out_f32 = out_f32 ? 1 : 0;
    A.mean = reduce == BGNN_REDUCE_MEAN;
    A.partial = partial;
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
        if (csr->group_rows == 8) hipLaunchKernelGGL((k_infer_group<8, 4>), gr, dim3(256), 0, s, A);
        else hipLaunchKernelGGL((k_infer_group<4, 8>), gr, dim3(256), 0, s, A);
    } else {
        hipLaunchKernelGGL(k_infer_row, dim3((unsigned)grid8(A.n_rows, 2048)), dim3(256), 0, s, A);
    }
    BGNN_CHECK_LAUNCH();
    if (A.n_chunks > 0) {
        hipLaunchKernelGGL(k_infer_chunk, dim3((unsigned)((A.n_chunks + 3) / 4)), dim3(256), 0, s, A);
        BGNN_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_infer_combine, dim3((unsigned)A.n_heavy), dim3(64 * kInferCombineWaves), 0, s, A);
        BGNN_CHECK_LAUNCH();
    }
    return BGNN_OK;
}
