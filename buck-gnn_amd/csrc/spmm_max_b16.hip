// Max aggregation of bf16 rows (bgnn_spmm_max_bf16): out[r] = max_{e in row r} x[col[e]], the
// semantics of bgnn_spmm_fwd(MAX) on the upcast input (spmm.hip): the accumulator starts at -inf,
// an edge replaces it only when strictly greater -- so the first maximising edge in CSR order wins
// and a NaN never does -- and empty rows give 0. The maximum of bf16 values is one of them: there
// is no rounding and no accumulator, the bf16 store is exact.
//
// Mapping: a lane owns 8 consecutive columns (one 16-byte load of bf16), as in spmm_b16.hip: a
// 512-column source row is 8 lines of 128 B instead of the f32 kernel's 16.
//   without arg (inference): light rows (deg <= chunk) run on the CSR's row-group plan as
//     k_b16_group does (XCD sweep over the groups, keys and masks distributed by readlane, a
//     wave-uniform branch per mask bit); the plan lists a row's keys in edge order, and without an
//     argmax to resolve the deduplicated gather costs nothing extra. No plan: one row per wave.
//   with arg (training): light rows run one row per wave and write the argmax state of
//     bgnn_spmm_max_arg_bytes (seg_common.h), which bgnn_spmm_bwd_max reads.
// Heavy rows: one wave per chunk into `partial` (f32 values, and with arg an int32 plane of CSR
// positions behind them), then one wave per heavy row walks its chunks in chunk order with the same
// strict >. No atomics: results are bit-identical run to run.
#include "common.h"
#include "seg_common.h"

namespace bgnn {

namespace {

struct MaxArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const int32_t* heavy_row;
    const int32_t* heavy_chunk0;
    const int32_t* chunk_heavy;
    int64_t n_rows;
    int32_t n_heavy, n_chunks, chunk, H;
    const uint16_t* x;      int64_t ldx;    // bf16 source rows
    uint16_t* out;          int64_t ldo;    // bf16 [n_rows, ldo]
    uint8_t* arg8;                          // argmax state (NULL: none), seg_common.h
    int32_t* heavy_of;
    int32_t* arg_h;
    float* partial;                         // [n_chunks, H]
    int32_t* partial_arg;                   // [n_chunks, H] CSR positions (with arg)
    const int32_t* gsrc;
    const uint8_t* gmask;
    const int32_t* gcnt;
    const int32_t* grow;
    int64_t n_groups;
};

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint4 ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }

// a = max(a, v) by strict > (a NaN in v never wins); g: the CSR position of the winner
template <bool ARG>
__device__ __forceinline__ void max8(float (&a)[8], int32_t (&g)[8], const uint4 v, int32_t e) {
    float f[8];
    bf16x8_unpack(v, f);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const bool better = f[q] > a[q];
        a[q] = better ? f[q] : a[q];
        if (ARG) g[q] = better ? e : g[q];
    }
}

__device__ __forceinline__ void init8(float (&a)[8], int32_t (&g)[8]) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        a[q] = -INFINITY;
        g[q] = -1;
    }
}

// Row r's result, held by the lanes with ok: 0 for an empty row, stored once (exact), non-temporal.
// ARG: the row's argmax offsets (rb = rowptr[r]); h >= 0: a heavy row, marker bytes and int32 offsets.
template <bool ARG>
__device__ __forceinline__ void store_row(const MaxArgs& A, int64_t r, int32_t deg, int32_t rb, const float (&a)[8],
                                          const int32_t (&g)[8], int c, int32_t h) {
    float y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = deg > 0 ? a[q] : 0.f;
    const u32x4_t v = {bf16_pack2(y[0], y[1]), bf16_pack2(y[2], y[3]), bf16_pack2(y[4], y[5]),
                       bf16_pack2(y[6], y[7])};
    __builtin_nontemporal_store(v, reinterpret_cast<u32x4_t*>(A.out + r * A.ldo + c));
    if (ARG) {
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint32_t o = h >= 0 ? kArgHeavy : (deg > 0 ? (uint32_t)(g[q] - rb) : 0u);
            w[q >> 2] |= (o & 0xffu) << (8 * (q & 3));
        }
        const u32x2_t wv = {w[0], w[1]};
        *reinterpret_cast<u32x2_t*>(A.arg8 + r * A.H + c) = wv;
        if (h >= 0) {
            int4* p = reinterpret_cast<int4*>(A.arg_h + (int64_t)h * A.H + c);
            p[0] = make_int4(g[0] - rb, g[1] - rb, g[2] - rb, g[3] - rb);
            p[1] = make_int4(g[4] - rb, g[5] - rb, g[6] - rb, g[7] - rb);
        }
    }
}

// (a, g) = max over the rows col[beg .. end), in CSR order, 8 rows per gather batch (wave-uniform
// indices)
template <bool ARG>
__device__ __forceinline__ void gather_edges(const MaxArgs& A, int32_t beg, int32_t end, int cs, float (&a)[8],
                                             int32_t (&g)[8]) {
    for (int32_t e0 = beg; e0 < end; e0 += 8) {
        const int n = min(8, end - e0);
        uint4 val[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int32_t j = A.col[e0 + (u < n ? u : 0)];   // masked slots re-read the first row
            val[u] = ld16(A.x + (int64_t)j * A.ldx + cs);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (u < n) max8<ARG>(a, g, val[u], e0 + u);
        }
    }
}

// ---------------------------------------------------------------------------
// Light rows on the row-group plan (no argmax): k_b16_group's structure (spmm_b16.hip) with the
// strict-> maximum in place of the sum. R rows per wave, U keys per gather batch.
template <int R, int U>
__global__ __launch_bounds__(256) void k_max_group(MaxArgs A) {
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
                for (int q = 0; q < 8; ++q) a[t][q] = -INFINITY;
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
                    for (int u = 0; u < U; ++u) val[u] = ld16(A.x + (int64_t)j[u] * A.ldx + cs);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        float f[8];
                        bf16x8_unpack(val[u], f);
#pragma unroll
                        for (int t = 0; t < R; ++t) {
                            // the mask bit is wave-uniform (j[u], m[u] come from readlane): compare
                            // only where the key is used, by a scalar branch
                            if (__builtin_amdgcn_readfirstlane((int)((m[u] >> t) & 1u))) {
#pragma unroll
                                for (int q = 0; q < 8; ++q) a[t][q] = f[q] > a[t][q] ? f[q] : a[t][q];
                            }
                        }
                    }
                }
            }
            const int32_t none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int t = 0; t < R; ++t) {
                const int32_t rb = __builtin_amdgcn_readlane(rp, t);
                const int32_t deg = __builtin_amdgcn_readlane(rp, t + 1) - rb;
                if (t >= rows || deg > chunk) continue;   // heavy row: chunk + combine
                if (ok) store_row<false>(A, r0 + t, deg, rb, a[t], none, cs, -1);
            }
        }
    }
}

// Light rows, one row per wave, CSR order: a CSR without a row-group plan, and every argmax run.
template <bool ARG>
__global__ __launch_bounds__(256) void k_max_row(MaxArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool ok = lane * 8 < A.H;
    const int cs = ok ? lane * 8 : 0;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < A.n_rows; r += (int64_t)gridDim.x * 4) {
        const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
        if (end - beg > A.chunk) continue;   // heavy row: chunk + combine
        float a[8];
        int32_t g[8];
        init8(a, g);
        gather_edges<ARG>(A, beg, end, cs, a, g);
        if (ok) store_row<ARG>(A, r, end - beg, beg, a, g, cs, -1);
    }
}

// Heavy chunks: one wave per chunk -> partial[c, :] (and partial_arg[c, :]). 256 threads (4 chunks).
template <bool ARG>
__global__ __launch_bounds__(256) void k_max_chunk(MaxArgs A) {
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
    float a[8];
    int32_t g[8];
    init8(a, g);
    gather_edges<ARG>(A, beg, end, cs, a, g);
    if (!ok) return;
    float4* p = reinterpret_cast<float4*>(A.partial + c * A.H + cs);
    p[0] = make_float4(a[0], a[1], a[2], a[3]);
    p[1] = make_float4(a[4], a[5], a[6], a[7]);
    if (ARG) {
        int4* pg = reinterpret_cast<int4*>(A.partial_arg + c * A.H + cs);
        pg[0] = make_int4(g[0], g[1], g[2], g[3]);
        pg[1] = make_int4(g[4], g[5], g[6], g[7]);
    }
}

// Combine heavy rows: one wave per heavy row walks the row's chunk partials in chunk order (the
// first maximising chunk wins, as the first maximising edge did inside it) and stores.
template <bool ARG>
__global__ __launch_bounds__(64) void k_max_combine(MaxArgs A) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x;
    if (h >= A.n_heavy) return;
    const bool ok = lane * 8 < A.H;
    if (!ok) return;
    const int cs = lane * 8;
    const int64_t r = A.heavy_row[h];
    const int32_t rb = A.rowptr[r], deg = A.rowptr[r + 1] - rb;
    const int32_t c0 = A.heavy_chunk0[h], c1 = A.heavy_chunk0[h + 1];
    float a[8];
    int32_t g[8];
    init8(a, g);
#pragma unroll 4
    for (int32_t c = c0; c < c1; ++c) {
        const float4* p = reinterpret_cast<const float4*>(A.partial + (int64_t)c * A.H + cs);
        const float4 p0 = p[0], p1 = p[1];
        const float f[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        int32_t pa[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (ARG) {
            const int4* pg = reinterpret_cast<const int4*>(A.partial_arg + (int64_t)c * A.H + cs);
            const int4 g0 = pg[0], g1 = pg[1];
            pa[0] = g0.x; pa[1] = g0.y; pa[2] = g0.z; pa[3] = g0.w;
            pa[4] = g1.x; pa[5] = g1.y; pa[6] = g1.z; pa[7] = g1.w;
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const bool better = f[q] > a[q];
            a[q] = better ? f[q] : a[q];
            if (ARG) g[q] = better ? pa[q] : g[q];
        }
    }
    store_row<ARG>(A, r, deg, rb, a, g, cs, h);
    if (ARG && lane == 0) A.heavy_of[r] = h;
}

inline int64_t grid8(int64_t waves_wanted, int64_t cap) {
    int64_t blocks = (waves_wanted + 3) / 4;   // at most one row / group per wave
    if (blocks > cap) blocks = cap;
    blocks = (blocks + 7) / 8 * 8;
    return blocks < 8 ? 8 : blocks;
}

template <bool ARG>
int launch(const bgnn_csr_t* csr, MaxArgs& A, void* stream) {
    // the row-group plan needs every light row's keys to fit the 8-bit masks and one key vector;
    // an argmax run takes one row per wave (the group form would resolve an argmax per key and row)
    const bool group = !ARG && csr->gsrc && csr->gmask && csr->gcnt &&
                       (csr->group_rows == 4 || csr->group_rows == 8) && A.chunk <= 64;
    hipStream_t s = as_stream(stream);
    if (group) {
        A.gsrc = csr->gsrc;
        A.gmask = csr->gmask;
        A.gcnt = csr->gcnt;
        A.grow = csr->grow;
        A.n_groups = csr->grow ? csr->n_groups : (csr->n_rows + csr->group_rows - 1) / csr->group_rows;
        const dim3 gr((unsigned)grid8(A.n_groups, 1024));   // 4 blocks of 4 waves per CU
        if (csr->group_rows == 8) hipLaunchKernelGGL((k_max_group<8, 4>), gr, dim3(256), 0, s, A);
        else hipLaunchKernelGGL((k_max_group<4, 8>), gr, dim3(256), 0, s, A);
    } else {
        hipLaunchKernelGGL(k_max_row<ARG>, dim3((unsigned)grid8(A.n_rows, 2048)), dim3(256), 0, s, A);
    }
    BGNN_CHECK_LAUNCH();
    if (A.n_chunks > 0) {
        hipLaunchKernelGGL(k_max_chunk<ARG>, dim3((unsigned)((A.n_chunks + 3) / 4)), dim3(256), 0, s, A);
        BGNN_CHECK_LAUNCH();
        hipLaunchKernelGGL(k_max_combine<ARG>, dim3((unsigned)A.n_heavy), dim3(64), 0, s, A);
        BGNN_CHECK_LAUNCH();
    }
    return BGNN_OK;
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_spmm_max_bf16(const bgnn_csr_t* csr, const void* x, int64_t ldx, int32_t H, void* out,
                                  int64_t ldo, void* arg, float* partial, void* stream) {
    BGNN_REQUIRE(csr && csr->rowptr, "spmm_max_bf16: null csr");
    BGNN_REQUIRE(x && out, "spmm_max_bf16: null x / out");
    BGNN_REQUIRE(H >= 8 && H % 8 == 0 && H <= 512, "spmm_max_bf16: H=%d unsupported (need H%%8==0, 8<=H<=512)", H);
    BGNN_REQUIRE(ldx >= H && ldx % 8 == 0, "spmm_max_bf16: ldx must be >= H and a multiple of 8");
    BGNN_REQUIRE(ldo >= H && ldo % 8 == 0, "spmm_max_bf16: ldo must be >= H and a multiple of 8");
    BGNN_REQUIRE(csr->n_chunks == 0 || partial, "spmm_max_bf16: partial scratch required for heavy rows");
    BGNN_REQUIRE(csr->n_chunks == 0 || (csr->heavy_row && csr->heavy_chunk0 && csr->chunk_heavy && csr->chunk > 0 &&
                                        csr->n_heavy > 0),
                 "spmm_max_bf16: heavy rows need the CSR's chunk plan");
    // the compact state stores a light row's argmax as a byte offset (deg <= chunk) and marks heavy
    // rows with 255 (bgnn_spmm_fwd has the same rule)
    BGNN_REQUIRE(!arg || (csr->chunk > 0 && csr->chunk < 255),
                 "spmm_max_bf16(arg): the CSR's chunk must be in [1, 254] for the compact argmax (got %d)", csr->chunk);
    BGNN_REQUIRE(aligned16(x) && aligned16(out) && (!partial || aligned16(partial)) && (!arg || aligned16(arg)),
                 "spmm_max_bf16: x / out / arg / partial must be 16-byte aligned");
    if (csr->n_rows <= 0) return BGNN_OK;
    BGNN_REQUIRE(csr->col || csr->nnz == 0, "spmm_max_bf16: null col");

    MaxArgs A{};
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
    A.out = static_cast<uint16_t*>(out);
    A.ldo = ldo;
    A.partial = partial;
    if (!arg) return launch<false>(csr, A, stream);
    const MaxArgLayout L = max_arg_layout(csr->n_rows, H);
    A.arg8 = static_cast<uint8_t*>(arg);
    A.heavy_of = reinterpret_cast<int32_t*>(static_cast<char*>(arg) + L.heavy_of);
    A.arg_h = reinterpret_cast<int32_t*>(static_cast<char*>(arg) + L.arg_h);
    A.partial_arg = partial ? reinterpret_cast<int32_t*>(partial + (int64_t)csr->n_chunks * H) : nullptr;
    return launch<true>(csr, A, stream);
}
