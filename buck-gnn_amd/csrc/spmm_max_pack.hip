// Max aggregation of f32 rows packed as the bf16 A operand of the max layer's GEMM
// (bgnn_spmm_max_pack_bf16, the bf16 training mode of GraphSage_maxAggr): for every row r
//   out[r, 0:H)  = bf16(max_{e in row r} x[col[e], :])     plane 0
//   out[r, H:2H) = bf16(x[r, :])                            plane 1
// The maximum and its argmax are taken on the f32 values, with the semantics and the argmax state
// of bgnn_spmm_fwd(MAX) (spmm.hip): the accumulator starts at -inf, an edge replaces it only when
// strictly greater -- the first maximising edge in CSR order wins, a NaN never does -- and empty
// rows give 0. Rounding is monotone, so plane 0 holds the values bgnn_spmm_max_bf16 would give on
// the rounded rows; the argmax is not the same (rows that tie after rounding need not tie before),
// which is why this kernel reads f32 and rounds only what it stores.
//
// Mapping: a lane owns 8 consecutive columns, as in b16_gather.h -- two 16-byte loads of a source
// row, one 16-byte bf16 store per plane, 8 state bytes -- so the store, the chunk partials and the
// combine have the layout of spmm_max_b16.hip's argmax run.
//   light rows (deg <= chunk): one row per wave in CSR order; the wave also packs the row's own x
//     (plane 1), for heavy rows too
//   heavy rows: one wave per chunk into `partial` (f32 values, an int32 plane of CSR positions
//     behind them), then one wave per heavy row walks its chunks in chunk order with the same
//     strict >
// No atomics: results are bit-identical run to run.
#include "common.h"
#include "seg_common.h"
#include "b16_gather.h"

namespace bgnn {

namespace {

struct PackArgs : GatherArgs {              // (GatherArgs::x is not read: the source rows are f32)
    const float* xf;                        // f32 [*, ldx]
    uint16_t* out;          int64_t ldo;    // bf16 [n_rows, ldo], ldo >= 2H
    uint8_t* arg8;                          // argmax state, seg_common.h
    int32_t* heavy_of;
    int32_t* arg_h;
    int32_t* partial_arg;                   // [n_chunks, H] CSR positions
};

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// columns [c, c + 8) of an f32 row
__device__ __forceinline__ void ld8_f32(const float* p, float4& lo, float4& hi) {
    lo = *reinterpret_cast<const float4*>(p);
    hi = *reinterpret_cast<const float4*>(p + 4);
}

// (a, g) absorb the source rows col[beg .. end) in CSR order by strict > (a NaN never wins), U
// rows per gather batch (wave-uniform indices); g tracks the CSR position of each column's winner.
template <int U>
__device__ __forceinline__ void gather_max(const PackArgs& A, int32_t beg, int32_t end, int cs, float (&a)[8],
                                           int32_t (&g)[8]) {
    for (int32_t e0 = beg; e0 < end; e0 += U) {
        const int n = min(U, end - e0);
        float4 lo[U], hi[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int32_t j = A.col[e0 + (u < n ? u : 0)];   // masked slots re-read the first row
            ld8_f32(A.xf + (int64_t)j * A.ldx + cs, lo[u], hi[u]);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (u < n) {
                const float f[8] = {lo[u].x, lo[u].y, lo[u].z, lo[u].w, hi[u].x, hi[u].y, hi[u].z, hi[u].w};
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const bool better = f[q] > a[q];
                    a[q] = better ? f[q] : a[q];
                    g[q] = better ? e0 + u : g[q];
                }
            }
        }
    }
}

// Row r's aggregate (plane 0), held by the lanes inside H: 0 for an empty row, rounded to bf16 and
// stored once, with the row's argmax offsets (rb = rowptr[r]); h >= 0: a heavy row, marker bytes
// and int32 offsets. The state is spmm_max_b16.hip's store_row<true>.
__device__ __forceinline__ void store_agg(const PackArgs& A, int64_t r, int32_t deg, int32_t rb, const float (&a)[8],
                                          const int32_t (&g)[8], int c, int32_t h) {
    float y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = deg > 0 ? a[q] : 0.f;
    store8_bf16_nt(A.out + r * A.ldo + c, y);
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t o = h >= 0 ? kArgHeavy : (deg > 0 ? (uint32_t)arg_offset(g[q], rb) : 0u);
        w[q >> 2] |= (o & 0xffu) << (8 * (q & 3));
    }
    const u32x2_t wv = {w[0], w[1]};
    *reinterpret_cast<u32x2_t*>(A.arg8 + r * A.H + c) = wv;
    if (h >= 0) {
        int4* p = reinterpret_cast<int4*>(A.arg_h + (int64_t)h * A.H + c);
        p[0] = make_int4(arg_offset(g[0], rb), arg_offset(g[1], rb), arg_offset(g[2], rb), arg_offset(g[3], rb));
        p[1] = make_int4(arg_offset(g[4], rb), arg_offset(g[5], rb), arg_offset(g[6], rb), arg_offset(g[7], rb));
    }
}

// Every row's own x into plane 1; light rows' aggregate and state. One row per wave, CSR order.
template <int U>
__global__ __launch_bounds__(256) void k_pack_row(PackArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < A.n_rows; r += (int64_t)gridDim.x * 4) {
        const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
        float4 lo, hi;
        ld8_f32(A.xf + r * A.ldx + cs, lo, hi);
        const bool light = end - beg <= A.chunk;   // heavy row: chunk + combine
        float a[8];
        int32_t g[8];
        fill(a, -INFINITY);
        fill(g, -1);
        if (light) gather_max<U>(A, beg, end, cs, a, g);
        if (!ok) continue;
        const float xr[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        store8_bf16_nt(A.out + r * A.ldo + A.H + cs, xr);
        if (light) store_agg(A, r, end - beg, beg, a, g, cs, -1);
    }
}

// Heavy chunks: one wave per chunk -> partial[c, :] and partial_arg[c, :].
template <int U>
__global__ __launch_bounds__(256) void k_pack_chunk(PackArgs A) {
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
    fill(a, -INFINITY);
    fill(g, -1);
    gather_max<U>(A, beg, end, cs, a, g);
    if (!ok) return;
    float4* p = reinterpret_cast<float4*>(A.partial + c * A.H + cs);
    p[0] = make_float4(a[0], a[1], a[2], a[3]);
    p[1] = make_float4(a[4], a[5], a[6], a[7]);
    int4* pg = reinterpret_cast<int4*>(A.partial_arg + c * A.H + cs);
    pg[0] = make_int4(g[0], g[1], g[2], g[3]);
    pg[1] = make_int4(g[4], g[5], g[6], g[7]);
}

// Combine heavy rows: one wave per heavy row walks the row's chunk partials in chunk order (the
// first maximising chunk wins, as the first maximising edge did inside it) and stores.
__global__ __launch_bounds__(64) void k_pack_combine(PackArgs A) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x;
    if (h >= A.n_heavy) return;
    if (lane * 8 >= A.H) return;
    const int cs = lane * 8;
    const int64_t r = A.heavy_row[h];
    const int32_t rb = A.rowptr[r], deg = A.rowptr[r + 1] - rb;
    const int32_t c0 = A.heavy_chunk0[h], c1 = A.heavy_chunk0[h + 1];
    float a[8];
    int32_t g[8];
    fill(a, -INFINITY);
    fill(g, -1);
#pragma unroll 4
    for (int32_t c = c0; c < c1; ++c) {
        const float4* p = reinterpret_cast<const float4*>(A.partial + (int64_t)c * A.H + cs);
        const int4* pg = reinterpret_cast<const int4*>(A.partial_arg + (int64_t)c * A.H + cs);
        const float4 p0 = p[0], p1 = p[1];
        const int4 g0 = pg[0], g1 = pg[1];
        const float f[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        const int32_t pa[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const bool better = f[q] > a[q];
            a[q] = better ? f[q] : a[q];
            g[q] = better ? pa[q] : g[q];
        }
    }
    store_agg(A, r, deg, rb, a, g, cs, h);
    if (lane == 0) A.heavy_of[r] = h;
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_spmm_max_pack_bf16(const bgnn_csr_t* csr, const float* x, int64_t ldx, int32_t H, void* out,
                                       int64_t ldo, void* arg, float* partial, void* stream) {
    const char* name = "spmm_max_pack_bf16";
    BGNN_TRY(check_operands(name, "x", "out", "8<=H<=512", csr, x, out, H, BGNN_REDUCE_SUM));
    BGNN_REQUIRE(arg, "%s: null arg (the argmax state is required)", name);
    BGNN_TRY(check_ld(name, "ldx", ldx, H, 4));
    BGNN_REQUIRE(ldo >= 2 * (int64_t)H && ldo % 8 == 0, "%s: ldo must be >= 2H and a multiple of 8", name);
    BGNN_TRY(check_heavy_plan(name, csr, partial));
    // the compact state stores a light row's argmax as a byte offset (deg <= chunk) and marks heavy
    // rows with 255 (bgnn_spmm_fwd has the same rule)
    BGNN_REQUIRE(csr->chunk > 0 && csr->chunk < 255,
                 "%s: the CSR's chunk must be in [1, 254] for the compact argmax (got %d)", name, csr->chunk);
    PackArgs A{};
    int go = 0;
    BGNN_TRY(check_aligned_and_fill(name, "x / out / arg / partial", csr, x, ldx, H, out, arg, partial, A, &go));
    if (!go) return BGNN_OK;
    A.xf = x;
    A.out = static_cast<uint16_t*>(out);
    A.ldo = ldo;
    const MaxArgLayout L = max_arg_layout(csr->n_rows, H);
    A.arg8 = static_cast<uint8_t*>(arg);
    A.heavy_of = reinterpret_cast<int32_t*>(static_cast<char*>(arg) + L.heavy_of);
    A.arg_h = reinterpret_cast<int32_t*>(static_cast<char*>(arg) + L.arg_h);
    A.partial_arg = partial ? reinterpret_cast<int32_t*>(partial + (int64_t)csr->n_chunks * H) : nullptr;
    const GatherKernels<PackArgs> K = {nullptr, nullptr, k_pack_row<8>, k_pack_chunk<8>, k_pack_combine, 64};
    return launch_gather(csr, A, K, stream);
}
