// Max aggregation of bf16 rows (bgnn_spmm_max_bf16): out[r] = max_{e in row r} x[col[e]], the
// semantics of bgnn_spmm_fwd(MAX) on the upcast input (spmm.hip): the accumulator starts at -inf,
// an edge replaces it only when strictly greater -- so the first maximising edge in CSR order wins
// and a NaN never does -- and empty rows give 0. The maximum of bf16 values is one of them: there
// is no rounding and no accumulator, the bf16 store is exact.
//
// The gather is b16_gather.h's skeleton with the strict-> maximum as the policy. This file adds
// that policy, the exact store with the argmax state, and the heavy rows' one-wave combine.
//   without arg (inference): light rows (deg <= chunk) run on the CSR's row-group plan; the plan
//     lists a row's keys in edge order, and without an argmax to resolve the deduplicated gather
//     costs nothing extra. No plan: one row per wave.
//   with arg (training): light rows run one row per wave and write the argmax state of
//     bgnn_spmm_max_arg_bytes (seg_common.h), which bgnn_spmm_bwd_max reads.
// Heavy rows: one wave per chunk into `partial` (f32 values, and with arg an int32 plane of CSR
// positions behind them), then one wave per heavy row walks its chunks in chunk order with the same
// strict >. No atomics: results are bit-identical run to run.
#include "common.h"
#include "seg_common.h"
#include "b16_gather.h"

namespace bgnn {

namespace {

struct MaxArgs : GatherArgs {
    uint16_t* out;          int64_t ldo;    // bf16 [n_rows, ldo]
    uint8_t* arg8;                          // argmax state (NULL: none), seg_common.h
    int32_t* heavy_of;
    int32_t* arg_h;
    int32_t* partial_arg;                   // [n_chunks, H] CSR positions (with arg)
};

typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

// a = max(a, f) by strict > (a NaN in f never wins)
struct Max {
    static constexpr bool kWeighted = false;
    static __device__ __forceinline__ float init() { return -INFINITY; }
    static __device__ __forceinline__ float prepare(float f, float) { return f; }
    static __device__ __forceinline__ bool wins(float f, float a) { return f > a; }
    static __device__ __forceinline__ float absorb(float a, float f) { return wins(f, a) ? f : a; }
};

// Row r's result, held by the lanes with ok: 0 for an empty row, stored once (exact), non-temporal.
// ARG: the row's argmax offsets (rb = rowptr[r]); h >= 0: a heavy row, marker bytes and int32 offsets.
template <bool ARG>
__device__ __forceinline__ void store_row(const MaxArgs& A, int64_t r, int32_t deg, int32_t rb, const float (&a)[8],
                                          const int32_t (&g)[8], int c, int32_t h) {
    float y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = deg > 0 ? a[q] : 0.f;
    store8_bf16_nt(A.out + r * A.ldo + c, y);
    if (ARG) {
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
}

template <int R>
struct GroupStore {
    const MaxArgs& A;
    __device__ __forceinline__ void operator()(int64_t r0, int rows, int32_t rp, int32_t chunk, float (&a)[R][8],
                                               int cs, bool ok) const {
        const int32_t none[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int32_t rb = __builtin_amdgcn_readlane(rp, t);
            const int32_t deg = __builtin_amdgcn_readlane(rp, t + 1) - rb;
            if (t >= rows || deg > chunk) continue;   // heavy row: chunk + combine
            if (ok) store_row<false>(A, r0 + t, deg, rb, a[t], none, cs, -1);
        }
    }
};

// Light rows on the row-group plan (no argmax), the exact store as the epilogue.
template <int R, int U>
__global__ __launch_bounds__(256) void k_max_group(MaxArgs A) {
    walk_groups<R, U>(A, Max{}, GroupStore<R>{A});
}

// Light rows, one row per wave, CSR order: a CSR without a row-group plan, and every argmax run.
template <bool ARG>
__global__ __launch_bounds__(256) void k_max_row(MaxArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < A.n_rows; r += (int64_t)gridDim.x * 4) {
        const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
        if (end - beg > A.chunk) continue;   // heavy row: chunk + combine
        float a[8];
        int32_t g[8];
        fill(a, Max::init());
        fill(g, -1);
        gather_edges<ARG>(A, Max{}, beg, end, cs, a, g);
        if (ok) store_row<ARG>(A, r, end - beg, beg, a, g, cs, -1);
    }
}

// Heavy chunks: one wave per chunk -> partial[c, :] (and partial_arg[c, :]).
template <bool ARG>
__global__ __launch_bounds__(256) void k_max_chunk(MaxArgs A) {
    chunk_body<ARG>(A, Max{}, A.partial_arg);
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
    fill(a, Max::init());
    fill(g, -1);
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

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_spmm_max_bf16(const bgnn_csr_t* csr, const void* x, int64_t ldx, int32_t H, void* out,
                                  int64_t ldo, void* arg, float* partial, void* stream) {
    const char* name = "spmm_max_bf16";
    BGNN_TRY(check_operands(name, "x", "out", "8<=H<=512", csr, x, out, H, BGNN_REDUCE_SUM));
    BGNN_TRY(check_ld(name, "ldx", ldx, H, 8));
    BGNN_TRY(check_ld(name, "ldo", ldo, H, 8));
    BGNN_TRY(check_heavy_plan(name, csr, partial));
    // the compact state stores a light row's argmax as a byte offset (deg <= chunk) and marks heavy
    // rows with 255 (bgnn_spmm_fwd has the same rule)
    BGNN_REQUIRE(!arg || (csr->chunk > 0 && csr->chunk < 255),
                 "spmm_max_bf16(arg): the CSR's chunk must be in [1, 254] for the compact argmax (got %d)", csr->chunk);
    MaxArgs A{};
    int go = 0;
    BGNN_TRY(check_aligned_and_fill(name, "x / out / arg / partial", csr, x, ldx, H, out, arg, partial, A, &go));
    if (!go) return BGNN_OK;
    A.out = static_cast<uint16_t*>(out);
    A.ldo = ldo;
    // an argmax run takes one row per wave (the group form would resolve an argmax per key and row)
    if (!arg) {
        const GatherKernels<MaxArgs> K = {k_max_group<8, 4>,  k_max_group<4, 8>,    k_max_row<false>,
                                          k_max_chunk<false>, k_max_combine<false>, 64};
        return launch_gather(csr, A, K, stream);
    }
    const MaxArgLayout L = max_arg_layout(csr->n_rows, H);
    A.arg8 = static_cast<uint8_t*>(arg);
    A.heavy_of = reinterpret_cast<int32_t*>(static_cast<char*>(arg) + L.heavy_of);
    A.arg_h = reinterpret_cast<int32_t*>(static_cast<char*>(arg) + L.arg_h);
    A.partial_arg = partial ? reinterpret_cast<int32_t*>(partial + (int64_t)csr->n_chunks * H) : nullptr;
    const GatherKernels<MaxArgs> K = {nullptr,           nullptr,             k_max_row<true>,
                                      k_max_chunk<true>, k_max_combine<true>, 64};
    return launch_gather(csr, A, K, stream);
}
