// Neighbour aggregation of bf16 rows with a plain store epilogue, and its transpose
// (bgnn_spmm_fwd_bf16 / bgnn_spmm_bwd_bf16):
//   forward : out[r] = s_r * sum_{e in row r} x[col[e]]          s_r = 1, or 1 / max(deg r, 1) (MEAN)
//   backward: gx[j]  = sum_{q in rowT j} w(t_q) * g[t_q]         w(t) = 1, or 1 / max(deg_fwd t, 1)
// bf16 rows in, f32 accumulation, one rounding at the store (bf16, or f32 with out_f32).
//
// The gather is b16_gather.h's skeleton: light rows (deg <= chunk) on the CSR's row-group plan, or
// one row per wave for a CSR without a plan; heavy rows per chunk into f32 partials, combined in
// chunk order by one block per row. This file adds the policy -- a sum, for the transposed MEAN
// weighted per key -- and the epilogue, a scaled store. No atomics: every row's summation order is
// fixed by the plan, so results are bit-identical run to run.
#include "common.h"
#include "seg_common.h"
#include "b16_gather.h"

namespace bgnn {

namespace {

struct B16Args : GatherArgs {
    const int32_t* wrp;                     // weighted (transposed MEAN): the forward rowptr
    void* out;              int64_t ldo;
    int32_t out_f32, mean;                  // mean: scale row r by 1 / max(deg r, 1) (forward MEAN)
};

// WT: the transposed MEAN, where source row t weighs 1 / max(forward in-degree of t, 1). On the
// row-group plan the product is rounded once per key and added per row; where a key feeds one row
// it is one fma.
template <bool WT>
struct Sum {
    static constexpr bool kWeighted = WT;
    const int32_t* wrp;
    __device__ __forceinline__ float weight(int32_t t) const { return inv_deg(wrp[t + 1] - wrp[t]); }
    static __device__ __forceinline__ float init() { return 0.f; }
    static __device__ __forceinline__ float prepare(float f, float w) { return WT ? __fmul_rn(w, f) : f; }
    static __device__ __forceinline__ float absorb(float a, float f) { return a + f; }
    static __device__ __forceinline__ float absorb_weighted(float a, float f, float w) { return fmaf(w, f, a); }
};

// Row r's result, held by the lanes with ok: scaled (forward MEAN) and stored once, non-temporal.
__device__ __forceinline__ void store_row(const B16Args& A, int64_t r, int32_t deg, const float (&a)[8], int c) {
    const float sc = A.mean ? inv_deg(deg) : 1.f;
    float y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[q] = __fmul_rn(a[q], sc);
    store8_nt(A.out, r * A.ldo, c, A.out_f32, y);
}

template <int R>
struct GroupStore {
    const B16Args& A;
    __device__ __forceinline__ void operator()(int64_t r0, int rows, int32_t rp, int32_t chunk, float (&a)[R][8],
                                               int cs, bool ok) const {
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int32_t rb = __builtin_amdgcn_readlane(rp, t);
            const int32_t deg = __builtin_amdgcn_readlane(rp, t + 1) - rb;
            if (t >= rows || deg > chunk) continue;   // heavy row: chunk + combine
            if (ok) store_row(A, r0 + t, deg, a[t], cs);
        }
    }
};

// Light rows on the row-group plan, the scaled store as the epilogue.
template <int R, int U, bool WT>
__global__ __launch_bounds__(256) void k_b16_group(B16Args A) {
    walk_groups<R, U>(A, Sum<WT>{A.wrp}, GroupStore<R>{A});
}

// Light rows without a row-group plan: one row per wave, CSR order.
template <bool WT>
__global__ __launch_bounds__(256) void k_b16_row(B16Args A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < A.n_rows; r += (int64_t)gridDim.x * 4) {
        const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
        if (end - beg > A.chunk) continue;   // heavy row: chunk + combine
        float a[8];
        fill(a, Sum<WT>::init());
        gather_edges(A, Sum<WT>{A.wrp}, beg, end, cs, a);
        if (ok) store_row(A, r, end - beg, a, cs);
    }
}

// Heavy chunks: one wave per chunk -> partial[c, :] (f32).
template <bool WT>
__global__ __launch_bounds__(256) void k_b16_chunk(B16Args A) {
    chunk_body<false>(A, Sum<WT>{A.wrp}, nullptr);
}

// Combine heavy rows: one block of 16 waves per heavy row; wave 0 stores the row's sum.
__global__ __launch_bounds__(1024) void k_b16_combine(B16Args A) {
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x;
    if (h >= A.n_heavy) return;   // uniform over the block
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    const int64_t r = A.heavy_row[h];
    const int32_t deg = A.rowptr[r + 1] - A.rowptr[r];
    float a[8];
    if (!combine_chunks(A, h, cs, ok, a) || !ok) return;
    store_row(A, r, deg, a, cs);
}

template <bool WT>
int launch(const bgnn_csr_t* csr, B16Args& A, void* stream) {
    const GatherKernels<B16Args> K = {k_b16_group<8, 4, WT>, k_b16_group<4, 8, WT>, k_b16_row<WT>,
                                      k_b16_chunk<WT>,       k_b16_combine,         64 * kCombineWaves};
    return launch_gather(csr, A, K, stream);
}

// Both entry points (name: the entry point; xn / ldxn / on / ldon: its operand names; ops: the
// aligned operands in words). bwd: the transpose, whose MEAN weighs key t by fwd_rowptr's degree of
// t where the forward's scales the finished row.
int run(const char* name, const char* xn, const char* ldxn, const char* on, const char* ldon, const char* ops,
        bool bwd, const bgnn_csr_t* csr, const int32_t* fwd_rowptr, const void* x, int64_t ldx, int32_t H,
        int32_t reduce, void* out, int64_t ldo, int32_t out_f32, float* partial, void* stream) {
    B16Args A{};
    int go = 0;
    BGNN_TRY(check_operands(name, xn, on, "H<=512", csr, x, out, H, reduce));
    BGNN_TRY(check_ld(name, ldxn, ldx, H, 8));
    BGNN_TRY(check_ld(name, ldon, ldo, H, out_f32 ? 4 : 8));
    BGNN_TRY(check_heavy_plan(name, csr, partial));
    BGNN_TRY(check_aligned_and_fill(name, ops, csr, x, ldx, H, out, nullptr, partial, A, &go));
    const bool mean = reduce == BGNN_REDUCE_MEAN;
    BGNN_REQUIRE(!(bwd && mean) || fwd_rowptr, "spmm_bwd_bf16: MEAN needs fwd_rowptr");
    if (!go) return BGNN_OK;
    A.out = out;
    A.ldo = ldo;
    A.out_f32 = out_f32 ? 1 : 0;
    A.mean = !bwd && mean;
    if (!(bwd && mean)) return launch<false>(csr, A, stream);
    A.wrp = fwd_rowptr;
    return launch<true>(csr, A, stream);
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_spmm_fwd_bf16(const bgnn_csr_t* csr, const void* x, int64_t ldx, int32_t H, int32_t reduce,
                                  void* out, int64_t ldo, int32_t out_f32, float* partial, void* stream) {
    return run("spmm_fwd_bf16", "x", "ldx", "out", "ldo", "x / out / partial", false, csr, nullptr, x, ldx, H, reduce,
               out, ldo, out_f32, partial, stream);
}

extern "C" int bgnn_spmm_bwd_bf16(const bgnn_csr_t* csr_t, const int32_t* fwd_rowptr, const void* g, int64_t ldg,
                                  int32_t H, int32_t reduce, void* gx, int64_t ldgx, int32_t out_f32,
                                  float* partial, void* stream) {
    return run("spmm_bwd_bf16", "g", "ldg", "gx", "ldgx", "g / gx / partial", true, csr_t, fwd_rowptr, g, ldg, H,
               reduce, gx, ldgx, out_f32, partial, stream);
}
