// Eval-mode GraphSAGE layer on bf16 rows (bgnn_sage_infer_bf16): the neighbour aggregation of
// bf16 z_l rows with the whole layer tail in its epilogue,
//   h = s_i * sum_e z_l[col[e]] + z_r[i] + b;  o = h / max(||h||, 1e-12);
//   y = ReLU(o * scale + shift) (+ x_prev[i]),
// everything in f32 with one rounding at the store (bf16, or f32 for the last layer). BatchNorm
// is in eval mode, so scale / shift are known before the layer starts (bgnn_bn_eval_coeffs) and
// the f32 o [N, H] round trip between bgnn_sage_fwd and bgnn_sage_apply disappears.
//
// The gather is b16_gather.h's skeleton with a plain sum as the policy: light rows (deg <= chunk)
// on the CSR's row-group plan, or one row per wave for a CSR without a plan; heavy rows (super
// nodes) per chunk into f32 partials, combined in chunk order by a block. This file adds the
// epilogue: the layer tail (sage_tail.h), for which a group loads its rows' z_r / x_prev before the
// first tail. No atomics; the summation order of every row is fixed by the plan, so results are
// deterministic run to run.
#include "common.h"
#include "seg_common.h"
#include "b16_gather.h"
#include "sage_tail.h"

namespace bgnn {

namespace {

// x / ldx: bf16 z [N, 2H] with its ldz: z_l = cols [0, H) (the gathered rows), z_r = cols [H, 2H)
struct InferArgs : GatherArgs {
    TailArgs T;
};

struct Sum {
    static constexpr bool kWeighted = false;
    static __device__ __forceinline__ float init() { return 0.f; }
    static __device__ __forceinline__ float prepare(float f, float) { return f; }
    static __device__ __forceinline__ float absorb(float a, float f) { return a + f; }
};

// row r's own stream-once loads, then its tail
__device__ __forceinline__ uint4 load_zr(const InferArgs& A, int64_t r, int cs) {
    return ld16_nt(A.x + r * A.ldx + A.H + cs);
}
__device__ __forceinline__ uint4 load_xprev(const InferArgs& A, int64_t r, int cs) {
    return A.T.xprev ? ld16_nt(A.T.xprev + r * A.T.ldxp + cs) : make_uint4(0, 0, 0, 0);
}

// A group's epilogue: the rows' z_r / x_prev loads, all issued before the first tail.
template <int R>
struct GroupTail {
    const InferArgs& A;
    const Coef& C;
    __device__ __forceinline__ void operator()(int64_t r0, int rows, int32_t rp, int32_t chunk, float (&a)[R][8],
                                               int cs, bool ok) const {
        uint4 zq[R], xq[R];
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int64_t r = r0 + (t < rows ? t : 0);
            zq[t] = load_zr(A, r, cs);
            xq[t] = load_xprev(A, r, cs);
        }
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int32_t rb = __builtin_amdgcn_readlane(rp, t);
            const int32_t deg = __builtin_amdgcn_readlane(rp, t + 1) - rb;
            if (t >= rows || deg > chunk) continue;   // heavy row: chunk + combine
            infer_tail(A.T, C, r0 + t, deg, a[t], zq[t], xq[t], cs, ok);
        }
    }
};

// Light rows on the row-group plan, the layer tail as the epilogue.
template <int R, int U>
__global__ __launch_bounds__(256) void k_infer_group(InferArgs A) {
    __shared__ __attribute__((aligned(16))) Coef C;
    stage_coef(A.T, A.H, C);
    walk_groups<R, U>(A, Sum{}, GroupTail<R>{A, C});
}

// Light rows without a row-group plan: one row per wave, CSR order.
__global__ __launch_bounds__(256) void k_infer_row(InferArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    __shared__ __attribute__((aligned(16))) Coef C;
    stage_coef(A.T, A.H, C);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < A.n_rows; r += (int64_t)gridDim.x * 4) {
        const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
        if (end - beg > A.chunk) continue;   // heavy row: chunk + combine
        const uint4 zq = load_zr(A, r, cs), xq = load_xprev(A, r, cs);
        float a[8];
        fill(a, Sum::init());
        gather_edges(A, Sum{}, beg, end, cs, a);
        infer_tail(A.T, C, r, end - beg, a, zq, xq, cs, ok);
    }
}

// Heavy chunks: one wave per chunk -> partial[c, :] (f32).
__global__ __launch_bounds__(256) void k_infer_chunk(InferArgs A) { chunk_body<false>(A, Sum{}, nullptr); }

// Combine heavy rows: one block of 16 waves per heavy row; wave 0 runs the tail on the row's sum.
__global__ __launch_bounds__(1024) void k_infer_combine(InferArgs A) {
    __shared__ __attribute__((aligned(16))) Coef C;
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x;
    if (h >= A.n_heavy) return;   // uniform over the block
    stage_coef(A.T, A.H, C);
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    const int64_t r = A.heavy_row[h];
    const int32_t deg = A.rowptr[r + 1] - A.rowptr[r];
    float a[8];
    if (!combine_chunks(A, h, cs, ok, a)) return;
    infer_tail(A.T, C, r, deg, a, load_zr(A, r, cs), load_xprev(A, r, cs), cs, ok);
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_sage_infer_bf16(const bgnn_csr_t* csr, const void* z, int64_t ldz, const float* bias,
                                    const float* scale, const float* shift, const void* x_prev, int64_t ldx,
                                    int32_t H, int32_t reduce, void* out, int64_t ldo, int32_t out_f32,
                                    float* partial, void* stream) {
    const char* name = "sage_infer_bf16";
    BGNN_TRY(check_operands(name, "z", "out", "H<=512", csr, z, out, H, reduce));
    BGNN_REQUIRE(ldz >= 2 * (int64_t)H && ldz % 8 == 0, "sage_infer_bf16: ldz must be >= 2H and a multiple of 8");
    if (x_prev) BGNN_TRY(check_ld(name, "ldx", ldx, H, 8));
    BGNN_TRY(check_ld(name, "ldo", ldo, H, out_f32 ? 4 : 8));
    BGNN_REQUIRE((scale == nullptr) == (shift == nullptr), "sage_infer_bf16: scale and shift go together");
    BGNN_TRY(check_heavy_plan(name, csr, partial));
    InferArgs A{};
    int go = 0;
    BGNN_TRY(check_aligned_and_fill(name, "z / x_prev / out / partial", csr, z, ldz, H, out, x_prev, partial, A, &go));
    if (!go) return BGNN_OK;
    A.T.bias = bias;
    A.T.scale = scale;
    A.T.shift = shift;
    A.T.xprev = static_cast<const uint16_t*>(x_prev);
    A.T.ldxp = ldx;
    A.T.out = out;
    A.T.ldo = ldo;
    A.T.out_f32 = out_f32 ? 1 : 0;
    A.T.mean = reduce == BGNN_REDUCE_MEAN;
    const GatherKernels<InferArgs> K = {k_infer_group<8, 4>, k_infer_group<4, 8>, k_infer_row,
                                        k_infer_chunk,       k_infer_combine,     64 * kCombineWaves};
    return launch_gather(csr, A, K, stream);
}
