// The eval-mode SAGE layer tail on finished bf16 rows (bgnn_sage_tail_bf16): the max-aggregation
// inference layer transforms [agg | x] in one GEMM, so its tail has no aggregation left to ride on:
//   h = y + b;  o = h / max(||h||, 1e-12);  v = ReLU(o * scale + shift) (+ x_prev),
// everything in f32 with one rounding at the store (bf16, or f32 for the last layer). This is
// infer_tail (sage_tail.h) with a zero aggregate: the function bgnn_sage_infer_bf16 compiles.
//
// Mapping: one wave per row, a lane owns 8 consecutive columns (one 16-byte load each of y and
// x_prev, both non-temporal: read once), the coefficients in LDS, a non-temporal store.
#include "common.h"
#include "seg_common.h"
#include "sage_tail.h"

namespace bgnn {

namespace {

struct RowTailArgs {
    int32_t H;
    TailArgs T;
    const uint16_t* y;      int64_t ldy;    // bf16 [n_rows, H]
    int64_t n_rows;
};

// rows per wave trip: all their loads are issued before the first tail (measured at N = 80,656,
// H = 512, 1024 blocks: 2 rows 70 us, 4 rows 69 us, 8 rows 87 us)
constexpr int kTailRows = 2;
// at most 4 blocks of 4 waves per CU, all resident at once (2048 blocks: 77 us against 70 us)
constexpr int64_t kTailMaxBlocks = 1024;

__global__ __launch_bounds__(256) void k_tail_row(RowTailArgs A) {
    constexpr int R = kTailRows;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool ok = lane * 8 < A.H;
    const int cs = ok ? lane * 8 : 0;
    __shared__ __attribute__((aligned(16))) Coef C;
    stage_coef(A.T, A.H, C);
    const float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int64_t step = (int64_t)gridDim.x * 4;
    for (int64_t r0 = (int64_t)blockIdx.x * 4 + wave; r0 < A.n_rows; r0 += R * step) {
        uint4 yq[R], xq[R];
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int64_t rt = r0 + t * step;
            const int64_t rl = rt < A.n_rows ? rt : r0;   // (wave-uniform) past the end: re-read the first row
            yq[t] = ld16_nt(A.y + rl * A.ldy + cs);
            xq[t] = A.T.xprev ? ld16_nt(A.T.xprev + rl * A.T.ldxp + cs) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int64_t rt = r0 + t * step;
            if (rt < A.n_rows) infer_tail(A.T, C, rt, 0, a, yq[t], xq[t], cs, ok);
        }
    }
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_sage_tail_bf16(const void* y, int64_t ldy, const float* bias, const float* scale,
                                   const float* shift, const void* x_prev, int64_t ldx, int64_t n_rows, int32_t H,
                                   void* out, int64_t ldo, int32_t out_f32, void* stream) {
    BGNN_REQUIRE(y && out, "sage_tail_bf16: null y / out");
    BGNN_REQUIRE(H > 0 && H % 8 == 0 && H <= 512, "sage_tail_bf16: H=%d unsupported (need H%%8==0, H<=512)", H);
    BGNN_REQUIRE(ldy >= H && ldy % 8 == 0, "sage_tail_bf16: ldy must be >= H and a multiple of 8");
    BGNN_REQUIRE(!x_prev || (ldx >= H && ldx % 8 == 0), "sage_tail_bf16: ldx must be >= H and a multiple of 8");
    BGNN_REQUIRE(ldo >= H && ldo % (out_f32 ? 4 : 8) == 0, "sage_tail_bf16: ldo must be >= H and a multiple of %d",
                 out_f32 ? 4 : 8);
    BGNN_REQUIRE((scale == nullptr) == (shift == nullptr), "sage_tail_bf16: scale and shift go together");
    BGNN_REQUIRE(aligned16(y) && aligned16(out) && (!x_prev || aligned16(x_prev)),
                 "sage_tail_bf16: y / x_prev / out must be 16-byte aligned");
    if (n_rows <= 0) return BGNN_OK;

    RowTailArgs A{};
    A.H = H;
    A.T.bias = bias;
    A.T.scale = scale;
    A.T.shift = shift;
    A.T.xprev = static_cast<const uint16_t*>(x_prev);
    A.T.ldxp = ldx;
    A.T.out = out;
    A.T.ldo = ldo;
    A.T.out_f32 = out_f32 ? 1 : 0;
    A.T.mean = 0;
    A.y = static_cast<const uint16_t*>(y);
    A.ldy = ldy;
    A.n_rows = n_rows;
    int64_t blocks = (n_rows + 4 * kTailRows - 1) / (4 * kTailRows);   // 4 waves, kTailRows rows per trip
    if (blocks > kTailMaxBlocks) blocks = kTailMaxBlocks;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_tail_row, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), A);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}
