// f16x3 GEMM C = A B^T with K-contiguous operands, as gemm_x6_nt.hip, with the row-segment C stores
// (knob BGNN_TUNE_GEMM_CSTORE = 1; x6_epilogue<ROWS>, gemm_x6.h): the same kernels with PPV bit 5, in
// a translation unit of their own so the two sets compile side by side.
#include "gemm_x6_kernel.h"

namespace bgnn {

void launch_x6_nt_rows(int cfg, int abl, dim3 grid, hipStream_t s, const GemmArgs& g) {
    if (abl == 8) launch_x6_a<1, 0, 1, 8, 32>(cfg, grid, s, g);
    else launch_x6_a<1, 0, 1, 0, 32>(cfg, grid, s, g);
}

}  // namespace bgnn
