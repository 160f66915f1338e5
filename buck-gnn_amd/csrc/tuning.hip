// The tuning knobs' entry points (bgnn_get_tuning / bgnn_set_tuning, include/bgnn.h BGNN_TUNE_*).
// The knobs themselves live with the kernels they steer: the aggregation's in spmm.hip (SegTuning),
// the row-wise SAGE kernels' in sage.hip, the GEMMs' in gemm.hip, gemm_x6.hip and gemm_h3p.hip.
// Process-wide; the defaults are the production choice.
#include "common.h"

namespace bgnn {

extern int g_x6_bdma;   // gemm_x6.hip
extern int g_x6_rowseg;
extern int g_h3p_nsb;   // gemm_h3p.hip
#ifdef BGNN_H3P_ABLATION
extern int g_h3p_abl;
#endif

}  // namespace bgnn

using namespace bgnn;

extern "C" int32_t bgnn_get_tuning(int32_t knob) {
    switch (knob) {
        case BGNN_TUNE_SEG_KERNEL: return g_seg.kernel;
        case BGNN_TUNE_SEG_BLOCKS: return g_seg.blocks;
        case BGNN_TUNE_SEG_U: return g_seg.u;
        case BGNN_TUNE_SEG_NT: return g_seg.nt;
        case BGNN_TUNE_GEMM_MODE: return gemm_mode();
        case BGNN_TUNE_ROWS_NT: return rows_nt();
        case BGNN_TUNE_GROUP_BLOCKS: return g_seg.grp_blocks;
        case BGNN_TUNE_ROWS_REV: return rows_rev();
        case BGNN_TUNE_GEMM_BDMA: return g_x6_bdma == 2 && g_h3p_nsb == 4 ? 3 : g_x6_bdma;
        case BGNN_TUNE_GEMM_CSTORE: return g_x6_rowseg;
        default: return -1;
    }
}

extern "C" int bgnn_set_tuning(int32_t knob, int32_t value) {
    switch (knob) {
        case BGNN_TUNE_SEG_KERNEL:
            BGNN_REQUIRE(value >= 0 && value <= 2, "set_tuning: kernel must be 0 (auto), 1 (blocked) or 2 (sweep)");
            g_seg.kernel = value;
            return BGNN_OK;
        case BGNN_TUNE_SEG_BLOCKS:
            BGNN_REQUIRE(value >= 8 && value <= 65536, "set_tuning: blocks out of range");
            g_seg.blocks = value;
            return BGNN_OK;
        case BGNN_TUNE_SEG_U:
            BGNN_REQUIRE(value == 0 || value == 8 || value == 12 || value == 16,
                         "set_tuning: U must be 0 (auto), 8, 12 or 16");
            g_seg.u = value;
            return BGNN_OK;
        case BGNN_TUNE_SEG_NT: g_seg.nt = value ? 1 : 0; return BGNN_OK;
        case BGNN_TUNE_GROUP_BLOCKS:
            BGNN_REQUIRE(value >= 8 && value <= 65536, "set_tuning: group blocks out of range");
            g_seg.grp_blocks = value;
            return BGNN_OK;
        case BGNN_TUNE_ROWS_NT: set_rows_nt(value); return BGNN_OK;
        case BGNN_TUNE_ROWS_REV: set_rows_rev(value); return BGNN_OK;
        case BGNN_TUNE_GEMM_BDMA:
#ifdef BGNN_H3P_ABLATION
            if (value >= 16) {   // measurement build: the pipelined kernel (4 slots) with ablation value / 16
                g_x6_bdma = 2;
                g_h3p_nsb = 4;
                g_h3p_abl = value / 16;
                return BGNN_OK;
            }
            g_h3p_abl = 0;
            BGNN_REQUIRE(value >= 0 && value <= 4, "set_tuning: gemm B staging must be 0 .. 4");
#else
            BGNN_REQUIRE(value == 0 || value == 2 || value == 3,
                         "set_tuning: gemm B staging must be 0 (k_gemm_x6, register copy) or 2 / 3 (the pipelined "
                         "kernel, 3 / 4 slots); 1 and 4 are measurement-build forms (make abl)");
#endif
            g_x6_bdma = value == 3 ? 2 : value;
            g_h3p_nsb = value == 3 ? 4 : 3;
            return BGNN_OK;
        case BGNN_TUNE_GEMM_CSTORE:
            BGNN_REQUIRE(value == 0 || value == 1, "set_tuning: gemm C store shape must be 0 (column blocks) or 1 "
                                                   "(row segments)");
            g_x6_rowseg = value;
            return BGNN_OK;
        case BGNN_TUNE_GEMM_MODE:
            BGNN_REQUIRE(value == 0 || value == 2, "set_tuning: gemm mode must be 0 (f32 MFMA) or 2 (f16x3)");
            set_gemm_mode(value);
            return BGNN_OK;
        default: return fail(BGNN_E_ARG, "set_tuning: unknown knob %d", knob);
    }
}
