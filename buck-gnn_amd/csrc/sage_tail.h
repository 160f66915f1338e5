// The eval-mode SAGE layer tail on bf16 rows, shared by bgnn_sage_infer_bf16 (sage_infer.hip: the
// tail as the aggregation's epilogue) and bgnn_sage_tail_bf16 (sage_tail.hip: the tail alone, on a
// finished y = [agg | x] [W_l | W_r]^T). Both compile this one function, with -ffp-contract=off.
#pragma once

#include "b16_gather.h"   // ld16_nt, store8_nt; common.h and seg_common.h with it

namespace bgnn {

// What the tail reads and writes besides the row's own h terms. The row width H is its caller's
// (GatherArgs::H in sage_infer.hip), and so is the name ldx: x_prev's leading dimension is ldxp.
struct TailArgs {
    const float* bias;
    const float* scale;
    const float* shift;
    const uint16_t* xprev;  int64_t ldxp;   // bf16 [N, H] or NULL
    void* out;              int64_t ldo;
    int32_t out_f32, mean;
};

// Per-channel coefficients of the tail in LDS: bias (0 when NULL), scale and shift (when given).
struct Coef {
    float b[512], sc[512], sh[512];
};

__device__ __forceinline__ void stage_coef(const TailArgs& A, int32_t H, Coef& C) {
    for (int c = threadIdx.x; c < H; c += blockDim.x) {
        C.b[c] = A.bias ? A.bias[c] : 0.f;
        if (A.scale) {
            C.sc[c] = A.scale[c];
            C.sh[c] = A.shift[c];
        }
    }
    __syncthreads();
}

// The layer tail of row r, held by a full wave: lane owns columns [c, c + 8) (ok: inside H; a
// lane outside H passes c = 0 and only takes part in the norm's wave sum, with zeros).
//   h = s * a + zq + b;  o = h / max(||h||, 1e-12);  y = ReLU(o * scale + shift) (+ xq)
__device__ __forceinline__ void infer_tail(const TailArgs& A, const Coef& C, int64_t r, int32_t deg,
                                           const float (&a)[8], const uint4 zq, const uint4 xq, int c, bool ok) {
    const float sc = A.mean ? inv_deg(deg) : 1.f;
    float zr[8], h[8];
    bf16x8_unpack(zq, zr);
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        h[q] = ok ? sage_h(a[q], sc, zr[q], C.b[c + q]) : 0.f;
        ss = fmaf(h[q], h[q], ss);
    }
    ss = group_sum(ss, kWave);
    const float d = fmaxf(sqrtf(ss), 1e-12f);
    if (!ok) return;
    float y[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        float o = h[q] / d;
        if (A.scale) o = fmaf(o, C.sc[c + q], C.sh[c + q]);
        y[q] = fmaxf(o, 0.f);
    }
    if (A.xprev) {
        float xp[8];
        bf16x8_unpack(xq, xp);
#pragma unroll
        for (int q = 0; q < 8; ++q) y[q] += xp[q];
    }
    store8_nt(A.out, r * A.ldo, c, A.out_f32, y);
}

}  // namespace bgnn
