// The eval-mode SAGE layer tail on bf16 rows, shared by bgnn_sage_infer_bf16 (sage_infer.hip: the
// tail as the aggregation's epilogue) and bgnn_sage_tail_bf16 (sage_tail.hip: the tail alone, on a
// finished y = [agg | x] [W_l | W_r]^T). Both compile this one function, with -ffp-contract=off.
#pragma once

#include "common.h"
#include "seg_common.h"

namespace bgnn {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 ld16(const uint16_t* p) { return *reinterpret_cast<const uint4*>(p); }

// stream-once rows (z_r, y, x_prev): non-temporal, so they do not displace gathered rows
__device__ __forceinline__ uint4 ld16_nt(const uint16_t* p) {
    const u32x4_t q = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p));
    return make_uint4(q[0], q[1], q[2], q[3]);
}

// What the tail reads and writes besides the row's own h terms.
struct TailArgs {
    int32_t H;
    const float* bias;
    const float* scale;
    const float* shift;
    const uint16_t* xprev;  int64_t ldx;    // bf16 [N, H] or NULL
    void* out;              int64_t ldo;
    int32_t out_f32, mean;
};

// Per-channel coefficients of the tail in LDS: bias (0 when NULL), scale and shift (when given).
struct Coef {
    float b[512], sc[512], sh[512];
};

__device__ __forceinline__ void stage_coef(const TailArgs& A, Coef& C) {
    for (int c = threadIdx.x; c < A.H; c += blockDim.x) {
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
    if (A.out_f32) {
        float* p = static_cast<float*>(A.out) + r * A.ldo + c;
        const f32x4_t v0 = {y[0], y[1], y[2], y[3]}, v1 = {y[4], y[5], y[6], y[7]};
        __builtin_nontemporal_store(v0, reinterpret_cast<f32x4_t*>(p));
        __builtin_nontemporal_store(v1, reinterpret_cast<f32x4_t*>(p + 4));
    } else {
        uint16_t* p = static_cast<uint16_t*>(A.out) + r * A.ldo + c;
        const u32x4_t v = {bf16_pack2(y[0], y[1]), bf16_pack2(y[2], y[3]), bf16_pack2(y[4], y[5]),
                           bf16_pack2(y[6], y[7])};
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4_t*>(p));
    }
}

}  // namespace bgnn
