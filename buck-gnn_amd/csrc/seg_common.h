// Helpers shared by the CSR aggregation kernels (spmm.hip, and through b16_gather.h the bf16 ones:
// sage_infer.hip, spmm_b16.hip, spmm_max_b16.hip), the tail (sage_tail.h) and the bf16 element-wise
// kernels (elem.hip): the canonical SAGE row arithmetic, the XCD sweep's row assignment and grid, a
// lane's column positions, the four-wave slot tree, the MAX argmax state's layout and the bf16
// pack / unpack of one 16-byte vector.
#pragma once

#include "common.h"

namespace bgnn {

// 1 / max(deg, 1), correctly rounded, identical in every kernel (MEAN backward weights)
__device__ __forceinline__ float inv_deg(int32_t d) { return __frcp_rn((float)(d > 0 ? d : 1)); }

// Canonical SAGE row arithmetic, written with explicit roundings so that every kernel
// (blocked, sweep, combine: spmm.hip's sage_row) produces bit-identical o / nrm regardless of how
// the compiler would contract it: h = (a * sc + zr) + b, ss = fma(h, h, ss).
__device__ __forceinline__ float sage_h(float a, float sc, float zr, float b) {
    return __fadd_rn(__fadd_rn(__fmul_rn(a, sc), zr), b);
}

template <int VEC, int NV, int LPR>
__device__ __forceinline__ void lane_cols(int cb, int lir, int H, int (&cpos)[NV], bool (&cok)[NV]) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        cpos[v] = cb + (lir + LPR * v) * VEC;
        cok[v] = cpos[v] < H;
    }
}

// Row (or row-group) assignment of the XCD sweep kernels: the grid (a multiple of 8 blocks) is
// split into the 8 groups of blocks that share an XCD under round-robin dispatch (b % 8). Group x
// owns the contiguous region [x*N/8, (x+1)*N/8) and its 4*G/8 waves sweep that region together:
// wave q takes lo + q, lo + q + W, lo + q + 2W, ... (spmm.hip, "XCD sweep kernel").
struct Sweep {
    int64_t lo, hi, first;
    int W, T;
};

__device__ __forceinline__ Sweep sweep_rows(int64_t n_rows, int wave) {
    Sweep s;
    const int G = gridDim.x;                 // multiple of 8
    const int x = blockIdx.x & 7, i = blockIdx.x >> 3;
    const int64_t lo = n_rows * x / kNumXcd, hi = n_rows * (x + 1) / kNumXcd;
    s.W = 4 * (G >> 3);
    s.lo = lo;
    s.hi = hi;
    s.first = lo + i * 4 + wave;
    s.T = s.first < hi ? (int)((hi - s.first + s.W - 1) / s.W) : 0;
    return s;
}

// The grid of a sweep kernel: at most one row / group per wave (4 per block), at most `cap` blocks,
// a multiple of 8 (one share per XCD).
inline int64_t grid8(int64_t waves_wanted, int64_t cap) {
    int64_t blocks = (waves_wanted + 3) / 4;
    if (blocks > cap) blocks = cap;
    blocks = (blocks + 7) / 8 * 8;
    return blocks < 8 ? 8 : blocks;
}

// The heavy rows' combine: the waves of its block (SUM / MEAN), each summing one contiguous run of
// the row's chunks.
constexpr int kCombineWaves = 16;

// A block's slot from its four waves' LDS partials red[wave][q][c]: a fixed tree.
template <int Q, int C>
__device__ __forceinline__ float wave_tree(const float (&red)[4][Q][C], int q, int c) {
    return (red[0][q][c] + red[1][q][c]) + (red[2][q][c] + red[3][q][c]);
}

// The MAX argmax state (bgnn_spmm_max_arg_bytes), written by bgnn_spmm_fwd(MAX) and
// bgnn_spmm_max_bf16 and read by bgnn_spmm_bwd_max: a uint8 [rows, H] plane of edge offsets (heavy
// rows hold kArgHeavy), then heavy_of int32 [rows], then arg_h int32 [n_heavy, H], each 256-byte
// aligned.
constexpr uint8_t kArgHeavy = 255;
// The offset a writer stores for a column of a row with deg > 0: g = the winner's CSR position, or
// -1 when no edge won (every neighbour -inf or NaN: the strict > never fires). Such a column takes
// offset 0, the row's first edge, so every stored offset is in [0, deg) and the backward never
// takes a light row for a heavy one (include/bgnn.h, the MAX argmax state).
__device__ __forceinline__ int32_t arg_offset(int32_t g, int32_t rb) { return g < 0 ? 0 : g - rb; }
struct MaxArgLayout {
    int64_t heavy_of, arg_h;
};
inline MaxArgLayout max_arg_layout(int64_t rows, int64_t H) {
    MaxArgLayout L;
    L.heavy_of = (int64_t)align_up((size_t)(rows * H), 256);
    L.arg_h = L.heavy_of + (int64_t)align_up((size_t)(rows * 4), 256);
    return L;
}

// bf16 storage: 8 elements per 16-byte vector, widened exactly / rounded to nearest even
__device__ __forceinline__ void bf16x8_unpack(const uint4 q, float (&f)[8]) {
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int h = 0; h < 4; ++h) {
        f[2 * h] = __uint_as_float(w[h] << 16);
        f[2 * h + 1] = __uint_as_float(w[h] & 0xffff0000u);
    }
}

__device__ __forceinline__ uint32_t bf16_pack2(float x, float y) {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const f32x2 v = {x, y};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

}  // namespace bgnn
