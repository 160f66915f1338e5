// Shared helpers for the libbgnn HIP kernels (gfx950 / CDNA4, wave64).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>

#include "../../include/bgnn.h"

namespace bgnn {

constexpr int kWave = 64;     // CDNA wavefront width (hard-coded, see guide §1)
constexpr int kNumXcd = 8;    // MI355X: 8 XCDs, each with its own L2

// ---- error reporting (per calling thread; never crosses the ABI as an exception)
void set_error(const char* fmt, ...);
int fail(int code, const char* fmt, ...);

#define BGNN_HIP(expr)                                                              \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess)                                                       \
            return ::bgnn::fail((int)_e, "%s failed: %s (%s:%d)", #expr,            \
                                hipGetErrorString(_e), __FILE__, __LINE__);         \
    } while (0)

#define BGNN_CHECK_LAUNCH() BGNN_HIP(hipGetLastError())

#define BGNN_REQUIRE(cond, ...)                                                     \
    do {                                                                            \
        if (!(cond)) return ::bgnn::fail(BGNN_E_ARG, __VA_ARGS__);                  \
    } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bijective XCD-aware remap of a block index (cdna_hip_programming.md §5, T1):
// blocks b and b+8 share an XCD under round-robin dispatch, so give every group of
// blocks that shares an XCD a contiguous range of logical tiles (L2 locality for
// mesh neighbourhoods). Speed only — correctness never depends on placement.
__device__ __forceinline__ int xcd_remap(int b, int nblk) {
    const int q = nblk / kNumXcd, r = nblk % kNumXcd;
    const int x = b % kNumXcd, i = b / kNumXcd;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// xcd_remap with each XCD's share walked from its last block down
__device__ __forceinline__ int xcd_remap_rev(int b, int nblk) {
    const int q = nblk / kNumXcd, r = nblk % kNumXcd;
    const int x = b % kNumXcd, i = b / kNumXcd;
    const int len = x < r ? q + 1 : q;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + len - 1 - i;
}

// Wave-wide sum over groups of `width` lanes (width a power of two ≤ 64).
__device__ __forceinline__ float group_sum(float v, int width) {
    for (int m = width >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// Fold a thread's running max |value| (f32 bits) into *amax: block max over 256 threads,
// then one atomic per block (same-address atomics serialise in L2). Must be reached by every
// thread of the block.
__device__ __forceinline__ void block_amax(uint32_t* amax, uint32_t m) {
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, kWave));
    __shared__ uint32_t red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        if (m) atomicMax(amax, m);
    }
}

// Store tail of a column-sum pass over [rows, C] with C4 = C / 4 threads per row and 256 / C4 row
// phases per block: thread t = ph * C4 + c4 brings the two sums s0 / s1 of its float4 column over
// its phase's rows; they are added over the phases in phase order and stored as the two halves of
// the block's partial slot dst[2][C]. Must be reached by every thread of the block.
__device__ __forceinline__ void block_col_partials(const float (&s0)[4], const float (&s1)[4], int C, float* dst) {
    __shared__ __attribute__((aligned(16))) float red[256][8];
    const int C4 = C / 4, rpi = 256 / C4, t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) { red[t][k] = s0[k]; red[t][4 + k] = s1[k]; }
    __syncthreads();
    if (t < C4) {
        float a0[4] = {0.f, 0.f, 0.f, 0.f}, a1[4] = {0.f, 0.f, 0.f, 0.f};
        for (int q = 0; q < rpi; ++q)
#pragma unroll
            for (int k = 0; k < 4; ++k) { a0[k] += red[q * C4 + t][k]; a1[k] += red[q * C4 + t][4 + k]; }
        *reinterpret_cast<float4*>(dst + 4 * t) = make_float4(a0[0], a0[1], a0[2], a0[3]);
        *reinterpret_cast<float4*>(dst + C + 4 * t) = make_float4(a1[0], a1[1], a1[2], a1[3]);
    }
}

// Counter-based dropout hash: 64 random bits for (seed, 4-element group index).
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// keep-mask bits for the 4 elements [4*g, 4*g+4): element k kept iff its 16-bit
// lane of the hash is >= threshold (threshold = round(p * 65536)).
__device__ __forceinline__ uint32_t keep_bits4(uint64_t seed, uint64_t g, uint32_t thr) {
    const uint64_t h = mix64(seed ^ (g * 0xD1B54A32D192ED03ull));
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) m |= (((uint32_t)(h >> (16 * k)) & 0xFFFFu) >= thr ? 1u : 0u) << k;
    return m;
}

static inline uint32_t dropout_threshold(float p) {
    if (!(p > 0.f)) return 0u;
    double t = (double)p * 65536.0 + 0.5;
    if (t > 65536.0) t = 65536.0;
    return (uint32_t)t;
}

// Dropout(p) as the row kernels take it: the keep threshold and the kept elements' scale
struct Dropout {
    uint32_t thr;
    float inv_keep;
};
static inline Dropout dropout_of(float p) {
    const uint32_t thr = dropout_threshold(p);
    return {thr, thr ? 1.f / (1.f - p) : 1.f};
}

// GEMM kernel family (gemm.hip): 0 = f32 MFMA, 1 = bf16x6, 2 = f16x3 (f32-accurate split products)
void set_gemm_mode(int mode);
int gemm_mode();
// non-temporal output stores of the row-wise SAGE kernels (sage.hip)
void set_rows_nt(int on);
int rows_nt();
void set_rows_rev(int on);
int rows_rev();
// the aggregation kernels' knobs (spmm.hip; BGNN_TUNE_SEG_* / BGNN_TUNE_GROUP_BLOCKS, tuning.hip)
struct SegTuning {
    int kernel, grp_blocks, blocks, nt, u;
};
extern SegTuning g_seg;
// bgnn_spmm_fwd's combine of the heavy rows' chunk partials [n_chunks, H] into out [n_rows, H]
// (SUM / MEAN, float4 geometry: H % 4 == 0, 16-B aligned partial / out), launched alone (spmm.hip)
int seg_combine_plain(const bgnn_csr_t* csr, int32_t H, int32_t reduce, float* partial, float* out, hipStream_t s);

// 16-byte store, non-temporal (streamed once: no write-allocate in L2 / Infinity Cache)
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d, bool nt) {
    typedef float f32x4_t __attribute__((ext_vector_type(4)));
    const f32x4_t t = {a, b, c, d};
    if (nt) __builtin_nontemporal_store(t, reinterpret_cast<f32x4_t*>(p));
    else *reinterpret_cast<f32x4_t*>(p) = t;
}

}  // namespace bgnn
