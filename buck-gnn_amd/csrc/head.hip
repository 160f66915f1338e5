// The node-level decoder's tail as one kernel: y = ReLU(x W1^T + b1) W2^T + b2 per node,
// x [N, D0] (D0 = 64 or 128), W1 [64, D0], W2 [C, 64], 1 <= C <= 8 (Models/BuckGNN.py:76-100 for
// prediction_type static_disp / static_stress / mode_shape: the whole decoder at h <= 128, its
// last two Linears at h >= 256). The mirror image of the encoder's k_mlp2 (mlp.hip): the output
// is 4 to 32 bytes per node, so a library GEMM pair spends its time on the [N, 64] hidden
// activation it writes and reads back. Here a workgroup keeps both weights in LDS and runs 32
// nodes per tile through both layers on the VALU in fp32; nothing between the layers is stored.
//
// LDS (static, under 64 KB so that two workgroups fit a CU's 160 KB): W1 is kept ONCE, row-major
// [64][D0 + 4]. The hidden layer reads it with hidden unit tk + 16 c per lane (row stride D0 + 4
// words = 4 banks: 16 lanes x float4 cover the 64 banks once); the backward's dx = g1 W1 reads
// the same rows along f. A second, transposed copy (the k_mlp2 layout) would be 32 KB more at
// D0 = 128. With the 32-node x tile (16.5 KB at D0 = 128), the hidden tile (8.5 KB; the backward
// overwrites it in place with g1), W2 and the dy tile the backward uses 61.4 KB at D0 = 128.
//
// The backward recomputes the hidden layer from x with the same function (bit-identical to the
// forward's) and accumulates dW1 / db1 / dW2 / db2 per workgroup; two kernels sum the
// per-workgroup partials in a fixed order (no atomics: bit-identical from run to run).
//
// The forward also takes bf16 rows (bgnn_head2_fwd_bf16, eval-mode inference): only the x loader
// differs, widening each bf16 exactly into the same fp32 tile, so y has the f32 entry's bits on
// the widened rows.
#include "common.h"

namespace bgnn {

namespace {

constexpr int kHT = 32;            // nodes per tile
constexpr int kHD1 = 64;           // hidden width
constexpr int kHCmax = 8;          // output columns
constexpr int kHeadThreads = 256;
constexpr int kHeadFwdBlocks = 512;   // persistent workgroups, forward (two per CU)
constexpr int kHeadBwdBlocks = 256;   // backward: one partial slot each
constexpr int kHeadSumGroups = 16;

template <int D0>
struct HeadSmem {
    float w1[kHD1][D0 + 4];        // W1, row-major (row stride = 4 banks)
    float xs[kHT][D0 + 4];
    float h1[kHT][kHD1 + 4];       // hidden tile; the backward's g1 in place
    float w2[kHCmax][kHD1 + 4];    // W2 rows (rows >= C are zero)
    float gy[kHT][kHCmax];         // backward: dy tile (zero past N and past C)
    float b1[kHD1];
    float b2[kHCmax];
};

__device__ __forceinline__ float4 ldf4(const float* p) { return *reinterpret_cast<const float4*>(p); }

template <int D0>
__device__ __forceinline__ void head_load_weights(HeadSmem<D0>& S, const float* W1, const float* b1,
                                                  const float* W2, const float* b2, int C) {
    for (int i = threadIdx.x; i < kHD1 * D0; i += kHeadThreads) S.w1[i / D0][i % D0] = W1[i];
    for (int i = threadIdx.x; i < kHCmax * kHD1; i += kHeadThreads) {
        const int c = i / kHD1, k = i % kHD1;
        S.w2[c][k] = c < C ? W2[c * kHD1 + k] : 0.f;
    }
    for (int i = threadIdx.x; i < kHD1; i += kHeadThreads) S.b1[i] = b1 ? b1[i] : 0.f;
    for (int i = threadIdx.x; i < kHCmax; i += kHeadThreads) S.b2[i] = (b2 && i < C) ? b2[i] : 0.f;
}

// a bf16 row element: the high half of the f32 it widens to
struct HeadBf16 {
    uint16_t bits;
};

// the tile's x rows in 16-byte vectors (x 16-byte aligned, row stride ldx elements a multiple of
// the vector): 4 f32, or 8 bf16 widened exactly into the f32 tile; rows past N are zero
template <int D0, typename T>
__device__ __forceinline__ void head_load_x(HeadSmem<D0>& S, const T* x, int64_t ldx, int64_t n0, int64_t N) {
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int G = D0 / V;
    for (int i = threadIdx.x; i < kHT * G; i += kHeadThreads) {
        const int n = i / G, f = (i % G) * V;
        if constexpr (sizeof(T) == 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (n0 + n < N) v = ldf4(x + (n0 + n) * ldx + f);
            *reinterpret_cast<float4*>(&S.xs[n][f]) = v;
        } else {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (n0 + n < N) v = *reinterpret_cast<const uint4*>(x + (n0 + n) * ldx + f);
            *reinterpret_cast<float4*>(&S.xs[n][f]) =
                make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u),
                            __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
            *reinterpret_cast<float4*>(&S.xs[n][f + 4]) =
                make_float4(__uint_as_float(v.z << 16), __uint_as_float(v.z & 0xffff0000u),
                            __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xffff0000u));
        }
    }
}

// h1 = ReLU(x W1^T + b1) for the tile: thread = 2 nodes x hidden units tk, tk + 16, tk + 32,
// tk + 48; every unit's sum runs over f in order
template <int D0>
__device__ __forceinline__ void head_hidden(HeadSmem<D0>& S) {
    const int tn = threadIdx.x >> 4, tk = threadIdx.x & 15;
    float acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = S.b1[tk + 16 * c];
#pragma unroll 4
    for (int f = 0; f < D0; f += 4) {
        float4 w[4], xv[2];
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = ldf4(&S.w1[tk + 16 * c][f]);
#pragma unroll
        for (int i = 0; i < 2; ++i) xv[i] = ldf4(&S.xs[tn * 2 + i][f]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float a = acc[i][c];
                a = fmaf(xv[i].x, w[c].x, a);
                a = fmaf(xv[i].y, w[c].y, a);
                a = fmaf(xv[i].z, w[c].z, a);
                a = fmaf(xv[i].w, w[c].w, a);
                acc[i][c] = a;
            }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) S.h1[tn * 2 + i][tk + 16 * c] = fmaxf(acc[i][c], 0.f);
}

// forward: after the hidden tile, thread e < 32 C owns element e of the tile's [32, C] output
// block, which is contiguous in y: a wave stores one unbroken span
// (T = float: ldx is D0, a constant at the call; T = HeadBf16: the caller's row stride)
template <int D0, typename T>
__global__ __launch_bounds__(kHeadThreads) void k_head2_fwd(const T* __restrict__ x, int64_t ldx, int64_t N,
                                                            const float* W1, const float* b1, const float* W2,
                                                            const float* b2, int C, float* __restrict__ y) {
    __shared__ HeadSmem<D0> S;
    head_load_weights<D0>(S, W1, b1, W2, b2, C);
    const int e = threadIdx.x;
    const int en = e / C, ec = e - en * C;
    const int64_t tiles = (N + kHT - 1) / kHT;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t n0 = t * kHT;
        __syncthreads();
        head_load_x<D0>(S, x, sizeof(T) == 4 ? (int64_t)D0 : ldx, n0, N);
        __syncthreads();
        head_hidden<D0>(S);
        __syncthreads();
        if (en < kHT && n0 + en < N) {
            float a = S.b2[ec];
#pragma unroll
            for (int k = 0; k < kHD1; k += 4) {
                const float4 hv = ldf4(&S.h1[en][k]), wv = ldf4(&S.w2[ec][k]);
                a = fmaf(hv.x, wv.x, a);
                a = fmaf(hv.y, wv.y, a);
                a = fmaf(hv.z, wv.z, a);
                a = fmaf(hv.w, wv.w, a);
            }
            y[n0 * C + e] = a;
        }
    }
}

// Backward. dW2 += dy^T h1, db2 += sum dy;  g1 = (dy W2) (.) [h1 > 0];  dx = g1 W1;
// dW1 += g1^T x, db1 += sum g1. Per-workgroup partial: [dW1 64 D0 | db1 64 | dW2 64 C | db2 C],
// slot stride Lp = that length rounded up to 4 floats (float4 stores of dW1).
template <int D0>
__global__ __launch_bounds__(kHeadThreads) void k_head2_bwd(const float* __restrict__ x, int64_t N, const float* W1,
                                                            const float* b1, const float* W2, int C,
                                                            const float* __restrict__ dy, float* __restrict__ dx,
                                                            float* __restrict__ part, int Lp) {
    constexpr int FG = D0 / 4;                   // float4 column groups of x / W1
    constexpr int NG = kHeadThreads / FG;        // row groups: 8 (D0 = 128) or 16 (D0 = 64)
    constexpr int NPX = kHT / NG;                // dx: nodes per thread (4 or 2)
    constexpr int KP = kHD1 / NG;                // dW1: hidden units per thread (8 or 4)
    __shared__ HeadSmem<D0> S;
    head_load_weights<D0>(S, W1, b1, W2, nullptr, C);
    const int tid = threadIdx.x;
    const int k2 = tid & 63, cg = tid >> 6;      // dW2 rows cg and cg + 4, column k2; g1: rows cg * 8 ..
    const int fq = tid % FG, rg = tid / FG;      // dx / dW1: columns fq * 4 .., row group rg
    float dw2a = 0.f, dw2b = 0.f, db2a = 0.f, db2b = 0.f;
    float dw1[KP][4], db1[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        db1[j] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) dw1[j][q] = 0.f;
    }
    const int64_t tiles = (N + kHT - 1) / kHT;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t n0 = t * kHT;
        __syncthreads();
        head_load_x<D0>(S, x, (int64_t)D0, n0, N);
        {
            const int n = tid >> 3, c = tid & 7;
            S.gy[n][c] = (c < C && n0 + n < N) ? dy[(n0 + n) * C + c] : 0.f;
        }
        __syncthreads();
        head_hidden<D0>(S);
        __syncthreads();
        // layer-2 weight / bias gradients (rows of padded tail nodes are zero in gy)
        for (int n = 0; n < kHT; ++n) {
            const float hv = S.h1[n][k2];
            const float ga = S.gy[n][cg], gb = S.gy[n][cg + 4];
            dw2a = fmaf(ga, hv, dw2a);
            dw2b = fmaf(gb, hv, dw2b);
            if (k2 == 0) {
                db2a += ga;
                db2b += gb;
            }
        }
        __syncthreads();
        // g1 over h1, in place: each element is read (the ReLU mask) and written by one thread
#pragma unroll
        for (int i = 0; i < kHT / 4; ++i) {
            const int n = cg * (kHT / 4) + i;
            float s = 0.f;
            for (int c = 0; c < C; ++c) s = fmaf(S.gy[n][c], S.w2[c][k2], s);
            S.h1[n][k2] = S.h1[n][k2] > 0.f ? s : 0.f;
        }
        __syncthreads();
        // dx = g1 W1: thread = NPX nodes x 4 columns, the sum over k in order
        {
            float acc[NPX][4];
#pragma unroll
            for (int i = 0; i < NPX; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[i][q] = 0.f;
#pragma unroll 4
            for (int k = 0; k < kHD1; ++k) {
                const float4 w = ldf4(&S.w1[k][fq * 4]);
#pragma unroll
                for (int i = 0; i < NPX; ++i) {
                    const float g = S.h1[rg * NPX + i][k];
                    acc[i][0] = fmaf(g, w.x, acc[i][0]);
                    acc[i][1] = fmaf(g, w.y, acc[i][1]);
                    acc[i][2] = fmaf(g, w.z, acc[i][2]);
                    acc[i][3] = fmaf(g, w.w, acc[i][3]);
                }
            }
#pragma unroll
            for (int i = 0; i < NPX; ++i) {
                const int64_t node = n0 + rg * NPX + i;
                if (node < N)
                    *reinterpret_cast<float4*>(dx + node * D0 + fq * 4) =
                        make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
            }
        }
        // dW1 / db1: thread = KP hidden units x 4 columns, the sum over the tile's nodes in order
        for (int n = 0; n < kHT; ++n) {
            const float4 xv = ldf4(&S.xs[n][fq * 4]);
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                const float g = S.h1[n][rg * KP + j];
                dw1[j][0] = fmaf(g, xv.x, dw1[j][0]);
                dw1[j][1] = fmaf(g, xv.y, dw1[j][1]);
                dw1[j][2] = fmaf(g, xv.z, dw1[j][2]);
                dw1[j][3] = fmaf(g, xv.w, dw1[j][3]);
                if (fq == 0) db1[j] += g;
            }
        }
    }
    float* p = part + (int64_t)blockIdx.x * Lp;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        *reinterpret_cast<float4*>(p + (rg * KP + j) * D0 + fq * 4) =
            make_float4(dw1[j][0], dw1[j][1], dw1[j][2], dw1[j][3]);
        if (fq == 0) p[kHD1 * D0 + rg * KP + j] = db1[j];
    }
    float* p2 = p + kHD1 * D0 + kHD1;
    if (cg < C) p2[cg * kHD1 + k2] = dw2a;
    if (cg + 4 < C) p2[(cg + 4) * kHD1 + k2] = dw2b;
    if (k2 == 0) {
        if (cg < C) p2[C * kHD1 + cg] = db2a;
        if (cg + 4 < C) p2[C * kHD1 + cg + 4] = db2b;
    }
}

// two-stage, fixed-order slot sums (as mlp.hip's): stage 1 sums slot group y of column i into
// tmp[y][i]; stage 2 sums the groups in order into [dW1 | db1 | dW2 | db2]
__global__ __launch_bounds__(256) void k_head2_sum1(const float* __restrict__ part, int slots, int L, int Lp,
                                                    float* __restrict__ tmp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L) return;
    const int per = (slots + kHeadSumGroups - 1) / kHeadSumGroups;
    const int s0 = blockIdx.y * per, s1 = min(slots, s0 + per);
    float s = 0.f;
    for (int k = s0; k < s1; ++k) s += part[(int64_t)k * Lp + i];
    tmp[(int64_t)blockIdx.y * Lp + i] = s;
}

__global__ __launch_bounds__(256) void k_head2_sum2(const float* __restrict__ tmp, int L, int Lp, int L0, int L1, int L2,
                                                    float* __restrict__ o0, float* __restrict__ o1,
                                                    float* __restrict__ o2, float* __restrict__ o3) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= L) return;
    float s = 0.f;
    for (int k = 0; k < kHeadSumGroups; ++k) s += tmp[(int64_t)k * Lp + i];
    if (i < L0) o0[i] = s;
    else if (i < L0 + L1) o1[i - L0] = s;
    else if (i < L0 + L1 + L2) o2[i - L0 - L1] = s;
    else o3[i - L0 - L1 - L2] = s;
}

inline int head_blocks(int64_t N, int cap) {
    const int64_t tiles = (N + kHT - 1) / kHT;
    return (int)(tiles < cap ? (tiles > 0 ? tiles : 1) : cap);
}

inline int head_part_len(int D0, int C) { return kHD1 * D0 + kHD1 + kHD1 * C + C; }

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_head2_supported(int32_t D0, int32_t D1, int32_t C) {
    return (D0 == 64 || D0 == 128) && D1 == kHD1 && C >= 1 && C <= kHCmax;
}

extern "C" int bgnn_head2_geometry(int32_t which) {
    switch (which) {
        case 0: return kHT;
        case 1: return kHeadFwdBlocks;
        case 2: return kHeadBwdBlocks;
        default: return -1;
    }
}

extern "C" int bgnn_head2_fwd(const float* x, int64_t N, int32_t D0, int32_t D1, int32_t C, const float* W1,
                              const float* b1, const float* W2, const float* b2, float* y, void* stream) {
    BGNN_REQUIRE(bgnn_head2_supported(D0, D1, C), "head2: shape %dx%dx%d not built (D0 64 or 128, D1 64, C 1..8)", D0,
                 D1, C);
    BGNN_REQUIRE(N >= 0, "head2: N < 0");
    if (N == 0) return BGNN_OK;
    BGNN_REQUIRE(x && W1 && W2 && y, "head2: null pointer");
    BGNN_REQUIRE(aligned16(x), "head2: x must be 16-byte aligned");
    const int blocks = head_blocks(N, kHeadFwdBlocks);
    hipStream_t s = as_stream(stream);
    if (D0 == 64)
        hipLaunchKernelGGL((k_head2_fwd<64, float>), dim3(blocks), dim3(kHeadThreads), 0, s, x, (int64_t)64, N, W1, b1,
                           W2, b2, (int)C, y);
    else
        hipLaunchKernelGGL((k_head2_fwd<128, float>), dim3(blocks), dim3(kHeadThreads), 0, s, x, (int64_t)128, N, W1,
                           b1, W2, b2, (int)C, y);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

extern "C" int bgnn_head2_fwd_bf16(const void* x, int64_t ldx, int64_t N, int32_t D0, int32_t D1, int32_t C,
                                   const float* W1, const float* b1, const float* W2, const float* b2, float* y,
                                   void* stream) {
    BGNN_REQUIRE(bgnn_head2_supported(D0, D1, C), "head2_bf16: shape %dx%dx%d not built (D0 64 or 128, D1 64, C 1..8)",
                 D0, D1, C);
    BGNN_REQUIRE(N >= 0, "head2_bf16: N < 0");
    if (N == 0) return BGNN_OK;
    BGNN_REQUIRE(x && W1 && W2 && y, "head2_bf16: null pointer");
    BGNN_REQUIRE(aligned16(x), "head2_bf16: x must be 16-byte aligned");
    BGNN_REQUIRE(ldx >= D0 && ldx % 8 == 0, "head2_bf16: ldx=%lld must be >= D0 and a multiple of 8", (long long)ldx);
    const int blocks = head_blocks(N, kHeadFwdBlocks);
    hipStream_t s = as_stream(stream);
    const HeadBf16* xb = static_cast<const HeadBf16*>(x);
    if (D0 == 64)
        hipLaunchKernelGGL((k_head2_fwd<64, HeadBf16>), dim3(blocks), dim3(kHeadThreads), 0, s, xb, ldx, N, W1, b1, W2,
                           b2, (int)C, y);
    else
        hipLaunchKernelGGL((k_head2_fwd<128, HeadBf16>), dim3(blocks), dim3(kHeadThreads), 0, s, xb, ldx, N, W1, b1, W2,
                           b2, (int)C, y);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

extern "C" size_t bgnn_head2_bwd_ws_bytes(int64_t N, int32_t D0, int32_t C) {
    if (!bgnn_head2_supported(D0, kHD1, C)) return 0;
    const size_t Lp = align_up((size_t)head_part_len(D0, C), 4);
    return (size_t)(head_blocks(N, kHeadBwdBlocks) + kHeadSumGroups) * Lp * sizeof(float);
}

extern "C" int bgnn_head2_bwd(const float* x, int64_t N, int32_t D0, int32_t D1, int32_t C, const float* W1,
                              const float* b1, const float* W2, const float* dy, float* dx, float* dW1, float* db1,
                              float* dW2, float* db2, void* ws, size_t ws_bytes, void* stream) {
    BGNN_REQUIRE(bgnn_head2_supported(D0, D1, C), "head2: shape %dx%dx%d not built (D0 64 or 128, D1 64, C 1..8)", D0,
                 D1, C);
    BGNN_REQUIRE(N >= 0, "head2: N < 0");
    BGNN_REQUIRE(dW1 && db1 && dW2 && db2, "head2_bwd: null gradient output");
    hipStream_t s = as_stream(stream);
    if (N == 0) {
        BGNN_HIP(hipMemsetAsync(dW1, 0, sizeof(float) * kHD1 * D0, s));
        BGNN_HIP(hipMemsetAsync(db1, 0, sizeof(float) * kHD1, s));
        BGNN_HIP(hipMemsetAsync(dW2, 0, sizeof(float) * C * kHD1, s));
        BGNN_HIP(hipMemsetAsync(db2, 0, sizeof(float) * C, s));
        return BGNN_OK;
    }
    BGNN_REQUIRE(x && W1 && W2 && dy && dx, "head2_bwd: null pointer");
    BGNN_REQUIRE(aligned16(x) && aligned16(dx), "head2_bwd: x and dx must be 16-byte aligned");
    BGNN_REQUIRE(ws && aligned16(ws) && ws_bytes >= bgnn_head2_bwd_ws_bytes(N, D0, C),
                 "head2_bwd: workspace too small or not 16-byte aligned");
    const int blocks = head_blocks(N, kHeadBwdBlocks);
    const int L = head_part_len(D0, C), Lp = (int)align_up((size_t)L, 4);
    float* part = static_cast<float*>(ws);
    if (D0 == 64)
        hipLaunchKernelGGL((k_head2_bwd<64>), dim3(blocks), dim3(kHeadThreads), 0, s, x, N, W1, b1, W2, (int)C, dy, dx,
                           part, Lp);
    else
        hipLaunchKernelGGL((k_head2_bwd<128>), dim3(blocks), dim3(kHeadThreads), 0, s, x, N, W1, b1, W2, (int)C, dy, dx,
                           part, Lp);
    BGNN_CHECK_LAUNCH();
    float* tmp = part + (int64_t)blocks * Lp;
    hipLaunchKernelGGL(k_head2_sum1, dim3((L + 255) / 256, kHeadSumGroups), dim3(256), 0, s, part, blocks, L, Lp, tmp);
    BGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_head2_sum2, dim3((L + 255) / 256), dim3(256), 0, s, tmp, L, Lp, kHD1 * D0, kHD1, kHD1 * C,
                       dW1, db1, dW2, db2);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}
