// SAGPooling on bf16 rows (BuckGNN.infer_bf16_sag): the scorer and the gather of the kept rows.
//
// bgnn_sag_score_bf16 is SAGPooling(H, ratio, GNN=SAGEConv, aggr='add')'s score, transform first
// (sum aggregation is linear, and the scorer has one output channel), in two launches:
//   pass 1   s_l[i] = <x_i, w_l>, s_r[i] = <x_i, w_r>               -> ws [N, 2] f32
//   pass 2   attn[i] = sum_{e in row i, CSR order} s_l[col[e]] + b + s_r[i]
//            score[i] = tanh(sgn * attn[i])                          -> score [N] f32
// bgnn_gather_scale_bf16 is x[perm] * score[perm] (* multiplier) from bf16 rows to bf16 rows.
//
// Mapping of the two row passes (pass 1, the gather): a lane owns 8 consecutive columns, one
// 16-byte load of bf16; a row takes a group of G = the power of two >= H / 8 lanes and a wave
// 64 / G rows (H = 512: one row per wave, H = 64: eight). Pass 1 keeps a lane's 8 + 8 weights in
// registers, multiplies in f32 and adds its 8 products in column order, then the group's lanes in a
// fixed butterfly. Pass 2 gives a light row (in-degree <= the CSR plan's chunk) one lane, which adds
// in CSR order, and a heavy row a wave: lane l adds the edges l, l + 64, ... in order, then the 64
// lane sums meet in the same butterfly. No atomics and no LDS; every sum has one order, so the
// results are bit-identical run to run. Compiled without FMA contraction: a product is rounded,
// then added.
#include "common.h"
#include "seg_common.h"
#include "b16_gather.h"

namespace bgnn {

namespace {

constexpr int kSlabs = 4;   // wave row slabs in flight per step of a row pass

// lane group of a row of H columns: the power of two >= H / 8 (H <= 512: at most 64)
inline int group_lanes(int32_t H) {
    int g = 1;
    while (g * 8 < H) g *= 2;
    return g;
}

struct ScoreArgs {
    const uint16_t* x;   int64_t ldx;   // bf16 [N, H]
    int64_t N;
    int32_t H, G;
    const float* w_l;
    const float* w_r;
    float* ws;           // [N, 2]: s_l, s_r
};

// Pass 1: both dot products of every row.
__global__ __launch_bounds__(256) void k_sag_dots(ScoreArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = A.G, rpw = 64 / G;   // rows per wave slab
    const int sub = lane / G, c = (lane % G) * 8;
    const bool col_ok = c < A.H;
    float wl[8], wr[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        wl[q] = col_ok ? A.w_l[c + q] : 0.f;
        wr[q] = col_ok ? A.w_r[c + q] : 0.f;
    }
    const int64_t n_slabs = (A.N + rpw - 1) / rpw;
    const int64_t step = (int64_t)gridDim.x * 4 * kSlabs;
    for (int64_t s0 = ((int64_t)blockIdx.x * 4 + wave) * kSlabs; s0 < n_slabs; s0 += step) {   // wave-uniform
        uint4 v[kSlabs];
#pragma unroll
        for (int u = 0; u < kSlabs; ++u) {
            const int64_t r = (s0 + u) * rpw + sub;
            v[u] = (col_ok && r < A.N) ? ld16(A.x + r * A.ldx + c) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < kSlabs; ++u) {
            float f[8];
            bf16x8_unpack(v[u], f);
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                a += f[q] * wl[q];
                b += f[q] * wr[q];
            }
            a = group_sum(a, G);
            b = group_sum(b, G);
            const int64_t r = (s0 + u) * rpw + sub;
            if (c == 0 && r < A.N) *reinterpret_cast<float2*>(A.ws + 2 * r) = make_float2(a, b);
        }
    }
}

struct AttnArgs {
    const int32_t* rowptr;
    const int32_t* col;
    const int32_t* heavy_row;
    int64_t N;
    int32_t n_heavy, chunk;
    unsigned light_blocks;
    const float* ws;     // [N, 2]
    const float* bias;   // one element, or NULL
    float sgn;
    float* score;
};

__device__ __forceinline__ void store_score(const AttnArgs& A, int64_t r, float agg) {
    const float b = A.bias ? A.bias[0] : 0.f;
    const float attn = (agg + b) + A.ws[2 * r + 1];
    A.score[r] = tanhf(A.sgn * attn);
}

// Pass 2: blocks [0, light_blocks) give every light row a lane; the blocks behind them give every
// heavy row a wave.
__global__ __launch_bounds__(256) void k_sag_attn(AttnArgs A) {
    if (blockIdx.x < A.light_blocks) {
        const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (r >= A.N) return;
        const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
        if (end - beg > A.chunk) return;   // heavy row: a wave's
        float a = 0.f;
        for (int32_t e = beg; e < end; ++e) a += A.ws[2 * (int64_t)A.col[e]];
        store_score(A, r, a);
        return;
    }
    const int lane = threadIdx.x & 63;
    const int64_t h = (int64_t)(blockIdx.x - A.light_blocks) * 4 + (threadIdx.x >> 6);
    if (h >= A.n_heavy) return;   // uniform over the wave
    const int64_t r = A.heavy_row[h];
    const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
    float a = 0.f;
    for (int32_t e = beg + lane; e < end; e += 64) a += A.ws[2 * (int64_t)A.col[e]];
    a = group_sum(a, 64);
    if (lane == 0) store_score(A, r, a);
}

struct GatherScaleArgs {
    const uint16_t* x;   int64_t ldx;   // bf16 [N, H]
    uint16_t* out;       int64_t ldo;   // bf16 [K, H]
    const int64_t* perm;
    const float* score;
    int64_t K;
    int32_t H, G;
    float mult;
};

// out[k] = bf16((f32(x[perm[k]]) * score[perm[k]]) * mult): a lane's 8 columns, loaded and stored once
__global__ __launch_bounds__(256) void k_gather_scale_b16(GatherScaleArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int G = A.G, rpw = 64 / G;
    const int sub = lane / G, c = (lane % G) * 8;
    const bool col_ok = c < A.H;
    const int64_t n_slabs = (A.K + rpw - 1) / rpw;
    const int64_t step = (int64_t)gridDim.x * 4 * kSlabs;
    for (int64_t s0 = ((int64_t)blockIdx.x * 4 + wave) * kSlabs; s0 < n_slabs; s0 += step) {
        uint4 v[kSlabs];
        float s[kSlabs];
#pragma unroll
        for (int u = 0; u < kSlabs; ++u) {
            const int64_t k = (s0 + u) * rpw + sub;
            const bool ok = col_ok && k < A.K;
            const int64_t i = ok ? A.perm[k] : 0;
            s[u] = ok ? A.score[i] : 0.f;
            v[u] = ok ? ld16(A.x + i * A.ldx + c) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < kSlabs; ++u) {
            const int64_t k = (s0 + u) * rpw + sub;
            if (!(col_ok && k < A.K)) continue;
            float f[8];
            bf16x8_unpack(v[u], f);
#pragma unroll
            for (int q = 0; q < 8; ++q) f[q] = (f[q] * s[u]) * A.mult;
            store8_bf16_nt(A.out + k * A.ldo + c, f);
        }
    }
}

// the checks both entry points make on a bf16 [rows, H] operand
int check_rows(const char* name, const char* xn, const char* ldn, const void* x, int64_t ld, int32_t H) {
    BGNN_REQUIRE(x, "%s: null %s", name, xn);
    BGNN_REQUIRE(ld >= H && ld % 8 == 0, "%s: %s=%lld must be >= H and a multiple of 8", name, ldn, (long long)ld);
    BGNN_REQUIRE(aligned16(x), "%s: %s must be 16-byte aligned", name, xn);
    return BGNN_OK;
}

unsigned row_pass_blocks(int64_t rows, int G) {
    const int64_t slabs = (rows + 64 / G - 1) / (64 / G);
    return (unsigned)grid8((slabs + kSlabs - 1) / kSlabs, 2048);
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int bgnn_sag_score_bf16(const bgnn_csr_t* csr, const void* x, int64_t ldx, int64_t N, int32_t H,
                                   const float* w_l, const float* w_r, const float* bias, float sgn,
                                   float* score, float* ws, void* stream) {
    const char* name = "sag_score_bf16";
    BGNN_REQUIRE(N >= 0 && N < ((int64_t)1 << 31), "%s: N < 0 (or N >= 2^31)", name);
    BGNN_REQUIRE(H >= 8 && H <= 512 && H % 8 == 0, "%s: H=%d unsupported (need H%%8==0, 8<=H<=512)", name, H);
    if (N == 0) return BGNN_OK;
    BGNN_TRY(check_rows(name, "x", "ldx", x, ldx, H));
    BGNN_REQUIRE(w_l && w_r && score && ws, "%s: null w_l / w_r / score / ws", name);
    BGNN_REQUIRE(((uintptr_t)ws & 7) == 0, "%s: ws must be 8-byte aligned", name);
    BGNN_REQUIRE(csr && csr->rowptr, "%s: null csr", name);
    BGNN_REQUIRE(csr->n_rows == N, "%s: the CSR has %lld rows, x %lld", name, (long long)csr->n_rows, (long long)N);
    BGNN_REQUIRE(csr->col || csr->nnz == 0, "%s: null col", name);
    BGNN_REQUIRE(csr->n_heavy >= 0 && (csr->n_heavy == 0 || (csr->heavy_row && csr->chunk > 0)),
                 "%s: heavy rows need the CSR's chunk plan", name);
    hipStream_t s = as_stream(stream);

    ScoreArgs D{};
    D.x = static_cast<const uint16_t*>(x);
    D.ldx = ldx;
    D.N = N;
    D.H = H;
    D.G = group_lanes(H);
    D.w_l = w_l;
    D.w_r = w_r;
    D.ws = ws;
    hipLaunchKernelGGL(k_sag_dots, dim3(row_pass_blocks(N, D.G)), dim3(256), 0, s, D);
    BGNN_CHECK_LAUNCH();

    AttnArgs A{};
    A.rowptr = csr->rowptr;
    A.col = csr->col;
    A.heavy_row = csr->heavy_row;
    A.N = N;
    A.n_heavy = csr->n_heavy;
    A.chunk = csr->n_heavy > 0 ? csr->chunk : 0x7fffffff;   // without a plan every row is a lane's
    A.light_blocks = (unsigned)((N + 255) / 256);
    A.ws = ws;
    A.bias = bias;
    A.sgn = sgn;
    A.score = score;
    hipLaunchKernelGGL(k_sag_attn, dim3(A.light_blocks + (unsigned)((A.n_heavy + 3) / 4)), dim3(256), 0, s, A);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

extern "C" int bgnn_gather_scale_bf16(const void* x, int64_t ldx, int32_t H, const int64_t* perm,
                                      const float* score, int64_t k, float multiplier, void* out, int64_t ldo,
                                      void* stream) {
    const char* name = "gather_scale_bf16";
    BGNN_REQUIRE(k >= 0, "%s: K < 0", name);
    BGNN_REQUIRE(H >= 8 && H <= 512 && H % 8 == 0, "%s: H=%d unsupported (need H%%8==0, 8<=H<=512)", name, H);
    if (k == 0) return BGNN_OK;
    BGNN_TRY(check_rows(name, "x", "ldx", x, ldx, H));
    BGNN_TRY(check_rows(name, "out", "ldo", out, ldo, H));
    BGNN_REQUIRE(perm && score, "%s: null perm / score", name);
    GatherScaleArgs A{};
    A.x = static_cast<const uint16_t*>(x);
    A.ldx = ldx;
    A.out = static_cast<uint16_t*>(out);
    A.ldo = ldo;
    A.perm = perm;
    A.score = score;
    A.K = k;
    A.H = H;
    A.G = group_lanes(H);
    A.mult = multiplier;
    hipLaunchKernelGGL(k_gather_scale_b16, dim3(row_pass_blocks(k, A.G)), dim3(256), 0, as_stream(stream), A);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}
