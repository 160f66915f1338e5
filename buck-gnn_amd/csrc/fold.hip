// The folded first layer's weight-by-weight chain (bgnn/fused.py, SageLayerFn with w_in) in one
// grouped launch per direction:
//   forward   Wf = Wcat W_in [2H, K_in], bf = Wcat b_in [2H] (+ Wf^T, max|Wf|)
//   backward  dWcat = dWf W_in^T + dbf (x) b_in [2H, H], dW_in = Wcat^T dWf [H, K_in],
//             db_in = Wcat^T dbf [H]
// Each product is the f16x3 GEMM bgnn_gemm_f32_scaled runs on its 4-wave 128 x 128 tile (2 x 2
// waves of 64 x 64, 32x32x16 MFMAs), cut into workgroup tiles of four waves with one 32 x 32 block
// each (64 x 64 backward, 32 x 128 forward), so that the chain fills 64-224 workgroups instead of
// 4-32. An output element's bits are fixed by the operand scales (h3_scale of the two maxima), the
// piece split (x6_store / split2h), the MFMA shape and fragment map, the k order (32-deep slices
// from the K range's start, two 16-deep steps each, the three piece products small terms first:
// x6_mma), and the epilogue's unscale -- all the device functions of k_gemm_x6, none of which
// depends on the tile an element sits in. The one tile-dependent choice is the epilogue's interior
// path (one multiply by ia * ib) against its edge path (two multiplies), taken per 64 x 64 wave
// block there: each wave here takes the choice of the 64 x 64 block its 32 x 32 lies in. Split-K
// products write the same K ranges as slabs and a second launch sums them in slab order
// (k_splitk_reduce's arithmetic). The plan (split, K range per slab) is the GEMM planner's own
// (small_h3_plan).
#include "gemm_x6_kernel.h"

namespace bgnn {

// workgroup tile = WM x WN waves of one 32 x 32 block each: 2 x 2 (64 x 64) for the backward, 1 x 4
// (32 x 128) for the forward, whose two products then fill 64 workgroups at H = 512, K_in = 128
constexpr int FNT = 256;    // threads
constexpr int FSL = 4;      // 32-deep slices staged per step
constexpr int f_u4(int rows) { return 2 * rows * 4; }   // uint4 per operand image of one slice (two pieces)

struct FoldProb {
    const float* A;
    const float* B;
    float* C;
    float* slabs;            // split > 1: [split][M][N]
    int64_t M, N, K, lda, ldb, ldc, kchunk;
    int split, ta, tb;
    const float* a_amax;
    const float* b_amax;
    int tiles_n, tiles, wg0;   // workgroup tiles; first workgroup of the product
};

struct FoldArgs {
    FoldProb p[3];
    int np;
    float alpha;             // 1 (the epilogue's alpha multiply, kept as an instruction)
    // product 0 only
    float* c_amax;           // max |C| folded in (forward: max|Wf|), or NULL
    float* ct;               // C^T written as well (forward: Wf^T), or NULL
    int64_t ldct;
    const float* ou;         // C += ou (x) ov, product and sum each rounded (backward: dbf, b_in)
    const float* ov;
    // product np - 1 of the backward: its B operand is the vector vmax_src [vmax_n] whose maximum is
    // folded into *b_amax by this launch (max|dbf|), so every workgroup of it recomputes the maximum
    const float* vmax_src;
    int64_t vmax_n;
};

__device__ __forceinline__ bool dev_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// staging of one operand's R x (FSL x 32) panel: registers, then the [piece][row][4 chunks] images of
// its FSL slices (image of slice u at S + u * stride). K-contiguous: x6_load / x6_store units per
// slice. k-major: kq_load / kq_store quads (4 rows x 8 k, eight float4 loads along the rows instead
// of 32 dword loads), the R quads of each slice dealt over the threads across the FSL slices; they
// write the same images (gemm_x6_kernel.h), so the same bits.
template <int KC, int R>
struct FoldStage {
    static constexpr int NQ = R * FSL / FNT;   // k-major: quads per thread and step
    static_assert(KC || (NQ >= 1 && R * FSL % FNT == 0), "k-major operand: whole quads per thread");
    float v[KC ? FSL : NQ][KC ? x6_nu(R, FNT) : 4][8];

    __device__ __forceinline__ void load(const float* __restrict__ P, int64_t ld, int64_t Rlim, int64_t r0, int64_t k0,
                                         int64_t s0, int64_t nk, int64_t ke, bool vec_ok, int t) {
        if constexpr (KC) {
#pragma unroll
            for (int u = 0; u < FSL; ++u)
                if (s0 + u < nk) x6_load<1, R, FNT, false>(P, ld, Rlim, r0, k0 + (s0 + u) * X6_BK, ke, vec_ok, v[u], t);
        } else {
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const int g = t + FNT * j, u = g / R, q = g % R;
                if (s0 + u < nk) kq_load<R, false>(P, ld, Rlim, r0, k0 + (s0 + u) * X6_BK, ke, vec_ok, v[j], q);
            }
        }
    }
    __device__ __forceinline__ void store(uint4* __restrict__ S, int stride, int64_t s0, int64_t nk, float sc, int t) {
        if constexpr (KC) {
#pragma unroll
            for (int u = 0; u < FSL; ++u)
                if (s0 + u < nk) x6_store<1, R, FNT, 1>(S + u * stride, v[u], t, sc);
        } else {
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const int g = t + FNT * j, u = g / R, q = g % R;
                if (s0 + u < nk) kq_store<R, 1>(S + u * stride, v[j], q, sc);
            }
        }
    }
};

template <int WM, int WN, int AK, int BK>
__device__ __forceinline__ void fold_mainloop(const FoldProb& P, int64_t m0, int64_t n0, int64_t kb, int64_t ke,
                                              float sa, float sb, uint4* __restrict__ smem, bool active,
                                              floatx16 (&acc)[1][1]) {
    constexpr int BM = 32 * WM, BN = 32 * WN, A_U4 = f_u4(BM), B_U4 = f_u4(BN);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;
    const bool a_vec = dev_aligned16(P.A) && P.lda % 4 == 0;
    const bool b_vec = dev_aligned16(P.B) && P.ldb % 4 == 0;
    const int64_t nk = ke > kb ? (ke - kb + X6_BK - 1) / X6_BK : 0;
    FoldStage<AK, BM> ra;
    FoldStage<BK, BN> rb;
    ra.load(P.A, P.lda, P.M, m0, kb, 0, nk, ke, a_vec, t);
    rb.load(P.B, P.ldb, P.N, n0, kb, 0, nk, ke, b_vec, t);
    for (int64_t s0 = 0; s0 < nk; s0 += FSL) {
        ra.store(smem, A_U4 + B_U4, s0, nk, sa, t);
        rb.store(smem + A_U4, A_U4 + B_U4, s0, nk, sb, t);
        __syncthreads();
        if (s0 + FSL < nk) {   // in flight under the MFMAs below
            ra.load(P.A, P.lda, P.M, m0, kb, s0 + FSL, nk, ke, a_vec, t);
            rb.load(P.B, P.ldb, P.N, n0, kb, s0 + FSL, nk, ke, b_vec, t);
        }
        if (active) {
#pragma unroll
            for (int u = 0; u < FSL; ++u) {
                if (s0 + u < nk) {
                    const uint4* As = smem + u * (A_U4 + B_U4);
                    const uint4* Bs = As + A_U4;
#pragma unroll
                    for (int kk = 0; kk < X6_BK / 16; ++kk) {
                        uint4 a[1][2], b[1][2];
#pragma unroll
                        for (int p = 0; p < 2; ++p) {
                            a[0][p] = As[p * BM * 4 + x6_pos(wm * 32 + li, 2 * kk + lh)];
                            b[0][p] = Bs[p * BN * 4 + x6_pos(wn * 32 + li, 2 * kk + lh)];
                        }
                        x6_mma<1, 1, 1, 2>(acc, a, b);
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <int WM, int WN>
__global__ __launch_bounds__(FNT) void k_fold_products(FoldArgs fa) {
    static_assert(WM * WN * 64 == FNT, "four waves");
    constexpr int BM = 32 * WM, BN = 32 * WN;
    __shared__ uint4 smem[FSL * (f_u4(BM) + f_u4(BN))];
    __shared__ uint32_t red[4];
    int pi = 0;
#pragma unroll
    for (int q = 1; q < 3; ++q)
        if (q < fa.np && (int)blockIdx.x >= fa.p[q].wg0) pi = q;
    const FoldProb& P = fa.p[pi];
    const int local = (int)blockIdx.x - P.wg0;
    const int lt = local % P.tiles, ks = local / P.tiles;
    const int64_t m0 = (int64_t)(lt / P.tiles_n) * BM, n0 = (int64_t)(lt % P.tiles_n) * BN;
    const int64_t kb = (int64_t)ks * P.kchunk;
    const int64_t ke = min(P.K, kb + P.kchunk);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave / WN, wn = wave % WN;

    float amax_a = *P.a_amax, amax_b = *P.b_amax;
    const bool own_vmax = fa.vmax_src != nullptr && pi == fa.np - 1;
    if (own_vmax) {   // max(*b_amax, max |vmax_src|): what the slot holds once this launch has folded it in
        uint32_t m = __float_as_uint(amax_b);
        for (int64_t i = t; i < fa.vmax_n; i += FNT) m = max(m, __float_as_uint(fa.vmax_src[i]) & 0x7fffffffu);
        for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, kWave));
        if (lane == 0) red[wave] = m;
        __syncthreads();
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        amax_b = __uint_as_float(m);
        if (local == 0 && t == 0 && m) atomicMax(reinterpret_cast<uint32_t*>(const_cast<float*>(P.b_amax)), m);
    }
    float sa, sb, ia, ib;
    h3_scale(amax_a, sa, ia);
    h3_scale(amax_b, sb, ib);

    floatx16 acc[1][1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][0][r] = 0.f;
    const int64_t r0 = m0 + wm * 32, c0 = n0 + wn * 32;
    const bool active = r0 < P.M && c0 < P.N;
    // (the forward's 32 x 128 launch holds A B products only, the backward's 64 x 64 the other two)
    if constexpr (WM == 1) {
        fold_mainloop<WM, WN, 1, 0>(P, m0, n0, kb, ke, sa, sb, smem, active, acc);
    } else {
        if (P.ta == 0 && P.tb == 0) fold_mainloop<WM, WN, 1, 0>(P, m0, n0, kb, ke, sa, sb, smem, active, acc);
        else if (P.ta == 0) fold_mainloop<WM, WN, 1, 1>(P, m0, n0, kb, ke, sa, sb, smem, active, acc);
        else fold_mainloop<WM, WN, 0, 0>(P, m0, n0, kb, ke, sa, sb, smem, active, acc);
    }
    if (!active) return;

    // epilogue (x6_epilogue's arithmetic; C/D map of the 32x32 MFMA: col = lane & 31,
    // row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5))
    const bool split = P.split > 1;
    float* dst = split ? P.slabs + (int64_t)ks * P.M * P.N : P.C;
    const int64_t ldd = split ? P.N : P.ldc;
    const bool vec = dev_aligned16(dst) && ldd % 4 == 0;
    // the interior path is taken per 64 x 64 wave block of the 128 x 128 tile: the block this wave's
    // 32 x 32 lies in (blocks start at multiples of 64)
    const bool fast = !split && vec && (r0 & ~(int64_t)63) + 64 <= P.M && (c0 & ~(int64_t)63) + 64 <= P.N;
    const float iab = ia * ib;
    const bool one_mul = iab != 0.f && iab < 3.0e38f;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t col = c0 + li;
    const bool first = pi == 0;
    const bool outer = first && fa.ou != nullptr && !split;
    const float ovc = (outer && col < P.N) ? fa.ov[col] : 0.f;
    uint32_t cmax = 0;
    float vals[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = r0 + (r & 3) + 8 * (r >> 2) + 4 * lh;
        const float e = acc[0][0][r];
        float v;
        if (split) {
            v = (e * ia) * ib;
        } else {
            v = (fast && one_mul) ? e * iab : (e * ia) * ib;
            v *= fa.alpha;
            if (outer && row < P.M) v = __fadd_rn(v, __fmul_rn(fa.ou[row], ovc));
        }
        vals[r] = v;
        if (row < P.M && col < P.N) {
            dst[row * ldd + col] = v;
            cmax = max(cmax, __float_as_uint(v) & 0x7fffffffu);
        }
    }
    if (first && fa.ct != nullptr && !split && col < P.N) {   // C^T: four consecutive rows per store
        const bool tvec = dev_aligned16(fa.ct) && fa.ldct % 4 == 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t row = r0 + 8 * q + 4 * lh;
            float* p = fa.ct + col * fa.ldct + row;
            if (tvec && row + 3 < P.M) {
                *reinterpret_cast<float4*>(p) = make_float4(vals[4 * q], vals[4 * q + 1], vals[4 * q + 2], vals[4 * q + 3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (row + k < P.M) p[k] = vals[4 * q + k];
            }
        }
    }
    if (first && fa.c_amax != nullptr && !split) {
        for (int o = 32; o > 0; o >>= 1) cmax = max(cmax, (uint32_t)__shfl_xor((int)cmax, o, kWave));
        if (lane == 0 && cmax) atomicMax(reinterpret_cast<uint32_t*>(fa.c_amax), cmax);
    }
}

// the slab sums of the split-K products: C = alpha * (((0 + slab 0) + slab 1) + ...), k_splitk_reduce's order
__global__ __launch_bounds__(256) void k_fold_reduce(FoldArgs fa, int64_t e1, int64_t e2) {
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i0 >= e2) return;
    const int pi = i0 < e1 ? 1 : 2;
    const FoldProb& P = fa.p[pi];
    const int64_t i = i0 < e1 ? i0 : i0 - e1;
    const int64_t total = P.M * P.N;
    float s = 0.f;
    for (int k = 0; k < P.split; ++k) s += P.slabs[(int64_t)k * total + i];
    P.C[(i / P.N) * P.ldc + i % P.N] = fa.alpha * s;
}

// max |.| of the forward's three operands into their fold_amax slots (k_absmax's unsigned atomic max)
struct FoldMaxArgs {
    const float* P[3];
    int64_t rows[3], cols[3], ld[3];
    int b0[4];   // first block of each operand, b0[3] = the grid
    uint32_t* out;
};

__global__ __launch_bounds__(256) void k_fold_maxima(FoldMaxArgs a) {
    int pi = 0;
    if ((int)blockIdx.x >= a.b0[1]) pi = 1;
    if ((int)blockIdx.x >= a.b0[2]) pi = 2;
    const float* __restrict__ P = a.P[pi];
    const int64_t rows = a.rows[pi], cols = a.cols[pi], ld = a.ld[pi];
    const int64_t nb = a.b0[pi + 1] - a.b0[pi], b = (int)blockIdx.x - a.b0[pi];
    uint32_t m = 0;
    if (cols % 4 == 0 && ld % 4 == 0 && dev_aligned16(P)) {
        const int64_t c4 = cols / 4, n4 = rows * c4;
        for (int64_t i = b * 256 + threadIdx.x; i < n4; i += nb * 256) {
            const float4 v = *reinterpret_cast<const float4*>(P + (i / c4) * ld + (i % c4) * 4);
            m = max(m, max(max(__float_as_uint(v.x) & 0x7fffffffu, __float_as_uint(v.y) & 0x7fffffffu),
                           max(__float_as_uint(v.z) & 0x7fffffffu, __float_as_uint(v.w) & 0x7fffffffu)));
        }
    } else {
        const int64_t n = rows * cols;
        for (int64_t i = b * 256 + threadIdx.x; i < n; i += nb * 256)
            m = max(m, __float_as_uint(P[(i / cols) * ld + i % cols]) & 0x7fffffffu);
    }
    block_amax(a.out + pi, m);
}

// one product of the chain as the GEMM planner plans it, on bm x bn workgroup tiles; false: not the
// 4-wave 128 x 128 f16x3 tile, a split-K deep enough for the staged slab sum (which this file does
// not reproduce), or a split where the caller takes none (split_ok false)
static bool fold_prob(FoldProb& P, int bm, int bn, bool split_ok, int ta, int tb, int64_t M, int64_t N, int64_t K,
                      const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                      const float* a_amax, const float* b_amax, int& wg) {
    int split = 1;
    int64_t kchunk = 0;
    if (!small_h3_plan(M, N, K, ta, tb, &split, &kchunk) || split >= 16 || (split > 1 && !split_ok)) return false;
    P = FoldProb{A, B, C, nullptr, M, N, K, lda, ldb, ldc, kchunk, split, ta, tb, a_amax, b_amax, 0, 0, 0};
    P.tiles_n = (int)((N + bn - 1) / bn);
    P.tiles = (int)((M + bm - 1) / bm) * P.tiles_n;
    P.wg0 = wg;
    wg += P.tiles * split;
    return true;
}

// forward (32 x 128 tiles): Wf = Wcat W_in, bf = Wcat b_in; no split-K (max|Wf| and Wf^T come out of
// the product's epilogue)
static bool fold_plan_fwd(FoldArgs& fa, int& wg, int64_t H, int64_t K_in, const float* wcat, int64_t ld_wcat,
                          const float* w_in, int64_t ld_win, const float* b_in, float* fold_amax, float* wf,
                          int64_t ld_wf, float* bf) {
    wg = 0;
    fa.np = 2;
    return fold_prob(fa.p[0], 32, 128, false, 0, 0, 2 * H, K_in, H, wcat, ld_wcat, w_in, ld_win, wf, ld_wf, fold_amax,
                     fold_amax + 1, wg) &&
           fold_prob(fa.p[1], 32, 128, false, 0, 0, 2 * H, 1, H, wcat, ld_wcat, b_in, 1, bf, 1, fold_amax,
                     fold_amax + 2, wg);
}

// backward (64 x 64 tiles): dWcat = dWf W_in^T (+ dbf (x) b_in in the epilogue: no split-K),
// dW_in = Wcat^T dWf, db_in = Wcat^T dbf (split-K as planned)
static bool fold_plan_bwd(FoldArgs& fa, int& wg, int64_t H, int64_t K_in, const float* dwf, int64_t ld_dwf,
                          const float* dbf, const float* wcat, int64_t ld_wcat, const float* w_in, int64_t ld_win,
                          float* fold_amax, float* dwcat, int64_t ld_dwcat, float* dw_in, int64_t ld_dwin,
                          float* db_in) {
    wg = 0;
    fa.np = 3;
    return fold_prob(fa.p[0], 64, 64, false, 0, 1, 2 * H, H, K_in, dwf, ld_dwf, w_in, ld_win, dwcat, ld_dwcat,
                     fold_amax + 3, fold_amax + 1, wg) &&
           fold_prob(fa.p[1], 64, 64, true, 1, 0, H, K_in, 2 * H, wcat, ld_wcat, dwf, ld_dwf, dw_in, ld_dwin, fold_amax,
                     fold_amax + 3, wg) &&
           fold_prob(fa.p[2], 64, 64, true, 1, 0, H, 1, 2 * H, wcat, ld_wcat, dbf, 1, db_in, 1, fold_amax,
                     fold_amax + 4, wg);
}

// what both entry points accept: the plans above, on the f16x3 family
static bool fold_supported(int64_t H, int64_t K_in) {
    if (H <= 0 || K_in <= 0 || H > 4096 || K_in > 4096 || gemm_mode() != 2) return false;
    FoldArgs fa{};
    int wg = 0;
    float slots[5];   // (addresses only)
    return fold_plan_fwd(fa, wg, H, K_in, nullptr, H, nullptr, K_in, nullptr, slots, nullptr, K_in, nullptr) &&
           fold_plan_bwd(fa, wg, H, K_in, nullptr, K_in, nullptr, nullptr, H, nullptr, K_in, slots, nullptr, H,
                         nullptr, K_in, nullptr);
}

}  // namespace bgnn

using namespace bgnn;

extern "C" int32_t bgnn_fold_weights_supported(int64_t H, int64_t K_in) { return fold_supported(H, K_in) ? 1 : 0; }

extern "C" size_t bgnn_fold_weights_ws_bytes(int64_t H, int64_t K_in) {
    if (!fold_supported(H, K_in)) return 0;
    FoldArgs fa{};
    int wg = 0;
    float slots[5];   // (addresses only)
    fold_plan_bwd(fa, wg, H, K_in, nullptr, K_in, nullptr, nullptr, H, nullptr, K_in, slots, nullptr, H, nullptr, K_in,
                  nullptr);
    size_t n = 0;
    if (fa.p[1].split > 1) n += (size_t)fa.p[1].split * H * K_in;
    if (fa.p[2].split > 1) n += (size_t)fa.p[2].split * H;
    return n * sizeof(float);
}

extern "C" int bgnn_fold_weights_fwd(int64_t H, int64_t K_in, const float* wcat, int64_t ld_wcat, const float* w_in,
                                     int64_t ld_win, const float* b_in, float* fold_amax, float* wf, int64_t ld_wf,
                                     float* bf, float* wf_t, int64_t ld_wft, float* w_amax, void* stream) {
    BGNN_REQUIRE(wcat && w_in && b_in && fold_amax && wf && bf && w_amax, "fold_weights_fwd: null pointer");
    BGNN_REQUIRE(H > 0 && K_in > 0, "fold_weights_fwd: H and K_in must be positive (got %lld, %lld)", (long long)H,
                 (long long)K_in);
    BGNN_REQUIRE(ld_wcat >= H && ld_win >= K_in && ld_wf >= K_in && (!wf_t || ld_wft >= 2 * H),
                 "fold_weights_fwd: a leading dimension is shorter than its row");
    FoldArgs fa{};
    int wg = 0;
    BGNN_REQUIRE(fold_supported(H, K_in) &&
                     fold_plan_fwd(fa, wg, H, K_in, wcat, ld_wcat, w_in, ld_win, b_in, fold_amax, wf, ld_wf, bf),
                 "fold_weights_fwd: H=%lld, K_in=%lld unsupported (bgnn_fold_weights_supported)", (long long)H,
                 (long long)K_in);
    hipStream_t s = as_stream(stream);
    FoldMaxArgs ma{};
    ma.P[0] = wcat; ma.rows[0] = 2 * H; ma.cols[0] = H; ma.ld[0] = ld_wcat;
    ma.P[1] = w_in; ma.rows[1] = H; ma.cols[1] = K_in; ma.ld[1] = ld_win;
    ma.P[2] = b_in; ma.rows[2] = 1; ma.cols[2] = H; ma.ld[2] = H;
    ma.b0[0] = 0;
    for (int q = 0; q < 3; ++q) {   // ~2048 float4 per block, at most 64 blocks per operand
        int64_t nb = (ma.rows[q] * ma.cols[q] + 8191) / 8192;
        nb = nb < 1 ? 1 : (nb > 64 ? 64 : nb);
        ma.b0[q + 1] = ma.b0[q] + (int)nb;
    }
    ma.out = reinterpret_cast<uint32_t*>(fold_amax);
    hipLaunchKernelGGL(k_fold_maxima, dim3((unsigned)ma.b0[3]), dim3(256), 0, s, ma);
    BGNN_CHECK_LAUNCH();
    fa.alpha = 1.f;
    fa.c_amax = w_amax;
    fa.ct = wf_t;
    fa.ldct = ld_wft;
    hipLaunchKernelGGL((k_fold_products<1, 4>), dim3((unsigned)wg), dim3(FNT), 0, s, fa);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}

extern "C" int bgnn_fold_weights_bwd(int64_t H, int64_t K_in, const float* dwf, int64_t ld_dwf, const float* dbf,
                                     const float* wcat, int64_t ld_wcat, const float* w_in, int64_t ld_win,
                                     const float* b_in, float* fold_amax, float* dwcat, int64_t ld_dwcat,
                                     float* dw_in, int64_t ld_dwin, float* db_in, void* ws, size_t ws_bytes,
                                     void* stream) {
    BGNN_REQUIRE(dwf && dbf && wcat && w_in && b_in && fold_amax && dwcat && dw_in && db_in,
                 "fold_weights_bwd: null pointer");
    BGNN_REQUIRE(H > 0 && K_in > 0, "fold_weights_bwd: H and K_in must be positive (got %lld, %lld)", (long long)H,
                 (long long)K_in);
    BGNN_REQUIRE(ld_dwf >= K_in && ld_wcat >= H && ld_win >= K_in && ld_dwcat >= H && ld_dwin >= K_in,
                 "fold_weights_bwd: a leading dimension is shorter than its row");
    FoldArgs fa{};
    int wg = 0;
    BGNN_REQUIRE(fold_supported(H, K_in) &&
                     fold_plan_bwd(fa, wg, H, K_in, dwf, ld_dwf, dbf, wcat, ld_wcat, w_in, ld_win, fold_amax, dwcat,
                                   ld_dwcat, dw_in, ld_dwin, db_in),
                 "fold_weights_bwd: H=%lld, K_in=%lld unsupported (bgnn_fold_weights_supported)", (long long)H,
                 (long long)K_in);
    // (unlike bgnn_gemm_f32_scaled, which drops to one slab on a short workspace, the planned slabs are required)
    const size_t need = bgnn_fold_weights_ws_bytes(H, K_in);
    BGNN_REQUIRE(need == 0 || (ws != nullptr && ws_bytes >= need),
                 "fold_weights_bwd: workspace of %zu bytes, bgnn_fold_weights_ws_bytes() asks %zu", ws_bytes, need);
    hipStream_t s = as_stream(stream);
    float* slabs = static_cast<float*>(ws);
    int64_t e1 = 0, e2 = 0;
    if (fa.p[1].split > 1) {
        fa.p[1].slabs = slabs;
        slabs += (int64_t)fa.p[1].split * H * K_in;
        e1 = H * K_in;
    }
    e2 = e1;
    if (fa.p[2].split > 1) {
        fa.p[2].slabs = slabs;
        e2 += H;
    }
    fa.alpha = 1.f;
    fa.ou = dbf;
    fa.ov = b_in;
    fa.vmax_src = dbf;
    fa.vmax_n = 2 * H;
    hipLaunchKernelGGL((k_fold_products<2, 2>), dim3((unsigned)wg), dim3(FNT), 0, s, fa);
    BGNN_CHECK_LAUNCH();
    if (e2 > 0) {
        hipLaunchKernelGGL(k_fold_reduce, dim3((unsigned)((e2 + 255) / 256)), dim3(256), 0, s, fa, e1, e2);
        BGNN_CHECK_LAUNCH();
    }
    return BGNN_OK;
}
