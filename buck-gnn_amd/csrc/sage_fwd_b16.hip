// Training-mode GraphSAGE aggregation over bf16 rows (bgnn_sage_fwd_bf16): bgnn_sage_fwd's contract
// on z = x [W_l;W_r]^T stored as bf16 [N, 2H],
//   h = s_i * sum_e z_l[col[e]] + z_r[i] + b;  nrm[i] = ||h||;  o[i] = h / max(||h||, 1e-12),
// everything in f32, with o and nrm stored once as f32 and the BatchNorm batch statistics of o
// (per-slot f32 sums of o and o^2 over exactly the stored values) written beside them for
// bgnn_bn_finalize. It is sage_infer.hip with another epilogue: where the eval-mode layer folds
// BatchNorm's running statistics into its tail, training needs the normalised rows, their norms
// and the batch sums.
//
// The gather is b16_gather.h's skeleton with a plain sum as the policy: light rows (deg <= chunk)
// on the CSR's row-group plan, or one row per wave for a CSR without a plan; heavy rows (super
// nodes) per chunk into f32 partials, combined in chunk order by a block whose wave 0 runs the
// epilogue. Slots: one per light-row block, then one per heavy row. A wave keeps its BatchNorm
// sums in its own LDS rows between groups, added to once per group: carried in VGPRs across the
// groups they took k_fwd_group<4, 8> from 100 to 116 registers and <8, 4> from 136 to 142
// (DESIGN.md §3g); the block adds its four waves' rows in a fixed tree, as spmm.hip's SageLds does.
// No atomics; the summation order of every row and of every slot is fixed by the plan, so results
// are deterministic run to run.
#include "common.h"
#include "seg_common.h"
#include "b16_gather.h"

namespace bgnn {

namespace {

// x / ldx: bf16 z [N, 2H] with its ldz: z_l = cols [0, H) (the gathered rows), z_r = cols [H, 2H)
struct FwdArgs : GatherArgs {
    const float* bias;
    float* o;            // [N, H]
    float* nrm;          // [N]
    float* bn_partial;   // [light_slots + n_heavy, 2, H] or NULL
    int32_t mean, light_slots;
};

struct Sum {
    static constexpr bool kWeighted = false;
    static __device__ __forceinline__ float init() { return 0.f; }
    static __device__ __forceinline__ float prepare(float f, float) { return f; }
    static __device__ __forceinline__ float absorb(float a, float f) { return a + f; }
};

// A block's LDS: the bias (0 when NULL) and each wave's BatchNorm sums of o and o^2.
struct Lds {
    float b[512];
    float s[4][2][512];
};

// all threads of the block
__device__ __forceinline__ void stage_lds(const FwdArgs& A, Lds& L) {
    for (int c = threadIdx.x; c < A.H; c += blockDim.x) L.b[c] = A.bias ? A.bias[c] : 0.f;
    float* s = &L.s[0][0][0];
    for (int i = threadIdx.x; i < 4 * 2 * 512; i += blockDim.x) s[i] = 0.f;
    __syncthreads();
}

__device__ __forceinline__ uint4 load_zr(const FwdArgs& A, int64_t r, int cs) {
    return ld16_nt(A.x + r * A.ldx + A.H + cs);
}

// The epilogue of row r, held by a full wave: lane owns columns [c, c + 8) (ok: inside H; a lane
// outside H passes c = 0 and only takes part in the norm's wave sum, with zeros). o and nrm are
// stored; (bs, bq) absorb the stored o and o^2.
__device__ __forceinline__ void fwd_tail(const FwdArgs& A, const float* b, int64_t r, int32_t deg,
                                         const float (&a)[8], const uint4 zq, int c, bool ok, float (&bs)[8],
                                         float (&bq)[8]) {
    const float sc = A.mean ? inv_deg(deg) : 1.f;
    float zr[8], h[8];
    bf16x8_unpack(zq, zr);
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        h[q] = ok ? sage_h(a[q], sc, zr[q], b[c + q]) : 0.f;
        ss = fmaf(h[q], h[q], ss);
    }
    ss = group_sum(ss, kWave);
    const float n = sqrtf(ss);
    const float d = fmaxf(n, 1e-12f);
    if ((threadIdx.x & 63) == 0) __builtin_nontemporal_store(n, A.nrm + r);
    if (!ok) return;
    float o[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        o[q] = h[q] / d;
        bs[q] += o[q];
        bq[q] += o[q] * o[q];
    }
    store8_f32_nt(A.o + r * A.H + c, o);
}

// (bs, bq) added to the wave's LDS rows: lane-private columns, no barrier
__device__ __forceinline__ void flush_sums(Lds& L, int wave, int c, const float (&bs)[8], const float (&bq)[8]) {
    float4* ps = reinterpret_cast<float4*>(&L.s[wave][0][c]);
    float4* pq = reinterpret_cast<float4*>(&L.s[wave][1][c]);
    const float4 s0 = ps[0], s1 = ps[1], q0 = pq[0], q1 = pq[1];
    ps[0] = make_float4(s0.x + bs[0], s0.y + bs[1], s0.z + bs[2], s0.w + bs[3]);
    ps[1] = make_float4(s1.x + bs[4], s1.y + bs[5], s1.z + bs[6], s1.w + bs[7]);
    pq[0] = make_float4(q0.x + bq[0], q0.y + bq[1], q0.z + bq[2], q0.w + bq[3]);
    pq[1] = make_float4(q1.x + bq[4], q1.y + bq[5], q1.z + bq[6], q1.w + bq[7]);
}

// The block's slot: its four waves' sums, a fixed tree. All threads of the block.
__device__ __forceinline__ void store_slot(const FwdArgs& A, const Lds& L) {
    if (!A.bn_partial) return;
    __syncthreads();
    float* dst = A.bn_partial + (int64_t)blockIdx.x * 2 * A.H;
    for (int c = threadIdx.x; c < A.H; c += blockDim.x) {
        dst[c] = (L.s[0][0][c] + L.s[1][0][c]) + (L.s[2][0][c] + L.s[3][0][c]);
        dst[A.H + c] = (L.s[0][1][c] + L.s[1][1][c]) + (L.s[2][1][c] + L.s[3][1][c]);
    }
}

// A group's epilogue: the rows' z_r loads, all issued before the first row's arithmetic; the
// group's BatchNorm sums go to the wave's LDS rows once per group.
template <int R>
struct GroupTail {
    const FwdArgs& A;
    Lds& L;
    __device__ __forceinline__ void operator()(int64_t r0, int rows, int32_t rp, int32_t chunk, float (&a)[R][8],
                                               int cs, bool ok) const {
        uint4 zq[R];
#pragma unroll
        for (int t = 0; t < R; ++t) zq[t] = load_zr(A, r0 + (t < rows ? t : 0), cs);
        float bs[8], bq[8];
        fill(bs, 0.f);
        fill(bq, 0.f);
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int32_t rb = __builtin_amdgcn_readlane(rp, t);
            const int32_t deg = __builtin_amdgcn_readlane(rp, t + 1) - rb;
            if (t >= rows || deg > chunk) continue;   // heavy row: chunk + combine
            fwd_tail(A, L.b, r0 + t, deg, a[t], zq[t], cs, ok, bs, bq);
        }
        if (A.bn_partial && ok) flush_sums(L, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), cs, bs, bq);
    }
};

// Light rows on the row-group plan.
template <int R, int U>
__global__ __launch_bounds__(256) void k_fwd_group(FwdArgs A) {
    __shared__ __attribute__((aligned(16))) Lds L;
    stage_lds(A, L);
    walk_groups<R, U>(A, Sum{}, GroupTail<R>{A, L});
    store_slot(A, L);
}

// Light rows without a row-group plan: one row per wave, CSR order.
__global__ __launch_bounds__(256) void k_fwd_row(FwdArgs A) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    __shared__ __attribute__((aligned(16))) Lds L;
    stage_lds(A, L);
    float bs[8], bq[8];
    fill(bs, 0.f);
    fill(bq, 0.f);
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < A.n_rows; r += (int64_t)gridDim.x * 4) {
        const int32_t beg = A.rowptr[r], end = A.rowptr[r + 1];
        if (end - beg > A.chunk) continue;   // heavy row: chunk + combine
        const uint4 zq = load_zr(A, r, cs);
        float a[8];
        fill(a, Sum::init());
        gather_edges(A, Sum{}, beg, end, cs, a);
        fwd_tail(A, L.b, r, end - beg, a, zq, cs, ok, bs, bq);
    }
    if (A.bn_partial && ok) flush_sums(L, wave, cs, bs, bq);
    store_slot(A, L);
}

// Heavy chunks: one wave per chunk -> partial[c, :] (f32).
__global__ __launch_bounds__(256) void k_fwd_chunk(FwdArgs A) { chunk_body<false>(A, Sum{}, nullptr); }

// Combine heavy rows: one block of 16 waves per heavy row; wave 0 runs the epilogue on the row's
// sum and stores the row's slot (o and o^2 of one row).
__global__ __launch_bounds__(1024) void k_fwd_combine(FwdArgs A) {
    __shared__ __attribute__((aligned(16))) float b[512];
    const int lane = threadIdx.x & 63;
    const int h = blockIdx.x;
    if (h >= A.n_heavy) return;   // uniform over the block
    for (int c = threadIdx.x; c < A.H; c += blockDim.x) b[c] = A.bias ? A.bias[c] : 0.f;
    __syncthreads();
    bool ok;
    const int cs = lane_col8(lane, A.H, ok);
    const int64_t r = A.heavy_row[h];
    const int32_t deg = A.rowptr[r + 1] - A.rowptr[r];
    float a[8];
    if (!combine_chunks(A, h, cs, ok, a)) return;
    float bs[8], bq[8];
    fill(bs, 0.f);
    fill(bq, 0.f);
    fwd_tail(A, b, r, deg, a, load_zr(A, r, cs), cs, ok, bs, bq);
    if (!A.bn_partial || !ok) return;
    float4* dst = reinterpret_cast<float4*>(A.bn_partial + (int64_t)(A.light_slots + h) * 2 * A.H + cs);
    float4* dsq = reinterpret_cast<float4*>(A.bn_partial + ((int64_t)(A.light_slots + h) * 2 + 1) * A.H + cs);
    dst[0] = make_float4(bs[0], bs[1], bs[2], bs[3]);
    dst[1] = make_float4(bs[4], bs[5], bs[6], bs[7]);
    dsq[0] = make_float4(bq[0], bq[1], bq[2], bq[3]);
    dsq[1] = make_float4(bq[4], bq[5], bq[6], bq[7]);
}

// the grid of the light-row kernel launch_gather will pick for this CSR
int64_t light_blocks(const bgnn_csr_t* csr) {
    GatherArgs A{};
    A.chunk = csr->chunk > 0 ? csr->chunk : 0x7fffffff;
    return use_group_plan(csr, A) ? grid8(A.n_groups, 1024) : grid8(csr->n_rows, 2048);
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" int32_t bgnn_sage_fwd_bf16_slots(const bgnn_csr_t* csr) {
    if (!csr) return -1;
    return (int32_t)(light_blocks(csr) + (csr->n_chunks > 0 ? csr->n_heavy : 0));
}

extern "C" int bgnn_sage_fwd_bf16(const bgnn_csr_t* csr, const void* z, int64_t ldz, const float* bias, int32_t H,
                                  int32_t reduce, float* o, float* nrm, float* bn_partial, float* partial,
                                  void* stream) {
    const char* name = "sage_fwd_bf16";
    BGNN_TRY(check_operands(name, "z", "o", "H<=512", csr, z, o, H, reduce));
    BGNN_REQUIRE(nrm, "sage_fwd_bf16: null nrm");
    BGNN_REQUIRE(ldz >= 2 * (int64_t)H && ldz % 8 == 0, "sage_fwd_bf16: ldz must be >= 2H and a multiple of 8");
    BGNN_TRY(check_heavy_plan(name, csr, partial));
    BGNN_REQUIRE(aligned16(bias) && aligned16(bn_partial), "sage_fwd_bf16: bias / bn_partial must be 16-byte aligned");
    FwdArgs A{};
    int go = 0;
    BGNN_TRY(check_aligned_and_fill(name, "z / o / partial", csr, z, ldz, H, o, nullptr, partial, A, &go));
    if (!go) return BGNN_OK;
    A.bias = bias;
    A.o = o;
    A.nrm = nrm;
    A.bn_partial = bn_partial;
    A.mean = reduce == BGNN_REDUCE_MEAN;
    A.light_slots = (int32_t)light_blocks(csr);
    const GatherKernels<FwdArgs> K = {k_fwd_group<8, 4>, k_fwd_group<4, 8>, k_fwd_row,
                                      k_fwd_chunk,       k_fwd_combine,     64 * kCombineWaves};
    return launch_gather(csr, A, K, stream);
}
