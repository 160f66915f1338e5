// The per-graph losses of the node-level heads (Utils/Losses.py:362-401, 445-507:
// GraphRelativeError, GraphMSELoss, GraphMAELoss with a batch vector), loss and d loss / d pred in
// one pass:
//   loss = mult / B * sum_g 1 / (n_g C) * sum_{i in g, c} f(p'_ic, t'_ic),
//   p' = pred * scale[c] + center[c], t' = target * scale[c] + center[c] (NULL: identity; the
//   reference's denormalize_displacement / denormalize_gp_stresses, Normalizer.py:298-312),
//   f = |p' - t'| / (|t'| + eps)   (kind 0),   |p' - t'|   (kind 1),   |p'^2 - t'^2|   (kind 2).
// One workgroup per (graph, segment-block) walks its share of the graph's rows through the batch
// vector's segment CSR (any row order): the element term in f32 with torch's roundings (every
// product and sum rounded, no contraction), each thread's sum in a double, the workgroup's 256 sums
// by a fixed tree. A one-workgroup finish kernel sums each graph's segment-blocks and then the
// per-graph means in a fixed order. No atomics: loss and gradient are bit-identical from run to run
// (the torch path's index_add_ is not).
#include "common.h"

namespace bgnn {

namespace {

// block tree sum over 256 doubles, fixed order; the result in red[0]
__device__ __forceinline__ void tree_sum256(double* red, int t) {
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
}

// block (g, s): segment-block s of graph g, elements [s * chunk, (s + 1) * chunk) of the graph's
// n_g C elements (chunk = the graph's count split S ways, rounded up); its sum goes to part[g * S + s]
__global__ __launch_bounds__(256) void k_graph_loss(const float* __restrict__ pred, const float* __restrict__ target,
                                                    int C, const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col, int B, int kind, float eps,
                                                    float mult, const float* __restrict__ scale,
                                                    const float* __restrict__ center, double* __restrict__ part,
                                                    float* __restrict__ dpred) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    const int S = gridDim.y, s = blockIdx.y, g = blockIdx.x;
    const int64_t r0 = rowptr[g], r1 = rowptr[g + 1];
    const int64_t cnt = (r1 - r0) * C;
    const int64_t chunk = (cnt + S - 1) / S;
    const int64_t e0 = s * chunk, e1 = min(cnt, e0 + chunk);
    // d loss / d f of this graph's elements: mult / (B n_g C)
    const double w = (double)mult / ((double)B * (double)cnt);
    double acc = 0.0;
    for (int64_t e = e0 + t; e < e1; e += 256) {
        const int64_t r = e / C;
        const int c = (int)(e - r * C);
        const int64_t i = (int64_t)col[r0 + r] * C + c;
        float p = pred[i], q = target[i], sc = 1.f;
        if (scale) {
            sc = scale[c];
            p = __fmul_rn(p, sc);
            q = __fmul_rn(q, sc);
        }
        if (center) {
            p = __fadd_rn(p, center[c]);
            q = __fadd_rn(q, center[c]);
        }
        float f, dir, den = 1.f, fac = 1.f;
        if (kind == 2) {
            dir = __fsub_rn(__fmul_rn(p, p), __fmul_rn(q, q));
            f = fabsf(dir);
            fac = 2.f * p;
        } else {
            dir = __fsub_rn(p, q);
            f = fabsf(dir);
            if (kind == 0) {
                den = __fadd_rn(fabsf(q), eps);
                f = __fdiv_rn(f, den);
            }
        }
        acc += (double)f;
        // sign(dir) with sign(0) = sign(NaN) = 0: torch's abs backward (grad * sgn(x)), as
        // k_rel_error_loss; the chain through p' = pred * scale + center adds the factor scale[c]
        const double sg = dir > 0.f ? 1.0 : (dir < 0.f ? -1.0 : 0.0);
        if (dpred) dpred[i] = (float)(sg * w * (double)fac * (double)sc / (double)den);
    }
    red[t] = acc;
    tree_sum256(red, t);
    if (t == 0) part[(int64_t)g * S + s] = red[0];
}

// one workgroup: per graph the S segment-block sums in order, over n_g C (no rows: 0 / 0 = NaN, as
// the torch path); the per-graph means by a fixed tree
__global__ __launch_bounds__(256) void k_graph_loss_finish(const double* __restrict__ part, int S, int B, int C,
                                                           const int32_t* __restrict__ rowptr, float mult,
                                                           float* __restrict__ loss) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int g = t; g < B; g += 256) {
        double sum = 0.0;
        for (int s = 0; s < S; ++s) sum += part[(int64_t)g * S + s];
        acc += sum / ((double)(rowptr[g + 1] - rowptr[g]) * (double)C);
    }
    red[t] = acc;
    tree_sum256(red, t);
    if (t == 0) *loss = (float)(red[0] / (double)B * (double)mult);
}

// segment-blocks per graph: about 2048 elements each at the mean graph size, at most 64
inline int loss_segments(int64_t N, int32_t C, int64_t B) {
    const int64_t per = (N * C + B - 1) / B;
    const int64_t S = (per + 2047) / 2048;
    return (int)(S < 1 ? 1 : (S > 64 ? 64 : S));
}

}  // namespace

}  // namespace bgnn

using namespace bgnn;

extern "C" size_t bgnn_graph_loss_ws_bytes(int64_t N, int32_t C, int64_t B) {
    return (B > 0 && N > 0 && C > 0) ? (size_t)B * loss_segments(N, C, B) * sizeof(double) : 0;
}

extern "C" int bgnn_graph_loss(const float* pred, const float* target, int64_t N, int32_t C, const int32_t* rowptr,
                               const int32_t* col, int64_t B, int32_t kind, float eps, float mult, const float* scale,
                               const float* center, float* loss, float* dpred, void* ws, size_t ws_bytes,
                               void* stream) {
    BGNN_REQUIRE(kind >= 0 && kind <= 2, "graph_loss: kind %d unknown (0 relative, 1 MAE, 2 squares)", kind);
    BGNN_REQUIRE(C >= 1 && C <= 8, "graph_loss: C=%d unsupported (1..8)", C);
    BGNN_REQUIRE(N >= 1 && N <= INT32_MAX && B >= 1 && B <= INT32_MAX, "graph_loss: N and B must be in [1, 2^31)");
    BGNN_REQUIRE(pred && target && rowptr && col && loss, "graph_loss: null pointer");
    BGNN_REQUIRE(ws && ((uintptr_t)ws & 7) == 0 && ws_bytes >= bgnn_graph_loss_ws_bytes(N, C, B),
                 "graph_loss: workspace too small or not 8-byte aligned");
    hipStream_t s = as_stream(stream);
    double* part = static_cast<double*>(ws);
    const int S = loss_segments(N, C, B);
    hipLaunchKernelGGL(k_graph_loss, dim3((unsigned)B, S), dim3(256), 0, s, pred, target, (int)C, rowptr, col, (int)B,
                       (int)kind, eps, mult, scale, center, part, dpred);
    BGNN_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_graph_loss_finish, dim3(1), dim3(256), 0, s, part, S, (int)B, (int)C, rowptr, mult, loss);
    BGNN_CHECK_LAUNCH();
    return BGNN_OK;
}
