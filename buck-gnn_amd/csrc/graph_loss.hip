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
#include "graph_loss_elem.h"

namespace bgnn {

namespace {

// block (g, s): segment-block s of graph g (graph_loss_elem.h); its sum goes to part[g * S + s]
__global__ __launch_bounds__(256) void k_graph_loss(const float* __restrict__ pred, const float* __restrict__ target,
                                                    int C, const int32_t* __restrict__ rowptr,
                                                    const int32_t* __restrict__ col, int B, int kind, float eps,
                                                    float mult, const float* __restrict__ scale,
                                                    const float* __restrict__ center, double* __restrict__ part,
                                                    float* __restrict__ dpred) {
    __shared__ double red[256];
    graph_loss_block(pred, target, C, rowptr, col, B, kind, eps, (double)mult, scale, center, part, dpred, red,
                     blockIdx.x, gridDim.y, blockIdx.y);
}

// one workgroup: the per-graph means and their mean over graphs (graph_loss_elem.h)
__global__ __launch_bounds__(256) void k_graph_loss_finish(const double* __restrict__ part, int S, int B, int C,
                                                           const int32_t* __restrict__ rowptr, float mult,
                                                           float* __restrict__ loss) {
    __shared__ double red[256];
    graph_loss_finish_block(part, S, B, C, rowptr, (double)mult, loss, red);
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
