// rih_anchor.hip -- contact anchors of the pose optimiser (manopth/anchorlayer.py, anchorutils.py:51-65 recover_anchor_batch) for
// gfx950: every anchor is a fixed affine combination of the three vertices of one face,
//   anchor[b][a] = w1 (v1 - v0) + w2 (v2 - v0) + v0,   (v0, v1, v2) = vertices[b][face_vert_idx[a][0..2]].
// Forward: thread = (sample, anchor, coordinate).  Backward: thread = (sample, vertex, coordinate) gathering through the
// vertex -> (anchor * 3 + corner) lists the host builds once per index tensor (renderih_amd.quat_mano.anchor_csr, which also
// range-checks the indices): no atomics, a fixed summation order, exact zeros for the vertices no anchor reads.
// Both are latency-bound at the optimiser's sizes (B x 108 x 3 outputs from B x 778 x 3 inputs): one short launch each.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"

namespace {

__global__ __launch_bounds__(256) void anchor_fwd_kernel(const float* __restrict__ verts, const int32_t* __restrict__ fvi,
                                                         const float* __restrict__ w, float* __restrict__ out, long long total,
                                                         int V, int A) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % 3), a = (int)((i / 3) % A);
    const long long b = i / (3LL * A);
    const float* vb = verts + b * V * 3;
    const float v0 = vb[fvi[a * 3] * 3 + c], v1 = vb[fvi[a * 3 + 1] * 3 + c], v2 = vb[fvi[a * 3 + 2] * 3 + c];
    out[i] = (w[a * 2] * (v1 - v0) + w[a * 2 + 1] * (v2 - v0)) + v0;
}

__global__ __launch_bounds__(256) void anchor_bwd_kernel(const float* __restrict__ g, const int32_t* __restrict__ vptr,
                                                         const int32_t* __restrict__ vlist, const float* __restrict__ w,
                                                         float* __restrict__ dverts, long long total, int V, int A) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % 3), v = (int)((i / 3) % V);
    const long long b = i / (3LL * V);
    const float* gb = g + b * A * 3;
    float acc = 0.f;
    for (int q = vptr[v]; q < vptr[v + 1]; ++q) {
        const int e = vlist[q], a = e / 3, corner = e - a * 3;
        const float ga = gb[a * 3 + c];
        // d anchor / d v0 = 1 - w1 - w2, / d v1 = w1, / d v2 = w2
        acc += (corner == 0) ? (ga - w[a * 2] * ga) - w[a * 2 + 1] * ga : w[a * 2 + corner - 1] * ga;
    }
    dverts[i] = acc;
}

}  // namespace

extern "C" int rih_anchor_fwd(const float* vertices, const int32_t* face_vert_idx, const float* weight, float* anchors, int B,
                              int V, int A, void* stream) {
    if (!vertices || !face_vert_idx || !weight || !anchors || B < 1 || V < 1 || A < 1) return RIH_EINVAL;
    const long long total = (long long)B * A * 3;
    if ((total + 255) / 256 > 0x7fffffffLL) return RIH_EINVAL;
    hipLaunchKernelGGL(anchor_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, vertices,
                       face_vert_idx, weight, anchors, total, V, A);
    return (int)hipGetLastError();
}

extern "C" int rih_anchor_bwd(const float* g_anchors, const int32_t* vptr, const int32_t* vlist, const float* weight,
                              float* g_vertices, int B, int V, int A, void* stream) {
    if (!g_anchors || !vptr || !vlist || !weight || !g_vertices || B < 1 || V < 1 || A < 1) return RIH_EINVAL;
    const long long total = (long long)B * V * 3;
    if ((total + 255) / 256 > 0x7fffffffLL) return RIH_EINVAL;
    hipLaunchKernelGGL(anchor_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g_anchors,
                       vptr, vlist, weight, g_vertices, total, V, A);
    return (int)hipGetLastError();
}
