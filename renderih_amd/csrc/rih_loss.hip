// rih_loss.hip -- fused training loss of the mesh decoder (core/Loss.py: GraphLoss.calc_loss + calc_loss_GCN) for gfx950.
//
// One workgroup per (image, hand).  The hand's predicted and ground-truth meshes (2 x 778 x 3 floats) live in LDS; the
// kernel produces in one pass (a) the raw sums of the seven loss terms of this hand and (b) the gradient of the weighted
// total with respect to every prediction tensor, so that neither the forward nor the backward of the loss launches
// anything else:
//   vertex, joint and face terms   rih_mesh_terms.h, the body shared with mano_loss_kernel (rih_mano_loss.hip)
//   coarse terms      SmoothL1 / MSE of the 252-vertex prediction against the ground truth gathered into graph order
//                     and average-pooled pairwise (vert_to_GCN + mesh_downsample, Loss.py:139-164)
// Every sum has a fixed order: no atomics, bit-reproducible.  Bound: latency (a few hundred KB per workgroup); it replaces ~600
// torch elementwise / index / fill launches per training step.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"
#include "rih_mesh_terms.h"

namespace {

constexpr int MAXPOOL = 16;

__global__ __launch_bounds__(TPB) void mesh_loss_kernel(rih_mesh_topo tp, const float* __restrict__ v3d_pred,
                                                        const float* __restrict__ v2d_pred,
                                                        const float* __restrict__ c3d_pred,
                                                        const float* __restrict__ c2d_pred,
                                                        const float* __restrict__ v3d_gt,
                                                        const float* __restrict__ v2d_gt,
                                                        const float* __restrict__ gt_shift,
                                                        const float* __restrict__ wdev, float img,
                                                        float* __restrict__ g_v3d, float* __restrict__ g_v2d,
                                                        float* __restrict__ g_c3d, float* __restrict__ g_c2d,
                                                        float* __restrict__ partial) {
    __shared__ float s_vp[MAXV * 3], s_vg[MAXV * 3];
    __shared__ float s_fg[MAXF * 9];
    __shared__ float s_gj[MAXJ * 3];
    __shared__ float s_red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const int V = tp.V;
    // term weights live in device memory so that a captured hipGraph follows the caller's epoch gate (edge term); each is
    // already divided by its element count and by 2 (hand average)
    float w[7];                                              // v2d, v3d, joint, norm, edge, c3d, c2d
#pragma unroll
    for (int i = 0; i < 7; ++i) w[i] = wdev[i];
    mesh_stage(tp, v3d_pred, v3d_gt, gt_shift, s_vp, s_vg);

    float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // raw sums, in the order of w
    mesh_terms(tp, w, img, v2d_pred, v2d_gt, g_v3d, g_v2d, s_vp, s_vg, s_fg, s_gj, s_red, acc);
    const float s2 = 2.f / img;
    // ---- coarse level: ground truth in graph order, average-pooled pairwise log2(pool) times
    for (int kc = t; kc < tp.Vc; kc += TPB) {
        float a3[MAXPOOL][3], a2[MAXPOOL][2];
        for (int i = 0; i < tp.pool; ++i) {
            const int v = tp.perm[kc * tp.pool + i];
#pragma unroll
            for (int c = 0; c < 3; ++c) a3[i][c] = s_vg[v * 3 + c];
#pragma unroll
            for (int c = 0; c < 2; ++c) a2[i][c] = v2d_gt[((long long)b * V + v) * 2 + c];
        }
        for (int m = tp.pool; m > 1; m >>= 1)
            for (int i = 0; i < m / 2; ++i) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a3[i][c] = (a3[2 * i][c] + a3[2 * i + 1][c]) * 0.5f;
#pragma unroll
                for (int c = 0; c < 2; ++c) a2[i][c] = (a2[2 * i][c] + a2[2 * i + 1][c]) * 0.5f;
            }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const long long o = ((long long)b * tp.Vc + kc) * 3 + c;
            const float d = c3d_pred[o] - a3[0][c];
            acc[5] += sl1(d);
            g_c3d[o] = w[5] * dsl1(d);
        }
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const long long o = ((long long)b * tp.Vc + kc) * 2 + c;
            const float d = (c2d_pred[o] * s2 - 1.f) - (a2[0][c] * s2 - 1.f);
            acc[6] += d * d;
            g_c2d[o] = w[6] * 2.f * d * s2;
        }
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) {
        const float s = block_sum(acc[i], s_red);
        if (t == 0) partial[b * 8 + i] = s;
    }
}

// out[0] = total; out[1..7] = the seven terms as the reference reports them (mean over elements, averaged over hands)
__global__ void mesh_loss_final_kernel(const float* __restrict__ pl, const float* __restrict__ pr, int B,
                                       const float* __restrict__ wdev, const float* __restrict__ cdev,
                                       float* __restrict__ out) {
    const int i = threadIdx.x;
    __shared__ float s_t[8];
    if (i < 7) {
        float sl = 0.f, sr = 0.f;
        for (int b = 0; b < B; ++b) { sl += pl[b * 8 + i]; sr += pr[b * 8 + i]; }
        const float wi = wdev[i], ci = cdev[i];
        s_t[i] = wi * (sl + sr);
        out[1 + i] = 0.5f * (sl + sr) / ci;
    }
    __syncthreads();
    if (i == 0) out[0] = ((s_t[0] + s_t[1]) + (s_t[2] + s_t[3])) + ((s_t[4] + s_t[5]) + s_t[6]);
}

}  // namespace

extern "C" int rih_mesh_loss(const rih_mesh_topo* tp, const float* v3d_pred, const float* v2d_pred, const float* c3d_pred,
                             const float* c2d_pred, const float* v3d_gt, const float* v2d_gt, const float* gt_shift,
                             const float* term_weights, float img_size, float* g_v3d, float* g_v2d, float* g_c3d,
                             float* g_c2d, float* partial, int B, void* stream) {
    if (!v3d_pred || !v2d_pred || !c3d_pred || !c2d_pred || !v3d_gt || !v2d_gt || !term_weights || !g_v3d || !g_v2d ||
        !g_c3d || !g_c2d || !partial || B < 1)
        return RIH_EINVAL;
    if (!mesh_topo_ok(tp) || !tp->perm || tp->Vc < 1 || tp->pool < 1 || tp->pool > MAXPOOL ||
        (tp->pool & (tp->pool - 1)) != 0 || img_size <= 0.f)
        return RIH_EINVAL;
    hipLaunchKernelGGL(mesh_loss_kernel, dim3(B), dim3(TPB), 0, (hipStream_t)stream, *tp, v3d_pred, v2d_pred, c3d_pred,
                       c2d_pred, v3d_gt, v2d_gt, gt_shift, term_weights, img_size, g_v3d, g_v2d, g_c3d, g_c2d, partial);
    return (int)hipGetLastError();
}

extern "C" int rih_mesh_loss_final(const float* partial_left, const float* partial_right, int B, const float* term_weights,
                                   const float* counts, float* out, void* stream) {
    if (!partial_left || !partial_right || !term_weights || !counts || !out || B < 1) return RIH_EINVAL;
    hipLaunchKernelGGL(mesh_loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial_left, partial_right, B,
                       term_weights, counts, out);
    return (int)hipGetLastError();
}
