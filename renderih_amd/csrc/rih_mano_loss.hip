// rih_mano_loss.hip -- fused training loss of the MANO-head model (core/Loss_mano.py: ManoLoss + mano_loss_GCN) for gfx950.
//
// One workgroup per (image, hand), like mesh_loss_kernel of rih_loss.hip: the mesh half of both kernels is the one body
// of rih_mesh_terms.h, so a guard or an epsilon of the vertex, joint and face terms is changed once for both losses.  The
// hand's predicted and ground-truth meshes (2 x 778 x 3 floats) and the per-face gradient staging (1538 x 9 floats) live
// in LDS, 77 KB of the 160 KB of a CU.  In one pass the kernel produces the raw sums of the seven per-hand terms plus the
// hand's sum of squared shape coefficients, and the gradient of the weighted total with respect to that hand's vertices,
// 2-D vertices, 48 pose and 10 shape entries:
//   vertex / joint / face terms   as GraphLoss.calc_mano_loss (Loss_mano.py:110-159): rih_mesh_terms.h, no coarse level
//   pose term                     MSE of batch_rodrigues(pred) against batch_rodrigues(label), 16 rotations, differentiated
//                                 as written (angle |a + 1e-8|, axis a / angle, quaternion, normalised again, quat2mat)
//   shape term + regulariser      MSE(shape, label) and 0.005 * sum(shape^2) (gradient 0.01 * shape)
// mano_loss_final_kernel (one workgroup) sums the partials in a fixed order, adds the root offset term and the
// regulariser, writes the gradient with respect to the predicted root_rel and the term vector.  Every sum has a fixed
// order: two evaluations are bit-identical.  Bound: latency.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"
#include "rih_mesh_terms.h"

namespace {

constexpr int NROT = 16, POSE = 48, SHAPE = 10;
constexpr int NPART = 8;            // v2d, v3d, joint, norm, edge, pose, shape (raw sums), sum(shape^2)
constexpr int NW = 9;               // term weights: the seven above, root offset, regulariser

// batch_rodrigues (Loss_mano.py:48-59) of one axis-angle; keeps what the backward needs
struct Rod {
    float a[3], s[3], n, u[3], c, sn, q[4], qn, nq[4], R[9];
};

__device__ __forceinline__ void rod_fwd(const float* a, Rod& r) {
    for (int i = 0; i < 3; ++i) {
        r.a[i] = a[i];
        r.s[i] = a[i] + 1e-8f;
    }
    r.n = sqrtf(r.s[0] * r.s[0] + r.s[1] * r.s[1] + r.s[2] * r.s[2]);
    for (int i = 0; i < 3; ++i) r.u[i] = a[i] / r.n;
    const float h = r.n * 0.5f;
    r.c = cosf(h);
    r.sn = sinf(h);
    r.q[0] = r.c;
    for (int i = 0; i < 3; ++i) r.q[i + 1] = r.sn * r.u[i];
    r.qn = sqrtf(r.q[0] * r.q[0] + r.q[1] * r.q[1] + r.q[2] * r.q[2] + r.q[3] * r.q[3]);
    for (int i = 0; i < 4; ++i) r.nq[i] = r.q[i] / r.qn;
    const float w = r.nq[0], x = r.nq[1], y = r.nq[2], z = r.nq[3];
    const float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    r.R[0] = w2 + x2 - y2 - z2; r.R[1] = 2.f * x * y - 2.f * w * z; r.R[2] = 2.f * w * y + 2.f * x * z;
    r.R[3] = 2.f * w * z + 2.f * x * y; r.R[4] = w2 - x2 + y2 - z2; r.R[5] = 2.f * y * z - 2.f * w * x;
    r.R[6] = 2.f * x * z - 2.f * w * y; r.R[7] = 2.f * w * x + 2.f * y * z; r.R[8] = w2 - x2 - y2 + z2;
}

// gradient with respect to the axis-angle, given the gradient g[9] with respect to R, through the chain as written
__device__ __forceinline__ void rod_bwd(const Rod& r, const float* g, float* ga) {
    const float w = r.nq[0], x = r.nq[1], y = r.nq[2], z = r.nq[3];
    const float gd = g[0] + g[4] + g[8];
    float gq[4];
    gq[0] = 2.f * (w * gd - z * g[1] + y * g[2] + z * g[3] - x * g[5] - y * g[6] + x * g[7]);
    gq[1] = 2.f * (x * (g[0] - g[4] - g[8]) + y * g[1] + z * g[2] + y * g[3] - w * g[5] + z * g[6] + w * g[7]);
    gq[2] = 2.f * (y * (g[4] - g[0] - g[8]) + x * g[1] + w * g[2] + x * g[3] + z * g[5] - w * g[6] + z * g[7]);
    gq[3] = 2.f * (z * (g[8] - g[0] - g[4]) - w * g[1] + x * g[2] + w * g[3] + y * g[5] + x * g[6] + y * g[7]);
    // q / |q|
    const float dot = gq[0] * w + gq[1] * x + gq[2] * y + gq[3] * z;
    float gqq[4];
    for (int i = 0; i < 4; ++i) gqq[i] = (gq[i] - r.nq[i] * dot) / r.qn;
    // q = [cos(n/2), sin(n/2) u]
    float gsn = 0.f, gu[3];
    for (int i = 0; i < 3; ++i) {
        gsn += gqq[i + 1] * r.u[i];
        gu[i] = r.sn * gqq[i + 1];
    }
    float gn = 0.5f * (-r.sn * gqq[0] + r.c * gsn);
    // u = a / n
    float gua = 0.f;
    for (int i = 0; i < 3; ++i) gua += gu[i] * r.a[i];
    gn -= gua / (r.n * r.n);
    // n = |a + 1e-8|
    for (int i = 0; i < 3; ++i) ga[i] = gu[i] / r.n + gn * r.s[i] / r.n;
}

__global__ __launch_bounds__(TPB) void mano_loss_kernel(rih_mesh_topo tp, const float* __restrict__ v3d_pred,
                                                        const float* __restrict__ v2d_pred,
                                                        const float* __restrict__ pose_pred,
                                                        const float* __restrict__ shape_pred,
                                                        const float* __restrict__ v3d_gt,
                                                        const float* __restrict__ v2d_gt,
                                                        const float* __restrict__ pose_gt,
                                                        const float* __restrict__ shape_gt,
                                                        const float* __restrict__ gt_shift,
                                                        const float* __restrict__ wdev, float img,
                                                        float* __restrict__ g_v3d, float* __restrict__ g_v2d,
                                                        float* __restrict__ g_pose, float* __restrict__ g_shape,
                                                        float* __restrict__ partial) {
    __shared__ float s_vp[MAXV * 3], s_vg[MAXV * 3];
    __shared__ float s_fg[MAXF * 9];
    __shared__ float s_gj[MAXJ * 3];
    __shared__ float s_red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    // term weights live in device memory so that a captured hipGraph follows the caller's epoch gate (edge term)
    float w[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = wdev[i];
    mesh_stage(tp, v3d_pred, v3d_gt, gt_shift, s_vp, s_vg);

    float acc[NPART] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    mesh_terms(tp, w, img, v2d_pred, v2d_gt, g_v3d, g_v2d, s_vp, s_vg, s_fg, s_gj, s_red, acc);
    // ---- pose term: one rotation per thread of the first 16, prediction and label both through batch_rodrigues
    if (t < NROT) {
        const long long o = (long long)b * POSE + t * 3;
        Rod rp, rg;
        rod_fwd(pose_pred + o, rp);
        rod_fwd(pose_gt + o, rg);
        float gR[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const float d = rp.R[i] - rg.R[i];
            acc[5] += d * d;
            gR[i] = w[5] * 2.f * d;
        }
        float ga[3];
        rod_bwd(rp, gR, ga);
        g_pose[o + 0] = ga[0]; g_pose[o + 1] = ga[1]; g_pose[o + 2] = ga[2];
    } else if (t >= 64 && t < 64 + SHAPE) {     // ---- shape term and regulariser (second wavefront)
        const long long o = (long long)b * SHAPE + (t - 64);
        const float s = shape_pred[o], d = s - shape_gt[o];
        acc[6] += d * d;
        acc[7] += s * s;
        g_shape[o] = w[6] * 2.f * d + w[8] * 2.f * s;
    }
#pragma unroll
    for (int i = 0; i < NPART; ++i) {
        const float s = block_sum(acc[i], s_red);
        if (t == 0) partial[b * NPART + i] = s;
    }
}

// out[0] = total; out[1..9] = vert2d, vert3d, joint, norm, edge, pose, shape (means, averaged over the hands), rootrel,
// regularize (as the reference reports them).  g_rootrel = gradient of the total with respect to the predicted root_rel.
__global__ __launch_bounds__(TPB) void mano_loss_final_kernel(const float* __restrict__ pl, const float* __restrict__ pr,
                                                              const float* __restrict__ rel_pred,
                                                              const float* __restrict__ rel_gt, int B,
                                                              const float* __restrict__ wdev,
                                                              const float* __restrict__ cdev,
                                                              float* __restrict__ g_rel, float* __restrict__ out) {
    const int t = threadIdx.x;
    __shared__ float s_t[NPART + 2];
    __shared__ float s_red[4];
    const float wrel = wdev[7];
    float r = 0.f;
    for (int i = t; i < B * 3; i += TPB) {          // fixed assignment and fixed reduction tree: reproducible
        const float d = rel_pred[i] - rel_gt[i];
        r += d * d;
        g_rel[i] = wrel * 2.f * d;
    }
    r = block_sum(r, s_red);
    if (t < NPART) {
        float sl = 0.f, sr = 0.f;
        for (int b = 0; b < B; ++b) { sl += pl[b * NPART + t]; sr += pr[b * NPART + t]; }
        if (t < 7) {
            s_t[t] = wdev[t] * (sl + sr);
            out[1 + t] = 0.5f * (sl + sr) / cdev[t];
        } else {                                    // regulariser: 0.005 * (sum left^2 + sum right^2), not halved
            s_t[8] = wdev[8] * (sl + sr);
            out[9] = s_t[8];
        }
    }
    if (t == 0) {
        s_t[7] = wrel * r;
        out[8] = s_t[7];
    }
    __syncthreads();
    if (t == 0)
        out[0] = (((s_t[0] + s_t[1]) + (s_t[2] + s_t[3])) + ((s_t[4] + s_t[5]) + (s_t[6] + s_t[7]))) + s_t[8];
}

}  // namespace

extern "C" int rih_mano_loss(const rih_mesh_topo* tp, const float* v3d_pred, const float* v2d_pred, const float* pose_pred,
                             const float* shape_pred, const float* v3d_gt, const float* v2d_gt, const float* pose_gt,
                             const float* shape_gt, const float* gt_shift, int pose_dim, int shape_dim,
                             const float* term_weights, float img_size, float* g_v3d, float* g_v2d, float* g_pose,
                             float* g_shape, float* partial, int B, void* stream) {
    if (!v3d_pred || !v2d_pred || !pose_pred || !shape_pred || !v3d_gt || !v2d_gt || !pose_gt || !shape_gt ||
        !term_weights || !g_v3d || !g_v2d || !g_pose || !g_shape || !partial || B < 1)
        return RIH_EINVAL;
    if (!mesh_topo_ok(tp) || pose_dim != POSE || shape_dim != SHAPE || !(img_size > 0.f)) return RIH_EINVAL;
    hipLaunchKernelGGL(mano_loss_kernel, dim3(B), dim3(TPB), 0, (hipStream_t)stream, *tp, v3d_pred, v2d_pred, pose_pred,
                       shape_pred, v3d_gt, v2d_gt, pose_gt, shape_gt, gt_shift, term_weights, img_size, g_v3d, g_v2d,
                       g_pose, g_shape, partial);
    return (int)hipGetLastError();
}

extern "C" int rih_mano_loss_final(const float* partial_left, const float* partial_right, const float* rootrel_pred,
                                   const float* rootrel_gt, int B, const float* term_weights, const float* counts,
                                   float* g_rootrel, float* out, void* stream) {
    if (!partial_left || !partial_right || !rootrel_pred || !rootrel_gt || !term_weights || !counts || !g_rootrel ||
        !out || B < 1)
        return RIH_EINVAL;
    hipLaunchKernelGGL(mano_loss_final_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, partial_left, partial_right,
                       rootrel_pred, rootrel_gt, B, term_weights, counts, g_rootrel, out);
    return (int)hipGetLastError();
}
