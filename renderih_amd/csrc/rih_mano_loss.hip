// rih_mano_loss.hip -- fused training loss of the MANO-head model (core/Loss_mano.py: ManoLoss + mano_loss_GCN) for gfx950.
//
// One workgroup per (image, hand), like mesh_loss_kernel of rih_loss.hip (whose arithmetic the mesh half repeats; that
// file is left untouched so that the family-(a) loss stays bit-identical).  The hand's predicted and ground-truth meshes
// (2 x 778 x 3 floats) and the per-face gradient staging (1538 x 9 floats) live in LDS, 77 KB of the 160 KB of a CU.  In
// one pass the kernel produces the raw sums of the seven per-hand terms plus the hand's sum of squared shape coefficients,
// and the gradient of the weighted total with respect to that hand's vertices, 2-D vertices, 48 pose and 10 shape entries:
//   vertex / joint / face terms   as GraphLoss.calc_mano_loss (Loss_mano.py:110-159), no coarse level
//   pose term                     MSE of batch_rodrigues(pred) against batch_rodrigues(label), 16 rotations, differentiated
//                                 as written (angle |a + 1e-8|, axis a / angle, quaternion, normalised again, quat2mat)
//   shape term + regulariser      MSE(shape, label) and 0.005 * sum(shape^2) (gradient 0.01 * shape)
// mano_loss_final_kernel (one workgroup) sums the partials in a fixed order, adds the root offset term and the
// regulariser, writes the gradient with respect to the predicted root_rel and the term vector.  Every sum has a fixed
// order: two evaluations are bit-identical.  Bound: latency.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"

namespace {

constexpr int TPB = 256;
constexpr int MAXV = 800, MAXF = 1600, MAXJ = 24;
constexpr int NROT = 16, POSE = 48, SHAPE = 10;
constexpr int NPART = 8;            // v2d, v3d, joint, norm, edge, pose, shape (raw sums), sum(shape^2)
constexpr int NW = 9;               // term weights: the seven above, root offset, regulariser

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sum over the 256 threads of the block; the result is valid in every thread
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float sl1(float x) {          // nn.SmoothL1Loss(beta=1)
    const float a = fabsf(x);
    return a < 1.f ? 0.5f * x * x : a - 0.5f;
}
__device__ __forceinline__ float dsl1(float x) { return fabsf(x) < 1.f ? x : (x > 0.f ? 1.f : -1.f); }

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

struct Topo {
    const int32_t* faces;
    const int32_t* vptr;
    const int32_t* vlist;
    const float* J;
    int V, F, NJ;
};

__global__ __launch_bounds__(TPB) void mano_loss_kernel(Topo tp, const float* __restrict__ v3d_pred,
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
    const int V = tp.V, F = tp.F;
    // term weights live in device memory so that a captured hipGraph follows the caller's epoch gate (edge term)
    float w[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = wdev[i];
    const float* vp = v3d_pred + (long long)b * V * 3;
    const float* vg = v3d_gt + (long long)b * V * 3;
    float sh[3] = {0.f, 0.f, 0.f};
    if (gt_shift != nullptr) {
        sh[0] = gt_shift[b * 3 + 0];
        sh[1] = gt_shift[b * 3 + 1];
        sh[2] = gt_shift[b * 3 + 2];
    }
    for (int i = t; i < V * 3; i += TPB) {
        s_vp[i] = vp[i];
        s_vg[i] = vg[i] + sh[i % 3];
    }
    __syncthreads();

    float acc[NPART] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    constexpr int VPT = (MAXV + TPB - 1) / TPB;              // vertices per thread
    float gv[VPT][3];
    // ---- vertex terms
    const float s2 = 2.f / img;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int v = t + TPB * k;
        gv[k][0] = gv[k][1] = gv[k][2] = 0.f;
        if (v < V) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float d = s_vp[v * 3 + c] - s_vg[v * 3 + c];
                acc[1] += sl1(d);
                gv[k][c] = w[1] * dsl1(d);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const long long o = ((long long)b * V + v) * 2 + c;
                const float d = (v2d_pred[o] * s2 - 1.f) - (v2d_gt[o] * s2 - 1.f);
                acc[0] += d * d;
                g_v2d[o] = w[0] * 2.f * d * s2;
            }
        }
    }
    // ---- joint term: jp = J vp, jg = J vg  (21 x 3 each)
    for (int j = 0; j < tp.NJ; ++j) {
        float p[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f};
        const float* Jr = tp.J + (long long)j * V;
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const int v = t + TPB * k;
            if (v < V) {
                const float jw = Jr[v];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    p[c] += jw * s_vp[v * 3 + c];
                    g[c] += jw * s_vg[v * 3 + c];
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = block_sum(p[c], s_red) - block_sum(g[c], s_red);
            if (t == 0) {
                acc[2] += sl1(d);
                s_gj[j * 3 + c] = w[2] * dsl1(d);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int v = t + TPB * k;
        if (v < V) {
            for (int j = 0; j < tp.NJ; ++j) {
                const float jw = tp.J[(long long)j * V + v];
#pragma unroll
                for (int c = 0; c < 3; ++c) gv[k][c] += jw * s_gj[j * 3 + c];
            }
        }
    }
    // ---- face terms: per face the gradient with respect to its three edge vectors, into LDS
    for (int f = t; f < F; f += TPB) {
        const int i0 = tp.faces[f * 3 + 0], i1 = tp.faces[f * 3 + 1], i2 = tp.faces[f * 3 + 2];
        float ep[3][3], eg[3][3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p0 = s_vp[i0 * 3 + c], p1 = s_vp[i1 * 3 + c], p2 = s_vp[i2 * 3 + c];
            const float q0 = s_vg[i0 * 3 + c], q1 = s_vg[i1 * 3 + c], q2 = s_vg[i2 * 3 + c];
            ep[0][c] = p0 - p1; ep[1][c] = p1 - p2; ep[2][c] = p2 - p0;
            eg[0][c] = q0 - q1; eg[1][c] = q1 - q2; eg[2][c] = q2 - q0;
        }
        float n[3] = {eg[0][1] * eg[1][2] - eg[0][2] * eg[1][1], eg[0][2] * eg[1][0] - eg[0][0] * eg[1][2],
                      eg[0][0] * eg[1][1] - eg[0][1] * eg[1][0]};
        const float nl = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-12f);      // F.normalize eps
        n[0] /= nl; n[1] /= nl; n[2] /= nl;
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const float len = sqrtf(ep[e][0] * ep[e][0] + ep[e][1] * ep[e][1] + ep[e][2] * ep[e][2]);
            const float leng = sqrtf(eg[e][0] * eg[e][0] + eg[e][1] * eg[e][1] + eg[e][2] * eg[e][2]);
            const float den = fmaxf(len, 1e-12f);
            const float u[3] = {ep[e][0] / den, ep[e][1] / den, ep[e][2] / den};
            const float d = u[0] * n[0] + u[1] * n[1] + u[2] * n[2];
            acc[3] += sl1(d);
            const float dl = len - leng;
            acc[4] += sl1(dl);
            const float gn = w[3] * dsl1(d), ge = w[4] * dsl1(dl);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // d<u,n>/de = (n - u <u,n>) / |e|   (|e| > eps);   d|e|/de = e / |e| (0 at e = 0, as torch)
                const float dn = (len > 1e-12f) ? (n[c] - u[c] * d) / den : n[c] / den;
                const float de = (len > 0.f) ? ep[e][c] / len : 0.f;
                s_fg[f * 9 + e * 3 + c] = gn * dn + ge * de;
            }
        }
    }
    __syncthreads();
    // ---- gather face gradients per vertex (fixed order), write the 3-D vertex gradient
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
        const int v = t + TPB * k;
        if (v < V) {
            for (int q = tp.vptr[v]; q < tp.vptr[v + 1]; ++q) {
                const int fc = tp.vlist[q];
                const int f = fc / 3, c0 = fc - f * 3;
                // corner c0 of the face is the head of edge c0 (e_c0 = v_c0 - v_{c0+1}) and the tail of edge c0-1
                const float* ga = s_fg + f * 9 + c0 * 3;
                const float* gb = s_fg + f * 9 + ((c0 + 2) % 3) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) gv[k][c] += ga[c] - gb[c];
            }
            float* o = g_v3d + ((long long)b * V + v) * 3;
            o[0] = gv[k][0]; o[1] = gv[k][1]; o[2] = gv[k][2];
        }
    }
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
    if (!tp || !v3d_pred || !v2d_pred || !pose_pred || !shape_pred || !v3d_gt || !v2d_gt || !pose_gt || !shape_gt ||
        !term_weights || !g_v3d || !g_v2d || !g_pose || !g_shape || !partial || B < 1)
        return RIH_EINVAL;
    if (!tp->faces || !tp->vptr || !tp->vlist || !tp->J || tp->V < 1 || tp->V > MAXV || tp->F < 1 || tp->F > MAXF ||
        tp->NJ < 1 || tp->NJ > MAXJ || pose_dim != POSE || shape_dim != SHAPE || !(img_size > 0.f))
        return RIH_EINVAL;
    Topo t{tp->faces, tp->vptr, tp->vlist, tp->J, tp->V, tp->F, tp->NJ};
    hipLaunchKernelGGL(mano_loss_kernel, dim3(B), dim3(TPB), 0, (hipStream_t)stream, t, v3d_pred, v2d_pred, pose_pred,
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
