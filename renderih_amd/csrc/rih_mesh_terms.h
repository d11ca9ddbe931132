// rih_mesh_terms.h -- the per-hand mesh terms that both fused training losses form (core/Loss.py: GraphLoss.calc_mano_loss,
// which core/Loss_mano.py's ManoLoss inherits), written once: mesh_loss_kernel (rih_loss.hip) and mano_loss_kernel
// (rih_mano_loss.hip) stage the two meshes with mesh_stage() and call mesh_terms().  One workgroup of TPB threads per
// (image, hand); the LDS arrays are declared by the kernels and passed in.
//   vertex terms      SmoothL1(v3d), MSE(v2d / img * 2 - 1)                                   (Loss.py:108-110)
//   joint term        SmoothL1(J v3d_pred, J v3d_gt), J = 21 x 778 regressor incl. tips      (Loss.py:38-53, 105-111)
//   face terms        normal consistency <e_pred / |e_pred|, n_gt> and edge length, 1538 faces x 3 edges  (Loss.py:68-102)
// Face gradients are written per face to LDS and gathered per vertex through a vertex->(face, corner) adjacency list
// in a fixed order: no atomics, bit-reproducible.  The order of every expression here is pinned bitwise by both losses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"
#include "rih_reduce.h"

constexpr int TPB = 256;
constexpr int MAXV = 800, MAXF = 1600, MAXJ = 24;

__device__ __forceinline__ float sl1(float x) {          // nn.SmoothL1Loss(beta=1)
    const float a = fabsf(x);
    return a < 1.f ? 0.5f * x * x : a - 0.5f;
}
__device__ __forceinline__ float dsl1(float x) { return fabsf(x) < 1.f ? x : (x > 0.f ? 1.f : -1.f); }

// The kernels take the caller's rih_mesh_topo by value (five device pointers, five ints).  The body reads faces, vptr, vlist,
// J, V, F and NJ; perm, Vc and pool belong to the coarse level of rih_loss.hip.  What both entry points require of it:
inline bool mesh_topo_ok(const rih_mesh_topo* tp) {
    return tp && tp->faces && tp->vptr && tp->vlist && tp->J && tp->V >= 1 && tp->V <= MAXV && tp->F >= 1 && tp->F <= MAXF &&
           tp->NJ >= 1 && tp->NJ <= MAXJ;
}

// s_vp = this workgroup's predicted mesh, s_vg = its ground truth + gt_shift (NULL: none); ends with a barrier
__device__ __forceinline__ void mesh_stage(const rih_mesh_topo& tp, const float* v3d_pred, const float* v3d_gt,
                                           const float* gt_shift, float* s_vp, float* s_vg) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int V = tp.V;
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
}

// Adds this thread's share of the raw sums into acc[0..4] (v2d, v3d, joint, norm, edge) and writes the gradient of the
// weighted total with respect to this workgroup's 2-D and 3-D vertices; w[0..4] = the weights of the five terms.
// LDS: s_fg[MAXF * 9], s_gj[MAXJ * 3], s_red[4].
__device__ __forceinline__ void mesh_terms(const rih_mesh_topo& tp, const float* w, float img, const float* v2d_pred,
                                           const float* v2d_gt, float* g_v3d, float* g_v2d, const float* s_vp,
                                           const float* s_vg, float* s_fg, float* s_gj, float* s_red, float* acc) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int V = tp.V, F = tp.F;
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
                // gn * dn + ge * de with the contraction spelled out: left to the compiler, either product is fused into
                // the sum, depending on the code around it, and the two forms differ in the last bit
                s_fg[f * 9 + e * 3 + c] = fmaf(gn, dn, ge * de);
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
}
