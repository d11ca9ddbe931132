// rih_pose_prior.hip -- hand-prior and contact terms of the pose optimiser's two-hand objective for gfx950
// (pose_data_optimize/hocontact/postprocess/geo_loss.py: HandLoss.batch_pose_quat_norm_loss, edge_len_loss,
// hand_pose_ergonomics_loss, FieldLoss.batch_contact_loss, summed as geo_optimizer_both_batch.py:805-824 does for mode='both';
// renderih_amd.pose_prior.FusedTwoHandPriorLoss, whose docstring lists the reference's quirks kept here).
//
// pose_prior_fwd_kernel: one workgroup of 256 threads per (sample, hand).
//   lanes 0..15   one quaternion each: the norm term on the raw quaternion; lanes 1..15 also the finger joint's relative
//                 frame rel = Lm R(q) Rm (R = quadratic form / |q|^2, which is R of the normalised quaternion; Lm, Rm: the
//                 host's products of the axis tables and the identity pose's frame), every ergonomics term of that joint and
//                 its analytic gradient d rel -> d R -> d q including the 1/|q|^2 term.  The pinky/ring coupling reads the two
//                 bends through LDS.
//   all threads   the E edges strided over the workgroup (value), then the vertices strided (gradient, gathered through the
//                 host-built vertex -> (edge * 2 + end) lists: no atomics, exact zeros for a vertex without an edge).
//   contact       the left (sub) hand's workgroup sums elastic * |sub[i] - main[id[i][d]]|^2 and writes the sub anchors'
//                 gradient; the right (main) hand's workgroup gathers the main anchors' gradient through the per-sample
//                 anchor -> (i * D + d) lists.
// Every workgroup writes its four partial terms (already scaled by 1/(16B), 1/(BE), 1/B.., 1/mask_sum) and the COMPLETE scaled
// gradient of the loss for its slices.  pose_prior_reduce_kernel sums the partials over the batch in index order;
// pose_prior_bwd_kernel multiplies the saved gradients by the upstream scalar.  All of it is launch-latency class
// (B <= 32: 64 workgroups, ~50 kB read); sums are taken in a fixed order, so two evaluations are bit-identical.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"
#include "rih_reduce.h"

namespace {

constexpr int TPB = 256;
constexpr float PI_F = 3.14159265358979323846f;

// degrees: bend range of each finger joint; splay range of the five finger bases (lo > hi: no splay term)
__constant__ float BEND_LO[15] = {-25, -4, -8, -25, -7, -8, -22, -8, -8, -25, -10, -8, -20, -35, -10};
__constant__ float BEND_HI[15] = {70, 110, 90, 80, 100, 90, 70, 90, 90, 70, 100, 90, 40, 50, 100};
__constant__ float SPLAY_LO[15] = {-25, 1, 1, -15, 1, 1, -20, 1, 1, -25, 1, 1, -30, 1, 1};
__constant__ float SPLAY_HI[15] = {15, 0, 0, 15, 0, 0, 30, 0, 0, 15, 0, 0, 30, 0, 0};

// max(relu(a - hi), relu(lo - a)) / 180 * pi, squared and weighted: adds to the loss, returns d loss / d a * (180 / pi)
__device__ __forceinline__ float hinge(float a, float lo, float hi, float wgt, float& loss) {
    const float up = fmaxf(a - hi, 0.f), down = fmaxf(lo - a, 0.f);
    const float h = fmaxf(up, down) / 180.f * PI_F;
    loss += h * h * wgt;
    return (up > down ? 2.f : (down > up ? -2.f : 0.f)) * h * wgt;
}

__device__ __forceinline__ void mul3(const float* a, const float* b, float* c) {         // c = a b
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[r * 3 + k] = a[r * 3] * b[k] + a[r * 3 + 1] * b[3 + k] + a[r * 3 + 2] * b[6 + k];
}

__device__ __forceinline__ void mul3_tn(const float* a, const float* b, float* c) {      // c = a^T b
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[r * 3 + k] = a[r] * b[k] + a[3 + r] * b[3 + k] + a[6 + r] * b[6 + k];
}

__device__ __forceinline__ void mul3_nt(const float* a, const float* b, float* c) {      // c = a b^T
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) c[r * 3 + k] = a[r * 3] * b[k * 3] + a[r * 3 + 1] * b[k * 3 + 1] + a[r * 3 + 2] * b[k * 3 + 2];
}

struct PriorArgs {
    const float* q[2];
    const float* verts[2];
    const float* anchors[2];
    const float* tables;            // [2][15][18]: Lm, Rm
    const int32_t* edges;           // [E][2]
    const float* static_len;        // [2][E]
    const int32_t* vptr;            // [V+1]
    const int32_t* vlist;           // [2E]: edge * 2 + end
    const int32_t* anchor_id;       // [B][A][D]
    const float* elastic;           // [B][A][D]
    const int32_t* cptr;            // [B][A+1]
    const int32_t* clist;           // [B][A*D]: i * D + d
    float inv_mask, lambda_contact;
    float* g_q[2];
    float* g_verts[2];
    float* g_anchors[2];
    float* partial;                 // [B][2][4]: quaternion norm, edge, ergonomics, contact (left hand's slot)
    int B, V, E, A, D;
};

__global__ __launch_bounds__(TPB) void pose_prior_fwd_kernel(const PriorArgs p) {
    __shared__ float s_bend[16], s_qn[16], s_er[16], s_red[4];
    const int hand = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float inv_b = 1.f / (float)p.B;

    // ---------------------------------------------------------------- quaternions: norm term, ergonomics
    float w = 1.f, x = 0.f, y = 0.f, z = 0.f, n2 = 1.f, l_er = 0.f, dth_bend = 0.f;
    float rel[9], G[9], Lm[9], Rm[9];
    float bend = 0.f;
    const int f = tid - 1;                                       // finger joint 0..14 on lanes 1..15
    const bool joint = tid >= 1 && tid < 16;
    if (tid < 16) {
        const float* q = p.q[hand] + ((size_t)b * 16 + tid) * 4;
        w = q[0], x = q[1], y = q[2], z = q[3];
        n2 = w * w + x * x + y * y + z * z;
        if (hand == 1) y = -y, z = -z;                           // the left hand's copy
    }
    if (joint) {
        const float* t = p.tables + ((size_t)hand * 15 + f) * 18;
#pragma unroll
        for (int i = 0; i < 9; ++i) Lm[i] = t[i], Rm[i] = t[9 + i], G[i] = 0.f;
        const float R[9] = {(w * w + x * x - y * y - z * z) / n2, 2.f * (x * y - w * z) / n2, 2.f * (w * y + x * z) / n2,
                            2.f * (w * z + x * y) / n2, (w * w - x * x + y * y - z * z) / n2, 2.f * (y * z - w * x) / n2,
                            2.f * (x * z - w * y) / n2, 2.f * (w * x + y * z) / n2, (w * w - x * x - y * y + z * z) / n2};
        float tmp[9];
        mul3(Lm, R, tmp);
        mul3(tmp, Rm, rel);
        // step 1: neither twist nor splay on the middle and end joints
        if (f % 3 != 0) {
            const float wgt = inv_b / 10.f;
            l_er += (rel[6] * rel[6] + rel[7] * rel[7] + (rel[8] - 1.f) * (rel[8] - 1.f)) * wgt;
            G[6] += 2.f * rel[6] * wgt, G[7] += 2.f * rel[7] * wgt, G[8] += 2.f * (rel[8] - 1.f) * wgt;
        } else {
            // step 2: no twist on the base joints (antisymmetric part about x); the thumb may twist up to 0.5
            const float c = (rel[7] - rel[5]) / 2.f;
            float dc;
            if (f == 12) {
                const float over = fmaxf(c - 0.5f, 0.f);
                l_er += over * over * inv_b;
                dc = 2.f * over * inv_b;
            } else {
                l_er += c * c * (inv_b / 4.f);
                dc = 2.f * c * (inv_b / 4.f);
            }
            G[7] += 0.5f * dc, G[5] -= 0.5f * dc;
        }
        // step 3: bend and splay ranges, in degrees
        bend = atan2f(rel[3], rel[0]) * 180.f / PI_F;
        dth_bend = hinge(bend, BEND_LO[f], BEND_HI[f], inv_b, l_er);
        if (f % 3 == 0) {
            const float splay = atan2f(-rel[6], rel[0]) * 180.f / PI_F;
            const float dth = hinge(splay, SPLAY_LO[f], SPLAY_HI[f], inv_b, l_er);
            const float yy = -rel[6], den = rel[0] * rel[0] + yy * yy;
            G[0] += -dth * yy / den;
            G[6] -= dth * rel[0] / den;
        }
        s_bend[f] = bend;
    }
    __syncthreads();
    if (joint) {
        // step 4: the pinky's middle joint bends with the ring finger's; negative bends count as 0 (and pass no gradient)
        if (f == 10 || f == 7) {
            const float b10 = s_bend[10], b7 = s_bend[7];
            const float p10 = fmaxf(b10, 0.f) / 180.f * PI_F, p7 = fmaxf(b7, 0.f) / 180.f * PI_F;
            const float t = fminf(p10 - p7 * 3.f / 4.f, 0.f);
            if (f == 10) {
                l_er += t * t * inv_b;
                if (b10 > 0.f) dth_bend += 2.f * t * inv_b;
            } else if (b7 > 0.f) {
                dth_bend -= 2.f * t * inv_b * 0.75f;
            }
        }
        const float den = rel[0] * rel[0] + rel[3] * rel[3];
        G[3] += dth_bend * rel[0] / den;
        G[0] -= dth_bend * rel[3] / den;
    }
    if (tid < 16) {
        const float d = n2 - 1.f, wq = inv_b / 16.f;
        float gw = 4.f * d * w * wq, gx = 4.f * d * x * wq, gy = 4.f * d * y * wq, gz = 4.f * d * z * wq;     // on (w, x, +-y, +-z)
        s_qn[tid] = d * d * wq;
        s_er[tid] = l_er;
        if (joint) {
            float tmp[9], dR[9];
            mul3_tn(Lm, G, tmp);
            mul3_nt(tmp, Rm, dR);
            const float R[9] = {(w * w + x * x - y * y - z * z) / n2, 2.f * (x * y - w * z) / n2, 2.f * (w * y + x * z) / n2,
                                2.f * (w * z + x * y) / n2, (w * w - x * x + y * y - z * z) / n2, 2.f * (y * z - w * x) / n2,
                                2.f * (x * z - w * y) / n2, 2.f * (w * x + y * z) / n2, (w * w - x * x - y * y + z * z) / n2};
            float S = 0.f;
#pragma unroll
            for (int i = 0; i < 9; ++i) S += dR[i] * R[i];
            const float tr = dR[0] + dR[4] + dR[8];
            const float a21 = dR[7] - dR[5], a02 = dR[2] - dR[6], a10 = dR[3] - dR[1];
            const float s01 = dR[1] + dR[3], s02 = dR[2] + dR[6], s12 = dR[5] + dR[7];
            gw += 2.f * ((w * tr + x * a21 + y * a02 + z * a10) - w * S) / n2;
            gx += 2.f * ((x * (dR[0] - dR[4] - dR[8]) + y * s01 + z * s02 + w * a21) - x * S) / n2;
            gy += 2.f * ((y * (dR[4] - dR[0] - dR[8]) + x * s01 + w * a02 + z * s12) - y * S) / n2;
            gz += 2.f * ((z * (dR[8] - dR[0] - dR[4]) + w * a10 + x * s02 + y * s12) - z * S) / n2;
        }
        float* g = p.g_q[hand] + ((size_t)b * 16 + tid) * 4;
        g[0] = gw, g[1] = gx;
        g[2] = hand == 1 ? -gy : gy, g[3] = hand == 1 ? -gz : gz;
    }

    // ---------------------------------------------------------------- edges
    const float* vb = p.verts[hand] + (size_t)b * p.V * 3;
    const float* sl = p.static_len + (size_t)hand * p.E;
    const float inv_be = 1.f / ((float)p.B * (float)p.E);
    float acc_e = 0.f;
    for (int e = tid; e < p.E; e += TPB) {
        const int a = p.edges[2 * e], c = p.edges[2 * e + 1];
        const float dx = vb[a * 3] - vb[c * 3], dy = vb[a * 3 + 1] - vb[c * 3 + 1], dz = vb[a * 3 + 2] - vb[c * 3 + 2];
        const float diff = sqrtf(dx * dx + dy * dy + dz * dz) - sl[e];
        acc_e += diff * diff;
    }
    float* gv = p.g_verts[hand] + (size_t)b * p.V * 3;
    for (int v = tid; v < p.V; v += TPB) {
        const float vx = vb[v * 3], vy = vb[v * 3 + 1], vz = vb[v * 3 + 2];
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int k = p.vptr[v]; k < p.vptr[v + 1]; ++k) {
            const int ent = p.vlist[k], e = ent >> 1, o = p.edges[2 * e + 1 - (ent & 1)];
            const float dx = vx - vb[o * 3], dy = vy - vb[o * 3 + 1], dz = vz - vb[o * 3 + 2];
            const float len = sqrtf(dx * dx + dy * dy + dz * dz);
            const float coef = len > 0.f ? 2.f * (len - sl[e]) * inv_be / len : 0.f;
            gx += coef * dx, gy += coef * dy, gz += coef * dz;
        }
        gv[v * 3] = gx, gv[v * 3 + 1] = gy, gv[v * 3 + 2] = gz;
    }

    // ---------------------------------------------------------------- contact
    const float* am = p.anchors[0] + (size_t)b * p.A * 3;
    const float* as = p.anchors[1] + (size_t)b * p.A * 3;
    const int32_t* ids = p.anchor_id + (size_t)b * p.A * p.D;
    const float* el = p.elastic + (size_t)b * p.A * p.D;
    const float scale_g = 2.f * p.lambda_contact * p.inv_mask;
    float* ga = p.g_anchors[hand] + (size_t)b * p.A * 3;
    float acc_c = 0.f;
    for (int i = tid; i < p.A; i += TPB) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (p.inv_mask != 0.f) {
            if (hand == 1) {
                for (int d = 0; d < p.D; ++d) {
                    const int m = ids[i * p.D + d];
                    const float k = el[i * p.D + d];
                    const float dx = as[i * 3] - am[m * 3], dy = as[i * 3 + 1] - am[m * 3 + 1], dz = as[i * 3 + 2] - am[m * 3 + 2];
                    acc_c += k * (dx * dx + dy * dy + dz * dz);
                    gx += k * dx, gy += k * dy, gz += k * dz;
                }
            } else {
                const int32_t* cp = p.cptr + (size_t)b * (p.A + 1);
                const int32_t* cl = p.clist + (size_t)b * p.A * p.D;
                for (int k = cp[i]; k < cp[i + 1]; ++k) {
                    const int ent = cl[k], s = ent / p.D;
                    const float kk = el[ent];
                    gx += kk * (am[i * 3] - as[s * 3]), gy += kk * (am[i * 3 + 1] - as[s * 3 + 1]), gz += kk * (am[i * 3 + 2] - as[s * 3 + 2]);
                }
            }
        }
        ga[i * 3] = scale_g * gx, ga[i * 3 + 1] = scale_g * gy, ga[i * 3 + 2] = scale_g * gz;
    }

    const float sum_e = block_sum(acc_e, s_red);
    const float sum_c = block_sum(acc_c, s_red);              // s_qn / s_er are visible after these barriers
    if (tid == 0) {
        float qn = 0.f, er = 0.f;
        for (int i = 0; i < 16; ++i) qn += s_qn[i], er += s_er[i];
        float* out = p.partial + ((size_t)b * 2 + hand) * 4;
        out[0] = qn, out[1] = sum_e * inv_be, out[2] = er, out[3] = sum_c * p.inv_mask;
    }
}

__global__ __launch_bounds__(64) void pose_prior_reduce_kernel(const float* __restrict__ partial, float lambda_contact,
                                                               float* __restrict__ terms, float* __restrict__ loss, int B) {
    __shared__ float s_t[8];
    const int t = threadIdx.x;
    if (t < 7) {
        // terms: norm r, norm l, edge r, edge l, contact, ergonomics r, ergonomics l -> (hand, slot) of the partials
        const int hand = (t == 4) ? 1 : (t > 4 ? t - 5 : (t & 1));
        const int slot = (t == 4) ? 3 : (t > 4 ? 2 : (t >> 1));
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += partial[((size_t)b * 2 + hand) * 4 + slot];
        s_t[t] = acc;
        terms[t] = acc;
    }
    __syncthreads();
    if (t == 0) loss[0] = ((((s_t[0] + s_t[1]) + s_t[2]) + s_t[3]) + lambda_contact * s_t[4]) + s_t[5] + s_t[6];
}

__global__ __launch_bounds__(TPB) void pose_prior_bwd_kernel(const float* __restrict__ grads, const float* __restrict__ g,
                                                             float* __restrict__ out, long long n) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i < n) out[i] = grads[i] * g[0];
}

}  // namespace

extern "C" int rih_pose_prior_fwd(const float* q_r, const float* q_l, const float* verts_r, const float* verts_l,
                                  const float* anchors_r, const float* anchors_l, const float* joint_tables,
                                  const int32_t* edges, const float* static_len, const int32_t* vptr, const int32_t* vlist,
                                  const int32_t* anchor_id, const float* elastic, const int32_t* cptr, const int32_t* clist,
                                  float inv_mask_sum, float lambda_contact, float* grads, float* partial, int B, int V, int E,
                                  int A, int D, void* stream) {
    if (!q_r || !q_l || !verts_r || !verts_l || !anchors_r || !anchors_l || !joint_tables || !edges || !static_len || !vptr ||
        !vlist || !anchor_id || !elastic || !cptr || !clist || !grads || !partial)
        return RIH_EINVAL;
    if (B < 1 || B > 65535 || V < 1 || E < 1 || A < 1 || D < 1 || !(inv_mask_sum >= 0.f)) return RIH_EINVAL;
    if ((long long)V * 3 > 0x7fffffffLL || (long long)A * D > 0x7fffffffLL) return RIH_EINVAL;
    PriorArgs p;
    p.q[0] = q_r, p.q[1] = q_l, p.verts[0] = verts_r, p.verts[1] = verts_l, p.anchors[0] = anchors_r, p.anchors[1] = anchors_l;
    p.tables = joint_tables, p.edges = edges, p.static_len = static_len, p.vptr = vptr, p.vlist = vlist;
    p.anchor_id = anchor_id, p.elastic = elastic, p.cptr = cptr, p.clist = clist;
    p.inv_mask = inv_mask_sum, p.lambda_contact = lambda_contact;
    float* g = grads;                                     // q_r, q_l, verts_r, verts_l, anchors_r, anchors_l, back to back
    p.g_q[0] = g, g += (size_t)B * 64;
    p.g_q[1] = g, g += (size_t)B * 64;
    p.g_verts[0] = g, g += (size_t)B * V * 3;
    p.g_verts[1] = g, g += (size_t)B * V * 3;
    p.g_anchors[0] = g, g += (size_t)B * A * 3;
    p.g_anchors[1] = g;
    p.partial = partial;
    p.B = B, p.V = V, p.E = E, p.A = A, p.D = D;
    hipLaunchKernelGGL(pose_prior_fwd_kernel, dim3(2, (unsigned)B), dim3(TPB), 0, (hipStream_t)stream, p);
    return (int)hipGetLastError();
}

extern "C" int rih_pose_prior_reduce(const float* partial, float lambda_contact, float* terms, float* loss, int B,
                                     void* stream) {
    if (!partial || !terms || !loss || B < 1) return RIH_EINVAL;
    hipLaunchKernelGGL(pose_prior_reduce_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partial, lambda_contact, terms,
                       loss, B);
    return (int)hipGetLastError();
}

extern "C" int rih_pose_prior_bwd(const float* grads, const float* grad_out, float* out, int64_t n, void* stream) {
    if (!grads || !grad_out || !out || n < 1) return RIH_EINVAL;
    const long long blocks = ((long long)n + TPB - 1) / TPB;
    if (blocks > 0x7fffffffLL) return RIH_EINVAL;
    hipLaunchKernelGGL(pose_prior_bwd_kernel, dim3((unsigned)blocks), dim3(TPB), 0, (hipStream_t)stream, grads, grad_out, out,
                       (long long)n);
    return (int)hipGetLastError();
}
