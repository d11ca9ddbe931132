// rih_contact.hip -- the contact search of the pose optimiser's driver (pose_data_optimize/batch_optimize_mocap_origin.py:
// `search_anchors` :62-130 with the anchors and face normals that `update_scene` :260-270 hands it) for gfx950: from the two
// hands' translated vertices to the contact tables of `set_opt_val`, one launch for a batch of frames, nothing differentiable.
//
// One workgroup per frame.  Phase 1: every (hand, anchor) pair -- anchor = w1 (v1 - v0) + w2 (v2 - v0) + v0, the expression of
// rih_anchor_fwd (which the compiler may contract differently there: equal to a rounding, not bit for bit), normal =
// cross(v1 - v0, v2 - v0) normalised, the sub hand's negated -- goes to LDS: 12 A floats of a static array that is sized for 128
// anchors (6 KB; the optimiser's table has 108) or, above that, for 1024 (48 KB).  Phase 2: a thread owns one sub anchor i and
// scans the main anchors j = 0 .. A-1 from LDS (every lane reads the same j: a broadcast, no bank conflict), keeping the D
// smallest (distance, j) in registers.
//   fresh   (prev_id == NULL): a pair with n_sub_i . n_main_j > against_cos counts as distance 1000; anchor_id[i] = the D
//           smallest, equal distances in ascending j (the list is filled in ascending j and an entry moves only for a strictly
//           smaller distance); vertex_contact[i] = any distance < radius.
//   refresh (prev_id given): anchor_id = prev_id, the TRUE distance to every previous id, no against rule; an id outside
//           [0, A) is copied through with elastic 0 and mask 0 and is never dereferenced.
//   both:   elastic = (dis < radius) cos^2(pi dis / (2 radius)) -- the reference's 0.5 cos(pi dis / radius) + 0.5, which in fp32
//           rounds to 0 just inside the radius, while the square of a positive cosine stays positive --, mask = elastic > 0, then
//           elastic *= damp where neither anchor's class is tip_class.
// Plain vector stores, no atomics, a fixed order: two runs are bit-identical.  Latency-class (A = 108: 216 phase-1 items,
// 108 x 108 distances per frame); what it removes is the driver's per-frame host loop and its copies.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"

namespace {

constexpr int CS_TPB = 128, CS_SMALL_A = 128, CS_MAX_A = 1024, CS_MAX_D = 8;
constexpr float CS_AGAINST_DIS = 1000.f;

__device__ inline float cs_elastic(float dis, float radius) {
    if (!(dis < radius)) return 0.f;
    const float c = cosf(1.57079632679489662f * dis / radius);
    return c * c;
}

template <int MAXA>
__global__ __launch_bounds__(CS_TPB) void contact_search_kernel(
    const float* __restrict__ verts_main, const float* __restrict__ verts_sub, const int32_t* __restrict__ fvi,
    const float* __restrict__ w, const int32_t* __restrict__ cls, const int64_t* __restrict__ prev_id, float radius,
    float against_cos, float damp, int tip_class, int64_t* __restrict__ anchor_id, float* __restrict__ elastic,
    int64_t* __restrict__ mask, int64_t* __restrict__ vertex_contact, int V, int A, int D) {
    // [0, 3A) main anchors, [3A, 6A) main normals, [6A, 9A) sub anchors, [9A, 12A) sub normals (negated)
    __shared__ float lds[12 * MAXA];
    const long long b = blockIdx.x;
    for (int t = threadIdx.x; t < 2 * A; t += CS_TPB) {
        const int hand = t >= A, a = t - hand * A;
        const float* vb = (hand ? verts_sub : verts_main) + b * V * 3;
        const float *p0 = vb + (long long)fvi[a * 3] * 3, *p1 = vb + (long long)fvi[a * 3 + 1] * 3,
                    *p2 = vb + (long long)fvi[a * 3 + 2] * 3;
        float e1[3], e2[3];
        float* pos = lds + hand * 6 * A + a * 3;
        for (int c = 0; c < 3; ++c) {
            e1[c] = p1[c] - p0[c];
            e2[c] = p2[c] - p0[c];
            pos[c] = (w[a * 2] * e1[c] + w[a * 2 + 1] * e2[c]) + p0[c];
        }
        const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        const float inv = (hand ? -1.f : 1.f) / sqrtf(nx * nx + ny * ny + nz * nz);
        pos[3 * A] = nx * inv;
        pos[3 * A + 1] = ny * inv;
        pos[3 * A + 2] = nz * inv;
    }
    __syncthreads();
    const float *mp = lds, *mn = lds + 3 * A, *sp = lds + 6 * A, *sn = lds + 9 * A;
    for (int i = threadIdx.x; i < A; i += CS_TPB) {
        const float sx = sp[i * 3], sy = sp[i * 3 + 1], sz = sp[i * 3 + 2];
        const long long row = (b * A + i) * D;
        const bool i_tip = cls[i] == tip_class;
        bool any = false;
        if (prev_id) {
            for (int d = 0; d < D; ++d) {
                const int64_t id = prev_id[row + d];
                float e = 0.f;
                if (id >= 0 && id < A) {
                    const float dx = sx - mp[id * 3], dy = sy - mp[id * 3 + 1], dz = sz - mp[id * 3 + 2];
                    const float dis = sqrtf(dx * dx + dy * dy + dz * dz);
                    any = any || dis < radius;
                    e = cs_elastic(dis, radius);
                }
                const bool m = e > 0.f;
                if (m && !i_tip && cls[id] != tip_class) e *= damp;
                anchor_id[row + d] = id;
                elastic[row + d] = e;
                mask[row + d] = m;
            }
        } else {
            const float ax = sn[i * 3], ay = sn[i * 3 + 1], az = sn[i * 3 + 2];
            float kd[CS_MAX_D];
            int kj[CS_MAX_D];
#pragma unroll
            for (int k = 0; k < CS_MAX_D; ++k) {
                kd[k] = INFINITY;
                kj[k] = 0;
            }
            for (int j = 0; j < A; ++j) {
                const float dx = sx - mp[j * 3], dy = sy - mp[j * 3 + 1], dz = sz - mp[j * 3 + 2];
                const float dot = ax * mn[j * 3] + ay * mn[j * 3 + 1] + az * mn[j * 3 + 2];
                float cd = dot > against_cos ? CS_AGAINST_DIS : sqrtf(dx * dx + dy * dy + dz * dz);
                int cj = j;
                any = any || cd < radius;
                bool moving = false;               // once the candidate has taken a slot, the displaced entries shift down
#pragma unroll
                for (int k = 0; k < CS_MAX_D; ++k) {
                    moving = moving || cd < kd[k];
                    if (k < D && moving) {
                        const float td = kd[k];
                        const int tj = kj[k];
                        kd[k] = cd;
                        kj[k] = cj;
                        cd = td;
                        cj = tj;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < CS_MAX_D; ++k) {
                if (k < D) {
                    float e = cs_elastic(kd[k], radius);
                    const bool m = e > 0.f;
                    if (m && !i_tip && cls[kj[k]] != tip_class) e *= damp;
                    anchor_id[row + k] = kj[k];
                    elastic[row + k] = e;
                    mask[row + k] = m;
                }
            }
        }
        vertex_contact[b * A + i] = any;
    }
}

}  // namespace

extern "C" int rih_contact_search(const float* verts_main, const float* verts_sub, const int32_t* face_vert_idx,
                                  const float* weight, const int32_t* class_type, const int64_t* prev_id, float radius,
                                  float against_cos, float damp, int tip_class, int64_t* anchor_id, float* elastic,
                                  int64_t* mask, int64_t* vertex_contact, int B, int V, int A, int D, void* stream) {
    if (!verts_main || !verts_sub || !face_vert_idx || !weight || !class_type || !anchor_id || !elastic || !mask ||
        !vertex_contact)
        return RIH_EINVAL;
    if (B < 1 || V < 1 || A < 1 || D < 1 || A > CS_MAX_A || D > CS_MAX_D || D > A || !(radius > 0.f)) return RIH_EINVAL;
    if (A <= CS_SMALL_A)
        hipLaunchKernelGGL(contact_search_kernel<CS_SMALL_A>, dim3((unsigned)B), dim3(CS_TPB), 0, (hipStream_t)stream, verts_main,
                           verts_sub, face_vert_idx, weight, class_type, prev_id, radius, against_cos, damp, tip_class, anchor_id,
                           elastic, mask, vertex_contact, V, A, D);
    else
        hipLaunchKernelGGL(contact_search_kernel<CS_MAX_A>, dim3((unsigned)B), dim3(CS_TPB), 0, (hipStream_t)stream, verts_main,
                           verts_sub, face_vert_idx, weight, class_type, prev_id, radius, against_cos, damp, tip_class, anchor_id,
                           elastic, mask, vertex_contact, V, A, D);
    return (int)hipGetLastError();
}
