// rih_pose_convert.hip -- the pose-data stages around the two-hand pose optimiser for gfx950: the reference's
// scripts/HandPoseConverter.py (annotation <-> MANO quaternion <-> "mocap" Euler degrees), scripts/HandPoseArguer.py and
// Ver2Code/NatureJudge/PoseArgue.py (`argue_pose`: random bend / splay variants inside per-joint limits) and
// Ver2Code/ValidJudge/ValidJudger.py (`ValidationJudge`: how far a frame's joints leave the anatomical ranges), which there are
// numpy / scipy `Rotation` objects in fp64 inside Python loops over frames.  renderih_amd/pose_convert.py holds the mirror
// and the surface; conventions in full: DESIGN.md 3.18.
//
// ONE kernel body, pc_kernel<IN, MID, OUT>, one thread per (sample, joint): the 16 joints of a sample are 16 consecutive
// lanes, a wavefront holds 4 samples, and because the block size and the grid stride are multiples of 16 a thread keeps ITS
// joint for the whole grid-stride loop -- its row of the constant table (the converter's two 3 x 3 axis tables, the zero
// frame, hands_mean, the limits: 41 floats) is read once, with ordinary vector loads (the address depends on lane % 16, so it
// is not wave-uniform and a scalar load does not apply; the 2.6 KB table stays in cache), and stays in registers.
//   IN   0 axis-angle (+ hands_mean on the finger joints)   1 Euler degrees   2 quaternion (w, x, y, z)
//   MID  0 nothing   1 augmentation, draws from rih_hash(seed, ((m * 16 + j) * 2 + which))   2 augmentation, draws from
//        uniforms[M][16][2]
//   OUT  0 Euler degrees   1 quaternion   2 axis-angle (- hands_mean)   3 validity residual (one float per sample and hand)
// Every conversion meets in one of two middle forms: the MANO quaternion Q (left hand: after its y, z sign flip) or the
// rotation E in the converter's finger frame, E = invM_U_n_0^T R(Q) invU_M_n_1^T (left root: diag(1,-1,-1) R first).
// Euler angles are scipy's lower-case 'xyz': E = Rz(c) Ry(b) Rx(a).  Back: c = atan2(E10, E00); b = atan2(-E20, |(E00, E10)|),
// which is -asin(E20) without its loss of digits next to +-90 degrees; a = atan2(s E02 - k E12, k E11 - s E01) with (k, s) =
// (cos c, sin c) = (E00, E10) / |(E00, E10)|, which is atan2(E21, E22) for an exact rotation and stays a rotation that
// reproduces E when cos b goes to 0; at lock ((E00, E10) = 0 in working precision) c = 0, k = 1, s = 0.
// The validity residual is a maximum over the 16 lanes of a sample (four __shfl_xor steps of 8, 4, 2, 1: they never leave the
// aligned group of 16).  Every lane of a block makes the same number of loop trips and takes part in every shuffle; a lane
// past the end loads and stores nothing and contributes 0.  Stores are plain vector stores; nothing is atomic; no LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"
#include "rih_hash.h"

namespace {

constexpr int PC_TPB = 256;
constexpr float PC_DEG = 57.29577951308232f, PC_RAD = 0.017453292519943295f;
// a joint's row of the table (RIH_POSE_TAB floats): see include/renderih_amd.h
enum { PC_T0 = 0, PC_T1 = 9, PC_ZERO = 18, PC_MEAN = 27, PC_BEND = 30, PC_SPLAY = 33, PC_VBEND = 36, PC_VSPLAY = 38, PC_SIGN = 40 };

__device__ inline void pc_mul(const float* a, const float* b, float* c) {                 // c = a b
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__device__ inline void pc_mul_tn(const float* a, const float* b, float* c) {              // c = a^T b
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[i] * b[j] + a[3 + i] * b[3 + j] + a[6 + i] * b[6 + j];
}
__device__ inline void pc_mul_nt(const float* a, const float* b, float* c) {              // c = a b^T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1] + a[3 * i + 2] * b[3 * j + 2];
}

// rotation vector -> unit quaternion with w >= 0 (scipy from_rotvec: the series below 1e-3)
__device__ inline void pc_rotvec_to_quat(const float* v, float* q) {
    const float n2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], n = sqrtf(n2);
    float s, c;
    sincosf(0.5f * n, &s, &c);
    const float k = n <= 1e-3f ? 0.5f - n2 * (1.f / 48.f) + n2 * n2 * (1.f / 3840.f) : s / n;
    const float sg = c < 0.f ? -1.f : 1.f;
    q[0] = sg * c, q[1] = sg * k * v[0], q[2] = sg * k * v[1], q[3] = sg * k * v[2];
}
// quaternion (any norm > 0) -> rotation vector with angle in [0, pi] (scipy as_rotvec: the series below 1e-3)
__device__ inline void pc_quat_to_rotvec(const float* q, float* v) {
    const float inv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float sg = q[0] < 0.f ? -inv : inv;
    const float w = q[0] * sg, x = q[1] * sg, y = q[2] * sg, z = q[3] * sg;
    const float n = sqrtf(x * x + y * y + z * z), angle = 2.f * atan2f(n, w), a2 = angle * angle;
    const float k = angle <= 1e-3f ? 2.f + a2 * (1.f / 12.f) + a2 * a2 * (7.f / 2880.f) : angle / n;
    v[0] = k * x, v[1] = k * y, v[2] = k * z;
}
// quaternion (any norm > 0) -> rotation matrix: the quadratic form over |q|^2, as manopth's quaternion_to_rotation_matrix
__device__ inline void pc_quat_to_mat(const float* q, float* R) {
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    const float inv = 1.f / (w * w + x * x + y * y + z * z);
    R[0] = (w * w + x * x - y * y - z * z) * inv, R[1] = 2.f * (x * y - w * z) * inv, R[2] = 2.f * (w * y + x * z) * inv;
    R[3] = 2.f * (w * z + x * y) * inv, R[4] = (w * w - x * x + y * y - z * z) * inv, R[5] = 2.f * (y * z - w * x) * inv;
    R[6] = 2.f * (x * z - w * y) * inv, R[7] = 2.f * (w * x + y * z) * inv, R[8] = (w * w - x * x - y * y + z * z) * inv;
}
// rotation matrix -> unit quaternion with w >= 0: the largest of (trace, R00, R11, R22) picks the component taken from a root
__device__ inline void pc_mat_to_quat(const float* R, float* q) {
    const float tr = R[0] + R[4] + R[8];
    float w, x, y, z;
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        w = 1.f + tr, x = R[7] - R[5], y = R[2] - R[6], z = R[3] - R[1];
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        w = R[7] - R[5], x = 1.f + R[0] - R[4] - R[8], y = R[1] + R[3], z = R[2] + R[6];
    } else if (R[4] >= R[8]) {
        w = R[2] - R[6], x = R[1] + R[3], y = 1.f - R[0] + R[4] - R[8], z = R[5] + R[7];
    } else {
        w = R[3] - R[1], x = R[2] + R[6], y = R[5] + R[7], z = 1.f - R[0] - R[4] + R[8];
    }
    const float inv = 1.f / sqrtf(w * w + x * x + y * y + z * z);
    const float sg = w < 0.f ? -inv : inv;
    q[0] = w * sg, q[1] = x * sg, q[2] = y * sg, q[3] = z * sg;
}
// The axis tables are fp32, orthogonal to 1e-7 only, and so is a product with them; scipy's Rotation.from_matrix replaces such a
// matrix by the nearest rotation.  One Newton step of the polar decomposition, (E + E^-T) / 2, leaves the square of that distance.
__device__ inline void pc_polar(float* E) {
    const float C[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                        E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                        E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
    const float inv = 0.5f / (E[0] * C[0] + E[1] * C[1] + E[2] * C[2]);
    for (int k = 0; k < 9; ++k) E[k] = 0.5f * E[k] + C[k] * inv;
}
// Euler degrees (a, b, c) -> E = Rz(c) Ry(b) Rx(a)
__device__ inline void pc_euler_to_mat(const float* e, float* E) {
    float sa, ca, sb, cb, sc, cc;
    sincosf(e[0] * PC_RAD, &sa, &ca);
    sincosf(e[1] * PC_RAD, &sb, &cb);
    sincosf(e[2] * PC_RAD, &sc, &cc);
    E[0] = cc * cb, E[1] = cc * sb * sa - sc * ca, E[2] = cc * sb * ca + sc * sa;
    E[3] = sc * cb, E[4] = sc * sb * sa + cc * ca, E[5] = sc * sb * ca - cc * sa;
    E[6] = -sb, E[7] = cb * sa, E[8] = cb * ca;
}
// E -> Euler degrees; see the head of the file
__device__ inline void pc_mat_to_euler(const float* E, float* e) {
    const float h = sqrtf(E[0] * E[0] + E[3] * E[3]);
    const bool lock = h < 9.5367431640625e-07f;                        // 8 eps, as the mirror's
    const float k = lock ? 1.f : E[0] / h, s = lock ? 0.f : E[3] / h;
    e[0] = atan2f(s * E[2] - k * E[5], k * E[4] - s * E[1]) * PC_DEG;
    e[1] = atan2f(-E[6], h) * PC_DEG;
    e[2] = lock ? 0.f : atan2f(E[3], E[0]) * PC_DEG;
}
// the adjustment of `angle_random_adjust`: uniform in [neg, pos], both clamped by the limits and by +-cap
__device__ inline float pc_delta(float angle, float lo, float hi, float cap, float u) {
    const float pos = fmaxf(fminf(cap, hi - angle), 0.f), neg = fminf(fmaxf(-cap, lo - angle), 0.f);
    return fmaf(pos - neg, u, neg);
}
__device__ inline float pc_excess(float angle, float lo, float hi) {
    return fmaxf(fmaxf(angle - hi, 0.f), fmaxf(lo - angle, 0.f)) / 180.f * 3.14159265358979323846f;
}

template <int IN, int MID, int OUT>
__global__ __launch_bounds__(PC_TPB) void pc_kernel(const float* __restrict__ in0, const float* __restrict__ in1,
                                                    float* __restrict__ out, const float* __restrict__ tables,
                                                    const float* __restrict__ uniforms, uint64_t seed, long long M, int A,
                                                    long long row0) {
    constexpr bool NEED_E = OUT == 0 || OUT == 3 || MID != 0;          // the finger-frame rotation is formed
    constexpr bool NEED_Q = OUT == 1 || OUT == 2;                      // the MANO quaternion is formed
    constexpr bool CROSS = (IN == 1) ? NEED_Q : NEED_E;                // ... from the other form, through the axis tables
    constexpr int WIN = IN == 2 ? 4 : 3, WOUT = OUT == 1 ? 4 : 3;
    const int tid = threadIdx.x, j = tid & 15, hand = blockIdx.y;
    const float* __restrict__ in = hand ? in1 : in0;
    const float* __restrict__ row = tables + ((long long)hand * 16 + j) * RIH_POSE_TAB;
    float t0[9], t1[9], zero[9], mean[3], lim[10];
    for (int k = 0; k < 9; ++k) {
        t0[k] = CROSS ? row[PC_T0 + k] : 0.f;
        t1[k] = CROSS ? row[PC_T1 + k] : 0.f;
        zero[k] = OUT == 3 ? row[PC_ZERO + k] : 0.f;
    }
    for (int k = 0; k < 3; ++k) mean[k] = (IN == 0 || OUT == 2) ? row[PC_MEAN + k] : 0.f;
    for (int k = 0; k < 10; ++k) lim[k] = (MID != 0 || OUT == 3) ? row[PC_BEND + k] : 0.f;
    const float sign = row[PC_SIGN];                                   // +1 right hand, -1 left hand
    const float flip = j == 0 ? sign : 1.f;                            // the left ROOT's diag(1, -1, -1)
    const uint64_t key = MID == 1 ? rih_seed_key(seed) : 0;
    const long long total = M * 16, stride = (long long)gridDim.x * PC_TPB;
    for (long long base = (long long)blockIdx.x * PC_TPB; base < total; base += stride) {
        const long long t = base + tid, m = t >> 4;
        const bool active = t < total;
        float x[4] = {IN == 2 ? 1.f : 0.f, 0.f, 0.f, 0.f};             // a lane past the end works on the identity
        if (active) {
            const long long n = MID == 0 ? m : (long long)((unsigned)m / (unsigned)A);      // M < 2^27: a 32-bit division
            const float* p = in + (n * 16 + j) * WIN;
            if (IN == 2) {
                const float4 v = *reinterpret_cast<const float4*>(p);
                x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
            } else {
                x[0] = p[0], x[1] = p[1], x[2] = p[2];
            }
        }
        float Q[4], E[9], euler[3];
        if (IN == 0) {
            const float v[3] = {x[0] + mean[0], x[1] + mean[1], x[2] + mean[2]};
            pc_rotvec_to_quat(v, Q);                                   // the left hand's y, z flip and its inverse below cancel
        } else if (IN == 2) {
            Q[0] = x[0], Q[1] = x[1], Q[2] = x[2] * sign, Q[3] = x[3] * sign;
        } else {
            euler[0] = x[0], euler[1] = x[1], euler[2] = x[2];
            pc_euler_to_mat(euler, E);
        }
        if (IN != 1 && NEED_E) {                                       // E = t0^T (D R(Q)) t1^T
            float R[9], T[9];
            pc_quat_to_mat(Q, R);
            for (int k = 3; k < 9; ++k) R[k] *= flip;
            pc_mul_tn(t0, R, T);
            pc_mul_nt(T, t1, E);
            if (OUT != 3) pc_polar(E);                                 // scipy's from_matrix; the judge takes the product as it is
            if (MID != 0) pc_mat_to_euler(E, euler);
        }
        if (MID != 0) {                                                // E' = E Rz(d_bend) Ry(d_splay), from the ORIGINAL angles
            float ub, us;
            if (MID == 1) {
                const uint64_t idx = (uint64_t)(((row0 + m) * 16 + j) * 2);
                ub = (float)(rih_hash_k64(key, idx) >> 8) * (1.f / 16777216.f);
                us = (float)(rih_hash_k64(key, idx + 1) >> 8) * (1.f / 16777216.f);
            } else {
                ub = active ? uniforms[t * 2] : 0.f;
                us = active ? uniforms[t * 2 + 1] : 0.f;
            }
            const float db = pc_delta(euler[2], lim[0], lim[1], lim[2], ub);
            const float ds = pc_delta(euler[1], lim[3], lim[4], lim[5], us);
            float sz, cz, sy, cy;
            sincosf(db * PC_RAD, &sz, &cz);
            sincosf(ds * PC_RAD, &sy, &cy);
            for (int r = 0; r < 3; ++r) {
                const float c0 = E[3 * r] * cz + E[3 * r + 1] * sz, c1 = E[3 * r + 1] * cz - E[3 * r] * sz, c2 = E[3 * r + 2];
                E[3 * r] = c0 * cy - c2 * sy, E[3 * r + 1] = c1, E[3 * r + 2] = c0 * sy + c2 * cy;
            }
        }
        if (NEED_Q && (IN == 1 || MID != 0)) {                         // Q = quat(D t0 E t1)
            float R[9], T[9];
            pc_mul(t0, E, T);
            pc_mul(T, t1, R);
            pc_polar(R);
            for (int k = 3; k < 9; ++k) R[k] *= flip;
            pc_mat_to_quat(R, Q);
        }
        float* o = out + t * WOUT;                                     // OUT == 3 (the only two-hand form) does not use it
        if (OUT == 0) {
            pc_mat_to_euler(E, euler);
            if (active) o[0] = euler[0], o[1] = euler[1], o[2] = euler[2];
        } else if (OUT == 1) {
            const float n = IN == 2 && MID == 0 ? 1.f / sqrtf(Q[0] * Q[0] + Q[1] * Q[1] + Q[2] * Q[2] + Q[3] * Q[3]) : 1.f;
            const float sg = Q[0] < 0.f ? -n : n;
            if (active) *reinterpret_cast<float4*>(o) = make_float4(Q[0] * sg, Q[1] * sg, Q[2] * sg * sign, Q[3] * sg * sign);
        } else if (OUT == 2) {
            float v[3];
            pc_quat_to_rotvec(Q, v);
            if (active) o[0] = v[0] - mean[0], o[1] = v[1] - mean[1], o[2] = v[2] - mean[2];
        } else {
            // first column of zero^T E; bend and splay in degrees; the root (j = 0) has no limits: lim = -+inf there
            float c[3];
            for (int i = 0; i < 3; ++i) c[i] = zero[i] * E[0] + zero[3 + i] * E[3] + zero[6 + i] * E[6];
            const float bend = atan2f(c[1], c[0]) * PC_DEG, splay = atan2f(-c[2], c[0]) * PC_DEG;
            float worst = active ? fmaxf(pc_excess(bend, lim[6], lim[7]), pc_excess(splay, lim[8], lim[9])) : 0.f;
            for (int s = 8; s > 0; s >>= 1) worst = fmaxf(worst, __shfl_xor(worst, s));
            if (active && j == 0) out[m * gridDim.y + hand] = worst;
        }
    }
}

template <int IN, int MID>
int pc_launch_out(int out_fmt, dim3 grid, hipStream_t st, const float* in0, const float* in1, float* out, const float* tables,
                  const float* uniforms, uint64_t seed, long long M, int A, long long row0) {
#define PC_GO(OUT)                                                                                                       \
    hipLaunchKernelGGL((pc_kernel<IN, MID, OUT>), grid, dim3(PC_TPB), 0, st, in0, in1, out, tables, uniforms, seed, M, A, \
                       row0);                                                                                            \
    return (int)hipGetLastError()
    switch (out_fmt) {
        case 0: PC_GO(0);
        case 1: PC_GO(1);
        case 2: PC_GO(2);
        case 3: PC_GO(3);
    }
#undef PC_GO
    return RIH_EINVAL;
}

template <int IN, typename... Args> int pc_launch_mid(int mid, Args... args) {
    switch (mid) {
        case 0: return pc_launch_out<IN, 0>(args...);
        case 1: return pc_launch_out<IN, 1>(args...);
        case 2: return pc_launch_out<IN, 2>(args...);
    }
    return RIH_EINVAL;
}

}  // namespace

extern "C" int rih_pose_convert(const float* in, const float* in_second, float* out, const float* tables, const float* uniforms,
                                uint64_t seed, int64_t row0, int64_t M, int A, int in_fmt, int mid, int out_fmt, void* stream) {
    if (!in || !out || !tables || M < 1 || A < 1 || row0 < 0) return RIH_EINVAL;
    if (in_fmt < 0 || in_fmt > 2 || mid < 0 || mid > 2 || out_fmt < 0 || out_fmt > 3) return RIH_EINVAL;
    if (mid == 2 && !uniforms) return RIH_EINVAL;
    if (mid == 0 && A != 1) return RIH_EINVAL;
    if (in_second && out_fmt != 3) return RIH_EINVAL;                  // two hands in one launch: the validity residual only
    if (M > (1LL << 27) || row0 > (1LL << 40)) return RIH_EINVAL;
    const long long blocks = (M * 16 + PC_TPB - 1) / PC_TPB;
    const dim3 grid((unsigned)(blocks < 8192 ? blocks : 8192), in_second ? 2 : 1);
    const hipStream_t st = (hipStream_t)stream;
    switch (in_fmt) {
        case 0: return pc_launch_mid<0>(mid, out_fmt, grid, st, in, in_second, out, tables, uniforms, seed, (long long)M, A, (long long)row0);
        case 1: return pc_launch_mid<1>(mid, out_fmt, grid, st, in, in_second, out, tables, uniforms, seed, (long long)M, A, (long long)row0);
        case 2: return pc_launch_mid<2>(mid, out_fmt, grid, st, in, in_second, out, tables, uniforms, seed, (long long)M, A, (long long)row0);
    }
    return RIH_EINVAL;
}
