// rih_joint_fit.hip -- fitting MANO pose and shape to 3-D joints (utils/mano_from_3djoint/: AIK.py `adaptive_IK`, utils.py
// `mat2aa`, convert2mano.py:158-204) for gfx950; renderih_amd.joint_fit drives it, DESIGN 3.16 describes it.
//   rih_aik             the analytic inverse-kinematics initialisation, batched: workgroup = 8 hands x 8 lanes.  Lane 0 of a hand
//                       solves the root rotation (Horn's quaternion form of rih_procrustes.h) and leaves it in LDS, lanes 0..4
//                       walk one finger's three-bone chain each.  Double arithmetic on fp32 inputs.
//   rih_mat2aa_fwd/bwd  thread = matrix: rotation matrix -> quaternion (four masked branches) -> axis-angle, and the gradient
//                       of the selected branch.  A (period, skip) pattern leaves out the first `skip` matrices of every `period`
//                       (the root of a hand's 16), which the forward copies out and the backward takes a gradient for.
//   rih_joint_l1        ONE workgroup, thread = hand: per-hand mean |(j - j0) - target|, its gradient, the row `step` of the loss
//                       history, then the sum over hands as a fixed tree over the 256 partial sums.
//   rih_lr_linear_step  one thread: lr = base * (n_iter - step) / n_iter in double, then step += 1; the only writer of the
//                       optimiser's state block (the place rih_plateau_step has in rih_pose_opt.hip).
//   rih_fit_select      workgroup = hand: keep the parameters of the lowest loss seen so far.
// All of it is latency class (a few thousand values at B <= 32).  fp32 in and out, plain vector stores, no atomics, a fixed
// order of every sum: two runs are bit-identical and hand b of a batch gets the bits it gets alone.  Nothing is read back.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"
#include "rih_procrustes.h"

namespace {

// ------------------------------------------------------------------------------------------------ inverse kinematics
constexpr int AIK_HANDS = RIH_AIK_HANDS_PER_GROUP, AIK_LANES = 8;
// joint order: wrist, then thumb, index, middle, ring, little, four joints each (parent of joint k: k - 1, or 0 for the
// knuckles 1, 5, 9, 13, 17).  Slot of the first bone rotation of each finger in the 16 output matrices (slot 0: the root).
__device__ const int AIK_FINGER_SLOT[5] = {13, 1, 4, 10, 7};

__device__ __forceinline__ void mat3_mul(const double A[9], const double B[9], double C[9]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}

__global__ __launch_bounds__(AIK_HANDS * AIK_LANES) void aik_kernel(const float* __restrict__ tmpl,
                                                                     const float* __restrict__ joints, float* __restrict__ out,
                                                                     int B, int normalize) {
#pragma clang fp contract(off)
    __shared__ double sP[AIK_HANDS][63];         // the hand's target joints after the optional normalisation
    __shared__ double sR0[AIK_HANDS][9];
    const int h = threadIdx.x / AIK_LANES, lane = threadIdx.x % AIK_LANES;
    const long long b = (long long)blockIdx.x * AIK_HANDS + h;
    const bool live = b < B;
    double T[63];
    for (int i = 0; i < 63; ++i) T[i] = (double)tmpl[i];
    if (live && lane == 0) {
        double* P = sP[h];
        const float* src = joints + b * 63;
        for (int i = 0; i < 63; ++i) P[i] = (double)src[i];
        if (normalize) {
            double nt = 0.0, np = 0.0;
            for (int c = 0; c < 3; ++c) {
                nt += (T[27 + c] - T[c]) * (T[27 + c] - T[c]);
                np += (P[27 + c] - P[c]) * (P[27 + c] - P[c]);
            }
            const double ratio = sqrt(nt) / sqrt(np);
            for (int i = 0; i < 63; ++i) P[i] *= ratio;
            const double p0[3] = {P[0], P[1], P[2]};
            for (int i = 0; i < 63; ++i) P[i] = P[i] - p0[i % 3] + T[i % 3];
        }
        // H = sum over the five knuckles of t p^T; the proper rotation maximising tr(R H) takes t onto p
        const double zero[3] = {0.0, 0.0, 0.0};
        double H[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int f = 0; f < 5; ++f) {
            const int k = 1 + 4 * f;
            for (int a = 0; a < 3; ++a)
                for (int c = 0; c < 3; ++c) H[a][c] += (T[k * 3 + a] - T[a]) * (P[k * 3 + c] - P[c]);
        }
        double R[3][3], scale, t[3];
        rih_similarity_from_moments(1, zero, zero, H, 1.0, R, &scale, t);
        for (int i = 0; i < 9; ++i) {
            sR0[h][i] = R[i / 3][i % 3];
            out[b * 144 + i] = (float)R[i / 3][i % 3];
        }
    }
    __syncthreads();
    if (!live || lane >= 5) return;
    const double* P = sP[h];
    const int base = 1 + 4 * lane;
    double Rpa[9], qpa[3];                       // global rotation of the parent bone and the parent joint's fitted position
    for (int i = 0; i < 9; ++i) Rpa[i] = sR0[h][i];
    for (int a = 0; a < 3; ++a) {
        const double d0 = T[base * 3] - T[0], d1 = T[base * 3 + 1] - T[1], d2 = T[base * 3 + 2] - T[2];
        qpa[a] = (Rpa[a * 3] * d0 + Rpa[a * 3 + 1] * d1 + Rpa[a * 3 + 2] * d2) + T[a];
    }
    for (int s = 0; s < 3; ++s) {
        const int k = base + 1 + s, pa = k - 1;
        double dt[3], w[3], dp[3];
        for (int a = 0; a < 3; ++a) {
            dt[a] = T[k * 3 + a] - T[pa * 3 + a];
            w[a] = P[k * 3 + a] - qpa[a];
        }
        for (int a = 0; a < 3; ++a) dp[a] = Rpa[a] * w[0] + Rpa[3 + a] * w[1] + Rpa[6 + a] * w[2];     // R_pa^T w
        double ax[3] = {dt[1] * dp[2] - dt[2] * dp[1], dt[2] * dp[0] - dt[0] * dp[2], dt[0] * dp[1] - dt[1] * dp[0]};
        double D[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (ax[0] != 0.0 || ax[1] != 0.0 || ax[2] != 0.0) {
            const double n1 = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]) + 1e-8;
            for (int a = 0; a < 3; ++a) ax[a] /= n1;
            const double n2 = sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);     // the axis-angle routine's own unit axis
            const double x = ax[0] / n2, y = ax[1] / n2, z = ax[2] / n2;
            const double den = (sqrt(dt[0] * dt[0] + dt[1] * dt[1] + dt[2] * dt[2]) + 1e-8) *
                               (sqrt(dp[0] * dp[0] + dp[1] * dp[1] + dp[2] * dp[2]) + 1e-8);
            double ca = (dt[0] * dp[0] + dt[1] * dp[1] + dt[2] * dp[2]) / den;
            ca = ca > 1.0 ? 1.0 : (ca < -1.0 ? -1.0 : ca);
            const double alpha = acos(ca), c = cos(alpha), sn = sin(alpha), C1 = 1.0 - c;
            D[0] = x * x * C1 + c;      D[1] = x * y * C1 - z * sn; D[2] = z * x * C1 + y * sn;
            D[3] = x * y * C1 + z * sn; D[4] = y * y * C1 + c;      D[5] = y * z * C1 - x * sn;
            D[6] = z * x * C1 - y * sn; D[7] = y * z * C1 + x * sn; D[8] = z * z * C1 + c;
        }
        float* o = out + b * 144 + (AIK_FINGER_SLOT[lane] + s) * 9;
        for (int i = 0; i < 9; ++i) o[i] = (float)D[i];
        if (s < 2) {
            double Rk[9];
            mat3_mul(Rpa, D, Rk);
            for (int a = 0; a < 3; ++a) qpa[a] = (Rk[a * 3] * dt[0] + Rk[a * 3 + 1] * dt[1] + Rk[a * 3 + 2] * dt[2]) + qpa[a];
            for (int i = 0; i < 9; ++i) Rpa[i] = Rk[i];
        }
    }
}

// ------------------------------------------------------------------------------------------------ matrix -> axis-angle
constexpr int M2A_TPB = RIH_MAT2AA_TPB;
constexpr float M2A_EPS = 1e-6f;

struct M2AQuat {
    int branch;           // which of the four numerators was selected
    float n[4], t;        // numerator (w, x, y, z) and the trace term under the square root
    float q[4];
};

__device__ __forceinline__ M2AQuat m2a_quat(const float r[9]) {
    M2AQuat o;
    const bool d2 = r[8] < M2A_EPS, d01 = r[0] > r[4], d0n1 = r[0] < -r[4];
    if (d2 && d01) {
        o.branch = 0; o.t = 1.f + r[0] - r[4] - r[8];
        o.n[0] = r[7] - r[5]; o.n[1] = o.t; o.n[2] = r[3] + r[1]; o.n[3] = r[2] + r[6];
    } else if (d2) {
        o.branch = 1; o.t = 1.f - r[0] + r[4] - r[8];
        o.n[0] = r[2] - r[6]; o.n[1] = r[3] + r[1]; o.n[2] = o.t; o.n[3] = r[7] + r[5];
    } else if (d0n1) {
        o.branch = 2; o.t = 1.f - r[0] - r[4] + r[8];
        o.n[0] = r[3] - r[1]; o.n[1] = r[2] + r[6]; o.n[2] = r[7] + r[5]; o.n[3] = o.t;
    } else {
        o.branch = 3; o.t = 1.f + r[0] + r[4] + r[8];
        o.n[0] = o.t; o.n[1] = r[7] - r[5]; o.n[2] = r[2] - r[6]; o.n[3] = r[3] - r[1];
    }
    const float rt = sqrtf(o.t);
    for (int i = 0; i < 4; ++i) o.q[i] = o.n[i] / rt * 0.5f;
    return o;
}

// quaternion -> axis-angle; false where a component is NaN (the reference zeroes those: the whole matrix counts as dead here)
__device__ __forceinline__ bool m2a_aa(const float q[4], float aa[3], float* k_out, float* s2_out, float* tt_out) {
    const float s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3], s = sqrtf(s2), c = q[0];
    const float two_theta = 2.f * (c < 0.f ? atan2f(-s, -c) : atan2f(s, c));
    const float k = s2 > 0.f ? two_theta / s : 2.f;
    for (int i = 0; i < 3; ++i) aa[i] = q[1 + i] * k;
    *k_out = k;
    *s2_out = s2;
    *tt_out = two_theta;
    return !(isnan(aa[0]) || isnan(aa[1]) || isnan(aa[2]));
}

__device__ __forceinline__ bool m2a_skipped(long long m, int period, int skip, long long* compact, long long* head) {
    if (period <= 0) {
        *compact = m;
        return false;
    }
    const long long g = m / period;
    const int r = (int)(m - g * period);
    *compact = g * (period - skip) + (r - skip);
    *head = g * skip + r;
    return r < skip;
}

__global__ __launch_bounds__(M2A_TPB) void mat2aa_fwd_kernel(const float* __restrict__ R, float* __restrict__ aa_out,
                                                             float* __restrict__ head_out, long long N, int period, int skip) {
#pragma clang fp contract(off)
    const long long m = (long long)blockIdx.x * M2A_TPB + threadIdx.x;
    if (m >= N) return;
    float r[9];
    for (int i = 0; i < 9; ++i) r[i] = R[m * 9 + i];
    long long compact = 0, head = 0;
    if (m2a_skipped(m, period, skip, &compact, &head)) {
        if (head_out)
            for (int i = 0; i < 9; ++i) head_out[head * 9 + i] = r[i];
        return;
    }
    const M2AQuat Q = m2a_quat(r);
    float aa[3], k, s2, two_theta;
    m2a_aa(Q.q, aa, &k, &s2, &two_theta);
    for (int i = 0; i < 3; ++i) aa_out[compact * 3 + i] = isnan(aa[i]) ? 0.f : aa[i];
}

__global__ __launch_bounds__(M2A_TPB) void mat2aa_bwd_kernel(const float* __restrict__ R, const float* __restrict__ g_aa,
                                                             const float* __restrict__ g_head, float* __restrict__ g_R,
                                                             long long N, int period, int skip) {
#pragma clang fp contract(off)
    const long long m = (long long)blockIdx.x * M2A_TPB + threadIdx.x;
    if (m >= N) return;
    long long compact = 0, head = 0;
    float* o = g_R + m * 9;
    if (m2a_skipped(m, period, skip, &compact, &head)) {
        for (int i = 0; i < 9; ++i) o[i] = g_head ? g_head[head * 9 + i] : 0.f;
        return;
    }
    float r[9];
    for (int i = 0; i < 9; ++i) r[i] = R[m * 9 + i];
    const M2AQuat Q = m2a_quat(r);
    float aa[3], k, s2, two_theta;
    const bool alive = m2a_aa(Q.q, aa, &k, &s2, &two_theta) && Q.t > 0.f;
    float gr[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (alive) {
        const float ga[3] = {g_aa[compact * 3], g_aa[compact * 3 + 1], g_aa[compact * 3 + 2]};
        // axis-angle -> quaternion
        float gq[4];
        if (s2 > 0.f) {
            const float s = sqrtf(s2), c = Q.q[0], nn = s2 + c * c;
            const float gk = ga[0] * Q.q[1] + ga[1] * Q.q[2] + ga[2] * Q.q[3];
            const float gtt = gk / s;
            const float gs = gtt * (2.f * c / nn) - gk * two_theta / s2;
            gq[0] = gtt * (-2.f * s / nn);
            for (int i = 0; i < 3; ++i) gq[1 + i] = ga[i] * k + gs * (Q.q[1 + i] / s);
        } else {                                 // the limit of the k = 2 branch
            gq[0] = 0.f;
            for (int i = 0; i < 3; ++i) gq[1 + i] = 2.f * ga[i];
        }
        // quaternion -> numerator and trace term:  q = 0.5 n / sqrt(t)
        const float rt = sqrtf(Q.t);
        float gn[4], gt = 0.f;
        for (int i = 0; i < 4; ++i) {
            gn[i] = 0.5f * gq[i] / rt;
            gt += gq[i] * Q.n[i];
        }
        gt = -0.25f * gt / (Q.t * rt);
        // numerator -> matrix.  d(a, b) adds g to r[a] and sign * g to r[b]
        #define M2A_PAIR(G, A, Bm, SIGN) { gr[A] += (G); gr[Bm] += (SIGN) * (G); }
        switch (Q.branch) {
        case 0:
            gt += gn[1];
            M2A_PAIR(gn[0], 7, 5, -1.f) M2A_PAIR(gn[2], 3, 1, 1.f) M2A_PAIR(gn[3], 2, 6, 1.f)
            gr[0] += gt; gr[4] -= gt; gr[8] -= gt;
            break;
        case 1:
            gt += gn[2];
            M2A_PAIR(gn[0], 2, 6, -1.f) M2A_PAIR(gn[1], 3, 1, 1.f) M2A_PAIR(gn[3], 7, 5, 1.f)
            gr[0] -= gt; gr[4] += gt; gr[8] -= gt;
            break;
        case 2:
            gt += gn[3];
            M2A_PAIR(gn[0], 3, 1, -1.f) M2A_PAIR(gn[1], 2, 6, 1.f) M2A_PAIR(gn[2], 7, 5, 1.f)
            gr[0] -= gt; gr[4] -= gt; gr[8] += gt;
            break;
        default:
            gt += gn[0];
            M2A_PAIR(gn[1], 7, 5, -1.f) M2A_PAIR(gn[2], 2, 6, -1.f) M2A_PAIR(gn[3], 3, 1, -1.f)
            gr[0] += gt; gr[4] += gt; gr[8] += gt;
            break;
        }
        #undef M2A_PAIR
    }
    for (int i = 0; i < 9; ++i) o[i] = gr[i];
}

// ------------------------------------------------------------------------------------------------ joint loss
constexpr int L1_TPB = 256;

__global__ __launch_bounds__(L1_TPB) void joint_l1_kernel(const float* __restrict__ j, const float* __restrict__ target,
                                                          const rih_opt_state* __restrict__ state, float* __restrict__ loss,
                                                          float* __restrict__ total, float* __restrict__ dj,
                                                          float* __restrict__ history, int hist_rows, int B) {
#pragma clang fp contract(off)
    __shared__ float part[L1_TPB];
    const long long row = state ? state->step : -1;
    const float w = 1.f / 63.f;
    float mine = 0.f;
    for (long long b = threadIdx.x; b < B; b += L1_TPB) {
        const float* jb = j + b * 63;
        const float* tb = target + b * 63;
        float* db = dj + b * 63;
        const float j0[3] = {jb[0], jb[1], jb[2]};
        float sum = 0.f, d0[3] = {0.f, 0.f, 0.f};
        for (int i = 0; i < 63; ++i) {
            const float diff = (jb[i] - j0[i % 3]) - tb[i];
            sum += fabsf(diff);
            if (i >= 3) {
                const float g = diff > 0.f ? w : (diff < 0.f ? -w : 0.f);
                db[i] = g;
                d0[i % 3] -= g;
            }
        }
        for (int c = 0; c < 3; ++c) db[c] = d0[c];
        const float l = sum / 63.f;
        loss[b] = l;
        if (history && row >= 0 && row < hist_rows) history[row * B + b] = l;
        mine += l;                               // hands b, b + 256, ... in ascending order
    }
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int step = L1_TPB / 2; step > 0; step >>= 1) {
        if ((int)threadIdx.x < step) part[threadIdx.x] += part[threadIdx.x + step];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = part[0];
}

// ------------------------------------------------------------------------------------------------ schedule, selection
__global__ __launch_bounds__(64) void lr_linear_step_kernel(rih_opt_state* __restrict__ st,
                                                            const rih_lr_linear* __restrict__ sched) {
#pragma clang fp contract(off)
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int64_t i = st->step, n = sched->n_iter;
    const double lr = sched->base_lr * (double)(n - i) / (double)n;
    const int ng = st->ngroups < RIH_OPT_MAX_GROUPS ? st->ngroups : RIH_OPT_MAX_GROUPS;
    for (int g = 0; g < ng; ++g) st->lr[g] = lr;
    st->step = i + 1;
}

constexpr int SEL_TPB = 192;                     // >= 144 + 10 values of a hand

__global__ __launch_bounds__(SEL_TPB) void fit_select_kernel(const float* __restrict__ loss, const float* __restrict__ P,
                                                             const float* __restrict__ beta, float* __restrict__ best_loss,
                                                             float* __restrict__ best_P, float* __restrict__ best_beta) {
    const long long b = blockIdx.x;
    const float l = loss[b], best = best_loss[b];
    __syncthreads();                             // every thread has read best_loss[b] before thread 0 replaces it
    if (!(l < best)) return;                     // uniform over the workgroup; a NaN loss is never the best
    const int t = threadIdx.x;
    if (t < 144) best_P[b * 144 + t] = P[b * 144 + t];
    else if (t < 154) best_beta[b * 10 + (t - 144)] = beta[b * 10 + (t - 144)];
    if (t == 0) best_loss[b] = l;
}

}  // namespace

extern "C" int rih_aik(const float* tmpl, const float* joints, int normalize, float* R, int B, void* stream) {
    if (!tmpl || !joints || !R || B < 1 || (normalize != 0 && normalize != 1)) return RIH_EINVAL;
    const int groups = (B + AIK_HANDS - 1) / AIK_HANDS;
    hipLaunchKernelGGL(aik_kernel, dim3((unsigned)groups), dim3(AIK_HANDS * AIK_LANES), 0, (hipStream_t)stream, tmpl, joints, R,
                       B, normalize);
    return (int)hipGetLastError();
}

static bool m2a_args_ok(int64_t N, int period, int skip) {
    if (N < 1 || (N + M2A_TPB - 1) / M2A_TPB > 0x7fffffffLL) return false;
    if (period < 0 || skip < 0 || (period == 0 && skip != 0) || (period > 0 && (skip >= period || N % period != 0))) return false;
    return true;
}

extern "C" int rih_mat2aa_fwd(const float* R, float* aa, float* head, int64_t N, int period, int skip, void* stream) {
    if (!R || !aa || !m2a_args_ok(N, period, skip)) return RIH_EINVAL;
    hipLaunchKernelGGL(mat2aa_fwd_kernel, dim3((unsigned)((N + M2A_TPB - 1) / M2A_TPB)), dim3(M2A_TPB), 0, (hipStream_t)stream,
                       R, aa, head, (long long)N, period, skip);
    return (int)hipGetLastError();
}

extern "C" int rih_mat2aa_bwd(const float* R, const float* g_aa, const float* g_head, float* g_R, int64_t N, int period,
                              int skip, void* stream) {
    if (!R || !g_aa || !g_R || !m2a_args_ok(N, period, skip)) return RIH_EINVAL;
    hipLaunchKernelGGL(mat2aa_bwd_kernel, dim3((unsigned)((N + M2A_TPB - 1) / M2A_TPB)), dim3(M2A_TPB), 0, (hipStream_t)stream,
                       R, g_aa, g_head, g_R, (long long)N, period, skip);
    return (int)hipGetLastError();
}

extern "C" int rih_joint_l1(const float* j, const float* target, const rih_opt_state* state, float* loss, float* total,
                            float* dj, float* history, int hist_rows, int B, void* stream) {
    if (!j || !target || !loss || !total || !dj || B < 1 || hist_rows < 0 || (history && (!state || hist_rows < 1)))
        return RIH_EINVAL;
    hipLaunchKernelGGL(joint_l1_kernel, dim3(1), dim3(L1_TPB), 0, (hipStream_t)stream, j, target, state, loss, total, dj,
                       history, hist_rows, B);
    return (int)hipGetLastError();
}

extern "C" int rih_lr_linear_step(rih_opt_state* state, const rih_lr_linear* sched, void* stream) {
    if (!state || !sched) return RIH_EINVAL;
    hipLaunchKernelGGL(lr_linear_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, sched);
    return (int)hipGetLastError();
}

extern "C" int rih_fit_select(const float* loss, const float* P, const float* beta, float* best_loss, float* best_P,
                              float* best_beta, int B, void* stream) {
    if (!loss || !P || !beta || !best_loss || !best_P || !best_beta || B < 1) return RIH_EINVAL;
    hipLaunchKernelGGL(fit_select_kernel, dim3((unsigned)B), dim3(SEL_TPB), 0, (hipStream_t)stream, loss, P, beta, best_loss,
                       best_P, best_beta);
    return (int)hipGetLastError();
}
