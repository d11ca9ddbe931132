// rih_nature.hip -- the pose optimiser's NatureLoss for gfx950: a pose discriminator's verdict on both hands as a loss
// (pose_data_optimize/hocontact/postprocess/geo_optimizer_both_batch.py:110-132 `GeOptimizer.NatureLoss`, the network of
// Ver2Code/Discriminator/discrim.py:66-105 with the conversions of utlize.py; renderih_amd.nature.FusedTwoHandNatureLoss, whose
// docstring lists what is kept of the reference and the one deviation).
//
// Rows are the 2B hands, right hands first, then left; a workgroup of H threads owns a tile of R consecutive rows (a tile may
// hold hands of both sides; rows past 2B compute on zeros and write nothing).
//   nature_fwd_kernel     per row the 15 finger quaternions -> normalised -> matrix (with the conversion's own 2 / |q|^2) ->
//                         XYZ Euler angles (asin's argument clamped to [-1, 1]) = 45 inputs; Linear 45->H, H->H, H->H (+ the
//                         first layer's output), H->H without activation, H->H, each other one with LeakyReLU(0.01): the
//                         weights stream once per tile from the packed [in][out] copies (dense() below: 16-byte loads, four
//                         k-slices, partial sums added in slice order), the activations sit in LDS as [k][R] (one broadcast
//                         read per k), thread j finishes output column j for the R rows;
//                         Linear H->2 by one wavefront per (row, class), softmax, the mask p1 < 1.5 p0 and the row's BCE.
//                         Saved for the backward: the four activated layers (their signs are the LeakyReLU slopes) and
//                         (p0, p1, bce, mask) per row.
//   nature_reduce_kernel  one workgroup, one wavefront per side: count and sum of the masked rows in a fixed order,
//                         mean (exactly 0 for an empty side), loss, terms, and the per-row scale 1 / n_side (0: unmasked).
//   nature_bwd_kernel     the same tiles: d loss / d logits from the saved probabilities, the row scale and the upstream scalar
//                         (both read from device memory), the chain transposed on torch's own [out][in] weights (coalesced over
//                         the input column), the Euler, matrix and normalisation Jacobians, dq [B][16][4] with a zero root.
// Arithmetic: fp32 FMA chains (fp32 MFMA runs at the vector rate on gfx950 and the work is weight-streaming and latency bound:
// 8 H^2 weights for <= 64 rows).  Plain stores, fixed summation orders: two runs are bit-identical.  The load width, R and the
// unroll depth of the weight stream (the loads in flight per thread) are compile-time choices, measured in
// profiles/nature_loss/tile_and_unroll.log: 16-byte loads, R = 4, unroll 8 (forward + backward 105 us at B = 32, H = 512, against
// 221 us for 4-byte loads; forward 120 VGPRs and 57376 B of LDS, backward 120 VGPRs and 49184 B, no scratch).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"
#include "rih_reduce.h"

#ifndef RIH_NATURE_R
#define RIH_NATURE_R 4
#endif
#ifndef RIH_NATURE_UNROLL
#define RIH_NATURE_UNROLL 8
#endif
#ifndef RIH_NATURE_VEC
#define RIH_NATURE_VEC 1
#endif

namespace {

constexpr int R = RIH_NATURE_R;
constexpr int HMAX = 512, NJ = 15, NX = 45;
constexpr float SLOPE = 0.01f;
constexpr int KS = RIH_NATURE_VEC ? 4 : 1;          // k-slices of a dense layer (see dense())
static_assert(R >= 1 && R <= 8 && (!RIH_NATURE_VEC || R <= 4), "the activation and partial-sum buffers must fit 64 kB of LDS");

struct NatureW {
    const float *w1t, *w2t, *w3t, *w4t, *wlt;      // [in][out]: the forward's
    const float *w1, *w2, *w3, *w4, *wl;           // [out][in]: torch's own, the backward's
    const float *wp;                               // [2][H]
    const float *b1, *b2, *b3, *b4, *bl, *bp;
};

inline NatureW carve(const float* p, int H) {
    const size_t h = (size_t)H, hh = h * h;
    NatureW w;
    w.w1t = p, p += NX * h;
    w.w2t = p, p += hh;
    w.w3t = p, p += hh;
    w.w4t = p, p += hh;
    w.wlt = p, p += hh;
    w.w1 = p, p += NX * h;
    w.w2 = p, p += hh;
    w.w3 = p, p += hh;
    w.w4 = p, p += hh;
    w.wl = p, p += hh;
    w.wp = p, p += 2 * h;
    w.b1 = p, p += h;
    w.b2 = p, p += h;
    w.b3 = p, p += h;
    w.b4 = p, p += h;
    w.bl = p, p += h;
    w.bp = p;
    return w;
}

inline long long pack_floats(int H) { return 8LL * H * H + 97LL * H + 4; }
// [2B][4][H] activations, [2B][4] (p0, p1, bce, mask), [2B] scale
inline long long ws_floats(int B, int H) { return 2LL * B * (4LL * H + 4 + 1) + 2; }
inline bool bad_h(int H) { return H < 64 || H > HMAX || H % 64 != 0; }

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : v * SLOPE; }
__device__ __forceinline__ float slope_of(float act) { return act > 0.f ? 1.f : SLOPE; }

// acc[r] += sum_k in[k][r] * W[k][j], W row pitch H: the weight column of thread j against the tile's rows in LDS
__device__ __forceinline__ void matvec(const float* __restrict__ W, const float* in, int K, int H, int j, float acc[R]) {
    const float* wj = W + j;
#pragma unroll RIH_NATURE_UNROLL
    for (int k = 0; k < K; ++k) {
        const float w = wj[(size_t)k * H];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fmaf(in[k * R + r], w, acc[r]);
    }
}

// One H-wide layer for the tile: acc[r] += sum_k in[k][r] * W[k][j] for the caller's column j = tid, W [K][H].
// RIH_NATURE_VEC = 0: every thread walks all K rows of its own column (4-byte loads).
// RIH_NATURE_VEC = 1: the H threads are 4 k-slices x H/4 column quads; a thread walks a quarter of the rows with 16-byte loads
// of four neighbouring columns (four times the bytes in flight per thread: the layer is bound by how much one CU keeps in
// flight), the 4 x [H][R] partial sums meet in `part` and are added in slice order.  Ends with every thread past a barrier
// behind its reads of `in`; the caller puts a barrier behind its own writes before the next layer.
__device__ __forceinline__ void dense(const float* __restrict__ W, const float* in, float* part, int K, int H, int tid,
                                      float acc[R]) {
#if RIH_NATURE_VEC
    const int quads = H >> 2, cq = tid % quads, ks = tid / quads, kper = (K + 3) >> 2;
    const int k0 = ks * kper, k1 = min(K, k0 + kper);
    float p[R][4];
#pragma unroll
    for (int r = 0; r < R; ++r) p[r][0] = p[r][1] = p[r][2] = p[r][3] = 0.f;
    const float* wq = W + 4 * cq;
#pragma unroll RIH_NATURE_UNROLL
    for (int k = k0; k < k1; ++k) {
        const float4 w = *reinterpret_cast<const float4*>(wq + (size_t)k * H);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float a = in[k * R + r];
            p[r][0] = fmaf(a, w.x, p[r][0]), p[r][1] = fmaf(a, w.y, p[r][1]);
            p[r][2] = fmaf(a, w.z, p[r][2]), p[r][3] = fmaf(a, w.w, p[r][3]);
        }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < R; ++r) part[((size_t)ks * H + 4 * cq + c) * R + r] = p[r][c];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += part[((size_t)s * H + tid) * R + r];
#else
    (void)part;
    matvec(W, in, K, H, tid, acc);
#endif
}

// one finger joint: the raw quaternion -> what the Euler angles and their Jacobian need
struct Joint {
    float q[4];          // normalised (w, x, y, z)
    float n, s;          // max(|q_raw|, 1e-12), 2 / |q|^2 of the normalised quaternion
    float m00, m01, m02, m12, m22;
};

__device__ __forceinline__ Joint joint_of(const float* raw) {
    Joint t;
    const float w = raw[0], x = raw[1], y = raw[2], z = raw[3];
    t.n = fmaxf(sqrtf(w * w + x * x + y * y + z * z), 1e-12f);
    t.q[0] = w / t.n, t.q[1] = x / t.n, t.q[2] = y / t.n, t.q[3] = z / t.n;
    const float r = t.q[0], i = t.q[1], j = t.q[2], k = t.q[3];
    t.s = 2.f / (r * r + i * i + j * j + k * k);
    t.m00 = 1.f - t.s * (j * j + k * k);
    t.m01 = t.s * (i * j - k * r);
    t.m02 = t.s * (i * k + j * r);
    t.m12 = t.s * (j * k - i * r);
    t.m22 = 1.f - t.s * (i * i + j * j);
    return t;
}

__global__ __launch_bounds__(HMAX) void nature_fwd_kernel(const NatureW w, const float* __restrict__ q_r,
                                                          const float* __restrict__ q_l, float* __restrict__ ws, int B, int H) {
    __shared__ float s_a[HMAX * R], s_b[HMAX * R], s_c[HMAX * R], s_z[2 * R];
    __shared__ float s_p[RIH_NATURE_VEC ? KS * HMAX * R : 1];
    const int tid = threadIdx.x, row0 = blockIdx.x * R, rows = 2 * B;
    float* act = ws;
    float* rowdata = ws + (size_t)rows * 4 * H;

    for (int t = tid; t < R * NJ; t += H) {
        const int r = t / NJ, jn = t % NJ, row = row0 + r;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        if (row < rows) {
            const float* q = (row < B ? q_r + (size_t)row * 64 : q_l + (size_t)(row - B) * 64) + (jn + 1) * 4;
            const Joint m = joint_of(q);
            a0 = atan2f(-m.m12, m.m22);
            a1 = asinf(fminf(fmaxf(m.m02, -1.f), 1.f));
            a2 = atan2f(-m.m01, m.m00);
        }
        s_a[(jn * 3) * R + r] = a0, s_a[(jn * 3 + 1) * R + r] = a1, s_a[(jn * 3 + 2) * R + r] = a2;
    }
    __syncthreads();

    const int j = tid;
    float acc[R], d1[R];
    // d1 = leaky(layer_1(x))
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = w.b1[j];
    dense(w.w1t, s_a, s_p, NX, H, j, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        d1[r] = leaky(acc[r]);
        s_c[j * R + r] = d1[r];
        if (row0 + r < rows) act[((size_t)(row0 + r) * 4 + 0) * H + j] = d1[r];
    }
    __syncthreads();
    // d2 = leaky(layer_2(d1))
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = w.b2[j];
    dense(w.w2t, s_c, s_p, H, H, j, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float v = leaky(acc[r]);
        s_b[j * R + r] = v;
        if (row0 + r < rows) act[((size_t)(row0 + r) * 4 + 1) * H + j] = v;
    }
    __syncthreads();
    // d3 = leaky(layer_3(d2) + d1)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = w.b3[j];
    dense(w.w3t, s_b, s_p, H, H, j, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float v = leaky(acc[r] + d1[r]);
        s_a[j * R + r] = v;
        if (row0 + r < rows) act[((size_t)(row0 + r) * 4 + 2) * H + j] = v;
    }
    __syncthreads();
    // d4 = layer_4(d3)
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = w.b4[j];
    dense(w.w4t, s_a, s_p, H, H, j, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) s_b[j * R + r] = acc[r];
    __syncthreads();
    // d_last = leaky(layer_last(d4))
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = w.bl[j];
    dense(w.wlt, s_b, s_p, H, H, j, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float v = leaky(acc[r]);
        s_a[j * R + r] = v;
        if (row0 + r < rows) act[((size_t)(row0 + r) * 4 + 3) * H + j] = v;
    }
    __syncthreads();
    // layer_pred: one wavefront per (row, class)
    const int lane = tid & 63, wave = tid >> 6, nwaves = H >> 6;
    for (int p = wave; p < 2 * R; p += nwaves) {
        const int r = p >> 1, o = p & 1;
        float s = 0.f;
        for (int k = lane; k < H; k += 64) s = fmaf(s_a[k * R + r], w.wp[o * H + k], s);
        s = wave_sum(s);
        if (lane == 0) s_z[p] = s + w.bp[o];
    }
    __syncthreads();
    if (tid < R && row0 + tid < rows) {
        const float z0 = s_z[2 * tid], z1 = s_z[2 * tid + 1], zm = fmaxf(z0, z1);
        const float e0 = expf(z0 - zm), e1 = expf(z1 - zm), sum = e0 + e1;
        const float p0 = e0 / sum, p1 = e1 / sum;
        float* out = rowdata + (size_t)(row0 + tid) * 4;
        out[0] = p0, out[1] = p1;
        out[2] = -(fmaxf(logf(1.f - p0), -100.f) + fmaxf(logf(p1), -100.f)) * 0.5f;       // binary_cross_entropy's log floor
        out[3] = p1 < 1.5f * p0 ? 1.f : 0.f;
    }
}

__global__ __launch_bounds__(128) void nature_reduce_kernel(float* __restrict__ ws, float* __restrict__ loss,
                                                            float* __restrict__ terms, int B, int H) {
    __shared__ float s_n[2], s_m[2];
    const int tid = threadIdx.x, side = tid >> 6, lane = tid & 63, rows = 2 * B;
    const float* rowdata = ws + (size_t)rows * 4 * H;
    float* scale = ws + (size_t)rows * (4 * H + 4);
    float n = 0.f, sum = 0.f;
    for (int b = lane; b < B; b += 64) {
        const float* rd = rowdata + ((size_t)side * B + b) * 4;
        if (rd[3] != 0.f) n += 1.f, sum += rd[2];
    }
    n = wave_sum(n), sum = wave_sum(sum);
    if (lane == 0) s_n[side] = n, s_m[side] = n > 0.f ? sum / n : 0.f;
    __syncthreads();
    if (tid == 0) {
        loss[0] = s_m[0] + s_m[1];
        terms[0] = s_m[0], terms[1] = s_m[1], terms[2] = s_n[0], terms[3] = s_n[1];
    }
    for (int row = tid; row < rows; row += 128)
        scale[row] = rowdata[(size_t)row * 4 + 3] != 0.f ? 1.f / s_n[row < B ? 0 : 1] : 0.f;
}

__global__ __launch_bounds__(HMAX) void nature_bwd_kernel(const NatureW w, const float* __restrict__ q_r,
                                                          const float* __restrict__ q_l, const float* __restrict__ ws,
                                                          const float* __restrict__ grad_out, float* __restrict__ dq_r,
                                                          float* __restrict__ dq_l, int B, int H) {
    __shared__ float s_a[HMAX * R], s_b[HMAX * R], s_z[2 * R];
    __shared__ float s_p[RIH_NATURE_VEC ? KS * HMAX * R : 1];
    const int tid = threadIdx.x, row0 = blockIdx.x * R, rows = 2 * B;
    const float* act = ws;
    const float* rowdata = ws + (size_t)rows * 4 * H;
    const float* scale = ws + (size_t)rows * (4 * H + 4);

    if (tid < R) {
        float dz0 = 0.f, dz1 = 0.f;
        if (row0 + tid < rows) {
            const float* rd = rowdata + (size_t)(row0 + tid) * 4;
            const float p0 = rd[0], p1 = rd[1], s = scale[row0 + tid] * grad_out[0] * 0.5f;
            // binary_cross_entropy's backward (target (0, 1)), then softmax's
            const float g0 = s * p0 / fmaxf((1.f - p0) * p0, 1e-12f), g1 = s * (p1 - 1.f) / fmaxf((1.f - p1) * p1, 1e-12f);
            const float dot = g0 * p0 + g1 * p1;
            dz0 = p0 * (g0 - dot), dz1 = p1 * (g1 - dot);
        }
        s_z[2 * tid] = dz0, s_z[2 * tid + 1] = dz1;
    }
    __syncthreads();

    const int j = tid;
    float acc[R], res[R], sl[R];
    // through layer_pred and d_last's LeakyReLU
    {
        const float wp0 = w.wp[j], wp1 = w.wp[H + j];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const float a = row0 + r < rows ? act[((size_t)(row0 + r) * 4 + 3) * H + j] : 0.f;
            s_a[j * R + r] = (s_z[2 * r] * wp0 + s_z[2 * r + 1] * wp1) * slope_of(a);
        }
    }
    __syncthreads();
    // layer_last^T -> g d4
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.f;
    dense(w.wl, s_a, s_p, H, H, j, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) s_b[j * R + r] = acc[r];
    __syncthreads();
    // layer_4^T, d3's LeakyReLU -> g of (layer_3(d2) + d1): feeds layer_3 and, as it is, d1
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = 0.f;
        sl[r] = slope_of(row0 + r < rows ? act[((size_t)(row0 + r) * 4 + 2) * H + j] : 0.f);
    }
    dense(w.w4, s_b, s_p, H, H, j, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        res[r] = acc[r] * sl[r];
        s_a[j * R + r] = res[r];
    }
    __syncthreads();
    // layer_3^T, d2's LeakyReLU
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = 0.f;
        sl[r] = slope_of(row0 + r < rows ? act[((size_t)(row0 + r) * 4 + 1) * H + j] : 0.f);
    }
    dense(w.w3, s_a, s_p, H, H, j, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) s_b[j * R + r] = acc[r] * sl[r];
    __syncthreads();
    // layer_2^T plus the residual branch, d1's LeakyReLU
#pragma unroll
    for (int r = 0; r < R; ++r) {
        acc[r] = 0.f;
        sl[r] = slope_of(row0 + r < rows ? act[((size_t)(row0 + r) * 4 + 0) * H + j] : 0.f);
    }
    dense(w.w2, s_b, s_p, H, H, j, acc);
#pragma unroll
    for (int r = 0; r < R; ++r) s_a[j * R + r] = (acc[r] + res[r]) * sl[r];
    __syncthreads();
    // layer_1^T: wavefront v sums its 64 output columns for input i = lane, the partials are added in wavefront order below
    const int lane = tid & 63, wave = tid >> 6, nwaves = H >> 6;
    if (lane < NX) {
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 0.f;
        matvec(w.w1 + (size_t)wave * 64 * NX, s_a + wave * 64 * R, 64, NX, lane, acc);
#pragma unroll
        for (int r = 0; r < R; ++r) s_b[(wave * NX + lane) * R + r] = acc[r];
    }
    __syncthreads();
    for (int t = tid; t < R * NJ; t += H) {
        const int r = t / NJ, jn = t % NJ, row = row0 + r;
        if (row >= rows) continue;
        float ga[3] = {0.f, 0.f, 0.f};
        for (int v = 0; v < nwaves; ++v)
#pragma unroll
            for (int c = 0; c < 3; ++c) ga[c] += s_b[(v * NX + jn * 3 + c) * R + r];
        const size_t at = row < B ? (size_t)row * 64 : (size_t)(row - B) * 64;
        const float* q = (row < B ? q_r : q_l) + at + (jn + 1) * 4;
        float* dq = (row < B ? dq_r : dq_l) + at;
        const Joint m = joint_of(q);
        // Euler angles -> matrix entries (a zero denominator is gimbal lock: atan2(0, 0), no gradient)
        const float den0 = m.m12 * m.m12 + m.m22 * m.m22, den2 = m.m01 * m.m01 + m.m00 * m.m00;
        const float c1 = 1.f - m.m02 * m.m02;
        const float g12 = den0 > 0.f ? -ga[0] * m.m22 / den0 : 0.f, g22 = den0 > 0.f ? ga[0] * m.m12 / den0 : 0.f;
        const float g02 = c1 > 0.f ? ga[1] / sqrtf(c1) : 0.f;                      // clamped asin: zero derivative
        const float g01 = den2 > 0.f ? -ga[2] * m.m00 / den2 : 0.f, g00 = den2 > 0.f ? ga[2] * m.m01 / den2 : 0.f;
        // matrix entries -> normalised quaternion: m = const + s * t(q), s = 2 / |q|^2
        const float qr = m.q[0], qi = m.q[1], qj = m.q[2], qk = m.q[3];
        const float gs = g00 * -(qj * qj + qk * qk) + g01 * (qi * qj - qk * qr) + g02 * (qi * qk + qj * qr) +
                         g12 * (qj * qk - qi * qr) + g22 * -(qi * qi + qj * qj);
        const float t00 = g00 * m.s, t01 = g01 * m.s, t02 = g02 * m.s, t12 = g12 * m.s, t22 = g22 * m.s;
        const float ds = -gs * m.s * m.s;
        float gq[4];
        gq[0] = -t01 * qk + t02 * qj - t12 * qi + ds * qr;
        gq[1] = t01 * qj + t02 * qk - t12 * qr - 2.f * t22 * qi + ds * qi;
        gq[2] = -2.f * t00 * qj + t01 * qi + t02 * qr + t12 * qk - 2.f * t22 * qj + ds * qj;
        gq[3] = -2.f * t00 * qk - t01 * qr + t02 * qi + t12 * qj + ds * qk;
        // q / max(|q|, eps)
        const float dot = gq[0] * qr + gq[1] * qi + gq[2] * qj + gq[3] * qk;
#pragma unroll
        for (int c = 0; c < 4; ++c) dq[(jn + 1) * 4 + c] = (gq[c] - m.q[c] * dot) / m.n;
        if (jn == 0) dq[0] = 0.f, dq[1] = 0.f, dq[2] = 0.f, dq[3] = 0.f;           // the root is not an input of the term
    }
}

struct PackSeg {
    const float* src;
    long long dst;
    int rows, cols, transpose;       // src [rows][cols]; transpose: dst [cols][rows]
};
struct PackArgs {
    PackSeg seg[17];
};

__global__ __launch_bounds__(256) void nature_pack_kernel(const PackArgs a, float* __restrict__ packed) {
    const PackSeg s = a.seg[blockIdx.y];
    const long long n = (long long)s.rows * s.cols;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        // i walks the destination, so the stores are coalesced
        const long long from = s.transpose ? (i % s.rows) * s.cols + i / s.rows : i;
        packed[s.dst + i] = s.src[from];
    }
}

}  // namespace

extern "C" int64_t rih_nature_pack_floats(int H) { return bad_h(H) ? 0 : pack_floats(H); }
extern "C" int64_t rih_nature_ws_floats(int B, int H) { return (bad_h(H) || B < 1 || B > RIH_NATURE_MAX_B) ? 0 : ws_floats(B, H); }
extern "C" int rih_nature_tile_rows(void) { return R; }

extern "C" int rih_nature_pack(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                               const float* b3, const float* w4, const float* b4, const float* w_last, const float* b_last,
                               const float* w_pred, const float* b_pred, float* packed, int H, void* stream) {
    if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !w4 || !b4 || !w_last || !b_last || !w_pred || !b_pred || !packed)
        return RIH_EINVAL;
    if (bad_h(H) || ((uintptr_t)packed & 15)) return RIH_EINVAL;
    const NatureW w = carve(packed, H);
    PackArgs a;
    const float* dst[17] = {w.w1t, w.w2t, w.w3t, w.w4t, w.wlt, w.w1, w.w2, w.w3, w.w4, w.wl, w.wp,
                            w.b1, w.b2, w.b3, w.b4, w.bl, w.bp};
    const float* src[17] = {w1, w2, w3, w4, w_last, w1, w2, w3, w4, w_last, w_pred, b1, b2, b3, b4, b_last, b_pred};
    for (int i = 0; i < 17; ++i) {
        a.seg[i].src = src[i];
        a.seg[i].dst = (long long)(dst[i] - packed);
        a.seg[i].rows = i < 10 ? H : (i == 10 ? 2 : 1);
        a.seg[i].cols = (i == 0 || i == 5) ? NX : (i == 16 ? 2 : H);
        a.seg[i].transpose = i < 5;
    }
    hipLaunchKernelGGL(nature_pack_kernel, dim3(64, 17), dim3(256), 0, (hipStream_t)stream, a, packed);
    return (int)hipGetLastError();
}

extern "C" int rih_nature_fwd(const float* packed, const float* q_r, const float* q_l, float* ws, int B, int H, void* stream) {
    if (!packed || !q_r || !q_l || !ws) return RIH_EINVAL;
    if (bad_h(H) || B < 1 || B > RIH_NATURE_MAX_B || ((uintptr_t)ws & 15) || ((uintptr_t)packed & 15)) return RIH_EINVAL;
    const unsigned tiles = (unsigned)((2 * B + R - 1) / R);
    hipLaunchKernelGGL(nature_fwd_kernel, dim3(tiles), dim3((unsigned)H), 0, (hipStream_t)stream, carve(packed, H), q_r, q_l, ws,
                       B, H);
    return (int)hipGetLastError();
}

extern "C" int rih_nature_reduce(float* ws, float* loss, float* terms, int B, int H, void* stream) {
    if (!ws || !loss || !terms) return RIH_EINVAL;
    if (bad_h(H) || B < 1 || B > RIH_NATURE_MAX_B || ((uintptr_t)ws & 15)) return RIH_EINVAL;
    hipLaunchKernelGGL(nature_reduce_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, ws, loss, terms, B, H);
    return (int)hipGetLastError();
}

extern "C" int rih_nature_bwd(const float* packed, const float* q_r, const float* q_l, const float* ws, const float* grad_out,
                              float* dq_r, float* dq_l, int B, int H, void* stream) {
    if (!packed || !q_r || !q_l || !ws || !grad_out || !dq_r || !dq_l) return RIH_EINVAL;
    if (bad_h(H) || B < 1 || B > RIH_NATURE_MAX_B || ((uintptr_t)ws & 15) || ((uintptr_t)packed & 15)) return RIH_EINVAL;
    const unsigned tiles = (unsigned)((2 * B + R - 1) / R);
    hipLaunchKernelGGL(nature_bwd_kernel, dim3(tiles), dim3((unsigned)H), 0, (hipStream_t)stream, carve(packed, H), q_r, q_l, ws,
                       grad_out, dq_r, dq_l, B, H);
    return (int)hipGetLastError();
}
