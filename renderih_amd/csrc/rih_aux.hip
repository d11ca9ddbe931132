// rih_aux.hip -- the auxiliary heads of the encoders (heat maps, hand mask, dense correspondence) for gfx950: the label
// generator of dataset/heatmap.py, calc_aux_loss of core/Loss.py:180-198 with the gradients of its total, and the heat-map
// decoder get_final_preds2 of dataset/inference.py:113-127.
//
//   heatmaps_kernel   one workgroup per map (grid-stride over maps), 16-byte stores; the pixel value comes from hm_value().
//   aux_loss_kernel   a pure stream.  The work is cut into items of 1024 pixels: an item of the first kind covers one pixel
//                     range of one image for the mask AND the dense term together (the two mask labels and the three dense
//                     labels are read once and used by all eight prediction planes), an item of the second kind one pixel
//                     range of one heat map.  Every operand is read once, every gradient written once; the heat-map target
//                     is either read or produced by hm_value() from the joint (then no target tensor exists at all).  Each
//                     workgroup leaves three raw sums; aux_loss_final_kernel adds them in a fixed order.  No atomics: two
//                     runs give the same bits.
//   decode_kernel     one workgroup per map, the map in LDS.  The blurred map is never stored: its maximum is formed on the
//                     fly and the 25 values around the arg-max are computed again, each as the column pass over row passes,
//                     the order of a separable filter.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"
#include "rih_reduce.h"

namespace {

constexpr int TPB = 256;
constexpr int CHUNK = TPB * 4;                 // pixels per work item
constexpr int MAX_BLOCKS = 2048;               // 8 workgroups per CU: every SIMD holds 8 waves of independent 16-byte loads

// nn.SmoothL1Loss(beta): 0.5 x^2 / beta below beta, |x| - 0.5 beta from beta on
__device__ __forceinline__ float sl1(float x, float beta) {
    const float a = fabsf(x);
    return a < beta ? 0.5f * x * x / beta : a - 0.5f * beta;
}
__device__ __forceinline__ float dsl1(float x, float beta) { return fabsf(x) < beta ? x / beta : (x > 0.f ? 1.f : -1.f); }

// ---------------------------------------------------------------------------------------------- heat-map labels
struct HmJoint {
    float x, y;
    bool on;
};

// heatmap.py:33-38: drawn when the third column (if there is one) is > 0 and 0 <= x, y < R
__device__ __forceinline__ HmJoint hm_joint(const float* __restrict__ joints, long long map, int C, int R) {
    const float* p = joints + map * C;
    HmJoint j;
    j.x = p[0];
    j.y = p[1];
    j.on = !(j.x < 0.f || j.y < 0.f || j.x >= (float)R || j.y >= (float)R) && (C == 2 || p[2] > 0.f);
    return j;
}

// build_hm at flat pixel idx: the ONE place the label value is computed (rih_heatmaps and the joints form of rih_aux_loss)
__device__ __forceinline__ float hm_value(const HmJoint& j, int idx, int R, float two_s2) {
    const int y = idx / R, x = idx - y * R;
    const float dx = (float)x - j.x, dy = (float)y - j.y;
    return j.on ? expf(-(dx * dx + dy * dy) / two_s2) : 0.f;
}

template <bool VEC>
__global__ __launch_bounds__(TPB) void heatmaps_kernel(const float* __restrict__ joints, float* __restrict__ hms,
                                                       long long maps, int C, int R, float two_s2) {
    const int P = R * R;
    for (long long m = blockIdx.x; m < maps; m += gridDim.x) {
        const HmJoint j = hm_joint(joints, m, C, R);
        float* o = hms + m * P;
        if (VEC) {
            for (int i = threadIdx.x * 4; i < P; i += CHUNK)
                *reinterpret_cast<float4*>(o + i) = make_float4(hm_value(j, i, R, two_s2), hm_value(j, i + 1, R, two_s2),
                                                                hm_value(j, i + 2, R, two_s2), hm_value(j, i + 3, R, two_s2));
        } else {
            for (int i = threadIdx.x; i < P; i += TPB) o[i] = hm_value(j, i, R, two_s2);
        }
    }
}

// ---------------------------------------------------------------------------------------------- loss
// the four pixels of this thread inside the item that starts at `base`: VEC = four neighbours (one 16-byte access, P % 4 == 0
// so a quad is inside the plane or outside it as a whole), otherwise four pixels 256 apart (coalesced dwords)
template <bool VEC> __device__ __forceinline__ int px_index(int base, int k) {
    return VEC ? base + (int)threadIdx.x * 4 + k : base + (int)threadIdx.x + TPB * k;
}

template <bool VEC> __device__ __forceinline__ void ld4(const float* __restrict__ p, int base, int P, float v[4]) {
    if (VEC) {
        const int i = px_index<true>(base, 0);
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < P) q = *reinterpret_cast<const float4*>(p + i);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = px_index<false>(base, k);
            v[k] = i < P ? p[i] : 0.f;
        }
    }
}

template <bool VEC> __device__ __forceinline__ void st4(float* __restrict__ p, int base, int P, const float v[4]) {
    if (VEC) {
        const int i = px_index<true>(base, 0);
        if (i < P) *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = px_index<false>(base, k);
            if (i < P) p[i] = v[k];
        }
    }
}

struct AuxArgs {
    const float *p_hms, *p_mask, *p_dense, *t_hms, *t_joints, *t_mask, *t_dense, *w;
    float *g_hms, *g_mask, *g_dense, *partial;
    int Jh, S, C, chunks;
    long long md_items, items;
    float two_s2, beta, inv_mask, inv_dense, inv_hms;
};

template <bool VEC> __global__ __launch_bounds__(TPB) void aux_loss_kernel(AuxArgs a) {
    __shared__ float s_red[4];
    const int P = a.S * a.S;
    // the weights live in device memory: a captured graph follows a change of them
    const float gm = a.w[0] * a.inv_mask, gd = a.w[1] * 0.5f * a.inv_dense, gh = a.w[2] * 2.f * a.inv_hms;
    const float beta = a.beta;
    float acc_m = 0.f, acc_d = 0.f, acc_h = 0.f;
    for (long long it = blockIdx.x; it < a.items; it += gridDim.x) {
        if (it < a.md_items) {                                             // mask + dense, one pixel range of one image
            const long long b = it / a.chunks;
            const int base = (int)(it - b * a.chunks) * CHUNK;
            float tm[2][4], g[4];
#pragma unroll
            for (int h = 0; h < 2; ++h) ld4<VEC>(a.t_mask + (b * 2 + h) * P, base, P, tm[h]);
            if (a.p_mask != nullptr) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float pm[4];
                    ld4<VEC>(a.p_mask + (b * 2 + h) * P, base, P, pm);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const float d = pm[k] - tm[h][k];
                        acc_m += sl1(d, beta);
                        g[k] = gm * dsl1(d, beta);
                    }
                    st4<VEC>(a.g_mask + (b * 2 + h) * P, base, P, g);
                }
            }
            if (a.p_dense != nullptr) {
                float td[3][4];
#pragma unroll
                for (int c = 0; c < 3; ++c) ld4<VEC>(a.t_dense + (b * 3 + c) * P, base, P, td[c]);
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        float pd[4];
                        ld4<VEC>(a.p_dense + (b * 6 + h * 3 + c) * P, base, P, pd);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float m = tm[h][k];                      // a float factor, not a flag
                            const float d = pd[k] * m - td[c][k] * m;
                            acc_d += sl1(d, beta);
                            g[k] = gd * dsl1(d, beta) * m;
                        }
                        st4<VEC>(a.g_dense + (b * 6 + h * 3 + c) * P, base, P, g);
                    }
            }
        } else {                                                           // one pixel range of one heat map
            const long long q = it - a.md_items, map = q / a.chunks;
            const int base = (int)(q - map * a.chunks) * CHUNK;
            float ph[4], th[4], g[4];
            ld4<VEC>(a.p_hms + map * P, base, P, ph);
            if (a.t_hms != nullptr) {
                ld4<VEC>(a.t_hms + map * P, base, P, th);
            } else {
                const HmJoint j = hm_joint(a.t_joints, map, a.C, a.S);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = px_index<VEC>(base, k);
                    th[k] = i < P ? hm_value(j, i, a.S, a.two_s2) : 0.f;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float d = ph[k] - th[k];
                acc_h += d * d;
                g[k] = gh * d;
            }
            st4<VEC>(a.g_hms + map * P, base, P, g);
        }
    }
    const float sm = block_sum(acc_m, s_red), sd = block_sum(acc_d, s_red), sh = block_sum(acc_h, s_red);
    if (threadIdx.x == 0) {
        float* o = a.partial + (long long)blockIdx.x * 4;
        o[0] = sm, o[1] = sd, o[2] = sh, o[3] = 0.f;
    }
}

// out[4] = total, mask, dense, hms
__global__ __launch_bounds__(TPB) void aux_loss_final_kernel(const float* __restrict__ partial, const float* __restrict__ w,
                                                             int nblk, float inv_mask, float inv_dense, float inv_hms,
                                                             float* __restrict__ out) {
    __shared__ float s_red[4];
    float s[3] = {0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < nblk; i += TPB) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] += partial[i * 4 + k];
    }
    const float sm = block_sum(s[0], s_red), sd = block_sum(s[1], s_red), sh = block_sum(s[2], s_red);
    if (threadIdx.x == 0) {
        const float mask = sm * inv_mask, dense = 0.5f * sd * inv_dense, hms = sh * inv_hms;
        out[0] = (w[0] * mask + w[1] * dense) + w[2] * hms;
        out[1] = mask, out[2] = dense, out[3] = hms;
    }
}

struct AuxShape {
    long long md_items, items;
    int chunks, nblk;
    float inv_mask, inv_dense, inv_hms;
};

bool aux_shape(int B, int Jh, int S, bool has_hms, bool has_md, AuxShape* s) {
    if (B < 1 || B > (1 << 20) || S < 1 || S > 4096 || (has_hms && (Jh < 1 || Jh > 4096)) || (!has_hms && !has_md)) return false;
    const long long P = (long long)S * S;
    s->chunks = (int)((P + CHUNK - 1) / CHUNK);
    s->md_items = has_md ? (long long)B * s->chunks : 0;
    s->items = s->md_items + (has_hms ? (long long)B * Jh * s->chunks : 0);
    s->nblk = (int)(s->items < MAX_BLOCKS ? s->items : MAX_BLOCKS);
    s->inv_mask = (float)(1.0 / (2.0 * B * P));
    s->inv_dense = (float)(1.0 / (3.0 * B * P));
    s->inv_hms = has_hms ? (float)(1.0 / ((double)B * Jh * P)) : 0.f;
    return true;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------- decoder
// OpenCV's fixed Gaussian taps for sigma = 0 (getGaussianKernel's small_gaussian_tab), centred in 7 entries
__device__ const float DEC_TAPS[3][7] = {{0.f, 0.f, 0.25f, 0.5f, 0.25f, 0.f, 0.f},
                                         {0.f, 0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f, 0.f},
                                         {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};

// the zero-padded separable blur at one pixel: rows first (left to right), then the column (top to bottom)
__device__ __forceinline__ float blur_at(const float* s, int y, int x, int H, int W, int r, const float* tp) {
    float acc = 0.f;
    for (int i = -r; i <= r; ++i) {
        const int yy = y + i;
        float row = 0.f;
        if (yy >= 0 && yy < H)
            for (int j = -r; j <= r; ++j) {
                const int xx = x + j;
                if (xx >= 0 && xx < W) row += tp[j + 3] * s[yy * W + xx];
            }
        acc += tp[i + 3] * row;
    }
    return acc;
}

template <int NPIX>
__global__ __launch_bounds__(TPB) void decode_kernel(const float* __restrict__ hm, float* __restrict__ preds,
                                                     float* __restrict__ maxvals, long long maps, int H, int W, int ksize,
                                                     int vec) {
    __shared__ float s_map[NPIX];
    __shared__ float s_v[4];
    __shared__ int s_i[4];
    __shared__ float s_nb[25];
    const int P = H * W, t = threadIdx.x, r = ksize / 2;
    const float* tp = DEC_TAPS[r > 0 ? r - 1 : 0];
    for (long long m = blockIdx.x; m < maps; m += gridDim.x) {
        __syncthreads();                                                   // the previous map is done with
        const float* src = hm + m * P;
        // ---- load, arg-max with the first flat index winning (np.argmax); NaNs never win
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        if (vec) {
            for (int i = t * 4; i < P; i += CHUNK) {
                const float4 q = *reinterpret_cast<const float4*>(src + i);
                const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    s_map[i + k] = v[k];
                    if (v[k] > bv) bv = v[k], bi = i + k;
                }
            }
        } else {
            for (int i = t; i < P; i += TPB) {
                const float v = src[i];
                s_map[i] = v;
                if (v > bv) bv = v, bi = i;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o, 64);
            const int i2 = __shfl_xor(bi, o, 64);
            if (v2 > bv || (v2 == bv && i2 < bi)) bv = v2, bi = i2;
        }
        if ((t & 63) == 0) s_v[t >> 6] = bv, s_i[t >> 6] = bi;
        __syncthreads();
        bv = s_v[0], bi = s_i[0];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (s_v[k] > bv || (s_v[k] == bv && s_i[k] < bi)) bv = s_v[k], bi = s_i[k];
        const float raw_max = bv;
        if (!(raw_max > 0.f)) {                                            // inference.py:44-47; nothing is refined at (0, 0)
            if (t == 0) preds[m * 2] = 0.f, preds[m * 2 + 1] = 0.f, maxvals[m] = raw_max;
            continue;
        }
        const int py = bi / W, px = bi - py * W;
        if (!(px > 1 && px < W - 2 && py > 1 && py < H - 2)) {             // taylor() leaves the integer coordinates
            if (t == 0) preds[m * 2] = (float)px, preds[m * 2 + 1] = (float)py, maxvals[m] = raw_max;
            continue;
        }
        float scale = 1.f;
        if (ksize > 1) {                                                   // origin_max / max of the blurred map
            float bm = -INFINITY;
            for (int i = t; i < P; i += TPB) {
                const int y = i / W;
                bm = fmaxf(bm, blur_at(s_map, y, i - y * W, H, W, r, tp));
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) bm = fmaxf(bm, __shfl_xor(bm, o, 64));
            __syncthreads();                                               // s_v was read above by every thread
            if ((t & 63) == 0) s_v[t >> 6] = bm;
            __syncthreads();
            scale = raw_max / fmaxf(fmaxf(s_v[0], s_v[1]), fmaxf(s_v[2], s_v[3]));
        }
        if (t < 25) {                                                      // log map on the 5 x 5 around the arg-max (inside the map)
            const int ny = py + t / 5 - 2, nx = px + t % 5 - 2;
            const float v = ksize > 1 ? blur_at(s_map, ny, nx, H, W, r, tp) * scale : s_map[ny * W + nx];
            s_nb[t] = logf(fmaxf(v, 1e-10f));
        }
        __syncthreads();
        if (t == 0) {
#define NB(dy, dx) s_nb[((dy) + 2) * 5 + (dx) + 2]
            const float dx = 0.5f * (NB(0, 1) - NB(0, -1)), dy = 0.5f * (NB(1, 0) - NB(-1, 0));
            const float dxx = 0.25f * (NB(0, 2) - 2.f * NB(0, 0) + NB(0, -2));
            const float dxy = 0.25f * (NB(1, 1) - NB(-1, 1) - NB(1, -1) + NB(-1, -1));
            const float dyy = 0.25f * (NB(2, 0) - 2.f * NB(0, 0) + NB(-2, 0));
#undef NB
            float ox = 0.f, oy = 0.f, det;
            {
#pragma clang fp contract(off)                                             // the test against 0 sees the two rounded products
                det = dxx * dyy - dxy * dxy;
            }
            if (det != 0.f) {
                ox = -(dyy * dx - dxy * dy) / det;
                oy = -(dxx * dy - dxy * dx) / det;
            }
            preds[m * 2] = (float)px + ox, preds[m * 2 + 1] = (float)py + oy, maxvals[m] = raw_max;
        }
    }
}

}  // namespace

extern "C" int rih_heatmaps(const float* joints, float* hms, int64_t maps, int C, int R, float sigma, void* stream) {
    if (!joints || !hms || maps < 1 || maps > (1LL << 31) || (C != 2 && C != 3) || R < 1 || R > 4096 || !(sigma > 0.f))
        return RIH_EINVAL;
    const unsigned grid = (unsigned)(maps < 65536 ? maps : 65536);
    const float two_s2 = 2.f * sigma * sigma;
    if ((R * R) % 4 == 0 && aligned16(hms))
        hipLaunchKernelGGL(heatmaps_kernel<true>, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, joints, hms, (long long)maps, C,
                           R, two_s2);
    else
        hipLaunchKernelGGL(heatmaps_kernel<false>, dim3(grid), dim3(TPB), 0, (hipStream_t)stream, joints, hms, (long long)maps,
                           C, R, two_s2);
    return (int)hipGetLastError();
}

extern "C" int rih_aux_loss_blocks(int B, int Jh, int S, int has_hms, int has_mask_or_dense) {
    AuxShape s;
    return aux_shape(B, Jh, S, has_hms != 0, has_mask_or_dense != 0, &s) ? s.nblk : 0;
}

extern "C" int rih_aux_loss(const float* p_hms, const float* p_mask, const float* p_dense, const float* t_hms,
                            const float* t_joints, const float* t_mask, const float* t_dense, const float* weights, int B,
                            int Jh, int S, int C, float sigma, float beta, float* g_hms, float* g_mask, float* g_dense,
                            float* partial, void* stream) {
    AuxShape s;
    if (!weights || !partial || !(beta > 0.f)) return RIH_EINVAL;
    if (!aux_shape(B, Jh, S, p_hms != nullptr, p_mask != nullptr || p_dense != nullptr, &s)) return RIH_EINVAL;
    if (p_hms) {
        if (!g_hms || (t_hms != nullptr) == (t_joints != nullptr)) return RIH_EINVAL;        // exactly one label form
        if (t_joints && ((C != 2 && C != 3) || !(sigma > 0.f))) return RIH_EINVAL;
    }
    if (p_mask && (!g_mask || !t_mask)) return RIH_EINVAL;
    if (p_dense && (!g_dense || !t_mask || !t_dense)) return RIH_EINVAL;
    AuxArgs a;
    a.p_hms = p_hms, a.p_mask = p_mask, a.p_dense = p_dense, a.t_hms = t_hms, a.t_joints = t_joints, a.t_mask = t_mask;
    a.t_dense = t_dense, a.w = weights, a.g_hms = g_hms, a.g_mask = g_mask, a.g_dense = g_dense, a.partial = partial;
    a.Jh = Jh, a.S = S, a.C = C, a.chunks = s.chunks, a.md_items = s.md_items, a.items = s.items;
    a.two_s2 = 2.f * sigma * sigma, a.beta = beta, a.inv_mask = s.inv_mask, a.inv_dense = s.inv_dense, a.inv_hms = s.inv_hms;
    const bool vec = (S * S) % 4 == 0 && aligned16(p_hms) && aligned16(p_mask) && aligned16(p_dense) && aligned16(t_hms) &&
                     aligned16(t_mask) && aligned16(t_dense) && aligned16(g_hms) && aligned16(g_mask) && aligned16(g_dense);
    if (vec)
        hipLaunchKernelGGL(aux_loss_kernel<true>, dim3(s.nblk), dim3(TPB), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(aux_loss_kernel<false>, dim3(s.nblk), dim3(TPB), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

extern "C" int rih_aux_loss_final(const float* partial, const float* weights, int B, int Jh, int S, int has_hms,
                                  int has_mask_or_dense, float* out, void* stream) {
    AuxShape s;
    if (!partial || !weights || !out) return RIH_EINVAL;
    if (!aux_shape(B, Jh, S, has_hms != 0, has_mask_or_dense != 0, &s)) return RIH_EINVAL;
    hipLaunchKernelGGL(aux_loss_final_kernel, dim3(1), dim3(TPB), 0, (hipStream_t)stream, partial, weights, s.nblk, s.inv_mask,
                       s.inv_dense, s.inv_hms, out);
    return (int)hipGetLastError();
}

extern "C" int rih_hms_decode(const float* hm, float* preds, float* maxvals, int64_t maps, int H, int W, int kernel,
                              void* stream) {
    if (!hm || !preds || !maxvals || maps < 1 || maps > (1LL << 31) || H < 1 || W < 1) return RIH_EINVAL;
    if ((long long)H * W * 4 > 65536) return RIH_EINVAL;                   // the map has to fit 64 KB of LDS
    if (kernel != 1 && kernel != 3 && kernel != 5 && kernel != 7) return RIH_EINVAL;
    const int P = H * W;
    const int vec = P % 4 == 0 && aligned16(hm);
    const dim3 grid((unsigned)(maps < 65536 ? maps : 65536));
    const hipStream_t st = (hipStream_t)stream;
    if (P <= 1024)
        hipLaunchKernelGGL(decode_kernel<1024>, grid, dim3(TPB), 0, st, hm, preds, maxvals, (long long)maps, H, W, kernel, vec);
    else if (P <= 4096)
        hipLaunchKernelGGL(decode_kernel<4096>, grid, dim3(TPB), 0, st, hm, preds, maxvals, (long long)maps, H, W, kernel, vec);
    else
        hipLaunchKernelGGL(decode_kernel<16384>, grid, dim3(TPB), 0, st, hm, preds, maxvals, (long long)maps, H, W, kernel, vec);
    return (int)hipGetLastError();
}
