// rih_demo.hip -- the glue of the reference's image-to-overlay path (core/test_utils.py::InterRender, apps/demo.py) for a
// whole batch resident on the GPU: uint8 BGR photographs in, uint8 BGR overlays out, no fp32 image crossing the bus.
//
// demo_prepare_kernel: one lane per destination pixel.  ragged uint8 BGR batch -> black border to a square (pad2squre) ->
//   8-bit bilinear resize (below) -> BGR->RGB, /255, ImageNet normalisation -> fp32 NCHW and/or fp16 NHWC8 (the fp16
//   backbone's input, one 16-byte store per lane) and/or the resized uint8 BGR image.  The padded square is never written:
//   a tap outside the image reads as 0.  rih_demo_resize is the same kernel with only the uint8 output.
// demo_compose_kernel: one lane per pixel.  uint8(fl(fl(img 255) mask) + fl(bg fl(1 - mask))) with the background resized
//   in the kernel (or white), every product and sum rounded to float32 (numpy's order, no contraction), truncation.
// demo_other_view_kernel: one workgroup per sample.  centre of the two hands' vertex means (fixed tree: lane partials in
//   index order, wave shuffle, LDS), subtract, rotate.
// demo_smooth_kernel: the constant-acceleration filter over a list of tensors, one launch.
//
// The resize is integer-only on the device: the per-axis taps (s, s', a0, a1) are built on the host in numpy
// (renderih_amd/demo.py::axis_table), so no result depends on how the device rounds or contracts a multiply-add.
//   copy   (PH == Sy, PW == Sx), box (PH == 2 Sy, PW == 2 Sx): (p00 + p01 + p10 + p11 + 2) >> 2,
//   else   T_r = P[r][s] a0 + P[r][s'] a1;  out = clamp((((b0 (T0 >> 4)) >> 16) + ((b1 (T1 >> 4)) >> 16) + 2) >> 2).
//
// STATUS: the resize restates cv::resize (CV_8U, INTER_LINEAR) from memory of the OpenCV 4 sources; conformity with a real
// OpenCV build is NOT verified (there is none to compare with).  Checked against the numpy oracle of tests/demo_cases.py.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"
#include "rih_reduce.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr int TPB = 256;
constexpr int MAX_GRID = 1048576;

struct alignas(16) Tap { int s0, s1, a0, a1; };

struct Image {                      // one row of the descriptor table, checked against the buffers it points into
    const uint8_t* px;              // nullptr: the row does not fit the source buffer -> the image reads as black
    int H, W, pt, pl, mode;
    const Tap* ty;
    const Tap* tx;
};

__device__ __forceinline__ Image load_image(const uint8_t* src, long long src_bytes, const long long* __restrict__ desc, int b,
                                            const int* __restrict__ tabs, long long tab_entries, int Sy, int Sx) {
    const long long* d = desc + (long long)b * RIH_DEMO_DESC;
    Image im;
    const long long off = d[0], H = d[1], W = d[2];
    const bool ok = off >= 0 && H >= 1 && W >= 1 && H <= 32767 && W <= 32767 && off + H * W * 3 <= src_bytes;
    im.px = ok ? src + off : nullptr;
    im.H = (int)H;
    im.W = (int)W;
    im.pt = (int)d[3];
    im.pl = (int)d[4];
    const long long PH = d[5], PW = d[6], ty = d[8], tx = d[9];
    im.mode = (PH == Sy && PW == Sx) ? 0 : ((PH == 2LL * Sy && PW == 2LL * Sx) ? 1 : 2);
    if (im.mode == 2 && !(tabs != nullptr && ty >= 0 && tx >= 0 && ty + Sy <= tab_entries && tx + Sx <= tab_entries)) im.px = nullptr;
    im.ty = (const Tap*)tabs + ty;
    im.tx = (const Tap*)tabs + tx;
    return im;
}

__device__ __forceinline__ void padded(const Image& im, int r, int c, int* p) {       // P[r][c], 0 on the border
    const int rr = r - im.pt, cc = c - im.pl;
    if (im.px != nullptr && rr >= 0 && rr < im.H && cc >= 0 && cc < im.W) {
        const uint8_t* q = im.px + ((long long)rr * im.W + cc) * 3;
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    } else {
        p[0] = p[1] = p[2] = 0;
    }
}

__device__ __forceinline__ void resize_pixel(const Image& im, int y, int x, int* out) {
    if (im.px == nullptr) { out[0] = out[1] = out[2] = 0; return; }
    if (im.mode == 0) {
        padded(im, y, x, out);
    } else if (im.mode == 1) {
        int a[3], b[3], c[3], d[3];
        padded(im, 2 * y, 2 * x, a);
        padded(im, 2 * y, 2 * x + 1, b);
        padded(im, 2 * y + 1, 2 * x, c);
        padded(im, 2 * y + 1, 2 * x + 1, d);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = (a[k] + b[k] + c[k] + d[k] + 2) >> 2;
    } else {
        const Tap ty = im.ty[y], tx = im.tx[x];
        int p00[3], p01[3], p10[3], p11[3];
        padded(im, ty.s0, tx.s0, p00);
        padded(im, ty.s0, tx.s1, p01);
        padded(im, ty.s1, tx.s0, p10);
        padded(im, ty.s1, tx.s1, p11);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int T0 = p00[k] * tx.a0 + p01[k] * tx.a1;
            const int T1 = p10[k] * tx.a0 + p11[k] * tx.a1;
            const int v = (((ty.a0 * (T0 >> 4)) >> 16) + ((ty.a1 * (T1 >> 4)) >> 16) + 2) >> 2;
            out[k] = v < 0 ? 0 : (v > 255 ? 255 : v);
        }
    }
}

__global__ __launch_bounds__(TPB) void demo_prepare_kernel(const uint8_t* __restrict__ src, long long src_bytes,
                                                           const long long* __restrict__ desc, const int* __restrict__ tabs,
                                                           long long tab_entries, int B, int Sy, int Sx,
                                                           float* __restrict__ norm, _Float16* __restrict__ norm_h8,
                                                           uint8_t* __restrict__ out_u8) {
    const long long plane = (long long)Sy * Sx, total = (long long)B * plane;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        const int x = (int)(i % Sx);
        const int y = (int)((i / Sx) % Sy);
        const int b = (int)(i / plane);
        const Image im = load_image(src, src_bytes, desc, b, tabs, tab_entries, Sy, Sx);
        int pix[3];
        resize_pixel(im, y, x, pix);
        if (out_u8 != nullptr) {
#pragma unroll
            for (int c = 0; c < 3; ++c) out_u8[i * 3 + c] = (uint8_t)pix[c];
        }
        if (norm == nullptr && norm_h8 == nullptr) continue;
        const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
        const long long at = (long long)y * Sx + x;
        float nr[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float rgb = (float)pix[2 - c] / 255.f;
            nr[c] = (rgb - mean[c]) / sd[c];
            if (norm != nullptr) norm[((long long)b * 3 + c) * plane + at] = nr[c];
        }
        if (norm_h8 != nullptr) {
            half8 h;
#pragma unroll
            for (int c = 0; c < 8; ++c) h[c] = c < 3 ? (_Float16)nr[c] : (_Float16)0.f;
            *(half8*)(norm_h8 + i * 8) = h;
        }
    }
}

__global__ __launch_bounds__(TPB) void demo_compose_kernel(const float* __restrict__ rgb, long long rgb_ld,
                                                           const float* __restrict__ mask, long long mask_ld,
                                                           const uint8_t* __restrict__ bg, long long bg_bytes,
                                                           const long long* __restrict__ desc, const int* __restrict__ tabs,
                                                           long long tab_entries, int B, int R, uint8_t* __restrict__ out) {
#pragma clang fp contract(off)
    const long long plane = (long long)R * R, total = (long long)B * plane;
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < total; i += (long long)gridDim.x * TPB) {
        int back[3] = {255, 255, 255};
        if (bg != nullptr) {
            const int x = (int)(i % R);
            const int y = (int)((i / R) % R);
            const int b = (int)(i / plane);
            const Image im = load_image(bg, bg_bytes, desc, b, tabs, tab_entries, R, R);
            resize_pixel(im, y, x, back);
        }
        const float m = mask[i * mask_ld];
        const float keep = 1.f - m;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float fg = rgb[i * rgb_ld + c] * 255.f;
            const float a = fg * m;
            const float bk = (float)back[c] * keep;
            const float v = a + bk;
            out[i * 3 + c] = (uint8_t)(v >= 255.f ? 255 : (v > 0.f ? (int)v : 0));     // truncation; saturates, NaN -> 0
        }
    }
}

struct Rot { float r[9]; };

__global__ __launch_bounds__(TPB) void demo_other_view_kernel(const float* __restrict__ vl, const float* __restrict__ vr,
                                                              const Rot rot, int V, float* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ float red[TPB / 64][6];
    const int b = blockIdx.x;
    const float* hand[2] = {vl + (long long)b * V * 3, vr + (long long)b * V * 3};
    float s[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < V; i += TPB) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int k = 0; k < 3; ++k) s[3 * h + k] += hand[h][3 * i + k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float w = wave_sum(s[k]);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = w;
    }
    __syncthreads();
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float ml = ((red[0][k] + red[1][k]) + (red[2][k] + red[3][k])) / (float)V;
        const float mr = ((red[0][3 + k] + red[1][3 + k]) + (red[2][3 + k] + red[3][3 + k])) / (float)V;
        c[k] = (ml + mr) / 2.f;
    }
    float* o = out + (long long)b * 2 * V * 3;
    for (int i = threadIdx.x; i < 2 * V; i += TPB) {
        const float* p = i < V ? hand[0] + 3 * i : hand[1] + 3 * (i - V);
        const float x0 = p[0] - c[0], x1 = p[1] - c[1], x2 = p[2] - c[2];
#pragma unroll
        for (int j = 0; j < 3; ++j) o[3 * i + j] = (x0 * rot.r[j] + x1 * rot.r[3 + j]) + x2 * rot.r[6 + j];
    }
}

struct SmoothArgs {
    const float* p[RIH_DEMO_SMOOTH_MAX];
    float* out[RIH_DEMO_SMOOTH_MAX];
    float* last[RIH_DEMO_SMOOTH_MAX];
    float* last_v[RIH_DEMO_SMOOTH_MAX];
    float* acc[RIH_DEMO_SMOOTH_MAX];
    long long n[RIH_DEMO_SMOOTH_MAX];
    int stage;
};

// stage = frames seen before this one: 0 nothing exists; 1 `last`; 2 `last`, `last_v`; >= 3 all three, so the prediction runs
__global__ __launch_bounds__(TPB) void demo_smooth_kernel(const SmoothArgs a) {
#pragma clang fp contract(off)
    const int e = blockIdx.y;
    const float* p = a.p[e];                     // no __restrict__ on these two: out may be p
    float* out = a.out[e];
    float* __restrict__ last = a.last[e];
    float* __restrict__ last_v = a.last_v[e];
    float* __restrict__ acc = a.acc[e];
    const long long n = a.n[e];
    for (long long i = (long long)blockIdx.x * TPB + threadIdx.x; i < n; i += (long long)gridDim.x * TPB) {
        float x = p[i];
        const float l = a.stage >= 1 ? last[i] : 0.f;
        const float lv = a.stage >= 2 ? last_v[i] : 0.f;
        if (a.stage >= 3) {
            const float pred = (l + lv) + 0.5f * acc[i];
            x = 0.7f * x + 0.3f * pred;
        }
        out[i] = x;
        if (a.stage >= 1) {
            const float v = x - l;
            if (a.stage >= 2) acc[i] = v - lv;
            last_v[i] = v;
        }
        last[i] = x;
    }
}

int grid_for(long long total) {
    const long long g = (total + TPB - 1) / TPB;
    return (int)(g < 1 ? 1 : (g > MAX_GRID ? MAX_GRID : g));
}

bool bad_tabs(const int32_t* tabs, long long tab_entries) {
    return tab_entries < 0 || (tab_entries > 0 && tabs == nullptr) || (reinterpret_cast<uintptr_t>(tabs) & 15);
}

}  // namespace

extern "C" int rih_demo_prepare(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int32_t* tabs,
                                int64_t tab_entries, int B, int S, float* norm, void* norm_h8, uint8_t* out_u8, void* stream) {
    if (!src || src_bytes < 3 || !desc || B < 1 || B > 65536 || S < 1 || S > 32767 || (!norm && !norm_h8 && !out_u8) ||
        bad_tabs(tabs, tab_entries))
        return RIH_EINVAL;
    if (norm_h8 && (reinterpret_cast<uintptr_t>(norm_h8) & 15)) return RIH_EINVAL;
    hipLaunchKernelGGL(demo_prepare_kernel, dim3(grid_for((long long)B * S * S)), dim3(TPB), 0, (hipStream_t)stream, src,
                       (long long)src_bytes, (const long long*)desc, tabs, (long long)tab_entries, B, S, S, norm,
                       (_Float16*)norm_h8, out_u8);
    return (int)hipGetLastError();
}

extern "C" int rih_demo_resize(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int32_t* tabs,
                               int64_t tab_entries, int B, int Sy, int Sx, uint8_t* out, void* stream) {
    if (!src || src_bytes < 3 || !desc || !out || B < 1 || B > 65536 || Sy < 1 || Sy > 32767 || Sx < 1 || Sx > 32767 ||
        bad_tabs(tabs, tab_entries))
        return RIH_EINVAL;
    hipLaunchKernelGGL(demo_prepare_kernel, dim3(grid_for((long long)B * Sy * Sx)), dim3(TPB), 0, (hipStream_t)stream, src,
                       (long long)src_bytes, (const long long*)desc, tabs, (long long)tab_entries, B, Sy, Sx, (float*)nullptr,
                       (_Float16*)nullptr, out);
    return (int)hipGetLastError();
}

extern "C" int rih_demo_compose(const float* rgb, int64_t rgb_ld, const float* mask, int64_t mask_ld, const uint8_t* bg,
                                int64_t bg_bytes, const int64_t* bg_desc, const int32_t* tabs, int64_t tab_entries, int B, int R,
                                uint8_t* out, void* stream) {
    if (!rgb || !mask || !out || rgb_ld < 3 || mask_ld < 1 || B < 1 || B > 65536 || R < 1 || R > 32767 ||
        bad_tabs(tabs, tab_entries) || (bg && (!bg_desc || bg_bytes < 3)))
        return RIH_EINVAL;
    hipLaunchKernelGGL(demo_compose_kernel, dim3(grid_for((long long)B * R * R)), dim3(TPB), 0, (hipStream_t)stream, rgb,
                       (long long)rgb_ld, mask, (long long)mask_ld, bg, (long long)bg_bytes, (const long long*)bg_desc, tabs,
                       (long long)tab_entries, B, R, out);
    return (int)hipGetLastError();
}

extern "C" int rih_demo_other_view(const float* v_left, const float* v_right, const float* rot_host, int B, int V, float* out,
                                   void* stream) {
    if (!v_left || !v_right || !rot_host || !out || B < 1 || B > 2147483647 || V < 1 || V > (1 << 24) || out == v_left ||
        out == v_right)
        return RIH_EINVAL;
    Rot rot;
    for (int k = 0; k < 9; ++k) rot.r[k] = rot_host[k];
    hipLaunchKernelGGL(demo_other_view_kernel, dim3(B), dim3(TPB), 0, (hipStream_t)stream, v_left, v_right, rot, V, out);
    return (int)hipGetLastError();
}

extern "C" int rih_demo_smooth(const int64_t* rows_host, int E, int stage, void* stream) {
    if (!rows_host || E < 1 || E > RIH_DEMO_SMOOTH_MAX || stage < 0) return RIH_EINVAL;
    SmoothArgs a;
    long long most = 0;
    for (int e = 0; e < E; ++e) {
        const int64_t* r = rows_host + 6 * e;
        if (!r[0] || !r[1] || !r[2] || !r[3] || !r[4] || r[5] < 1) return RIH_EINVAL;
        a.p[e] = (const float*)r[0];
        a.out[e] = (float*)r[1];
        a.last[e] = (float*)r[2];
        a.last_v[e] = (float*)r[3];
        a.acc[e] = (float*)r[4];
        a.n[e] = r[5];
        most = r[5] > most ? r[5] : most;
    }
    for (int e = E; e < RIH_DEMO_SMOOTH_MAX; ++e) {
        a.p[e] = nullptr; a.out[e] = a.last[e] = a.last_v[e] = a.acc[e] = nullptr; a.n[e] = 0;
    }
    a.stage = stage > 3 ? 3 : stage;
    const long long gx = (most + TPB - 1) / TPB;
    hipLaunchKernelGGL(demo_smooth_kernel, dim3((unsigned)(gx > 4096 ? 4096 : gx), E), dim3(TPB), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}
