// rih_render.hip -- hard rasteriser and shader of triangle meshes: the two-hand renderer of the reference
// (utils/vis_utils.py:39-289), which builds it on pytorch3d 0.7.2 (MeshRasterizer with blur_radius 0 and faces_per_pixel 1,
// HardPhongShader with PointLights or AmbientLights, TexturesVertex, hard_rgb_blend).  The semantics reproduced are written
// out in renderih_amd/render.py; tests/render_oracle.py restates them in numpy.
//
// Three launches, all fp32, no floating-point atomics:
//   rih_render_setup   one thread per (image, face): camera transform into pytorch3d screen space (NDC x / y, view z), one
//                      16-float face record (bounding box, screen vertices, view z, 1/(area + 1e-8), skip flag); one thread
//                      per (image, vertex): the vertex normal as Meshes.verts_normals defines it (sum of the unnormalised
//                      corner cross products of the incident faces, normalised with eps 1e-6), GATHERED through a vertex ->
//                      (face, corner) CSR in ascending order, so the sum has one fixed order.
//   rih_render_raster  one workgroup per (image, 32 x 32 pixel tile), four pixels per thread.  The face records stream through
//                      LDS one face per thread; each chunk is culled against the tile's rectangle (half a pixel of margin)
//                      and the survivors compacted into an LDS list with an LDS atomicAdd.  Every pixel keeps the minimum of
//                      (z, face index) compared lexicographically: the winner does not depend on the order in which the
//                      atomic filled the list, which makes the fragments bit-identical from run to run.
//   rih_render_shade   one thread per pixel: vertex colour, normal and world point interpolated with the fragment's
//                      barycentrics, hard Phong (one point light) or ambient only, hard_rgb_blend onto a white background.
// Beside them, on the same face records:
//   rih_mask_iou       the silhouette IoU of two meshes (utils/compute_maskiou.py:263-270; renderih_amd/mask_iou.py): the raster
//                      kernel's tiles and pixel test, two coverage flags per pixel instead of a fragment, three integer sums
//                      per image.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"

// No fused multiply-adds in this file: every expression rounds as its numpy restatement (tests/render_oracle.py) does, so the
// kernels agree with the oracle to the last bit wherever a pixel is not on an edge.  Division and sqrt are correctly rounded.
#pragma clang fp contract(off)

namespace {

constexpr int REC = 16;          // floats per face record
constexpr int STPB = 256;        // setup / shade threads per block
constexpr int TILE = 32;         // raster tile edge (pixels)
constexpr int RTPB = 256;        // raster threads per block = faces per LDS chunk
constexpr int PPT = TILE * TILE / RTPB;   // pixels per raster thread
constexpr int LREC = 10;         // floats of a face record the pixel test reads

// camera row [16]: R (3x3 row-major, world -> view is X R + T, row vectors), T, focal (2), principal point (2)
__device__ __forceinline__ void to_screen(const float* cam, int persp, const float* X, float* s) {
    const float xv = X[0] * cam[0] + X[1] * cam[3] + X[2] * cam[6] + cam[9];
    const float yv = X[0] * cam[1] + X[1] * cam[4] + X[2] * cam[7] + cam[10];
    const float zv = X[0] * cam[2] + X[1] * cam[5] + X[2] * cam[8] + cam[11];
    if (persp) {
        s[0] = cam[12] * xv / zv + cam[14];
        s[1] = cam[13] * yv / zv + cam[15];
    } else {
        s[0] = cam[12] * xv + cam[14];
        s[1] = cam[13] * yv + cam[15];
    }
    s[2] = zv;
}

__device__ __forceinline__ void cross3(const float* a, const float* b, float* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void normalize3(float* v) {   // F.normalize(v, eps=1e-6)
    const float n = fmaxf(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), 1e-6f);
    v[0] /= n; v[1] /= n; v[2] /= n;
}

__global__ __launch_bounds__(STPB) void setup_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                     const int32_t* __restrict__ vf_ptr, const int32_t* __restrict__ vf_list,
                                                     const float* __restrict__ cams, int persp, int V, int Vc, int F,
                                                     float* __restrict__ rec, float* __restrict__ vnormals) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * STPB + threadIdx.x;
    const float* vb = verts + (long long)b * V * 3;
    if (t < F) {
        if (!rec) return;
        const float* cam = cams + (long long)b * 16;
        float s[3][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) to_screen(cam, persp, vb + 3 * faces[3 * t + k], s[k]);
        // area = EdgeFunction(v2; v0, v1) in NDC
        const float area = (s[2][0] - s[0][0]) * (s[1][1] - s[0][1]) - (s[2][1] - s[0][1]) * (s[1][0] - s[0][0]);
        bool skip = fabsf(area) < 1e-8f;
        if (persp) skip = skip || s[0][2] <= 0.f || s[1][2] <= 0.f || s[2][2] <= 0.f;
        float* r = rec + ((long long)b * F + t) * REC;
        if (skip) {       // an inverted box: no tile ever keeps it
            r[0] = 3e38f; r[1] = -3e38f; r[2] = 3e38f; r[3] = -3e38f;
        } else {
            r[0] = fminf(fminf(s[0][0], s[1][0]), s[2][0]);
            r[1] = fmaxf(fmaxf(s[0][0], s[1][0]), s[2][0]);
            r[2] = fminf(fminf(s[0][1], s[1][1]), s[2][1]);
            r[3] = fmaxf(fmaxf(s[0][1], s[1][1]), s[2][1]);
        }
        r[4] = s[0][0]; r[5] = s[0][1]; r[6] = s[1][0]; r[7] = s[1][1]; r[8] = s[2][0]; r[9] = s[2][1];
        r[10] = s[0][2]; r[11] = s[1][2]; r[12] = s[2][2];
        r[13] = 1.f / (area + 1e-8f);
        r[14] = skip ? 1.f : 0.f;
        r[15] = 0.f;
        return;
    }
    const int v = t - F;
    if (v >= V || !vnormals) return;
    float n[3] = {0.f, 0.f, 0.f};
    const int e0 = v < Vc ? vf_ptr[v] : 0, e1 = v < Vc ? vf_ptr[v + 1] : 0;      // a vertex of no face: normal 0
    for (int e = e0; e < e1; ++e) {   // ascending (face, corner): one fixed summation order
        const int f = vf_list[e] / 3, c = vf_list[e] % 3;
        const float* p0 = vb + 3 * faces[3 * f + c];
        const float* p1 = vb + 3 * faces[3 * f + (c + 1) % 3];
        const float* p2 = vb + 3 * faces[3 * f + (c + 2) % 3];
        const float a[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const float d[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        float x[3];
        cross3(a, d, x);
        n[0] += x[0]; n[1] += x[1]; n[2] += x[2];
    }
    normalize3(n);
    float* o = vnormals + ((long long)b * V + v) * 3;
    o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
}

// pixel centre of column c (row r) of an S x S image in pytorch3d NDC: +X left, +Y up, row 0 at the top
__device__ __forceinline__ float ndc(int c, int S) { return 1.f - (float)(2 * c + 1) / (float)S; }

// the LREC floats of a face record that a chunk keeps in LDS
struct Face { float x0, y0, x1, y1, x2, y2, z0, z1, z2, ia; };

__device__ __forceinline__ Face load_face(const float* l) {
    return Face{l[0], l[1], l[2], l[3], l[4], l[5], l[6], l[7], l[8], l[9]};
}

// The pixel test of raster_kernel and mask_iou_kernel, in its two steps.  A pixel centre (px, py) is covered by a face when
// inside() holds -- w0, w1, w2 >= 0, the edge functions times 1/(area + 1e-8) -- and view_depth() is not < 0.
__device__ __forceinline__ bool inside(const Face& f, float px, float py, float& w0, float& w1, float& w2) {
    w0 = ((px - f.x1) * (f.y2 - f.y1) - (py - f.y1) * (f.x2 - f.x1)) * f.ia;
    w1 = ((px - f.x2) * (f.y0 - f.y2) - (py - f.y2) * (f.x0 - f.x2)) * f.ia;
    w2 = ((px - f.x0) * (f.y1 - f.y0) - (py - f.y0) * (f.x1 - f.x0)) * f.ia;
    return w0 >= 0.f && w1 >= 0.f && w2 >= 0.f;
}

// zbuf of a pixel that is inside(); under the perspective camera w becomes the perspective-corrected barycentrics first
__device__ __forceinline__ float view_depth(const Face& f, int persp, float& w0, float& w1, float& w2) {
    if (persp) {
        const float t0 = w0 * f.z1 * f.z2, t1 = f.z0 * w1 * f.z2, t2 = f.z0 * f.z1 * w2;
        const float d = fmaxf(t0 + t1 + t2, 1e-8f);
        w0 = t0 / d; w1 = t1 / d; w2 = t2 / d;
    }
    return w0 * f.z0 + w1 * f.z1 + w2 * f.z2;
}

__global__ __launch_bounds__(RTPB) void raster_kernel(const float* __restrict__ rec, int F, int S, int tiles_x, int persp,
                                                      int32_t* __restrict__ p2f, float* __restrict__ zbuf,
                                                      float* __restrict__ bary) {
    __shared__ float lrec[RTPB][LREC];
    __shared__ int lidx[RTPB];
    __shared__ unsigned cnt;
    const int b = blockIdx.y;
    const int c0 = (blockIdx.x % tiles_x) * TILE, r0 = (blockIdx.x / tiles_x) * TILE;
    const int c1 = min(c0 + TILE, S), r1 = min(r0 + TILE, S);
    const float m = 1.f / (float)S;       // half a pixel
    const float xhi = ndc(c0, S) + m, xlo = ndc(c1 - 1, S) - m;
    const float yhi = ndc(r0, S) + m, ylo = ndc(r1 - 1, S) - m;
    const int col = c0 + (int)threadIdx.x % TILE;
    const int row0 = r0 + (int)threadIdx.x / TILE;
    const float px = ndc(col, S);
    float py[PPT], bz[PPT], bw[PPT][3];
    int bf[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        py[k] = ndc(row0 + k * (RTPB / TILE), S);
        bz[k] = 0.f; bf[k] = -1; bw[k][0] = bw[k][1] = bw[k][2] = -1.f;
    }
    const float* rb = rec + (long long)b * F * REC;
    for (int f0 = 0; f0 < F; f0 += RTPB) {
        if (threadIdx.x == 0) cnt = 0u;
        __syncthreads();
        const int f = f0 + (int)threadIdx.x;
        if (f < F) {
            const float* r = rb + (long long)f * REC;
            if (!(r[1] < xlo || r[0] > xhi || r[3] < ylo || r[2] > yhi)) {
                const unsigned slot = atomicAdd(&cnt, 1u);
#pragma unroll
                for (int i = 0; i < LREC; ++i) lrec[slot][i] = r[4 + i];
                lidx[slot] = f;
            }
        }
        __syncthreads();
        const int n = (int)cnt;
        for (int j = 0; j < n; ++j) {
            const Face fc = load_face(lrec[j]);
            const int fj = lidx[j];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                float w0, w1, w2;
                if (!inside(fc, px, py[k], w0, w1, w2)) continue;
                const float z = view_depth(fc, persp, w0, w1, w2);
                if (z < 0.f) continue;                        // behind the image plane
                if (bf[k] < 0 || z < bz[k] || (z == bz[k] && fj < bf[k])) {
                    bz[k] = z; bf[k] = fj; bw[k][0] = w0; bw[k][1] = w1; bw[k][2] = w2;
                }
            }
        }
        __syncthreads();          // the list is rewritten by the next chunk
    }
    if (col >= S) return;
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int row = row0 + k * (RTPB / TILE);
        if (row >= S) continue;
        const long long p = ((long long)b * S + row) * S + col;
        const bool hit = bf[k] >= 0;
        p2f[p] = hit ? b * F + bf[k] : -1;
        zbuf[p] = hit ? bz[k] : -1.f;
        bary[3 * p] = bw[k][0]; bary[3 * p + 1] = bw[k][1]; bary[3 * p + 2] = bw[k][2];
    }
}

// how many lanes of the wavefront hold `p`; every lane of the wavefront calls it
__device__ __forceinline__ unsigned wave_count(bool p) {
#if defined(__HIPCC__)
    return (unsigned)__popcll(__ballot(p));               // 64-bit ballot: one bit per lane
#else                                                     // host build of the tests: no ballot there, a butterfly sum
    unsigned n = p ? 1u : 0u;
    for (int s = 32; s > 0; s >>= 1) n += __shfl_xor(n, s);
    return n;
#endif
}

__global__ __launch_bounds__(STPB) void mask_zero_kernel(int32_t* __restrict__ counts, int n) {
    const int i = blockIdx.x * STPB + threadIdx.x;
    if (i < n) counts[i] = 0;
}

// Coverage only: raster_kernel's tiles, chunks, cull and pixel test, but a pixel keeps two flags (bit 0: some face below
// F_left covers it, bit 1: some face from F_left on does) instead of the nearest fragment.  A face's hand is decided per face:
// the split falls anywhere in a chunk.  counts [B][3] += (pixels with bit 0, with bit 1, with both) of this tile: a ballot and a
// popcount per wavefront, the four wavefronts summed in LDS, one integer atomicAdd per tile and quantity (skipped when zero).
// Under the perspective camera view_depth() is left out, because there it cannot reject.  A face that reaches the test is not
// skipped, so its three z_i are > 0 or NaN; a NaN z_i makes the screen vertex, hence w, NaN, and such a pixel is not inside().
// With w_i >= 0 and z_i > 0 every product t_i is >= 0, d = max(sum, 1e-8) is > 0, every t_i / d is >= 0 or NaN (inf / inf),
// and z = sum (t_i / d) z_i is >= 0 or NaN: `z < 0` is false.  The orthographic z can be negative and is tested.
__global__ __launch_bounds__(RTPB) void mask_iou_kernel(const float* __restrict__ rec, int F, int F_left, int S, int tiles_x,
                                                        int persp, int32_t* __restrict__ counts, uint8_t* __restrict__ mask) {
    __shared__ float lrec[RTPB][LREC];
    __shared__ unsigned lhand[RTPB];
    __shared__ unsigned cnt;
    __shared__ unsigned wsum[RTPB / 64][3];
    const int b = blockIdx.y;
    const int c0 = (blockIdx.x % tiles_x) * TILE, r0 = (blockIdx.x / tiles_x) * TILE;
    const int c1 = min(c0 + TILE, S), r1 = min(r0 + TILE, S);
    const float m = 1.f / (float)S;       // half a pixel
    const float xhi = ndc(c0, S) + m, xlo = ndc(c1 - 1, S) - m;
    const float yhi = ndc(r0, S) + m, ylo = ndc(r1 - 1, S) - m;
    const int col = c0 + (int)threadIdx.x % TILE;
    const int row0 = r0 + (int)threadIdx.x / TILE;
    const float px = ndc(col, S);
    float py[PPT];
    unsigned hit[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        py[k] = ndc(row0 + k * (RTPB / TILE), S);
        hit[k] = 0u;
    }
    const float* rb = rec + (long long)b * F * REC;
    for (int f0 = 0; f0 < F; f0 += RTPB) {
        if (threadIdx.x == 0) cnt = 0u;
        __syncthreads();
        const int f = f0 + (int)threadIdx.x;
        if (f < F) {
            const float* r = rb + (long long)f * REC;
            if (!(r[1] < xlo || r[0] > xhi || r[3] < ylo || r[2] > yhi)) {
                const unsigned slot = atomicAdd(&cnt, 1u);
#pragma unroll
                for (int i = 0; i < LREC; ++i) lrec[slot][i] = r[4 + i];
                lhand[slot] = f < F_left ? 1u : 2u;
            }
        }
        __syncthreads();
        const int n = (int)cnt;
        for (int j = 0; j < n; ++j) {
            const Face fc = load_face(lrec[j]);
            const unsigned h = lhand[j];
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                float w0, w1, w2;
                if (!inside(fc, px, py[k], w0, w1, w2)) continue;
                if (!persp && view_depth(fc, 0, w0, w1, w2) < 0.f) continue;      // perspective: cannot reject, see above
                hit[k] |= h;
            }
        }
        __syncthreads();          // the list is rewritten by the next chunk
    }
    unsigned c[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const int row = row0 + k * (RTPB / TILE);
        const bool in = col < S && row < S;               // a partial tile's pixels beyond the image count for nothing
        const bool l = in && (hit[k] & 1u), r = in && (hit[k] & 2u);
        c[0] += wave_count(l);
        c[1] += wave_count(r);
        c[2] += wave_count(l && r);
        if (mask && in) mask[((long long)b * S + row) * S + col] = (uint8_t)hit[k];
    }
    const int lane = (int)threadIdx.x % 64, wave = (int)threadIdx.x / 64;
    if (lane == 0) { wsum[wave][0] = c[0]; wsum[wave][1] = c[1]; wsum[wave][2] = c[2]; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned total = 0u;
        for (int w = 0; w < RTPB / 64; ++w) total += wsum[w][threadIdx.x];
        if (total) atomicAdd((unsigned*)counts + (b * 3 + (int)threadIdx.x), total);
    }
}

// inter / union in fp32 (both are exact there: at most 4096^2 = 2^24 pixels); 0 where the union is empty
__global__ __launch_bounds__(STPB) void mask_ratio_kernel(const int32_t* __restrict__ counts, int B, float* __restrict__ iou) {
    const int b = blockIdx.x * STPB + threadIdx.x;
    if (b >= B) return;
    const int inter = counts[3 * b + 2], uni = counts[3 * b] + counts[3 * b + 1] - inter;
    iou[b] = uni > 0 ? (float)inter / (float)uni : 0.f;
}

__global__ __launch_bounds__(STPB) void shade_kernel(const int32_t* __restrict__ p2f, const float* __restrict__ bary,
                                                     const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                     const float* __restrict__ vnormals, const float* __restrict__ colors,
                                                     const float* __restrict__ cams, int ambient, int V, int F, int S,
                                                     float* __restrict__ rgba) {
    const int b = blockIdx.y;
    const long long i = (long long)blockIdx.x * STPB + threadIdx.x;
    if (i >= (long long)S * S) return;
    const long long p = (long long)b * S * S + i;
    float* o = rgba + 4 * p;
    const int pf = p2f[p];
    const int f = pf - b * F;
    if (pf < 0 || f < 0 || f >= F) {      // hard_rgb_blend: background colour (1, 1, 1), alpha 0
        o[0] = 1.f; o[1] = 1.f; o[2] = 1.f; o[3] = 0.f;
        return;
    }
    const float w[3] = {bary[3 * p], bary[3 * p + 1], bary[3 * p + 2]};
    int vi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vi[k] = b * V + faces[3 * f + k];
    // texel = c0 + w1 (c1 - c0) + w2 (c2 - c0): a face of one colour shades to exactly that colour (masks)
    float tex[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float c0 = colors[3 * (long long)vi[0] + c];
        tex[c] = c0 + w[1] * (colors[3 * (long long)vi[1] + c] - c0) + w[2] * (colors[3 * (long long)vi[2] + c] - c0);
    }
    if (ambient) {                // AmbientLights (1, 1, 1), materials 1: the texel
        o[0] = tex[0]; o[1] = tex[1]; o[2] = tex[2]; o[3] = 1.f;
        return;
    }
    float P[3] = {0.f, 0.f, 0.f}, N[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            P[c] += w[k] * verts[3 * (long long)vi[k] + c];
            N[c] += w[k] * vnormals[3 * (long long)vi[k] + c];
        }
    // PointLights at (0, 0, -1): ambient 0.5, diffuse 0.3, specular 0.2; Materials 1, shininess 64
    float L[3] = {0.f - P[0], 0.f - P[1], -1.f - P[2]};
    const float* cam = cams + (long long)b * 16;
    // camera centre -T R^T
    float Vd[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) Vd[j] = -(cam[9] * cam[3 * j] + cam[10] * cam[3 * j + 1] + cam[11] * cam[3 * j + 2]) - P[j];
    normalize3(N);
    normalize3(L);
    normalize3(Vd);
    const float cosl = N[0] * L[0] + N[1] * L[1] + N[2] * L[2];
    const float diffuse = 0.3f * fmaxf(cosl, 0.f);
    float a = 0.f;
    if (cosl > 0.f) {
        const float R[3] = {-L[0] + 2.f * cosl * N[0], -L[1] + 2.f * cosl * N[1], -L[2] + 2.f * cosl * N[2]};
        a = fmaxf(Vd[0] * R[0] + Vd[1] * R[1] + Vd[2] * R[2], 0.f);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) a *= a;                 // a^64
    const float spec = 0.2f * a;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (0.5f + diffuse) * tex[c] + spec;
    o[3] = 1.f;
}

bool bad_size(int B, int F, int H, int W) {
    return B < 1 || B > 65535 || F < 1 || H != W || H < 1 || H > 4096 || (long long)B * F > 0x7fffffffLL;
}

}  // namespace

extern "C" int rih_render_setup(const float* verts, const int32_t* faces, const int32_t* vf_ptr, const int32_t* vf_list,
                                const float* cams, int cam_kind, int B, int V, int Vc, int F, float* face_rec, float* vnormals,
                                void* stream) {
    if (!verts || !faces || !cams || (!face_rec && !vnormals) || (vnormals && (!vf_ptr || !vf_list)) || B < 1 || B > 65535 ||
        V < 1 || Vc < 1 || Vc > V || F < 1 || (long long)B * F > 0x7fffffffLL ||
        (cam_kind != RIH_CAM_ORTHOGRAPHIC && cam_kind != RIH_CAM_PERSPECTIVE))
        return RIH_EINVAL;
    const long long n = (long long)F + (vnormals ? V : 0);
    hipLaunchKernelGGL(setup_kernel, dim3((unsigned)((n + STPB - 1) / STPB), B), dim3(STPB), 0, (hipStream_t)stream, verts,
                       faces, vf_ptr, vf_list, cams, cam_kind == RIH_CAM_PERSPECTIVE ? 1 : 0, V, Vc, F, face_rec, vnormals);
    return (int)hipGetLastError();
}

extern "C" int rih_render_raster(const float* face_rec, int B, int F, int H, int W, int cam_kind, int32_t* pix_to_face,
                                 float* zbuf, float* bary, void* stream) {
    if (!face_rec || !pix_to_face || !zbuf || !bary || bad_size(B, F, H, W) ||
        (cam_kind != RIH_CAM_ORTHOGRAPHIC && cam_kind != RIH_CAM_PERSPECTIVE))
        return RIH_EINVAL;
    const int tiles = (H + TILE - 1) / TILE;
    hipLaunchKernelGGL(raster_kernel, dim3((unsigned)(tiles * tiles), B), dim3(RTPB), 0, (hipStream_t)stream, face_rec, F, H,
                       tiles, cam_kind == RIH_CAM_PERSPECTIVE ? 1 : 0, pix_to_face, zbuf, bary);
    return (int)hipGetLastError();
}

extern "C" int rih_mask_iou(const float* face_rec, int B, int F, int F_left, int H, int W, int cam_kind, int32_t* counts,
                            float* iou, uint8_t* mask, void* stream) {
    if (!face_rec || !counts || bad_size(B, F, H, W) || F_left < 0 || F_left > F ||
        (cam_kind != RIH_CAM_ORTHOGRAPHIC && cam_kind != RIH_CAM_PERSPECTIVE))
        return RIH_EINVAL;
    const int tiles = (H + TILE - 1) / TILE;
    hipLaunchKernelGGL(mask_zero_kernel, dim3((unsigned)((3 * B + STPB - 1) / STPB)), dim3(STPB), 0, (hipStream_t)stream,
                       counts, 3 * B);
    hipLaunchKernelGGL(mask_iou_kernel, dim3((unsigned)(tiles * tiles), B), dim3(RTPB), 0, (hipStream_t)stream, face_rec, F,
                       F_left, H, tiles, cam_kind == RIH_CAM_PERSPECTIVE ? 1 : 0, counts, mask);
    if (iou)
        hipLaunchKernelGGL(mask_ratio_kernel, dim3((unsigned)((B + STPB - 1) / STPB)), dim3(STPB), 0, (hipStream_t)stream,
                           counts, B, iou);
    return (int)hipGetLastError();
}

extern "C" int rih_render_shade(const int32_t* pix_to_face, const float* bary, const float* verts, const int32_t* faces,
                                const float* vnormals, const float* colors, const float* cams, int light_kind, int B, int V,
                                int F, int H, int W, float* rgba, void* stream) {
    if (!pix_to_face || !bary || !faces || !colors || !rgba || bad_size(B, F, H, W) || V < 1 ||
        (light_kind != RIH_LIGHT_POINT && light_kind != RIH_LIGHT_AMBIENT) ||
        (light_kind == RIH_LIGHT_POINT && (!verts || !vnormals || !cams)))
        return RIH_EINVAL;
    const long long px = (long long)H * W;
    hipLaunchKernelGGL(shade_kernel, dim3((unsigned)((px + STPB - 1) / STPB), B), dim3(STPB), 0, (hipStream_t)stream,
                       pix_to_face, bary, verts, faces, vnormals, colors, cams, light_kind == RIH_LIGHT_AMBIENT ? 1 : 0, V,
                       F, H, rgba);
    return (int)hipGetLastError();
}
