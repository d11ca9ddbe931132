// rih_sdf_loss.hip -- the two-hand penetration term of the reference's pose optimiser
// (pose_data_optimize/code_sdf/sdf_template.py:19-157 `NewLoss`) around the voxeliser of rih_sdf.hip: each hand of a sample
// is voxelised in its own padded cube and the OTHER hand's vertices sample that field (trilinear, align_corners = True, zero
// padding).  Three kernels here, the voxeliser (rih_sdf_sparse or rih_sdf) runs between the first two:
//   prep    one workgroup per (sample, hand): bounding box by an LDS min / max reduction, centre and scale, the normalised
//           vertices; then the voxels the other hand's vertices will read are marked with plain same-value byte stores and
//           compacted into an ascending list (a count per thread, a serial scan of the 256 counts, no atomics).
//   sample  one workgroup per sample: both hands' weighted samples, their gradient with respect to the sampled vertex
//           (stashed for the backward) and the sample's loss, summed in a fixed order.
//   bwd     elementwise: the stashed gradient times the upstream gradients of whichever outputs were used.
// The sample index ((p + 1) / 2) (G - 1) of a vertex is computed by ONE function (cell_of) for marking and for sampling, so
// that the sampler reads exactly the voxels the sparse voxeliser wrote.  fp32 VALU work on a few thousand elements per
// sample: latency-bound launches, no MFMA.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"

namespace {

constexpr int TPB = 256;

// Where vertex v samples the cube {centre, scale}: fractional voxel index per axis (x -> i, y -> j, z -> k of phi[k][j][i])
// and its floor.  `ok` is false when no corner of the cell can lie inside the grid (also for a non-finite index).
struct Cell { float f[3]; int i0[3]; bool ok; };

__device__ __forceinline__ Cell cell_of(const float* v, const float* box, int G) {
    Cell q;
    q.ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = (v[a] - box[a]) / box[3];
        q.f[a] = ((p + 1.f) / 2.f) * (float)(G - 1);
        const bool in = q.f[a] > -1.f && q.f[a] < (float)G;
        q.i0[a] = in ? (int)floorf(q.f[a]) : -2;
        q.ok = q.ok && in;
    }
    return q;
}

__global__ __launch_bounds__(TPB) void prep_kernel(const float* __restrict__ vertices, float scale_mul, float* __restrict__ box,
                                                   float* __restrict__ vnorm, uint8_t* __restrict__ flags,
                                                   int32_t* __restrict__ list, int32_t* __restrict__ count, int V, int G,
                                                   int max_count) {
    __shared__ float red[6][TPB];
    __shared__ int cnt[TPB];
    __shared__ float sbox[4];
    const int m = blockIdx.x, t = threadIdx.x;
    const int vox = G * G * G;
    const float* vm = vertices + (long long)m * V * 3;
    const float* vo = vertices + (long long)(m ^ 1) * V * 3;        // the other hand of the same sample
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int v = t; v < V; v += TPB)
#pragma unroll
        for (int a = 0; a < 3; ++a) { const float x = vm[3 * v + a]; lo[a] = fminf(lo[a], x); hi[a] = fmaxf(hi[a], x); }
#pragma unroll
    for (int a = 0; a < 3; ++a) { red[a][t] = lo[a]; red[3 + a][t] = hi[a]; }
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                red[a][t] = fminf(red[a][t], red[a][t + s]);
                red[3 + a][t] = fmaxf(red[3 + a][t], red[3 + a][t + s]);
            }
        __syncthreads();
    }
    if (t == 0) {
        float ext = -INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a) { sbox[a] = (red[a][0] + red[3 + a][0]) / 2.f; ext = fmaxf(ext, red[3 + a][0] - red[a][0]); }
        sbox[3] = scale_mul * ext;
#pragma unroll
        for (int a = 0; a < 4; ++a) box[4 * m + a] = sbox[a];
    }
    for (int i = t; i < vox; i += TPB) flags[(long long)m * vox + i] = 0;
    __syncthreads();
    const float bx[4] = {sbox[0], sbox[1], sbox[2], sbox[3]};
    for (int e = t; e < 3 * V; e += TPB) vnorm[(long long)m * V * 3 + e] = (vm[e] - bx[e % 3]) / bx[3];
    for (int v = t; v < V; v += TPB) {
        const Cell q = cell_of(vo + 3 * v, bx, G);
        if (!q.ok) continue;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int i = q.i0[0] + (d & 1), j = q.i0[1] + ((d >> 1) & 1), k = q.i0[2] + (d >> 2);
            if (i >= 0 && i < G && j >= 0 && j < G && k >= 0 && k < G) flags[(long long)m * vox + (k * G + j) * G + i] = 1;
        }
    }
    __syncthreads();
    // compaction: thread t owns the voxels [t * per, (t + 1) * per)
    const int per = (vox + TPB - 1) / TPB;
    const int beg = min(vox, t * per), end = min(vox, beg + per);
    int n = 0;
    for (int i = beg; i < end; ++i) n += flags[(long long)m * vox + i];
    cnt[t] = n;
    __syncthreads();
    if (t == 0) {
        int run = 0;
        for (int i = 0; i < TPB; ++i) { const int c = cnt[i]; cnt[i] = run; run += c; }
        count[m] = min(run, max_count);
    }
    __syncthreads();
    int pos = cnt[t];
    for (int i = beg; i < end; ++i)
        if (flags[(long long)m * vox + i]) {
            if (pos < max_count) list[(long long)m * max_count + pos] = i;
            ++pos;
        }
}

__global__ __launch_bounds__(TPB) void sample_kernel(const float* __restrict__ phi, const float* __restrict__ vertices,
                                                     const float* __restrict__ box, const int32_t* __restrict__ weight,
                                                     float* __restrict__ per_vert, float* __restrict__ ori,
                                                     float* __restrict__ grad, float* __restrict__ loss, int V, int G) {
    __shared__ float red[TPB];
    const int b = blockIdx.x, t = threadIdx.x;
    const int vox = G * G * G;
    const float gmul = (float)(G - 1) / 2.f;
    float acc = 0.f;
    for (int e = t; e < 2 * V; e += TPB) {
        const int s = e / V, v = e - s * V;                  // s = 0: LEFT vertices (hand 1) in the right hand's field (mesh 2b)
        const int fm = 2 * b + s;
        const float* bx = box + 4 * fm;
        const float* ph = phi + (long long)fm * vox;
        const Cell q = cell_of(vertices + ((long long)(2 * b + 1 - s) * V + v) * 3, bx, G);
        float val = 0.f, g[3] = {0.f, 0.f, 0.f};
        if (q.ok) {
            float w0[3], w1[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) { w1[a] = q.f[a] - (float)q.i0[a]; w0[a] = (float)(q.i0[a] + 1) - q.f[a]; }
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
                const int i = q.i0[0] + dx, j = q.i0[1] + dy, k = q.i0[2] + dz;
                if (i >= 0 && i < G && j >= 0 && j < G && k >= 0 && k < G) {
                    const float p = ph[(k * G + j) * G + i];
                    const float wx = dx ? w1[0] : w0[0], wy = dy ? w1[1] : w0[1], wz = dz ? w1[2] : w0[2];
                    val += p * wx * wy * wz;
                    g[0] += (dx ? p : -p) * wy * wz;
                    g[1] += (dy ? p : -p) * wx * wz;
                    g[2] += (dz ? p : -p) * wx * wy;
                }
            }
        }
        const float wv = (float)weight[v];
        const long long o = (long long)b * 2 * V + e;
        const float pv = wv * val * 0.25f;
        per_vert[o] = pv;
        ori[o] = wv * val * bx[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) grad[3 * o + a] = wv * (g[a] * gmul) / bx[3];
        acc += pv;
    }
    red[t] = acc;
    __syncthreads();
    for (int s = TPB / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) loss[b] = red[0];
}

__global__ __launch_bounds__(TPB) void bwd_kernel(const float* __restrict__ grad, const float* __restrict__ box,
                                                  const float* __restrict__ g_loss, const float* __restrict__ g_pv,
                                                  const float* __restrict__ g_ori, float* __restrict__ g_vertices, int V,
                                                  long long n) {
    const long long o = (long long)blockIdx.x * TPB + threadIdx.x;     // (b, s, v) of the stash
    if (o >= n) return;
    const int v = (int)(o % V), s = (int)((o / V) % 2);
    const long long b = o / (2 * V);
    float coef = 0.f;
    if (g_loss) coef += g_loss[b] * 0.25f;
    if (g_pv) coef += g_pv[o] * 0.25f;
    if (g_ori) coef += g_ori[o] * box[4 * (2 * b + s) + 3];
    const long long dst = ((2 * b + 1 - s) * V + v) * 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) g_vertices[dst + a] = grad[3 * o + a] * coef;
}

}  // namespace

extern "C" int rih_two_hand_prep(const float* vertices, float scale_mul, float* box, float* vnorm, uint8_t* flags,
                                 int32_t* list, int32_t* count, int bs, int V, int G, int max_count, void* stream) {
    if (!vertices || !box || !vnorm || !flags || !list || !count || bs < 1 || bs > (1 << 20) || V < 3 || V > (1 << 20) ||
        G < 2 || G > 256 || max_count < 1)
        return RIH_EINVAL;
    const long long vox = (long long)G * G * G, need = vox < 8LL * V ? vox : 8LL * V;
    if (max_count < need || max_count > vox) return RIH_EINVAL;
    hipLaunchKernelGGL(prep_kernel, dim3(2 * bs), dim3(TPB), 0, (hipStream_t)stream, vertices, scale_mul, box, vnorm, flags,
                       list, count, V, G, max_count);
    return (int)hipGetLastError();
}

extern "C" int rih_two_hand_sample(const float* phi, const float* vertices, const float* box, const int32_t* weight,
                                   float* per_vert, float* ori, float* grad, float* loss, int bs, int V, int G, void* stream) {
    if (!phi || !vertices || !box || !weight || !per_vert || !ori || !grad || !loss || bs < 1 || bs > (1 << 20) || V < 3 ||
        V > (1 << 20) || G < 2 || G > 256)
        return RIH_EINVAL;
    hipLaunchKernelGGL(sample_kernel, dim3(bs), dim3(TPB), 0, (hipStream_t)stream, phi, vertices, box, weight, per_vert, ori,
                       grad, loss, V, G);
    return (int)hipGetLastError();
}

extern "C" int rih_two_hand_bwd(const float* grad, const float* box, const float* g_loss, const float* g_pv, const float* g_ori,
                                float* g_vertices, int bs, int V, void* stream) {
    if (!grad || !box || !g_vertices || bs < 1 || bs > (1 << 20) || V < 3 || V > (1 << 20)) return RIH_EINVAL;
    const long long n = 2LL * bs * V;
    hipLaunchKernelGGL(bwd_kernel, dim3((unsigned)((n + TPB - 1) / TPB)), dim3(TPB), 0, (hipStream_t)stream, grad, box, g_loss,
                       g_pv, g_ori, g_vertices, V, n);
    return (int)hipGetLastError();
}
