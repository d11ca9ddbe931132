// rih_collision.hip -- the collision gate behind the pose optimiser (pose_data_optimize/collision/CollisionFilter.py and
// CollisionCheck.py rebuild both hand meshes per frame and ask FCL for contacts) for gfx950: from the two hands' vertices to the
// number of INTERSECTING TRIANGLE PAIRS per frame, per main face and per sub face, one launch for a batch of frames, all integers.
//
// The predicate (the contract of this kernel, of renderih_amd.collision's mirror and of the tests' oracle):
//   orient(a,b,c,d) = dot(cross(b - a, c - a), d - a).
//   An edge (p,q) pierces a triangle (a,b,c) when orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs (by
//   comparisons, not by a product's sign) and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all > 0 or all < 0.
//   A pair (main face i, sub face j) intersects when one of the six edge-against-triangle tests pierces: the edges of i against
//   j, then the edges of j against i.  Everything is strict: coplanar, touching and zero-area configurations do not intersect,
//   nor does any comparison with a NaN in it.  A VOID face -- a vertex that is not finite, or a normal cross(v1 - v0, v2 - v0)
//   that is exactly zero -- has an EMPTY box and intersects nothing (without this rule the edge between the two good vertices
//   of a face with a NaN, or the long edge of a zero-area face, could still pierce).  Only pairs whose axis-aligned boxes
//   overlap (<=, on the input values, so exact in every precision) are tested; disjoint boxes cannot intersect.
//   Every difference is taken from a vertex of the pair, so the result does not degrade with the distance from the origin.
//
// One workgroup of 256 threads per (frame, tile of 256 main faces); a thread keeps its main face's box in registers and puts the
// face into LDS.  The workgroup reduces the box of its tile and the box of the sub mesh's vertices; if they are disjoint it
// stores zeros and leaves -- for a frame whose hands are apart every tile takes this path, so it is the frame-level skip and,
// for hands that touch at the fingers only, skips the tiles of the wrist as well.  Otherwise the sub faces stream through LDS in
// chunks of 256: one thread builds one record (vertices and box), records that miss the tile's box are dropped and the
// survivors compacted with an LDS atomicAdd (their order varies from run to run; every output is an integer sum, so no result
// does).  The survivors are taken in rounds of 16:
//   box tests   every thread compares its box with the round's 16 boxes -- all lanes read the same record: a broadcast, no bank
//               conflict; the 32 reads of a round are issued together, not one behind a branch on the one before -- and appends
//               the (main face, survivor) pairs that overlap to a list in LDS (at most 256 x 16 per round);
//   pair tests  the list is dealt out one pair per lane, so the six edge tests run on full wavefronts instead of on the few
//               lanes of a wavefront whose box test passed.
// A hit is counted with LDS integer atomicAdds per main face and per survivor.  Row counts leave as plain stores; column counts
// are added to pairs_sub per chunk with an integer atomicAdd; count[b] gets each tile's integer row sum (reduced in the
// workgroup) with one integer atomicAdd.  pairs_sub and count must be ZERO on entry (the Python wrapper fills them on the
// stream).  No float atomics: two runs are bit-identical.  Latency-class, as the contact search: at B = 1 seven workgroups.
// Measured against the first shape of this kernel (every thread walks the survivor list and runs the six tests itself where
// its box test passes): DESIGN.md 3.15, profiles/collision/.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/renderih_amd.h"

namespace {

constexpr int CC_TPB = 256, CC_ROUND = 16;

struct cc_vec {
    float x, y, z;
};
__device__ inline cc_vec cc_sub(cc_vec a, cc_vec b) { return cc_vec{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ inline cc_vec cc_cross(cc_vec a, cc_vec b) {
    return cc_vec{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ inline float cc_dot(cc_vec a, cc_vec b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// edge (p,q) against the triangle (a,b,c) whose normal cross(b - a, c - a) is n
__device__ inline bool cc_pierces(cc_vec p, cc_vec q, cc_vec a, cc_vec b, cc_vec c, cc_vec n) {
    const float dp = cc_dot(n, cc_sub(p, a)), dq = cc_dot(n, cc_sub(q, a));
    if (!((dp > 0.f && dq < 0.f) || (dp < 0.f && dq > 0.f))) return false;
    const cc_vec d = cc_sub(q, p), A = cc_sub(a, p), B = cc_sub(b, p), C = cc_sub(c, p);
    const float s1 = cc_dot(cc_cross(d, A), B), s2 = cc_dot(cc_cross(d, B), C), s3 = cc_dot(cc_cross(d, C), A);
    return (s1 > 0.f && s2 > 0.f && s3 > 0.f) || (s1 < 0.f && s2 < 0.f && s3 < 0.f);
}

__device__ inline bool cc_intersects(const cc_vec* m, const cc_vec* s) {
    const cc_vec ns = cc_cross(cc_sub(s[1], s[0]), cc_sub(s[2], s[0]));
    if (cc_pierces(m[0], m[1], s[0], s[1], s[2], ns) || cc_pierces(m[1], m[2], s[0], s[1], s[2], ns) ||
        cc_pierces(m[2], m[0], s[0], s[1], s[2], ns))
        return true;
    const cc_vec nm = cc_cross(cc_sub(m[1], m[0]), cc_sub(m[2], m[0]));
    return cc_pierces(s[0], s[1], m[0], m[1], m[2], nm) || cc_pierces(s[1], s[2], m[0], m[1], m[2], nm) ||
           cc_pierces(s[2], s[0], m[0], m[1], m[2], nm);
}

// the three vertices of face f and their box; a void face (see above) gets the empty box (low = +inf, high = -inf)
__device__ inline void cc_face(const float* __restrict__ verts, const int32_t* __restrict__ faces, int f, cc_vec* t, float4* lo,
                               float4* hi) {
    float sum = 0.f;
    for (int k = 0; k < 3; ++k) {
        const float* p = verts + (long long)faces[f * 3 + k] * 3;
        t[k] = cc_vec{p[0], p[1], p[2]};
        sum += (p[0] - p[0]) + (p[1] - p[1]) + (p[2] - p[2]);          // 0 for finite coordinates, NaN otherwise
    }
    const cc_vec n = cc_cross(cc_sub(t[1], t[0]), cc_sub(t[2], t[0]));
    if (sum == 0.f && (n.x != 0.f || n.y != 0.f || n.z != 0.f)) {
        *lo = make_float4(fminf(t[0].x, fminf(t[1].x, t[2].x)), fminf(t[0].y, fminf(t[1].y, t[2].y)),
                          fminf(t[0].z, fminf(t[1].z, t[2].z)), 0.f);
        *hi = make_float4(fmaxf(t[0].x, fmaxf(t[1].x, t[2].x)), fmaxf(t[0].y, fmaxf(t[1].y, t[2].y)),
                          fmaxf(t[0].z, fmaxf(t[1].z, t[2].z)), 0.f);
    } else {
        *lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
        *hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    }
}

// all six comparisons, no short cut: nothing between the operands' loads depends on an earlier comparison
__device__ inline bool cc_overlap(float4 alo, float4 ahi, float4 blo, float4 bhi) {
    return (alo.x <= bhi.x) & (blo.x <= ahi.x) & (alo.y <= bhi.y) & (blo.y <= ahi.y) & (alo.z <= bhi.z) & (blo.z <= ahi.z);
}

__device__ inline void cc_put(float* r, const cc_vec* t) {
    r[0] = t[0].x, r[1] = t[0].y, r[2] = t[0].z, r[3] = t[1].x, r[4] = t[1].y, r[5] = t[1].z;
    r[6] = t[2].x, r[7] = t[2].y, r[8] = t[2].z;
}

__global__ __launch_bounds__(CC_TPB) void collision_count_kernel(
    const float* __restrict__ verts_main, const float* __restrict__ verts_sub, const int32_t* __restrict__ faces_main,
    const int32_t* __restrict__ faces_sub, int32_t* __restrict__ pairs_main, int32_t* __restrict__ pairs_sub,
    int32_t* __restrict__ count, int Vm, int Vs, int Fm, int Fs, int tiles) {
    // the tile's main faces and the chunk's surviving sub faces: 9 floats each (an odd stride: the pair tests gather them);
    // the survivors' boxes; the round's (main face << 8 | survivor) pairs
    __shared__ float mrec[CC_TPB * 9], srec[CC_TPB * 9];
    __shared__ float4 slo[CC_TPB], shi[CC_TPB];
    __shared__ unsigned plist[CC_TPB * CC_ROUND];
    __shared__ float red[(CC_TPB / 64) * 12];
    __shared__ unsigned row[CC_TPB], col[CC_TPB], slot[CC_TPB], wsum[CC_TPB / 64], nsurv, npairs[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x / tiles;
    const int i = (int)(blockIdx.x % tiles) * CC_TPB + tid;
    const float* vm = verts_main + b * Vm * 3;
    const float* vs = verts_sub + b * Vs * 3;
    const bool mine = i < Fm;

    // this thread's main face; box[0..6) of the tile's faces, box[6..12) of the sub mesh's vertices (NaNs drop out of fminf)
    cc_vec m[3] = {};
    float4 mlo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), mhi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (mine) cc_face(vm, faces_main, i, m, &mlo, &mhi);
    cc_put(mrec + tid * 9, m);
    row[tid] = 0;
    float box[12] = {mlo.x, mlo.y, mlo.z, mhi.x, mhi.y, mhi.z, INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int v = tid; v < Vs; v += CC_TPB)
        for (int c = 0; c < 3; ++c) {
            box[6 + c] = fminf(box[6 + c], vs[(long long)v * 3 + c]);
            box[9 + c] = fmaxf(box[9 + c], vs[(long long)v * 3 + c]);
        }
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const bool low = k % 6 < 3;
        for (int s = 32; s > 0; s >>= 1) {
            const float o = __shfl_xor(box[k], s);
            box[k] = low ? fminf(box[k], o) : fmaxf(box[k], o);
        }
        if (lane == 0) red[wave * 12 + k] = box[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const bool low = k % 6 < 3;
        box[k] = red[k];
        for (int w = 1; w < CC_TPB / 64; ++w) box[k] = low ? fminf(box[k], red[w * 12 + k]) : fmaxf(box[k], red[w * 12 + k]);
    }
    const float4 tlo = make_float4(box[0], box[1], box[2], 0.f), thi = make_float4(box[3], box[4], box[5], 0.f);
    if (!cc_overlap(tlo, thi, make_float4(box[6], box[7], box[8], 0.f), make_float4(box[9], box[10], box[11], 0.f))) {
        if (mine) pairs_main[b * Fm + i] = 0;                // the same in every thread: the tile cannot touch the sub mesh
        return;
    }

    for (int c0 = 0; c0 < Fs; c0 += CC_TPB) {
        if (tid == 0) nsurv = 0, npairs[0] = 0, npairs[1] = 0;
        col[tid] = 0;
        slo[tid] = make_float4(INFINITY, INFINITY, INFINITY, 0.f);      // past the survivors: boxes that overlap nothing
        shi[tid] = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
        __syncthreads();
        const int j = c0 + tid;
        if (j < Fs) {
            cc_vec s[3];
            float4 lo, hi;
            cc_face(vs, faces_sub, j, s, &lo, &hi);
            if (cc_overlap(lo, hi, tlo, thi)) {
                const unsigned at = atomicAdd(&nsurv, 1u);
                cc_put(srec + at * 9, s);
                slo[at] = lo;
                shi[at] = hi;
                slot[at] = (unsigned)tid;
            }
        }
        __syncthreads();
        const int n = (int)nsurv;
        // rounds of CC_ROUND survivors: at most CC_TPB * CC_ROUND pairs pass the box test, which is what plist holds.  n is the
        // same in every thread, so are the barriers.  The two counters alternate: a round's is zeroed during the next round's
        // pair tests, a barrier after its last reader and a barrier before its next writer.
        for (int k0 = 0, q = 0; k0 < n; k0 += CC_ROUND, q ^= 1) {
            if (mine) {
#pragma unroll
                for (int kk = 0; kk < CC_ROUND; ++kk)        // k0 + kk <= 255; records in [n, 256) hold the empty box
                    if (cc_overlap(mlo, mhi, slo[k0 + kk], shi[k0 + kk]))
                        plist[atomicAdd(&npairs[q], 1u)] = (unsigned)(tid << 8 | (k0 + kk));
            }
            __syncthreads();
            const int np = (int)npairs[q];
            if (tid == 0) npairs[q ^ 1] = 0;
            for (int t = tid; t < np; t += CC_TPB) {
                const unsigned p = plist[t];
                const float *a = mrec + (p >> 8) * 9, *r = srec + (p & 255u) * 9;
                const cc_vec mm[3] = {{a[0], a[1], a[2]}, {a[3], a[4], a[5]}, {a[6], a[7], a[8]}};
                const cc_vec s[3] = {{r[0], r[1], r[2]}, {r[3], r[4], r[5]}, {r[6], r[7], r[8]}};
                if (cc_intersects(mm, s)) {
                    atomicAdd(&row[p >> 8], 1u);
                    atomicAdd(&col[slot[p & 255u]], 1u);
                }
            }
            __syncthreads();
        }
        if (j < Fs && col[tid]) atomicAdd((unsigned*)pairs_sub + (b * Fs + j), col[tid]);
    }
    unsigned hits = row[tid];                                // complete: the last round ended in a barrier
    if (mine) pairs_main[b * Fm + i] = (int32_t)hits;
    for (int s = 32; s > 0; s >>= 1) hits += __shfl_xor(hits, s);
    if (lane == 0) wsum[wave] = hits;
    __syncthreads();
    if (tid == 0) {
        unsigned total = 0;
        for (int w = 0; w < CC_TPB / 64; ++w) total += wsum[w];
        if (total) atomicAdd((unsigned*)count + b, total);
    }
}

}  // namespace

extern "C" int rih_collision_count(const float* verts_main, const float* verts_sub, const int32_t* faces_main,
                                   const int32_t* faces_sub, int32_t* pairs_main, int32_t* pairs_sub, int32_t* count, int B,
                                   int Vm, int Vs, int Fm, int Fs, void* stream) {
    if (!verts_main || !verts_sub || !faces_main || !faces_sub || !pairs_main || !pairs_sub || !count) return RIH_EINVAL;
    if (B < 1 || Vm < 1 || Vs < 1 || Fm < 1 || Fs < 1) return RIH_EINVAL;
    const long long tiles = ((long long)Fm + CC_TPB - 1) / CC_TPB;
    if (tiles * B > 0x7fffffffLL) return RIH_EINVAL;
    hipLaunchKernelGGL(collision_count_kernel, dim3((unsigned)(tiles * B)), dim3(CC_TPB), 0, (hipStream_t)stream, verts_main,
                       verts_sub, faces_main, faces_sub, pairs_main, pairs_sub, count, Vm, Vs, Fm, Fs, (int)tiles);
    return (int)hipGetLastError();
}
