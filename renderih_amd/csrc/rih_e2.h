// rih_e2.h -- the engine-2 toolkit shared by rih_gemm.hip and rih_conv3.hip: each piece of the arithmetic exists here once.
//
// ENGINE 2: fp32 operands are scaled by a power of two s (so that s * max|x| lies in [2^14, 2^15), well inside the fp16 range)
// and split on the way into LDS into TWO fp16 planes, hi = fp16(s x) and lo = fp16((s x - hi) * 2^11) (round-to-nearest both;
// |s x - hi - 2^-11 lo| <= 2^-23 |s x|, and lo keeps its 11 bits down to |s x| = 2^-14 * 2^-11 thanks to the 2^11 pre-scale --
// the error-corrected tensor-core SGEMM scheme of Ootomo & Yokota).  The product is formed with THREE v_mfma_f32_32x32x16_f16
// per 32x32x16 block: hi*hi into one fp32 accumulator, hi*lo + lo*hi into a second one; the epilogue combines
// acc0 + 2^-11 acc1 and undoes the operand scales (exact: powers of two).  The dropped lo*lo term is <= 2^-22 relative.  Half
// the matrix-pipe work (and energy) per fp32 FLOP of the six-product bf16 engine: 2.5 PF / 3 = 833 TF.
// The kernels on this engine agree bit for bit per product because they share what is here: the scale derivation, the split,
// the order of the three products, the fold of the epilogue and the BatchNorm statistics.  The operand side is functions; the
// MFMA step, the fold and the statistics are macros (RIH_E2_*), which expand inside the kernel and leave its code as it was
// when they were written out there (profiles/e2_common/README.md).  Not yet shared: the wide epilogue around them.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/renderih_amd.h"

namespace {         // (internal linkage, as in the including files; the anonymous namespaces of a translation unit are one)

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

constexpr unsigned OOB = 0x80000000u;       // buffer-load offset that the hardware range check answers with zeros

// bijective "each XCD gets a contiguous chunk" remap of the workgroup id (blocks are dispatched round-robin over 8 XCDs)
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t r, unsigned off) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// The scale comes from a device-resident upper bound of max|x| (a bound block written by the kernel that produced the operand,
// or by rih_absmax; NULL = 1.0): any upper bound is correct, a loose one only costs range at the bottom (full 22-bit precision
// for |x| >= 2^-29 * bound).
__device__ __forceinline__ float e2_scale(const float* amax, bool at_least_one = false) {
    if (amax == nullptr) return 1.f;
    // the bound block: 64 partial maxima, one per 128-byte line (include/renderih_amd.h: rih_absmax) -- one vector load per
    // wavefront and an xor-shuffle maximum; the result is wave-uniform
    float a = amax[(threadIdx.x & 63) * (RIH_BOUND_FLOATS / 64)];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o, 64));
    a = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(a)));
    if (at_least_one) a = fmaxf(a, 1.f);            // the all-ones row of a weight-gradient's A operand must stay in range
    const int e = (int)((__float_as_uint(a) >> 23) & 0xffu);
    if (e == 0 || e == 255) return 1.f;             // zero / denormal bound (an all-zero operand), or inf / NaN (garbage either way)
    int se = 268 - e;                               // 2^(14 - (e - 127)), biased
    se = se > 253 ? 253 : se;                       // keep 1/s a normal number
    return __uint_as_float((unsigned)se << 23);
}
__device__ __forceinline__ unsigned e2_pk_f16(float a, float b) {
    const f16x2 v = {(_Float16)a, (_Float16)b};     // RNE; a in the low half
    return __builtin_bit_cast(unsigned, v);
}
// (a, b) * s -> packed fp16 hi pair h and packed fp16 pair l of the 2^11-scaled residuals.  Six mixed-precision FMAs per pair
// (hipcc's own selection for the C form below takes ten): the f16 result of v_fma_mix{lo,hi}_f16 is the RNE conversion of the
// exact product (a power-of-two scaling), v_fma_mix_f32 reads the f16 half back as an addend, so the residual a*s - hi is one
// instruction and exact.
#define RIH_E2_SPLIT(ASM_)                                                                                                  \
    float ra, rb;                                                                                                           \
    const float k2048 = 2048.f;                                                                                             \
    ASM_("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h) : "v"(a), "s"(s));                                                       \
    ASM_("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h) : "v"(b), "s"(s));                                                       \
    ASM_("v_fma_mix_f32 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(ra) : "v"(a), "s"(s), "v"(h));                            \
    ASM_("v_fma_mix_f32 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(rb) : "v"(b), "s"(s), "v"(h));             \
    ASM_("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(l) : "v"(ra), "s"(k2048));                                                  \
    ASM_("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(l) : "v"(rb), "s"(k2048));
__device__ __forceinline__ void e2_split2h(float a, float b, float s, unsigned& h, unsigned& l) {
#if defined(__HIP_DEVICE_COMPILE__)
    RIH_E2_SPLIT(asm)
#else       /* host build of tests/hipcpu: the same arithmetic in C */
    a *= s;
    b *= s;
    const f16x2 hv = {(_Float16)a, (_Float16)b};
    h = __builtin_bit_cast(unsigned, hv);
    l = e2_pk_f16((a - (float)hv.x) * 2048.f, (b - (float)hv.y) * 2048.f);     // the differences are exact in fp32
#endif
}
// e2_split2h pinned in program order (volatile), for a kernel that places the conversion behind a wait of its own (rows_kernel)
__device__ __forceinline__ void e2_split2h_pinned(float a, float b, float s, unsigned& h, unsigned& l) {
#if defined(__HIP_DEVICE_COMPILE__)
    RIH_E2_SPLIT(asm volatile)
#else
    e2_split2h(a, b, s, h, l);
#endif
}
#undef RIH_E2_SPLIT

constexpr int SLD = 36;             // floats per row of the epilogue's staging area: 32 + pad, keeps float4 alignment (RIH_E2_STAGE)

}  // namespace

// ---------------------------------------------------------------------------------------------------- MFMA step
// One 16-deep k-step of a wave tile of TM_ x TN_ 32x32 blocks: AV_ / BV_ = f16x8 [plane hi, lo][block], ACC_ / ACC1_ =
// floatx16 [TM_][TN_].  acc1 += lo*hi, acc += hi*hi, acc1 += hi*lo, each over all blocks: the ORDER is part of the contract.
#define RIH_E2_MMA1(TM_, TN_, AV_, BV_, ACC_, PA_, PB_)                                                                      \
    _Pragma("unroll") for (int i = 0; i < TM_; ++i) _Pragma("unroll") for (int jj = 0; jj < TN_; ++jj) ACC_[i][jj] =        \
        __builtin_amdgcn_mfma_f32_32x32x16_f16(AV_[PA_][i], BV_[PB_][jj], ACC_[i][jj], 0, 0, 0);
#define RIH_E2_MMA3(TM_, TN_, AV_, BV_, ACC_, ACC1_)                                                                         \
    RIH_E2_MMA1(TM_, TN_, AV_, BV_, ACC1_, 1, 0)                                                                            \
    RIH_E2_MMA1(TM_, TN_, AV_, BV_, ACC_, 0, 0)                                                                             \
    RIH_E2_MMA1(TM_, TN_, AV_, BV_, ACC1_, 0, 1)

// ---------------------------------------------------------------------------------------------------- epilogue
// Stage one 32x32 block (ACC_, ACC1_: floatx16) into a wave's 32 x PITCH_ floats of LDS, row-major: (acc + 2^-11 acc1) * inv_a *
// inv_b -- the correction accumulator folded in, the operand scales undone one after the other (exact powers of two).  L31_ =
// lane & 31, LHI_ = lane >> 5.  The caller orders the wavefront around it (__builtin_amdgcn_wave_barrier).
#define RIH_E2_STAGE(STG_, PITCH_, ACC_, ACC1_, INVA_, INVB_, L31_, LHI_)                                                    \
    _Pragma("unroll") for (int r = 0; r < 16; ++r)                                                                          \
        STG_[((r & 3) + 8 * (r >> 2) + 4 * (LHI_)) * (PITCH_) + (L31_)] = fmaf(ACC1_[r], 0x1p-11f, ACC_[r]) * (INVA_) * (INVB_);

// Per-column BatchNorm statistics of the float4 a lane stores per row in the wide epilogue.  RIH_E2_STATS_DECL declares, per
// column block j < TN_ (one dummy block where STATS_ is false: no registers, no code), the shift ssh (the lane's first stored
// row), the sums ssum / ssq of (v - shift) and of its square, and the row count scnt; RIH_E2_STATS_ADD adds a stored float4.
// RIH_E2_STATS_MERGE declares MEAN_ and M2_, the (mean, centred sum of squares) per column over the wave's rows: shifted sums
// per lane, then Chan's pairwise merge over the eight row-lanes (lane >> 3; xor-shuffle rounds o = 8, 16, 32) -- no
// E[x^2] - mean^2 cancellation.  Lane >> 3 == 0 then writes them, in the format of rih_gemm_desc.stats, which
// rih_bn_stats_from_blocks merges in double.
#define RIH_E2_STATS_DECL(STATS_, TN_)                                                                                       \
    float4 ssh[STATS_ ? TN_ : 1], ssum[STATS_ ? TN_ : 1], ssq[STATS_ ? TN_ : 1];                                            \
    float scnt[STATS_ ? TN_ : 1];                                                                                           \
    if (STATS_) {                                                                                                           \
        _Pragma("unroll") for (int j = 0; j < TN_; ++j) {                                                                   \
            ssh[j] = make_float4(0, 0, 0, 0); ssum[j] = make_float4(0, 0, 0, 0); ssq[j] = make_float4(0, 0, 0, 0);          \
            scnt[j] = 0.f;                                                                                                  \
        }                                                                                                                   \
    }
#define RIH_E2_STATS_ADD(J_, V_)                                                                                             \
    {                                                                                                                       \
        if (scnt[J_] == 0.f) ssh[J_] = V_;                                                                                  \
        scnt[J_] += 1.f;                                                                                                    \
        const float dx = V_.x - ssh[J_].x, dy = V_.y - ssh[J_].y, dz = V_.z - ssh[J_].z, dw = V_.w - ssh[J_].w;             \
        ssum[J_].x += dx; ssum[J_].y += dy; ssum[J_].z += dz; ssum[J_].w += dw;                                             \
        ssq[J_].x += dx * dx; ssq[J_].y += dy * dy; ssq[J_].z += dz * dz; ssq[J_].w += dw * dw;                             \
    }
#define RIH_E2_CHAN1(MEAN_, M2_, c_)                                                                                         \
    {                                                                                                                       \
        const float mb = __shfl_xor(MEAN_.c_, o, 64), qb = __shfl_xor(M2_.c_, o, 64);                                       \
        const float dl = mb - MEAN_.c_;                                                                                     \
        MEAN_.c_ += dl * wb;                                                                                                \
        M2_.c_ += qb + dl * dl * cf;                                                                                        \
    }
#define RIH_E2_STATS_MERGE(J_, MEAN_, M2_)                                                                                   \
    float n = scnt[J_];                                                                                                     \
    const float inv = n > 0.f ? 1.f / n : 0.f;                                                                              \
    float4 MEAN_ = make_float4(ssh[J_].x + ssum[J_].x * inv, ssh[J_].y + ssum[J_].y * inv, ssh[J_].z + ssum[J_].z * inv,    \
                               ssh[J_].w + ssum[J_].w * inv);                                                               \
    float4 M2_ = make_float4(ssq[J_].x - ssum[J_].x * ssum[J_].x * inv, ssq[J_].y - ssum[J_].y * ssum[J_].y * inv,          \
                             ssq[J_].z - ssum[J_].z * ssum[J_].z * inv, ssq[J_].w - ssum[J_].w * ssum[J_].w * inv);         \
    _Pragma("unroll") for (int o = 8; o < 64; o <<= 1) {                                                                    \
        const float nb = __shfl_xor(n, o, 64);                                                                              \
        const float nt = n + nb;                                                                                            \
        const float wb = nt > 0.f ? nb / nt : 0.f;          /* weight of the partner's mean */                              \
        const float cf = n * wb;                            /* n * nb / nt */                                               \
        RIH_E2_CHAN1(MEAN_, M2_, x) RIH_E2_CHAN1(MEAN_, M2_, y) RIH_E2_CHAN1(MEAN_, M2_, z) RIH_E2_CHAN1(MEAN_, M2_, w)     \
        n = nt;                                                                                                             \
    }
