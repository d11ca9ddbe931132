/*
 * renderih_amd.h -- C ABI of librenderih_amd.so (MI355X / gfx950 hot-path kernels).
 *
 * The reference (adwardlee/RenderIH) has no native boundary on this path: its hot path is
 * torch operators called from Python (models/encoder.py, models/model_attn/{gcn,self_attn,img_attn,inter_attn,DualGraph}.py, models/decoder.py,
 * models/manolayer.py), which dispatch to cuDNN/cuBLAS.  This header is the boundary a maintainer
 * binds instead (ctypes stub in INTEGRATION.md): each entry point names the reference op group
 * (file:line) it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (or int32 where said) owned by the caller
 *     (PyTorch's caching allocator); the library never allocates or frees device memory;
 *   - `stream` is a hipStream_t passed as void*; every call only enqueues work on it, no host sync;
 *   - return value: 0 = ok, otherwise a hipError_t (>0) or a negative argument-check code;
 *     no C++ exception crosses the ABI;
 *   - activations are NHWC ("pixels x channels", channel fastest); a matrix is the H=W=1 case.
 */
#ifndef RENDERIH_AMD_H
#define RENDERIH_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RIH_OK 0
#define RIH_EINVAL (-1)

/* ------------------------------------------------------------------------------------------------
 * rih_gemm: C = epilogue(alpha * A (*) B), fp32 in / fp32 out / fp32 accumulate on one of three MFMA engines (field `engine`):
 * 0 = native v_mfma_f32_32x32x2_f32, 1 = six bf16 products (v_mfma_f32_32x32x16_bf16), 2 (default where both operands have bounds) =
 * three fp16 products on a scaled two-term split (v_mfma_f32_32x32x16_f16).
 *
 * One kernel family covers every dense contraction of the path:
 *   conv2d forward / data-gradient (A gathered im2col-style from an NHWC tensor)
 *       replaces torch conv2d in models/encoder.py:52,112-116,172 + torchvision resnet50,
 *       models/model_attn/img_attn.py:62 (patch conv)
 *   conv2d / linear weight-gradient (A = im2col^T, split-K over pixels)
 *   nn.Linear forward/backward          models/model_attn/{gcn.py:66,self_attn.py:66-76,inter_attn.py:85-107}
 *   attention QK^T, PV and their gradients (two-level batch strides = batch x head)
 *       models/model_attn/self_attn.py:70-74, inter_attn.py:93-107
 *
 * a_mode 0: A(m,k): m = (img,ho,wo) output pixel, k = (kh,kw,ci); element =
 *           X[img][(ho*strideA - padH + kh)/upS][(wo*strideA - padW + kw)/upS][ci]  (0 when out of range or
 *           not divisible by upS; upS>1 expresses the data-gradient of a strided conv).  K-contiguous.
 * a_mode 1: A(m,k): m = (kh,kw,ci), k = (img,ho,wo) -- the transpose gather, M-contiguous (weight grad).
 * b_mode 0: B(k,n) = Bp[k*ldb + n]   (row-major [K][N])
 * b_mode 1: B(k,n) = Bp[n*ldb + k]   ([N][K], e.g. an nn.Linear / 1x1-conv weight as stored)
 * Epilogue (splitk==1): C[m*ldc+n] = act(alpha*acc + bias[n] + R[m*ldr+n]); with splitk>1 raw partial sums
 *           go to C + split*sCsplit and rih_splitk_reduce finishes.
 */
typedef struct rih_gemm_desc {
    const float* A;
    const float* B;
    float* C;
    const float* bias;   /* [N] or NULL */
    const float* R;      /* residual [M][ldr] or NULL */
    int32_t M, N, K;
    int32_t lda, ldb, ldc, ldr;
    int32_t a_mode, b_mode;
    /* batching: grid.z = nb1 * nb2 * splitk */
    int32_t nb1, nb2;
    int64_t sA1, sA2, sB1, sB2, sC1, sC2;
    int32_t splitk;      /* >= 1 */
    int32_t kchunk;      /* K range per split, multiple of 32 */
    int64_t sCsplit;
    float alpha;
    int32_t relu;
    /* im2col geometry of A (a plain matrix is H=W=Ho=Wo=KH=KW=1, strideA=upS=1, pad=0, Cin=K or M) */
    int32_t H, W, Cin, Ho, Wo, KH, KW, strideA, upS, padH, padW;
    int32_t tile;        /* 0: 128x128, 1: 128x64, 2: 64x64, 3: 128x32 (engine 0 only),
                            4: 256x128 software-pipelined (engine 1 only; operands must satisfy the split fast-path
                               preconditions documented at gemm_split_kernel, else RIH_EINVAL) */
    int32_t engine;      /* 0: native f32 MFMA (v_mfma_f32_32x32x2_f32, 157 TF peak);
                            1: fp32 emulated on the bf16 MFMA pipe: each operand split into three bf16 terms
                               (hi+mid+lo, 24 significand bits), six v_mfma_f32_32x32x16_bf16 products, fp32
                               accumulate -- same accuracy as engine 0 (error <= ~2^-23 relative per product),
                               2.5 PF / 6 = 417 TF peak.  Tiles 0,1,2 only (tile 3 always runs engine 0).
                            2: fp32 emulated on the fp16 MFMA pipe with THREE products: each operand is scaled by a power
                               of two (from amax_a / amax_b below) and split into two fp16 terms hi + 2^-11 lo (22-23
                               significand bits), hi*hi and hi*lo + lo*hi accumulate in two fp32 accumulators
                               (v_mfma_f32_32x32x16_f16), combined and un-scaled in the epilogue; 2.5 PF / 3 = 833 TF
                               peak.  Exists on the fast path of tiles 0,1,2 (a_mode / b_mode 0 or 1); a descriptor that asks
                               for it elsewhere runs engine 1 (rih_gemm_engine tells which). */
    /* Strided output rows (cS > 1; a_mode 0, splitk 1, no residual): GEMM row m = (img, i, j) over (Ho, Wo) is stored
     * to pixel (img, i*cS + cOH, j*cS + cOW) of a [*, cH, cW, ldc] tensor.  Used to compute the data gradient of a
     * stride-s convolution as s*s dense sub-convolutions, one per output parity class (each with the kernel taps
     * kh = kh0 + s*t that can reach that class, packed by rih_pack_conv_weight_sub), instead of one convolution over
     * a zero-stuffed gradient (upS) in which (s*s-1)/(s*s) of the products are structural zeros.  cS <= 1: off. */
    int32_t cS, cOH, cOW, cH, cW;
    /* a_mode 1 only: A(ones_row, k) = 1 for every k < K, whatever memory holds (rows > ones_row up to M are junk).
     * Appending this row to a weight-gradient GEMM makes C(ones_row, n) = sum_k B(k, n), the bias gradient, so that
     * no separate column-sum pass over dy is needed (rih_splitk_reduce_bias picks the row up).  0 = off. */
    int32_t ones_row;
    int32_t reserved0;   /* keeps the 64-bit fields below aligned; set 0 */
    /* Per-nb1-slice strides (in floats) of bias and R.  With nb1 = 2 and sB1 / sBias1 = the distance between the left-
     * and the right-hand parameter tensors, the two per-hand nn.Linear layers of the decoder
     * (models/model_attn/DualGraph.py:83-89 runs them one after the other) execute as ONE launch on activations
     * stacked [2][rows][K].  0 = bias / R shared by all slices. */
    int64_t sBias1, sR1;
    /* Optional statistics epilogue (split engine's fast path, a_mode 0, no split-K, no batch): per block of
     * rih_gemm_stats_rows(desc) GEMM rows the per-column mean and centred sum of squares of the stored values,
     * stats[ceil(M / rows)][2][N] -- the training statistics of the BatchNorm behind a convolution without a pass over its
     * output (rih_bn_stats_from_blocks merges them).  NULL = off.  rih_gemm returns RIH_EINVAL when stats is set and the
     * descriptor does not take that path; rih_gemm_stats_rows (stats field ignored) returns 0 for such a descriptor. */
    float* stats;
    /* Dropout in the epilogue (ABI 12; plain row-major GEMMs = nn.Linear on the split engine's fast path, no split-K, no stats):
     * C = dropout(act(alpha A B + bias)) + R with the mask stream of rih_add_dropout over the output -- element e (offset from C
     * in floats; the output is expected contiguous from C) is kept and scaled by 1 / (1 - drop_p) iff
     * rih_hash(drop_seed + *drop_seed_dev, e) >= drop_p * 2^32 -- so that rih_gemm with drop_p equals rih_gemm followed by
     * rih_add_dropout(R, ., drop_p, drop_seed, drop_seed_dev) bit for bit and rih_dropout_bwd re-draws the mask.  relu and R
     * together are refused.  drop_p = 0: off.  rih_gemm_dropout_ok(desc) tells in advance whether a descriptor takes that path
     * (rih_gemm returns RIH_EINVAL for drop_p != 0 otherwise). */
    float drop_p;
    int32_t reserved1;
    uint64_t drop_seed;
    const uint64_t* drop_seed_dev;
    /* Engine 2 only (ABI 13): DEVICE pointers to a BOUND BLOCK each (RIH_BOUND_FLOATS floats, see rih_absmax): an upper bound
     * of max|A| resp. max|B| over everything the launch reads (all batch slices).  The kernel derives the power-of-two operand
     * scale from it (s * bound in [2^14, 2^15)), so the bound is read at run time -- a step captured in a hipGraph follows the
     * data.  Any upper bound is correct: a bound 2^k too large costs k of the ~29 binades below the maximum that keep full
     * precision; a bound that is too SMALL can overflow fp16 (inf / NaN in the result).  Written by rih_absmax or by the
     * producing kernel (rih_bn_apply, rih_bn_bwd: `amax` arguments).  NULL = the operand is known to lie inside
     * [-2^15, 2^15] (scale 1). */
    const float* amax_a;
    const float* amax_b;
    /* Segmented A (ABI 13): A = [A | a_seg[0] | a_seg[1] | a_seg[2]] along K -- columns [0, k_seg[0]) come from A (pitch lda),
     * columns [k_seg[i], k_seg[i+1]) from a_seg[i] (pitch lda_seg[i]; the last piece ends at K); unused pieces NULL.  The
     * channel concatenation in front of a 1x1 convolution (models/encoder.py:165-173: `torch.cat((hms_fmaps[i], dp_fmaps[i],
     * img_fmaps[i]), dim=1)` -> conv1x1) is then read in place instead of being materialised.  Plain row-major pieces only
     * (a_mode 0 without im2col geometry), b_mode 1, one batch slice, no split-K; every k_seg a multiple of 32, pieces 16-byte
     * aligned; engines 1 and 2 on the fast path of tiles 0..2 (statistics epilogue available), RIH_EINVAL otherwise. */
    const float* a_seg[3];
    int32_t lda_seg[3];
    int32_t k_seg[3];
} rih_gemm_desc;
int rih_gemm_stats_rows(const rih_gemm_desc* d);
int rih_gemm_dropout_ok(const rih_gemm_desc* d);
/* The engine rih_gemm would run `d` on (0 / 1 / 2), or -1 for an invalid descriptor. */
int rih_gemm_engine(const rih_gemm_desc* d);
/* Bound block: RIH_BOUND_FLOATS floats = 64 partial maxima at a stride of 32 floats (one per 128-byte line; the other floats are
 * unused); THE BOUND IS THE MAXIMUM OF THE 64.  A producer merges its candidates into the lines with atomic maxima (64 lines so
 * that the same-address atomics of thousands of workgroups do not queue up behind one word), a consumer (rih_gemm engine 2) reads
 * the 64 words with one vector load per wavefront.  The caller zeroes a block (all 2048 floats, or at least the 64 words) before
 * its first producer runs; several producers may share a block.
 * rih_absmax: block <- max(block, max_i |x[i]|) over n floats (NaNs are ignored); one pass at streaming rate.
 * rih_absmax_multi: the same for n tensors in ceil(n / 120) launches (`descs` is HOST memory, read before the call returns):
 * the convolution weights of a training step. */
#define RIH_BOUND_FLOATS 2048
int rih_absmax(const float* x, int64_t n, float* out, void* stream);
typedef struct rih_absmax_desc {
    const float* x;
    float* out;             /* bound block */
    int64_t n;
} rih_absmax_desc;
int rih_absmax_multi(const rih_absmax_desc* descs, int n, void* stream);

int rih_gemm(const rih_gemm_desc* d, void* stream);

/* Grouped launch: n independent rih_gemm problems that take the SAME kernel variant run as ONE launch -- e.g. all weight
 * gradients of the decoder's nn.Linear layers of a backward stage (models/model_attn/gcn.py:99-110, self_attn.py:17-33: 116
 * GEMM launches of ~20 us per ResNet50 step, each a few hundred workgroups with short reductions) -- so that the chip stays
 * full across problems and the dependent-launch floor is paid once.  Because the problems then fill the machine together,
 * the caller can also use far fewer split-K slices per problem than a lone launch needs (less partial-slab traffic).
 *   rih_gemm_multi_variant(d): >= 0 = the variant id of a descriptor that can ride in a grouped launch (split engine's fast
 *     path; weight-gradient GEMMs a_mode 1 / b_mode 0 on 64x64 or 128x128 tiles), -1 otherwise.
 *   rih_gemm_multi_table_bytes / rih_gemm_multi_pack: size of, and fill, the launch table in HOST memory for n descriptors of
 *     one variant (returns the variant, or a negative error code; *total_blocks = grid size).  The table holds the prepared
 *     kernel arguments of every problem and a block -> problem map.
 *   rih_gemm_multi_launch(dev_table, variant, total_blocks, stream): the launch; `dev_table` = the packed table in DEVICE
 *     memory (the caller's stream-ordered copy; it must stay unchanged until the kernel has run).  No allocation, no sync. */
int rih_gemm_multi_variant(const rih_gemm_desc* d);
int64_t rih_gemm_multi_table_bytes(const rih_gemm_desc* descs, int n);
int rih_gemm_multi_pack(const rih_gemm_desc* descs, int n, void* host_table, int32_t* total_blocks);
int rih_gemm_multi_launch(const void* dev_table, int variant, int total_blocks, void* stream);

/* Sum split-K partials P[S][M][N] (M = taps*Cin rows ordered (tap,ci)) into a weight gradient laid out
 * like the parameter: dst[(n*CinValid + ci)*taps + tap]  (OIHW for convs, [out][in] for nn.Linear).
 * Rows with ci >= CinValid (channel padding) are dropped.  accumulate!=0 adds to dst.  One launch, fixed summation
 * order (deterministic). */
int rih_splitk_reduce(float* P, int S, int M, int N, float* dst, int Cin, int taps, int CinValid,
                      int accumulate, void* stream);
/* Same on slabs of Mp >= M rows; with db != NULL (Mp >= M+1) slab row M -- produced by a weight-gradient GEMM whose A
 * operand carries an all-ones row there (rih_gemm_desc.ones_row) -- is summed into the bias gradient db[N]. */
int rih_splitk_reduce_bias(const float* P, int S, int Mp, int M, int N, float* dst, int Cin, int taps, int CinValid,
                           int accumulate, float* db, void* stream);
/* Any number of independent reductions (each as rih_splitk_reduce_bias) in ceil(n/56) launches: the split-K partials of
 * the weight gradients of a whole backward stage are summed at the END of the stage instead of one small launch behind
 * every weight-gradient GEMM (157 launches of ~8 us per ResNet50 step; a dependent kernel costs >= 4.5 us on this
 * platform whatever its size).  `descs` is HOST memory, read before the call returns.  Same fixed summation order.
 * Two kernels, one result (bitwise): reductions with N % 4 == 0, 16-byte aligned P, M == taps * Cin, CinValid <= Cin and
 * taps <= 96 -- in rih_splitk_reduce_bias(_batched) too (batched: sP % 4 == 0) -- run on 16-byte loads and, below S = 32, write
 * runs of taps * (ci range) floats per n through LDS (from S = 32: the four partial sums of an element on four lanes, stores as
 * the reference); the others run on the reference kernel (one element per thread). */
typedef struct rih_reduce_desc {
    const float* P;         /* [S][Mp][N] partial slabs */
    float* dst;             /* parameter-layout gradient, see rih_splitk_reduce */
    float* db;              /* optional bias gradient [N] from slab row M, or NULL */
    int32_t S, Mp, M, N, Cin, taps, CinValid, accumulate;
    int32_t CinPitch;       /* 0: dst is the whole parameter [N][CinValid][taps]; > 0: dst points at the first of CinValid columns of a
                               wider parameter [N][CinPitch][taps] (the column slice of one part of a concatenated input, a_seg) */
    int32_t reserved;       /* 0; != 0 keeps this reduction on the reference kernel (below) */
} rih_reduce_desc;
int rih_splitk_reduce_multi(const rih_reduce_desc* descs, int n, void* stream);
/* nb independent reductions in one launch: slice b reads P + b*sP and writes dst + b*sDst, db + b*sDb (the split-K
 * partials of an nb1-batched weight-gradient GEMM, e.g. the paired left/right-hand layers). */
int rih_splitk_reduce_bias_batched(const float* P, int S, int Mp, int M, int N, float* dst, int Cin, int taps,
                                   int CinValid, int accumulate, float* db, int nb, int64_t sP, int64_t sDst,
                                   int64_t sDb, void* stream);

/* Training statistics (what rih_bn_stats produces, running buffers included) from the per-row-block (mean, M2) pairs that
 * rih_gemm's statistics epilogue writes (rih_gemm_desc.stats: part[T][2][C], T = ceil(rows / rows_per_block),
 * rows_per_block = rih_gemm_stats_rows(desc)): no pass over the convolution output; one launch. */
int rih_bn_stats_from_blocks(const float* part, int T, int C, int rows, int rows_per_block, float eps, float momentum,
                             float* mean, float* invstd, float* running_mean, float* running_var, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Halo-resident 3x3 convolution, stride 1, padding 1 (csrc/rih_conv3.hip, ABI 15) -- the 3x3 convolutions of the trunk's
 * Bottlenecks and of the aux decoders (torchvision Bottleneck.conv2 via models/encoder.py:81-83; models/encoder.py:44-54) and
 * their data gradients, on engine 2's arithmetic (fp32 = three fp16 MFMA products, see rih_gemm_desc.engine).  A workgroup owns
 * an 8 x 32 pixel patch and 128 (64) output channels, loads and converts each 32-channel chunk of the (8+2) x (32+2) input
 * halo ONCE and runs the nine taps on shifted windows of that LDS image; the weights arrive as two pre-split fp16 planes
 * ("H2": dst[n][k / 8][plane][8 halves], k = (tap, channel), written once per training step by rih_h2_multi) through LDS-DMA.
 *   y[img][i][j][n] = act(sum_{kh,kw,c} x[img][i+kh-1][j+kw-1][c] * W(n, (kh*3+kw)*C + c) (+ r[img][i][j][n]))        (zero padding)
 * Forward: W from rih_h2_desc.for_dgrad 0 (n = co).  Data gradient: x = dy, C = Cout, N = CinPad, for_dgrad 1 (flipped taps).
 * Preconditions (rih_conv3x3_ok returns 1): C % 32 == 0, N % 32 == 0, (H % 8 == 0 and W % 32 == 0: patches of 8 x 32 pixels) or
 * (H % 16 == 0 and W % 16 == 0: 16 x 16), Kpad == 9 * C, 16-byte aligned x / w_h2 / y / stats, ldx / ldy % 4 == 0, one image
 * below 2 GiB.  amax_x / amax_w: bound blocks (rih_absmax) -- amax_w must be the block the H2 planes were scaled with.  stats
 * (optional): [imgs * H * W / rows][2][N] (mean, M2) per block of rows = rih_conv3x3_stats_rows(desc) output rows (64; 32 when
 * N is not a multiple of 64), the format of rih_gemm_desc.stats (a block is a piece of a patch, every block full).
 * Not bit-identical to rih_gemm on the same convolution: the reduction runs chunk-major, (c / 32, tap, c % 32). */
typedef struct rih_conv3_desc {
    const float* x;         /* NHWC [imgs][H][W][ldx] */
    const void* w_h2;       /* [N][Kpad / 8][2][8] fp16 */
    float* y;               /* NHWC [imgs][H][W][ldy] */
    float* stats;           /* or NULL */
    const float* amax_x;
    const float* amax_w;
    int32_t imgs, H, W, C, N, ldx, ldy, Kpad, relu;
    int32_t ldr;            /* (ABI 19) pitch of r */
    const float* r;         /* (ABI 19) optional residual NHWC [imgs][H][W][ldr], added before the ReLU: the skip gradient that joins the
                             * data gradient of a residual block's first 3x3 convolution (torchvision BasicBlock.conv1; reference
                             * models/hrnet: BasicBlock.forward `out += residual`).  16-byte aligned, ldr >= N, ldr % 4 == 0; not
                             * together with stats; rih_stem takes none.  NULL: none */
} rih_conv3_desc;
int rih_conv3x3_ok(const rih_conv3_desc* d);
int rih_conv3x3_stats_rows(const rih_conv3_desc* d);
int rih_conv3x3(const rih_conv3_desc* d, void* stream);
typedef struct rih_h2_desc {
    const float* w;         /* OIHW parameter */
    void* dst;              /* [N][Kpad / 8][2][8] fp16: N = Cout (for_dgrad 0) or CinPad (1), Kpad >= KH*KW*CinPad (resp. *Cout), % 32 */
    const float* amax;      /* bound block of w */
    int32_t Cout, Cin, KH, KW, CinPad, for_dgrad, Kpad;
    int32_t reserved;       /* 0; != 0: the gathering reference kernel (below).  Takes the struct's former tail padding: same size */
} rih_h2_desc;
/* any number of H2 weight operands in ceil(n / 48) launches (`descs` is HOST memory, read before the call returns).  Operands with
 * KH * KW <= 127 and (forward: CinPad % 8 == 0, or CinPad * KH * KW < 4096 as for the stem; data gradient: Cout % 8 == 0) are read
 * coalesced through an LDS tile; the others, and descriptors with reserved != 0, by the gathering kernel.  Same bits either way. */
int rih_h2_multi(const rih_h2_desc* descs, int n, void* stream);

/* Short-reduction streaming GEMM (csrc/rih_conv3.hip `panel_kernel`, ABI 16): C[M][N] = act(A[M][K] W[N][K]^T (+ R)) for the 1x1
 * convolutions with K = 64 or 128 on large maps (torchvision Bottleneck.conv3 of layer1 / layer2 forward, conv1's data
 * gradient) -- HBM streams that the tiled kernels of rih_gemm ran at 2-3 TB/s.  Persistent workgroups (one per CU) keep their
 * column block of the H2 weight planes (rih_h2_multi with KH = KW = 1: forward n = co, k = ci; data gradient for_dgrad 1: n = ci,
 * k = co) in LDS and walk over row tiles with the next tile's rows in flight.  Engine-2 arithmetic (amax_a / amax_w as
 * rih_conv3_desc).  Preconditions (rih_panel_ok returns 1): K in {64, 128}, N % 64 == 0 (% 128 at K = 128), M % 128 == 0,
 * 16-byte aligned a / w_h2 / c / r / stats, lda / ldc / ldr % 4 == 0, M * lda * 4 < 2^31, not stats and r together.
 * stats (optional): [M / rows][2][N] per block of rows = rih_panel_stats_rows(desc) consecutive rows (rih_gemm_desc.stats format). */
typedef struct rih_panel_desc {
    const float* a;         /* [M][lda] */
    const void* w_h2;       /* [N][K / 8][2][8] fp16 */
    float* c;               /* [M][ldc] */
    const float* r;         /* [M][ldr] or NULL */
    float* stats;           /* or NULL */
    const float* amax_a;
    const float* amax_w;
    int32_t M, N, K, lda, ldc, ldr, relu;
} rih_panel_desc;
int rih_panel_ok(const rih_panel_desc* d);
int rih_panel_stats_rows(const rih_panel_desc* d);
int rih_panel(const rih_panel_desc* d, void* stream);
/* Long-K plain-row GEMM (csrc/rih_conv3.hip rows_kernel, ABI 18) -- the 1x1 convolutions with K >= 256 of Bottleneck.conv1 / conv3
 * and their data gradients (torchvision Bottleneck via models/encoder.py:75-89,107-126): the same descriptor and the same
 * arithmetic as rih_panel (engine 2, H2 weight planes), as 512-thread workgroups on 256 x 128 / 128 x 128 / 256 x 64 / 128 x 64 tiles
 * with the weights staged by LDS-DMA on three stages, two A stages in LDS and the A prefetch in registers.  Preconditions
 * (rih_rows_ok returns 1): K % 32 == 0, K >= 64, N % 64 == 0, M % 128 == 0, pitches % 4 == 0, 16-byte aligned operands,
 * M * lda * 4 < 2^31, not both stats and r.
 * stats (optional): [M / rows][2][N] per block of rows = rih_rows_stats_rows(desc) consecutive rows (64 or 32).
 * The tile is the library's choice (the largest that still gives every CU a workgroup).  ABI 26: rih_rows_tile reports that choice
 * (returns 1; 0 with *bm / *bn untouched when rih_rows_ok is 0) and rih_rows_tiled is the same launch on a tile the caller names --
 * (bm, bn) one of (256,128), (128,128), (256,64), (128,64) with M % bm == 0 and N % bn == 0, RIH_EINVAL otherwise; its statistics
 * blocks are bm / 4 rows high.  rih_rows(d) == rih_rows_tiled(d, the tile of rih_rows_tile(d)): same instantiation, same grid.
 * Nothing on the product path names a tile; the tests do, to reach every instantiation at shapes of a few workgroups. */
/* The stem convolution (ABI 18): 7 x 7 / stride 2 / padding 3 over a FOUR-channel NHWC image batch (encoder.resnet.conv1 of
 * torchvision ResNet-50 via models/encoder.py:107-116, on the 3 -> 4 channel padded input of rih_nchw_to_nhwc) on the rows kernel with
 * an im2col loader (one tap of one output pixel = one float4).  Descriptor = rih_conv3_desc: x [imgs][H][W][4] (C = ldx = 4), w_h2 =
 * H2 planes of the OIHW weight with CinPad 4 (rih_h2_desc: KH = KW = 7, Kpad = 224), y [imgs][H/2][W/2][ldy], N = 64, stats per 64
 * rows.  Preconditions (rih_stem_ok returns 1): H, W even, imgs * H/2 * W/2 % 256 == 0, the image batch < 2 GiB, 16-byte aligned. */
int rih_stem_ok(const rih_conv3_desc* d);
int rih_stem(const rih_conv3_desc* d, void* stream);
int rih_rows_ok(const rih_panel_desc* d);
int rih_rows_stats_rows(const rih_panel_desc* d);
int rih_rows(const rih_panel_desc* d, void* stream);
int rih_rows_tile(const rih_panel_desc* d, int* bm, int* bn);
int rih_rows_tiled(const rih_panel_desc* d, int bm, int bn, void* stream);

/* Finish a forward split-K GEMM: C[m*ldc+n] = act(alpha * sum_s P[s][m][n] + bias[n] + R[m*ldr+n]). */
int rih_splitk_finish(const float* P, int S, int M, int N, float* C, int ldc, const float* bias, const float* R,
                      int ldr, float alpha, int relu, void* stream);

/* Repack an OIHW conv weight for rih_gemm: dst[((kh*KW+kw)*Ci_pad + ci)*Cout + co] (forward, b_mode 0) or,
 * with for_dgrad!=0, dst[(((KH-1-kh)*KW + (KW-1-kw))*Cout + co)*Ci_pad + ci] (flipped, in/out swapped). */
int rih_pack_conv_weight(const float* w, float* dst, int Cout, int Cin, int KH, int KW, int CinPad,
                         int for_dgrad, void* stream);
/* Any number of weight operands packed in ceil(n/56) launches (every 3x3 / 7x7 / patch convolution of a training step needs
 * its forward and its data-gradient operand once per step: 58 launches of ~6 us otherwise).  mode 0 = rih_pack_conv_weight
 * (for_dgrad 0), mode 1 = rih_pack_conv_weight_sub (the full flipped operand is kh0 = kw0 = 0, step 1, Th = KH, Tw = KW).
 * `descs` is HOST memory, read before the call returns. */
typedef struct rih_pack_desc {
    const float* w;         /* OIHW parameter */
    float* dst;
    int32_t Cout, Cin, KH, KW, CinPad, mode, kh0, kw0, step, Th, Tw;
    int32_t reserved;       /* 0; != 0 keeps this operand on the reference kernel (one element per thread) instead of the tiled
                               transpose through LDS that operands with KH * KW <= 63 take.  Same bits either way. */
} rih_pack_desc;
int rih_pack_conv_weight_multi(const rih_pack_desc* descs, int n, void* stream);
/* Tap subset for one parity class of a strided data gradient:
 * dst[((th*Tw + tw)*Cout + co)*CinPad + ci] = w[co][ci][kh0 + step*(Th-1-th)][kw0 + step*(Tw-1-tw)]. */
int rih_pack_conv_weight_sub(const float* w, float* dst, int Cout, int Cin, int KH, int KW, int CinPad, int kh0,
                             int kw0, int step, int Th, int Tw, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Layout, pooling, resampling   (models/encoder.py:107-113 stem, :31 nn.Upsample, :155-158 avgpool)   */
int rih_nchw_to_nhwc(const float* x, float* y, int N, int C, int H, int W, int Cpad, void* stream);
int rih_nhwc_to_nchw(const float* x, float* y, int N, int C, int H, int W, int ldx, void* stream);
int rih_maxpool3x3s2_fwd(const float* x, float* y, int8_t* arg, int N, int H, int W, int C, void* stream);
int rih_maxpool3x3s2_bwd(const float* dy, const int8_t* arg, float* dx, int N, int H, int W, int C, void* stream);
int rih_avgpool_fwd(const float* x, float* y, int N, int HW, int C, void* stream);
int rih_avgpool_bwd(const float* dy, float* dx, int N, int HW, int C, void* stream);
int rih_upsample2x_fwd(const float* x, float* y, int N, int H, int W, int C, void* stream);
int rih_upsample2x_bwd(const float* dy, float* dx, int N, int H, int W, int C, void* stream);
/* bilinear x`factor`, align_corners=True: [N,H,W,C] -> [N,factor*H,factor*W,C]
 * (F.interpolate in models/encoder.py:228-230: the HRNet branches are brought to 64x64 with x2 / x4 / x8) */
int rih_upsample_bilinear_fwd(const float* x, float* y, int N, int H, int W, int C, int factor, void* stream);
int rih_upsample_bilinear_bwd(const float* dy, float* dx, int N, int H, int W, int C, int factor, void* stream);
/* nearest x`factor` upsample fused with the running sum of HighResolutionModule's fuse layer
 * (models/model_zoo/hrnet.py:181-183, 229-236): y = add + up(x) (add may be NULL); C % 4 == 0.
 * Backward of the upsample branch: dx = sum of dy over each factor x factor block (the `add` branch gets dy). */
int rih_nearest_up_add_fwd(const float* x, const float* add, float* y, int N, int H, int W, int C, int factor,
                           void* stream);
int rih_nearest_up_bwd(const float* dy, float* dx, int N, int H, int W, int C, int factor, void* stream);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm2d (NHWC, rows = N*H*W)   (torchvision resnet bn*, models/encoder.py:54, model_zoo/__init__.py:57)
 * ws: caller workspace, >= rih_bn_ws_floats(rows, C) floats.                                           */
int64_t rih_bn_ws_floats(int rows, int C);
/* training statistics: mean[C], invstd[C]; updates running_mean/var (momentum, unbiased var) when non-NULL */
int rih_bn_stats(const float* x, int rows, int C, float eps, float momentum, float* mean, float* invstd,
                 float* running_mean, float* running_var, float* ws, void* stream);
/* eval statistics from running buffers */
int rih_bn_eval_stats(const float* running_mean, const float* running_var, int C, float eps, float* mean,
                      float* invstd, void* stream);
/* y = act((x-mean)*invstd*gamma + beta + residual).  amax (optional, ABI 13): a bound block (rih_absmax) that receives max|y| --
 * the operand bound of the convolution that reads y (rih_gemm_desc.amax_a, engine 2) at no extra pass; zeroed by the caller. */
int rih_bn_apply(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                 const float* residual, float* y, int rows, int C, int relu, uint8_t* relu_mask, float* amax, void* stream);
/* relu_mask (optional, relu != 0): rows*C/4 bytes, byte q = sign pattern of output quad q (bit e set: element 4q+e > 0).
 * The backward then reads one byte per quad instead of the 16 bytes of y (it needs nothing else of y).
 * backward of the above (training statistics): given dy and the ReLU pattern (relu_mask, or the forward output y when
 * relu_mask == NULL), produces dx, dgamma, dbeta and, when dres != NULL, the residual-branch gradient (= masked dy).
 * frozen_stats bit 0: eval-mode backward (statistics are constants).  Bit 1: the BatchNorm's input x is itself a ReLU output
 * (Conv -> ReLU -> BN, models/encoder.py:52-54): dx is additionally gated by x > 0, so the convolution's backward needs no
 * separate ReLU pass over it. */
int rih_bn_bwd(const float* dy, const float* x, const float* y, const float* mean, const float* invstd,
               const float* gamma, float* dx, float* dres, float* dgamma, float* dbeta, int rows, int C,
               int relu, int frozen_stats, float* ws, const uint8_t* relu_mask, float* amax_dx, void* stream);
/* amax_dx (optional, ABI 13): a bound block that receives max|dx|, as `amax` of rih_bn_apply -- dx is the gradient operand of
 * the producing convolution's data- and weight-gradient GEMMs. */
/* BatchNorm pairs (ABI 30): y = act(BN_a(xa) + BN_b(xb)), the end of a residual block whose skip branch ends in a BatchNorm of
 * its own (torchvision Bottleneck.downsample).  rih_bn_apply2 leaves in y, relu_mask and amax exactly what
 * rih_bn_apply(xb, .., residual = NULL, relu = 0) followed by rih_bn_apply(xa, .., residual = that output, relu) leaves, without
 * the branch's output in memory.  rih_bn_bwd2 leaves in dxa, dxb, dgamma_*, dbeta_* and the two bound blocks exactly what
 * rih_bn_bwd(dy, xa, .., dres, relu, frozen_a, relu_mask) followed by rih_bn_bwd(dres, xb, .., relu = 0, frozen_b) leaves, without
 * dres in memory: one reduction pass with three sums (dbeta_a == dbeta_b), one apply pass with two outputs.  relu != 0 needs
 * relu_mask.  ws: >= rih_bn_ws2_floats(rows, C) floats. */
/* BatchNorm -> ReLU -> max-pool 3x3/2 (ABI 30; the ResNet stem, x: [N][H][W][C]): rih_bn_pool_fwd leaves in y_pooled, arg and amax
 * exactly what rih_bn_apply(relu = 1) followed by rih_maxpool3x3s2_fwd leaves (amax: max|y_pooled| = max|y|, every element of y
 * >= 0 lies in some window), rih_bn_pool_bwd in dx, dgamma, dbeta and amax_dx exactly what rih_maxpool3x3s2_bwd followed by
 * rih_bn_bwd(relu = 1) leaves; neither full-resolution intermediate is stored and no ReLU mask is needed (the sign of the
 * recomputed bn(x) gates).  Pointers 16-byte aligned, C % 4 == 0; ws: >= rih_bn_ws_floats(N*H*W, C) floats. */
int rih_bn_pool_fwd(const float* x, const float* mean, const float* invstd, const float* gamma, const float* beta,
                    float* y_pooled, int8_t* arg, int N, int H, int W, int C, float* amax, void* stream);
int rih_bn_pool_bwd(const float* dy_pooled, const int8_t* arg, const float* x, const float* mean, const float* invstd,
                    const float* gamma, const float* beta, float* dx, float* dgamma, float* dbeta, int N, int H, int W, int C,
                    int frozen_stats, float* ws, float* amax_dx, void* stream);
int64_t rih_bn_ws2_floats(int rows, int C);
int rih_bn_apply2(const float* xa, const float* mean_a, const float* invstd_a, const float* gamma_a, const float* beta_a,
                  const float* xb, const float* mean_b, const float* invstd_b, const float* gamma_b, const float* beta_b,
                  float* y, int rows, int C, int relu, uint8_t* relu_mask, float* amax, void* stream);
int rih_bn_bwd2(const float* dy, const float* xa, const float* mean_a, const float* invstd_a, const float* gamma_a,
                const float* xb, const float* mean_b, const float* invstd_b, const float* gamma_b, float* dxa, float* dxb,
                float* dgamma_a, float* dbeta_a, float* dgamma_b, float* dbeta_b, int rows, int C, int relu, int frozen_a,
                int frozen_b, float* ws, const uint8_t* relu_mask, float* amax_dxa, float* amax_dxb, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row-wise ops on [rows][D] matrices (decoder)                                                         */
/* y = act(LayerNorm(x (+ x2)) * g + b); saves mean/rstd per row   (nn.LayerNorm eps=1e-6, gcn.py:91-97 ...) */
int rih_layernorm_fwd(const float* x, const float* x2, const float* g, const float* b, float* y, float* mean,
                      float* rstd, int rows, int D, float eps, int relu, void* stream);
/* dx (= gradient wrt x and x2), dg/db accumulated via ws (>= 2*nblk*D floats, nblk = rih_ln_nblk(rows)).
 * dres (may be NULL): [rows][D] added to dx -- the gradient arriving over a skip connection around the norm
 * (x + f(LN(x)), self_attn.py:26-33, 84-85), so that autograd needs no separate accumulation pass. */
int rih_ln_nblk(int rows);
/* rih_layernorm_bwd[_grouped] with dg == db == NULL leaves the parameter gradients as partials in ws ([groups][nblk][2][D]);
 * rih_ln_param_final_multi finishes any number of them (one descriptor per group: ws + g*nblk*2*D, dg + g*D, db + g*D) in
 * ceil(n/100) launches -- a backward stage's 50 LayerNorms cost one finishing launch instead of 50 (>= 4.5 us each).
 * `descs` is HOST memory, read before the call returns. */
typedef struct rih_ln_final_desc {
    const float* ws;
    float* dg;
    float* db;
    int32_t D, nblk;
} rih_ln_final_desc;
int rih_ln_param_final_multi(const rih_ln_final_desc* descs, int n, void* stream);
int rih_layernorm_bwd(const float* dy, const float* x, const float* x2, const float* y, const float* g,
                      const float* mean, const float* rstd, const float* dres, float* dx, float* dg, float* db, int rows,
                      int D, int relu, float* ws, void* stream);
/* `groups` independent LayerNorms in one launch (the left- and the right-hand layer of DualGraph.py:83-89 on
 * activations stacked [groups][rows][D]): group q uses the parameters g + q*sG, b + q*sB (distances in floats between
 * the two layers' parameter tensors, may be negative) and, in the backward, writes dg + q*D, db + q*D; ws >= groups * 2*nblk*D floats. */
int rih_layernorm_fwd_grouped(const float* x, const float* x2, const float* g, const float* b, float* y, float* mean,
                              float* rstd, int groups, int rows, int D, int64_t sG, int64_t sB, float eps, int relu,
                              void* stream);
int rih_layernorm_bwd_grouped(const float* dy, const float* x, const float* x2, const float* y, const float* g,
                              const float* mean, const float* rstd, const float* dres, float* dx, float* dg, float* db,
                              int groups, int rows, int D, int64_t sG, int relu, float* ws, void* stream);
/* softmax over the last dim of [rows][ld] (first `cols` entries), optional inverted dropout with a
 * counter-based hash RNG (csrc/rih_hash.h: element idx of stream `seed` is kept iff mix32(lo32(idx) ^ hi32(idx) * 0x85EBCA6B ^
 * key(seed)) >= p * 2^32): P (pre-dropout probabilities) and Pd (post-dropout, may alias P when p==0).
 * Every dropout entry point takes the stream id of the mask as `seed` plus an optional DEVICE word `seed_dev` (may be
 * NULL) that is added to it on the GPU: a training step captured in a hipGraph advances that word inside the graph
 * and gets a fresh mask at every replay, with no host involvement. */
int rih_softmax_fwd(const float* S, float* P, float* Pd, int64_t rows, int cols, int ld, float drop_p,
                    uint64_t seed, const uint64_t* seed_dev, void* stream);
/* dS = alpha * P * (dPd*mask/(1-p) - sum_j(dPd*mask/(1-p) * P)), written in place over dPd */
int rih_softmax_bwd(const float* P, float* dPd, int64_t rows, int cols, int ld, float drop_p, uint64_t seed,
                    const uint64_t* seed_dev, float alpha, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Elementwise / gather                                                                                 */
/* Adam / AdamW step (torch.optim.Adam / AdamW semantics, amsgrad off) over a table of parameter tensors in ONE launch:
 * replaces the optimizer step of core/gcn_trainer.py:127 (torch.optim.Adam: 24 multi-tensor launches of ~37 us per ResNet50
 * step, 4.7x the HBM time of the 7 passes it needs).  `table` (DEVICE memory): one entry per tensor; block b of the launch
 * updates elements [blk_chunk[b]*C, (blk_chunk[b]+1)*C) of tensor blk_tensor[b], C = rih_adam_chunk() (both DEVICE int32
 * arrays of nblocks entries, built once by the caller).  step >= 1 is the 1-based step count of the bias corrections. */
typedef struct rih_adam_entry {
    float* p;           /* parameter, updated in place */
    const float* g;     /* gradient */
    float* m;           /* exp_avg */
    float* v;           /* exp_avg_sq */
    int64_t n;          /* elements */
} rih_adam_entry;
int rih_adam_multi(const rih_adam_entry* table, const int32_t* blk_tensor, const int32_t* blk_chunk, int nblocks, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, int adamw, void* stream);
int rih_adam_chunk(void);

/* y = a + dropout(b) (inverted dropout, p may be 0); b_bcast_rows>0: b is [b_bcast_rows][D] broadcast over the batch */
int rih_add_dropout(const float* a, const float* b, float* y, int64_t n, int D, int b_bcast_rows, float drop_p,
                    uint64_t seed, const uint64_t* seed_dev, void* stream);
/* backward of dropout: dx = dy * mask/(1-p) */
int rih_dropout_bwd(const float* dy, float* dx, int64_t n, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                    void* stream);
/* y = max(x,0);  dx = dy * (y>0) */
int rih_relu_fwd(const float* x, float* y, int64_t n, void* stream);
int rih_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);
/* column sums of [rows][C] (bias gradients); ws >= rih_colsum_ws_floats(rows,C) */
int64_t rih_colsum_ws_floats(int rows, int C);
int rih_colsum(const float* x, int rows, int C, int ldx, float* out, int accumulate, float* ws, void* stream);
/* out[b][i][:] = x[b][idx[i]][:]  (graph_perm gathers, nearest upsample along V, token slicing) */
int rih_gather_rows(const float* x, const int32_t* idx, float* y, int B, int Vin, int Vout, int D, void* stream);
/* dx[b][idx[i]][:] += dy[b][i][:]  with dx zero-initialised by the callee (deterministic, via inverse lists) */
int rih_scatter_rows_add(const float* dy, const int32_t* inv_ptr, const int32_t* inv_idx, float* dx, int B, int Vin,
                         int Vout, int D, void* stream);

/* Orthographic projection uv = (scale*img)*xyz[:2] + (trans*img/2 + img/2)   (utils/manoutils.py:26-44)
 * v[B][V][3], scale[B], trans[B][2] -> out[B][V][2]; backward gives dv (z component 0), dscale, dtrans. */
int rih_project_fwd(const float* v, const float* scale, const float* trans, float* out, int B, int V,
                    float img_size, void* stream);
int rih_project_bwd(const float* dout, const float* v, const float* scale, float* dv, float* dscale,
                    float* dtrans, int B, int V, float img_size, void* stream);

/* Chebyshev K=2 feature build: y[b][v][2f+0] = x[b][v][f], y[b][v][2f+1] = sum_j L[v][j] x[b][j][f]
 * with L in CSR (models/model_attn/gcn.py:34-69).  Backward takes CSR of L^T. */
int rih_cheby_fwd(const float* x, const int32_t* indptr, const int32_t* indices, const float* vals, float* y,
                  int B, int V, int F, void* stream);
int rih_cheby_bwd(const float* dy, const int32_t* t_indptr, const int32_t* t_indices, const float* t_vals,
                  float* dx, int B, int V, int F, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MANO linear-blend-skinning layer   (models/manolayer.py:250-322)
 * Constant model (uploaded once by the caller, device pointers):
 *   comps[45][45] (PCA basis rows), hands_mean[45], shapedirs[778][3][10], posedirs[778][3][135],
 *   v_template[778][3], J_reg[16][778] (dense), weights[778][16], parent[16] (host array).
 * Per call: root[B][9], pose (PCA coeffs [B][ncomp] if ncomp>0, else rotation matrices [B][15][9]),
 *   shape[B][10], trans[B][3] or NULL, scale[B] or NULL.  Outputs v[B][778][3], j[B][21][3].
 * packed: >= rih_mano_pack_floats() floats (16-byte aligned) written by rih_mano_pack from the model buffers: the blend
 *   bases as one k-major matrix [148][2496] (posedirs | shapedirs | v_template, coordinates padded to 13 tiles of 192) and
 *   the joint regressor folded onto template and shape basis, and (ABI 17) a compact [148][48] copy of the basis columns of the
 *   13 special vertices (finger tips, new_skel).  Re-pack whenever a model buffer changes (the reference's
 *   callers mutate shapedirs in place, dataset/interhand.py:22-25).
 * rih_mano_fwd variant 0: ONE fused launch (workgroup = 64-vertex tile of the packed basis pinned in LDS x group of hand
 *   chunks; pose chain per chunk, blend GEMM on v_mfma_f32_16x16x4_f32, skinning).  ws may be NULL (inference: only v and j
 *   are written); with ws (>= rih_mano_ws_floats(B) floats, kept by the caller) it also stores what rih_mano_bwd needs.
 *   From 256 hand chunks (4096 hands) on, variant 0 runs the same kernel hand-chunk major: a workgroup does the pose chain of
 *   its 16 hands once and streams the 13 basis tiles through the LDS buffer from L2 (the tile-major form repeats the pose
 *   work in each of the 13 tiles: 47 % of its cycles; measured 259 -> 212 us for 4096 hands).  variant 2 / 3 force the hand-major / tile-major form (tests, timing).
 *   variant 1: the two-kernel forward of round 1 (needs ws; kept for A/B timing).                                      */
typedef struct rih_mano_model {
    const float* comps;
    const float* hands_mean;
    const float* shapedirs;
    const float* posedirs;
    const float* v_template;
    const float* J_reg;
    const float* weights;
    int32_t parent[16];
} rih_mano_model;

int64_t rih_mano_ws_floats(int B);
int64_t rih_mano_pack_floats(void);
int rih_mano_debug_stamps(long long* device_buf_13x16);   /* development aid: phase timestamps of the fused forward; NULL = off */
int rih_mano_pack(const rih_mano_model* m, float* packed, void* stream);
int rih_mano_fwd(const rih_mano_model* m, const float* packed, const float* root, const float* pose, int ncomp,
                 const float* shape, const float* trans, const float* scale, int center_idx, int new_skel, float* v,
                 float* j, float* ws, int B, int variant, void* stream);
/* gradients wrt root/pose/shape/trans/scale (any may be NULL) given dv[B][778][3], dj[B][21][3] and the forward's ws (16-byte
 * aligned: the hand's SE3s are read with 16-byte scalar loads).
 * Three launches (round 5): (1) per hand the skinning / kinematic-chain part -- one workgroup per hand; the SE3s as wave-uniform
 * scalar operands, dG = W^T M on v_mfma_f32_16x16x4_f32; (2) the two contractions with the blend bases (pose-blend and shape
 * gradients: 0.33 MFLOP per hand against 1.26 MB of basis) TILE major: a workgroup pins one of the 13 tiles of `packed` in LDS
 * and walks over 16-hand chunks of dv_tpose, writing partial sums; (3) per hand (one wavefront) the sum of the 13 partials in
 * tile order, the pose-blend term, Rodrigues backward, PCA projection, shape gradient.  ws_bwd (>= rih_mano_bwd_ws_floats(B)
 * floats, 16-byte aligned) carries dv_tpose / rotation and rest-joint gradients / the partial sums between them.
 * 4096 hands: 175 us (rounds 3-4: 362); 128 hands: 39 us (174).  ws_bwd == NULL runs the one-kernel backward of rounds 1-2
 * (every workgroup re-reads the whole basis from L2: 1.17 ms for 4096 hands; A/B partner). */
int rih_mano_bwd(const rih_mano_model* m, const float* packed, const float* root, const float* pose, int ncomp,
                 const float* shape, const float* trans, const float* scale, int center_idx, int new_skel, const float* dv,
                 const float* dj, const float* ws, float* d_root, float* d_pose, float* d_shape, float* d_trans,
                 float* d_scale, float* ws_bwd, int B, void* stream);
int64_t rih_mano_bwd_ws_floats(int B);

/* Quaternion mode of the same kernels (ABI 23): manopth's ManoLayer as the pose optimiser builds it
 * (pose_data_optimize/manopth/manopth/manolayer.py:235-250,258-380 with joint_rot_mode = root_rot_mode = 'quat';
 * renderih_amd.quat_mano.FusedQuatManoLayer).  quat[B][16][4] in (w, x, y, z) order, root first, NOT normalised: R = the ceres
 * form / |q|^2 (quatutils.py:168-221, no epsilon); left != 0 negates y and z first (the left hand).  The model's comps and
 * hands_mean are not read (may be NULL); `packed` is rih_mano_pack's buffer, unchanged.  shape_stride = 10 (shape[B][10]) or 0
 * (one vector of 10 shared by the batch).  tips: host array of the 5 finger-tip vertices of this call (a tip outside the
 * packed buffer's compact copy reads its basis columns from the big matrix).  center_idx -1..20: -1 = nothing subtracted; the
 * caller passes -1 together with trans (manopth centres only without a translation).
 * rih_mano_quat_fwd: ONE launch (the conversion is the front end of the fused forward).  Outputs v[B][778][3], j[B][21][3]
 *   (the 16 posed joints + 5 tips, reordered) and, unless NULL, transf[B][16][4][4] = [R_global | posed joint - centre + trans;
 *   0 0 0 1].  ws as in rih_mano_fwd.
 * rih_mano_quat_bwd: three launches, no atomics, fixed summation order.  Upstream dv[B][778][3], dj[B][21][3],
 *   dtransf[B][16][4][4] (each may be NULL = zero); d_quat[B][16][4] includes the term of the division by |q|^2; d_shape[B][10]
 *   and d_trans[B][3] may be NULL.  ws_bwd as in rih_mano_bwd (required).
 * RIH_EINVAL: a null pointer that is not optional, B < 1, center_idx outside -1..20, a tip outside 0..777, another stride. */
int rih_mano_quat_fwd(const rih_mano_model* m, const float* packed, const float* quat, int left, const float* shape,
                      int shape_stride, const float* trans, int center_idx, const int32_t* tips, float* v, float* j,
                      float* transf, float* ws, int B, void* stream);
int rih_mano_quat_bwd(const rih_mano_model* m, const float* packed, const float* quat, int left, int center_idx,
                      const int32_t* tips, const float* dv, const float* dj, const float* dtransf, const float* ws,
                      float* d_quat, float* d_shape, float* d_trans, float* ws_bwd, int B, void* stream);

/* Contact anchors (manopth/anchorutils.py:51-65; csrc/rih_anchor.hip, ABI 23): anchors[b][a] = w1 (v1 - v0) + w2 (v2 - v0) + v0
 * over the vertices face_vert_idx[a][0..2] of vertices[B][V][3], weight[A][2].  Backward: g_vertices[B][V][3] gathered per
 * vertex through vptr[V+1] / vlist[3A] (entries anchor * 3 + corner, ascending), which the HOST builds and range-checks once
 * per index tensor; vertices that no anchor reads get exact zeros.  One launch each, no atomics.
 * RIH_EINVAL: a null pointer, B < 1, V < 1, A < 1. */
int rih_anchor_fwd(const float* vertices, const int32_t* face_vert_idx, const float* weight, float* anchors, int B, int V,
                   int A, void* stream);
int rih_anchor_bwd(const float* g_anchors, const int32_t* vptr, const int32_t* vlist, const float* weight, float* g_vertices,
                   int B, int V, int A, void* stream);

/* Hand-prior and contact terms of the pose optimiser's two-hand objective (hocontact/postprocess/geo_loss.py:
 * batch_pose_quat_norm_loss, edge_len_loss, hand_pose_ergonomics_loss, FieldLoss.batch_contact_loss, summed as
 * geo_optimizer_both_batch.py:805-824 does for mode='both'; csrc/rih_pose_prior.hip, ABI 24;
 * renderih_amd.pose_prior.FusedTwoHandPriorLoss builds every constant).  Index 0 / suffix _r is the right (main) hand, 1 / _l
 * the left (sub) hand.
 * rih_pose_prior_fwd (one launch, one workgroup per (sample, hand)): q_*[B][16][4] (w, x, y, z), NOT normalised;
 *   verts_*[B][V][3]; anchors_*[B][A][3].  joint_tables[2][15][18]: per hand and finger joint the 3x3 matrices Lm, Rm with
 *   relative frame = Lm R(q) Rm.  edges[E][2] (both hands), static_len[2][E]; vptr[V+1] / vlist[2E] (entries edge * 2 + end,
 *   ascending): the vertex -> edge lists, built and range-checked by the HOST.  anchor_id[B][A][D] (indices into the MAIN
 *   hand's anchors, range-checked by the host), elastic[B][A][D]; cptr[B][A+1] / clist[B][A*D] (entries i * D + d): per sample
 *   the main anchor -> contact pair lists.  inv_mask_sum = 1 / mask.sum(), or 0 for an empty mask (contact term and its
 *   gradients exactly 0).  Writes partial[B][2][4] (per sample and hand: quaternion norm, edge, ergonomics, contact -- the last
 *   in the left hand's slot -- each already divided by its element count) and grads: the gradient of
 *   norm_r + norm_l + edge_r + edge_l + lambda_contact * contact + ergo_r + ergo_l with respect to q_r, q_l, verts_r, verts_l,
 *   anchors_r, anchors_l, back to back in that order (B * (128 + 6 V + 6 A) floats).  No atomics; a vertex without an edge
 *   gets an exact zero.
 * rih_pose_prior_reduce (one workgroup): terms[7] = the seven terms in the order above (contact without its weight), summed
 *   over the batch in index order; loss[0] = their sum with lambda_contact applied.
 * rih_pose_prior_bwd (elementwise): out[i] = grads[i] * grad_out[0] over n floats (grad_out: DEVICE scalar).
 * RIH_EINVAL: a null pointer, B < 1 or > 65535, V, E, A, D or n < 1, a negative or NaN inv_mask_sum. */
int rih_pose_prior_fwd(const float* q_r, const float* q_l, const float* verts_r, const float* verts_l, const float* anchors_r,
                       const float* anchors_l, const float* joint_tables, const int32_t* edges, const float* static_len,
                       const int32_t* vptr, const int32_t* vlist, const int32_t* anchor_id, const float* elastic,
                       const int32_t* cptr, const int32_t* clist, float inv_mask_sum, float lambda_contact, float* grads,
                       float* partial, int B, int V, int E, int A, int D, void* stream);
int rih_pose_prior_reduce(const float* partial, float lambda_contact, float* terms, float* loss, int B, void* stream);
int rih_pose_prior_bwd(const float* grads, const float* grad_out, float* out, int64_t n, void* stream);

/* The pose optimiser's NatureLoss: a pose discriminator's verdict on both hands as a loss (geo_optimizer_both_batch.py:110-132
 * `GeOptimizer.NatureLoss`, added with weight 1 at :824; the network of Ver2Code/Discriminator/discrim.py:66-105;
 * csrc/rih_nature.hip, ABI 28; renderih_amd.nature.FusedTwoHandNatureLoss).  fp32.  H = the network's hidden width, a multiple
 * of 64 in [64, 512] (the reference's is 512).  Rows are the 2B hands, right hands first, then left.
 * rih_nature_pack: the twelve tensors of the state dict in torch layout (w1[H][45], b1[H], w2..w4 and w_last [H][H] with their
 *   biases [H], w_pred[2][H], b_pred[2]) -> packed (>= rih_nature_pack_floats(H) floats, 16-byte aligned): every weight once as
 *   [in][out] for the forward and once as [out][in] for the backward, then the biases.  Once per loaded weight set.
 * rih_nature_fwd (one workgroup of H threads per tile of rih_nature_tile_rows() rows): q_*[B][16][4] (w, x, y, z), NOT
 *   normalised; the root is not read.  Per row: normalise, matrix with the conversion's own 2 / |q|^2, XYZ Euler angles
 *   (atan2(-m12, m22), asin(m02), atan2(-m01, m00); asin's argument is CLAMPED to [-1, 1], the reference's is not), the six
 *   layers, softmax (p0, p1), mask = p1 < 1.5 p0, bce = -(log(1 - p0) + log(p1)) / 2 with torch's log floor of -100.  ws
 *   (>= rih_nature_ws_floats(B, H) floats, 16-byte aligned) receives the four activated layers [2B][4][H] and [2B][4] =
 *   (p0, p1, bce, mask).
 * rih_nature_reduce (one workgroup, fixed order): terms[4] = (mean bce of the masked right rows, of the masked left rows, the
 *   two counts); a side without a masked row gives exactly 0; loss[0] = terms[0] + terms[1]; the per-row scale (1 / count of
 *   its side, 0 for an unmasked row) goes into ws for the backward.  Nothing is read by the host.
 * rih_nature_bwd (same tiles): dq_*[B][16][4] = grad_out[0] (DEVICE scalar) * d loss / d q_*, through the normalisation; the
 *   root's gradient is written as 0; a clamped asin and a gimbal-locked atan2(0, 0) pass no gradient.  Every element of dq_* is
 *   written, with plain stores: two runs are bit-identical.
 * RIH_EINVAL: a null pointer, B < 1 or > RIH_NATURE_MAX_B, H not a multiple of 64 in [64, 512], packed or ws not 16-byte
 * aligned; the two size queries return 0 for such B or H. */
#define RIH_NATURE_MAX_B (1 << 20)
int64_t rih_nature_pack_floats(int H);
int64_t rih_nature_ws_floats(int B, int H);
int rih_nature_tile_rows(void);
int rih_nature_pack(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                    const float* w4, const float* b4, const float* w_last, const float* b_last, const float* w_pred,
                    const float* b_pred, float* packed, int H, void* stream);
int rih_nature_fwd(const float* packed, const float* q_r, const float* q_l, float* ws, int B, int H, void* stream);
int rih_nature_reduce(float* ws, float* loss, float* terms, int B, int H, void* stream);
int rih_nature_bwd(const float* packed, const float* q_r, const float* q_l, const float* ws, const float* grad_out, float* dq_r,
                   float* dq_l, int B, int H, void* stream);

/* Adam and the plateau scheduler of the pose optimiser with every scalar on the device (geo_optimizer_both_batch.py:428-432
 * `torch.optim.Adam` + `ReduceLROnPlateau`, :879-880 `optimizer.step(); scheduler.step(loss)`; csrc/rih_pose_opt.hip, ABI 25;
 * renderih_amd.pose_opt).  One optimiser iteration is rih_adam_dev then rih_plateau_step on the same stream, with no host read:
 * the pair can be captured in a hipGraph and replayed.
 * rih_opt_state (DEVICE memory, 8-byte aligned, filled by the host before the first step): `step` = iterations done (Adam's
 *   bias corrections use step + 1), `best` (+inf at the start) and `num_bad_epochs` of the scheduler, one learning rate per
 *   parameter group, and the scheduler's settings (mode 'min', threshold_mode 'rel', cooldown 0; one min_lr for all groups).
 * rih_adam_dev (grid: chunks of 1024 elements x tensors): torch.optim.Adam (amsgrad off, no weight decay) over `ntensors`
 *   table entries (DEVICE memory); max_n >= every entry's n sizes the grid.  The learning rate of entry.group and the step
 *   count are read from `state`; bias corrections in double, on the device.  Element i of an entry is FROZEN when
 *   period > 0 and (i % period) < skip: its p, m and v keep their bits.  prev (or NULL) receives p from before the step,
 *   frozen elements included.  The kernel only reads `state`.
 * rih_plateau_step (one workgroup): ReduceLROnPlateau.step(loss[0]) on `state`: better iff loss < best * (1 - threshold) in
 *   double (a NaN loss is not better); otherwise num_bad_epochs += 1; when num_bad_epochs > patience every group's lr
 *   becomes max(lr * factor, min_lr) if that lowers it by more than eps_lr, and num_bad_epochs = 0; then step += 1.
 * RIH_EINVAL: a null pointer, ntensors < 1, max_n < 1, betas outside [0, 1), a negative or NaN eps. */
#define RIH_OPT_MAX_GROUPS 8
typedef struct rih_opt_state {
    double best;
    double lr[RIH_OPT_MAX_GROUPS];
    double factor, threshold, min_lr, eps_lr;
    int64_t step;
    int32_t num_bad_epochs, patience, ngroups, reserved;
} rih_opt_state;
typedef struct rih_adam_dev_entry {
    float* p;           /* parameter, updated in place */
    const float* g;     /* gradient */
    float* m;           /* exp_avg */
    float* v;           /* exp_avg_sq */
    float* prev;        /* NULL, or n floats: the parameter before this step */
    int64_t n;          /* elements */
    int32_t group;      /* index into rih_opt_state.lr, 0 <= group < ngroups */
    int32_t period, skip;   /* frozen pattern; period = 0: none */
    int32_t reserved;
} rih_adam_dev_entry;
int rih_adam_dev(const rih_adam_dev_entry* table, int ntensors, int64_t max_n, const rih_opt_state* state, float beta1,
                 float beta2, float eps, void* stream);
int rih_plateau_step(rih_opt_state* state, const float* loss, void* stream);

/* Fitting MANO pose and shape to 3-D joints (utils/mano_from_3djoint/: AIK.py `adaptive_IK`, utils.py `mat2aa`,
 * convert2mano.py:158-204; csrc/rih_joint_fit.hip, ABI 32; renderih_amd.joint_fit).  fp32 in and out, no atomics, every sum in a
 * fixed order (two runs are bit-identical), nothing read back: all of it can be captured in a hipGraph.
 * rih_aik: `adaptive_IK(template, joints[b])` for B hands in one launch (RIH_AIK_HANDS_PER_GROUP hands per workgroup), in double
 *   on the fp32 inputs.  tmpl[21][3] (one per call), joints[B][21][3] in the reference's joint order (wrist, then thumb, index,
 *   middle, ring, little); normalize = 1 first scales the joints by |T9 - T0| / |P9 - P0| and moves joint 0 onto T0
 *   (convert2mano.py:167-169).  R[B][16][3][3]: slot 0 the root rotation, the others in the reference's ID2ROT order.
 *   Deviations from the reference: the root is always the PROPER rotation maximising tr(R H) (rih_procrustes.h; the reference
 *   returns a reflection where det(V U^T) = -1 and no singular value is below 1e-4); a bone whose cross product with its
 *   template bone is exactly zero gets the identity (the reference: NaN); the cosine is clamped to [-1, 1]; no twist.
 * rih_mat2aa_fwd: aa = mat2aa(R) for N matrices R[N][3][3]: the quaternion of the selected one of mat2quat's four branches
 *   (eps 1e-6), quat2aa, NaN components -> 0.  period > 0 (N a multiple of it, 0 <= skip < period): the first `skip` matrices
 *   of every `period` are left out -- aa[N / period * (period - skip)][3] is compact, and head (unless NULL) receives the
 *   left-out matrices [N / period * skip][9] (the root rotation as rih_mano_fwd takes it).  period = 0: all N.
 * rih_mat2aa_bwd: g_R[N][9] from g_aa (compact as above): the derivative of the selected branch; at sin^2 = 0 that of aa = 2 v;
 *   zero where the forward gave NaN or the term under the square root is not positive.  Left-out matrices receive
 *   g_head[N / period * skip][9] (zero if NULL): with (16, 1) g_R is the whole gradient of a hand's 16 matrices.
 * rih_joint_l1 (one workgroup): jr = j - j[:, 0], diff = jr - target, loss[b] = mean |diff[b]| over the 63 values,
 *   total[0] = sum_b loss[b], dj[b][k] = sign(diff) / 63 for k >= 1 (sign(0) = 0), dj[b][0] = -sum_k dj[b][k].  history
 *   (unless NULL) [hist_rows][B]: row state->step receives loss (no row outside 0..hist_rows-1 is written).
 * rih_lr_linear_step (one thread): every group's lr = base_lr * (n_iter - step) / n_iter in double, in that order of
 *   operations (convert2mano.py:202-203 after iteration `step`), then step += 1.  Runs after rih_adam_dev, in the place of
 *   rih_plateau_step; the only writer of `state`.  rih_lr_linear lives in DEVICE memory, 8-byte aligned.
 * rih_fit_select (workgroup = hand): where loss[b] < best_loss[b] (a NaN never is) best_P[b][144], best_beta[b][10] and
 *   best_loss[b] take P, beta and loss.  Launched between rih_joint_l1 and rih_adam_dev: the parameters that gave the loss.
 * RIH_EINVAL: a null pointer that is not optional, B or N < 1, normalize other than 0 / 1, a (period, skip) outside the above,
 *   a history without state or rows. */
#define RIH_AIK_HANDS_PER_GROUP 8
#define RIH_MAT2AA_TPB 256
typedef struct rih_lr_linear {
    double base_lr;
    int64_t n_iter;
} rih_lr_linear;
int rih_aik(const float* tmpl, const float* joints, int normalize, float* R, int B, void* stream);
int rih_mat2aa_fwd(const float* R, float* aa, float* head, int64_t N, int period, int skip, void* stream);
int rih_mat2aa_bwd(const float* R, const float* g_aa, const float* g_head, float* g_R, int64_t N, int period, int skip,
                   void* stream);
int rih_joint_l1(const float* j, const float* target, const rih_opt_state* state, float* loss, float* total, float* dj,
                 float* history, int hist_rows, int B, void* stream);
int rih_lr_linear_step(rih_opt_state* state, const rih_lr_linear* sched, void* stream);
int rih_fit_select(const float* loss, const float* P, const float* beta, float* best_loss, float* best_P, float* best_beta,
                   int B, void* stream);

/* Contact search of the pose optimiser's driver (pose_data_optimize/batch_optimize_mocap_origin.py: `search_anchors` :62-130 on
 * the anchors and face normals of `update_scene` :260-270; csrc/rih_contact.hip, ABI 27; renderih_amd.contact_search).  One
 * launch for B frames, one workgroup per frame, not differentiable.  verts_main / verts_sub[B][V][3]: the two hands' vertices,
 * already translated; face_vert_idx[A][3] (range-checked against V by the HOST), weight[A][2], class_type[A].  Anchors by
 * rih_anchor_fwd's expression; normals cross(v1 - v0, v2 - v0) normalised, the sub hand's negated (a degenerate face is
 * outside the contract).  For sub anchor i and main anchor j, dis = |sub_i - main_j|.
 *   prev_id == NULL (fresh search): dis counts as 1000 where n_sub_i . n_main_j > against_cos; anchor_id[b][i][0..D) = the D
 *     smallest, EQUAL distances in ascending j; vertex_contact[b][i] = any dis < radius.
 *   prev_id[B][A][D] (refresh): anchor_id = prev_id, the true distance to every previous id and no against rule;
 *     vertex_contact = any of the row's D ids within the radius.  An id outside [0, A) is copied through with elastic 0 and
 *     mask 0 and is not dereferenced.
 *   elastic = (dis < radius) cos^2(pi dis / (2 radius)) (= 0.5 cos(pi dis / radius) + 0.5, but positive up to the radius in
 *     fp32); mask = elastic > 0; elastic *= damp where class_type[i] != tip_class and class_type[id] != tip_class.
 * Plain stores in a fixed order: two runs are bit-identical.
 * RIH_EINVAL: a null pointer other than prev_id, B, V, A or D < 1, A > 1024, D > 8, D > A, a radius that is not positive. */
int rih_contact_search(const float* verts_main, const float* verts_sub, const int32_t* face_vert_idx, const float* weight,
                       const int32_t* class_type, const int64_t* prev_id, float radius, float against_cos, float damp,
                       int tip_class, int64_t* anchor_id, float* elastic, int64_t* mask, int64_t* vertex_contact, int B, int V,
                       int A, int D, void* stream);

/* Two-hand mesh collision count, the gate behind the pose optimiser (pose_data_optimize/collision/CollisionFilter.py and
 * CollisionCheck.py, which ask FCL for contact points; csrc/rih_collision.hip, ABI 31; renderih_amd.collision).  Counted here:
 * INTERSECTING TRIANGLE PAIRS, a lower bound of FCL's contact points, so the reference's thresholds do not carry over.  One
 * launch for B frames, one workgroup per (frame, 256 main faces).  verts_main[B][Vm][3], verts_sub[B][Vs][3];
 * faces_main[Fm][3], faces_sub[Fs][3] (range-checked against Vm and Vs by the HOST); any sizes.
 *   orient(a,b,c,d) = dot(cross(b - a, c - a), d - a).  An edge (p,q) pierces a triangle (a,b,c) when orient(a,b,c,p) and
 *   orient(a,b,c,q) have strictly opposite signs and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all > 0 or all < 0.
 *   Main face i and sub face j intersect when their boxes overlap and one of the six edge-against-triangle tests pierces.
 *   Strict throughout: coplanar, touching, zero-area and NaN configurations do not intersect; a face with a vertex that is
 *   not finite, or with a normal cross(v1 - v0, v2 - v0) that is exactly zero, intersects nothing.
 * pairs_main[B][Fm] = per main face the number of sub faces it intersects (plain stores); pairs_sub[B][Fs] and count[B] = the
 * same per sub face and per frame, ADDED with integer atomics: both must be zero on entry.  Nothing is read back by the host;
 * integer sums only, so two runs are bit-identical.
 * RIH_EINVAL: a null pointer, B, Vm, Vs, Fm or Fs < 1, more than 2^31 - 1 workgroups. */
int rih_collision_count(const float* verts_main, const float* verts_sub, const int32_t* faces_main, const int32_t* faces_sub,
                        int32_t* pairs_main, int32_t* pairs_sub, int32_t* count, int B, int Vm, int Vs, int Fm, int Fs,
                        void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused mesh loss   (core/Loss.py:68-164 GraphLoss.calc_loss, :201-277 calc_loss_GCN; aux loss disabled there)
 * Constant topology of one hand (device pointers, uploaded once by the caller):
 *   faces[F][3]; vptr[V+1], vlist[3F]: for every vertex the list of (face*3 + corner) it belongs to, ascending;
 *   J[NJ][V] dense joint regressor incl. the 5 finger tips, reordered (Loss.py:38-53); perm[Vc*pool] = graph_perm
 *   (vert_to_GCN); pool = 2^k consecutive graph-order vertices are average-pooled pairwise into one coarse vertex.
 * rih_mesh_loss (one launch per hand): predictions v3d_pred[B][V][3], v2d_pred[B][V][2], c3d_pred[B][Vc][3],
 *   c2d_pred[B][Vc][2]; labels v3d_gt, v2d_gt; gt_shift[B][3] or NULL is added to v3d_gt (root_rel of the right hand).
 *   term_weights[7] (DEVICE array, read by the kernel at run time so that a captured hipGraph follows in-place updates
 *   such as the epoch gate of the edge term; order v2d, v3d, joint, normal, edge, coarse-3d, coarse-2d) = weight of the
 *   raw SUM of each term in the total, i.e. LOSS_WEIGHT / element count / 2 (hand average).  Writes the gradient of the total
 *   with respect to the four prediction tensors and partial[B][8] (raw sums of the seven terms per image).
 * rih_mesh_loss_final: out[0] = total over both hands; out[1..7] = the seven terms as the reference reports them
 *   (mean over elements, averaged over the hands); counts[7] = element counts (DEVICE array). */
typedef struct rih_mesh_topo {
    const int32_t* faces;
    const int32_t* vptr;
    const int32_t* vlist;
    const float* J;
    const int32_t* perm;
    int32_t V, F, NJ, Vc, pool;
} rih_mesh_topo;

int rih_mesh_loss(const rih_mesh_topo* topo, const float* v3d_pred, const float* v2d_pred, const float* c3d_pred,
                  const float* c2d_pred, const float* v3d_gt, const float* v2d_gt, const float* gt_shift,
                  const float* term_weights, float img_size, float* g_v3d, float* g_v2d, float* g_c3d, float* g_c2d,
                  float* partial, int B, void* stream);
int rih_mesh_loss_final(const float* partial_left, const float* partial_right, int B, const float* term_weights,
                        const float* counts, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused MANO-head loss   (core/Loss_mano.py:62-219 ManoLoss, :245-335 mano_loss_GCN; csrc/rih_mano_loss.hip, ABI 21)
 * Topology: the rih_mesh_topo of one hand as above; faces, vptr, vlist, J, V, F, NJ are read, perm / Vc / pool are not.
 * rih_mano_loss (one launch per hand, one workgroup per image): predictions v3d_pred[B][V][3], v2d_pred[B][V][2],
 *   pose_pred[B][pose_dim] (16 axis-angles, pose_dim must be 48), shape_pred[B][shape_dim] (shape_dim must be 10); labels
 *   v3d_gt, v2d_gt, pose_gt, shape_gt; gt_shift[B][3] or NULL is added to v3d_gt (root_rel of the right hand).
 *   term_weights[9] (DEVICE array, read at run time so that a captured hipGraph follows the epoch gate of the edge term;
 *   order v2d, v3d, joint, normal, edge, pose, shape = LOSS_WEIGHT / element count / 2 (hand average), then MANO_REL / (3B),
 *   then the regulariser's 0.005).  Writes the gradient of the total with respect to the four prediction tensors (the shape
 *   gradient includes the regulariser's 0.01 * shape) and partial[B][8] (raw sums of the seven terms, then sum(shape^2)).
 * rih_mano_loss_final (one workgroup): out[0] = total without the up-sampling term; out[1..9] = vert2d, vert3d, joint,
 *   norm, edge, pose, shape (means, averaged over the hands), rootrel, regularize as the reference reports them;
 *   counts[7] = element counts of the seven per-hand terms (DEVICE array); g_rootrel[B][3] = gradient of the total with
 *   respect to rootrel_pred.  Partials are summed in a fixed order, no atomics: evaluations are bit-identical. */
int rih_mano_loss(const rih_mesh_topo* topo, const float* v3d_pred, const float* v2d_pred, const float* pose_pred,
                  const float* shape_pred, const float* v3d_gt, const float* v2d_gt, const float* pose_gt,
                  const float* shape_gt, const float* gt_shift, int pose_dim, int shape_dim, const float* term_weights,
                  float img_size, float* g_v3d, float* g_v2d, float* g_pose, float* g_shape, float* partial, int B,
                  void* stream);
int rih_mano_loss_final(const float* partial_left, const float* partial_right, const float* rootrel_pred,
                        const float* rootrel_gt, int B, const float* term_weights, const float* counts, float* g_rootrel,
                        float* out, void* stream);

/* library / device info.  RIH_ABI_VERSION is bumped whenever a struct layout or a signature of this header changes;
 * rih_version() returns the value the library was compiled with and rih_abi_sizes() the sizeof of EVERY by-pointer struct, in
 * this order: gemm desc, mano model, mesh topo, hconv desc, reduce desc, pack desc, ln final desc, adam entry, absmax desc,
 * conv3 desc, h2 desc, panel desc, opt state, adam dev entry (RIH_ABI_NSIZES values), so a host binding can refuse a stale binary instead of handing it
 * mis-laid-out structs. */
#define RIH_ABI_VERSION 36
#define RIH_ABI_NSIZES 14
int rih_version(void);
int rih_abi_sizes(int32_t* out10);
const char* rih_arch(void);

/* ------------------------------------------------------------------------------------------------
 * Attention without a score matrix in memory (csrc/rih_flash.hip) -- the default path of SelfAttn / inter_attn
 * (models/model_attn/self_attn.py:70-76: `attn = softmax(q k^T / sqrt(d_q)); attn = dropout(attn); out = attn v`;
 * inter_attn.py:93-107: the two cross-hand directions).  q / k / v are head-sliced in place: row pitches q_ld / kv_ld floats,
 * head h at column h*d, slice b at row b*Sq (b*Sk); d in {16, 32, 64}; B*heads <= 65535.
 *   rih_flash_attention_fwd: out[b][i][h*d + c] = sum_j Pd[i][j] v[j][c], Pd = dropout(softmax_j(alpha q_i . k_j)); one launch;
 *     lse[B*heads][Sq] receives log2(sum_j 2^(alpha log2(e) q_i . k_j)) -- all the backward needs besides q, k, v, out.
 *     Dropout: element (row r = (b*heads + h)*Sq + i, column j) is kept iff hash(seed (+ *seed_dev), r*Sk + j) >= p * 2^32, kept
 *     values scaled by 1/(1-p) -- the mask of rih_softmax_fwd, bit for bit.
 *   rih_flash_attention_bwd: dq, dk, dv (row pitches dq_ld / dkv_ld, same head slicing) from dO [B][Sq][do_ld] and the saved
 *     out / lse, recomputing the probabilities tile by tile; two launches (query side, then key side); Dws [B*heads][Sq] is
 *     workspace (receives rowsum(dO o out)).  Every element of the dq / dk / dv head slices is written exactly once. */
int rih_flash_attention_fwd(const float* q, int q_ld, const float* k, const float* v, int kv_ld, int B, int heads, int Sq,
                            int Sk, int d, float alpha, float drop_p, uint64_t seed, const uint64_t* seed_dev, float* out,
                            int ld_out, float* lse, void* stream);
int rih_flash_attention_bwd(const float* dO, int do_ld, const float* O, int o_ld, const float* q, int q_ld, const float* k,
                            const float* v, int kv_ld, int B, int heads, int Sq, int Sk, int d, float alpha, float drop_p,
                            uint64_t seed, const uint64_t* seed_dev, const float* lse, float* Dws, float* dq, int dq_ld,
                            float* dk, float* dv, int dkv_ld, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused attention forward, first generation (keeps P / Pd in memory; superseded by rih_flash_attention_*, kept as an opt-in
 * experiment RIH_FUSED_ATTN=1): out = softmax(alpha q k^T)
 * [dropout] v per (image, head) in ONE launch; q / k / v are head-sliced in place (row pitches q_ld / kv_ld, head h at
 * column h*d), out [B][Sq][ld_out] at column h*d.  P and Pd [B][heads][Sq][ldP] receive the probabilities before / after
 * dropout for the backward (Pd may equal P when drop_p == 0).  d in {16, 32, 64}, Sk <= 320.  Dropout mask and seed as
 * rih_softmax_fwd.  Not yet measured on hardware (see csrc/rih_attn.hip). */
int rih_attention_fwd_fused(const float* q, int q_ld, const float* k, const float* v, int kv_ld, int B, int heads, int Sq,
                            int Sk, int d, float alpha, float drop_p, uint64_t seed, const uint64_t* seed_dev, float* P,
                            float* Pd, int ldP, float* out, int ld_out, void* stream);
/* Query side of the attention backward in ONE launch (replaces the dO V^T GEMM, rih_softmax_bwd and the dS K GEMM):
 * dS = alpha * P * (m*dPd - rowsum(m*dPd*P)) with dPd = dO V^T and m the regenerated dropout mask (x 1/(1-p)), written to
 * dS [B][heads][Sq][ldP] for the key-side products (dK = dS^T q, dV = Pd^T dO stay batched GEMMs), and dq = dS k written
 * to dq [B][Sq][dq_ld] at column h*d.  dO [B][Sq][do_ld] head-sliced like q.  Same limits as the forward. */
int rih_attention_bwd_dq_fused(const float* dO, int do_ld, const float* k, const float* v, int kv_ld, int B, int heads,
                               int Sq, int Sk, int d, float alpha, float drop_p, uint64_t seed, const uint64_t* seed_dev,
                               const float* P, float* dS, int ldP, float* dq, int dq_ld, void* stream);
/* Key side of the attention backward in ONE launch (replaces two transposed batched GEMMs): dv = Pd^T dO and
 * dk = dS^T q, written to [B][Sk][dkv_ld] at column h*d.  Pd / dS [B][heads][Sq][ldP] (dS from the kernel above). */
int rih_attention_bwd_dkv_fused(const float* dO, int do_ld, const float* q, int q_ld, int B, int heads, int Sq, int Sk,
                                int d, const float* Pd, const float* dS, int ldP, float* dk, float* dv, int dkv_ld,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * fp16-storage inference backbone (BASELINE configs[4]; csrc/rih_half.hip).  Eval-mode only: every BatchNorm of
 * models/encoder.py is folded -- Conv->BN(->ReLU) (trunk, encoder.py:107-116) into weights (rih_hpack_conv_weight's
 * `scale`) and `bias`; Conv->ReLU->BN (aux decoders encoder.py:52-54, mid convs model_zoo/__init__.py:56-62) into
 * post_scale / post_shift.  Activations are NHWC fp16 with a pixel pitch (ldx / ldr / ldy, in elements) so that channel
 * slices of a wider tensor can be read and written in place (the channel concatenations of encoder.py:160-171 are never
 * copied).  fp32 accumulation (v_mfma_f32_32x32x16_f16), fp32 epilogue:
 *   y[pix][co] = post( relu?( sum_k x[...] w[co][k] + bias[co] + res[pix][co] ) ),  post(u) = u*post_scale[co] + post_shift[co]
 * Requirements: Cin % 8 == 0, ldx % 8 == 0, x / w / zero 16-byte aligned, Kpad % 64 == 0, Ho/Wo consistent with the
 * geometry; `zero` points at >= 16 bytes of zeros in device memory (source of every padded operand chunk).  16-byte
 * epilogue accesses are used when y / res rows are aligned (ldy % 8 (fp16) or % 4 (fp32), ldr % 8), scalar otherwise. */
typedef struct rih_hconv_desc {
    const void* x;            /* fp16 [N][H][W][ldx], channels [0, Cin) */
    const void* w;            /* fp16 [Cout][Kpad] from rih_hpack_conv_weight, k = (kh, kw, ci) */
    const void* zero;
    const float* bias;        /* [Cout] or NULL */
    const float* post_scale;  /* [Cout] or NULL (both or neither) */
    const float* post_shift;
    const void* res;          /* fp16 [pixels][ldr] or NULL */
    void* y;                  /* [pixels][ldy] fp16, or fp32 when out_f32 */
    int32_t N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo;
    int32_t ldx, ldr, ldy, Kpad;
    int32_t relu, out_f32;
} rih_hconv_desc;
int rih_hconv(const rih_hconv_desc* d, void* stream);
/* What rih_hconv would do with `d`, without launching anything: RIH_EINVAL where it refuses the descriptor, else
 * RIH_HCONV_PLAN_BASE plus the flags of the kernel it launches (the same helper decides for both, including the
 * RIH_HCONV_HALO / RIH_HCONV_GLDS / RIH_HCONV_BN switches of the process). */
#define RIH_HCONV_PLAN_BASE 0x10  /* always set: a plan is positive */
#define RIH_HCONV_PLAN_HALO 0x01  /* halo-resident 3x3 kernel (else the implicit GEMM) */
#define RIH_HCONV_PLAN_TW16 0x02  /* halo: 16 x 16 pixel patches (else 8 x 32) */
#define RIH_HCONV_PLAN_BN128 0x04 /* 128 output channels per workgroup (else 64) */
#define RIH_HCONV_PLAN_REGS 0x08  /* implicit GEMM: operands staged through registers (else LDS-DMA) */
int rih_hconv_plan(const rih_hconv_desc* d);
/* fp32 OIHW -> fp16 [Cout][Kpad], k = (kh*KW + kw)*CinPad + ci, times scale[co] when scale != NULL; zero padded. */
int rih_hpack_conv_weight(const float* w, const float* scale, void* dst, int Cout, int Cin, int KH, int KW, int CinPad,
                          int Kpad, void* stream);
/* Eval BatchNorm as an affine map: scale = gamma/sqrt(var+eps), shift = beta - mean*scale + scale*conv_bias
 * (gamma / beta / conv_bias may be NULL = 1 / 0 / 0). */
int rih_hbn_fold(const float* gamma, const float* beta, const float* mean, const float* var, const float* conv_bias,
                 float eps, float* scale, float* shift, int C, void* stream);
/* [N][C][H][W] fp32 (C <= 8) -> [N][H][W][8] fp16, channels >= C zero. */
int rih_himage_nchw_to_nhwc8(const float* img, void* out, int N, int C, int H, int W, void* stream);
/* fp16 NHWC 3x3 stride-2 pad-1 max-pool, bilinear x2 (align_corners=True), global average pool (fp32 [N][C] out). */
int rih_hmaxpool3x3s2(const void* x, void* y, int N, int H, int W, int C, int ldx, int ldy, void* stream);
int rih_hupsample2x(const void* x, void* y, int N, int H, int W, int C, int ldx, int ldy, void* stream);
int rih_havgpool(const void* x, float* y, int N, int HW, int C, int ldx, void* stream);

/* Contact deviation (apps/eval_interhand.py:481-490, utils/eval_metrics.py:30-50 `compute_cdev`): per sample, the mean over
 * the ground-truth right-hand vertices whose nearest ground-truth left-hand vertex is within `contact` (3e-3 m) of
 * |pred_left[nearest] - pred_right[v]|; NaN when there is no such vertex (the reference's nanmean then skips the sample).
 * All meshes [B][V][3], V <= 1024; out [B]. */
int rih_cdev(const float* pred_left, const float* pred_right, const float* gt_left, const float* gt_right, int B, int V,
             float contact, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Input preparation of a batch resident on the GPU (csrc/rih_input.hip) -- core/loader.py:104-219
 * `handDataset.process_data` and utils/manoutils.py:214-260 (`imgUtils.data_augmentation`, `add_noise`).
 * rih_prepare_images: src [B][S][S][3] uint8 BGR (decoded crops).  minv [B][6] = the INVERSE (destination -> source)
 *   of the matrix the reference hands to cv.warpAffine, in double precision (NULL: no warp); 8-bit INTER_LINEAR /
 *   BORDER_CONSTANT fixed-point algorithm of OpenCV.  bright [B][4] = per-channel gain a_b, a_g, a_r and offset b of
 *   `add_noise` (NULL: none).  flip [B] (NULL: none).  Outputs (each may be NULL): aug_u8 [B][S][S][3] the augmented
 *   crop, ori [B][3][S][S] = BGR / 255, norm [B][3][S][S] = ImageNet-normalised RGB, norm_h8 [B][S][S][8] fp16 NHWC
 *   (the input layout of rih_hconv's first layer).
 * rih_prepare_labels: p2 [B][NP][2], p3 [B][NP][3] with NP = 2*(NV+NJ) points ordered [verts_left, joints_left,
 *   verts_right, joints_right]; A [B][6] the first two rows of the float32 affine matrix (NULL: identity), R [B][9] the
 *   in-plane rotation (NULL: identity); root-relative to joint `root_joint` of each hand, scaled so that the mean
 *   |joint root - joint 0| equals bone_length (<= 0: off); flipped samples mirror x (2-D: img_size - x), negate
 *   root_rel y/z as the reference does, and swap the hands in the output. */
int rih_prepare_images(const uint8_t* src, int B, int S, const double* minv, const double* bright, const uint8_t* flip,
                       uint8_t* aug_u8, float* ori, float* norm, void* norm_h8, void* stream);
int rih_prepare_labels(const float* p2, const float* p3, int B, int NV, int NJ, const float* A, const float* R,
                       const uint8_t* flip, float bone_length, int root_joint, float img_size, float* o2, float* o3,
                       float* root_rel, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Interior distance field of closed triangle meshes (csrc/rih_sdf.hip) -- the reference's only native kernel,
 * pose_data_optimize/sdf/sdf/csrc/sdf_cuda_kernel.cu:242-335 (`sdf_cuda`).  faces [F][3] int32 (shared by the batch),
 * vertices [B][V][3] inside [-1,1]^3, phi [B][G][G][G] indexed [b][z][y][x]: distance from the voxel centre
 * -1 + (i + 0.5) * 2/(G-1) to the closest triangle when the centre is inside the mesh (odd crossing count towards the
 * corner (-1,-1,-1)), else 0.  No gradient (as in the reference). */
int rih_sdf(float* phi, const int32_t* faces, const float* vertices, int B, int F, int V, int G, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused two-hand penetration loss of the pose optimiser (pose_data_optimize/code_sdf/sdf_template.py:19-157 `NewLoss`;
 * csrc/rih_sdf_loss.hip + the sparse voxeliser of csrc/rih_sdf.hip; renderih_amd.sdf.FusedTwoHandSDFLoss, ABI 22).
 * vertices [bs][2][V][3], hand 0 = right, 1 = left; "mesh" m = 2 b + h, N = 2 bs meshes, 2 <= G <= 256.
 * rih_two_hand_prep (one workgroup per mesh): box[m] = {centre xyz = (lo + hi) / 2, scale = scale_mul * max axis of
 *   (hi - lo)}; vnorm[m][V][3] = (v - centre) / scale, the voxeliser's input; flags[m][G^3] (bytes) = 1 at every voxel that
 *   a vertex of the OTHER hand of the sample reads when it samples mesh m's field (its trilinear corners inside the grid,
 *   sample index ((p + 1) / 2) (G - 1), align_corners = True), else 0; list[m][max_count] = the flagged voxels in ascending
 *   order, count[m] of them.  max_count = min(G^3, 8 V) is the stride of `list`.
 * rih_sdf_sparse: rih_sdf at the voxels list[b][0 .. count[b]) only (same per-voxel device function, bit-identical values);
 *   the other voxels of phi are not written.  The grid covers max_count voxels per mesh; workgroups beyond count[b] exit.
 * rih_two_hand_sample (one workgroup per sample): s = trilinear sample (zero padding) of phi[other hand's mesh] at every
 *   vertex; per_vert[b][2][V] = weight[v] s / 4 (index 0 = LEFT vertices in the right hand's field, 1 = right: the order of
 *   the reference's loss_per_vert); ori[b][2][V] = weight[v] s scale(sampled cube); grad[b][2][V][3] = weight[v] ds/dvertex
 *   (grid_sample's backward x (G - 1) / 2 / scale; corners outside the grid contribute 0); loss[b] = sum of per_vert[b] in a
 *   fixed order.  weight[V] int32 = how many of the 16 hand parts hold the vertex.
 * rih_two_hand_bwd (elementwise): g_vertices[b][h][v][:] = grad[b][1 - h][v][:] * (g_loss[b] / 4 + g_pv[b][1 - h][v] / 4 +
 *   g_ori[b][1 - h][v] * scale(sampled cube)); each of g_loss, g_pv, g_ori may be NULL (that output was not used).
 * No float atomics, fixed summation order: evaluations are bit-identical. */
int rih_two_hand_prep(const float* vertices, float scale_mul, float* box, float* vnorm, uint8_t* flags, int32_t* list,
                      int32_t* count, int bs, int V, int G, int max_count, void* stream);
int rih_sdf_sparse(float* phi, const int32_t* faces, const float* vertices, const int32_t* list, const int32_t* count,
                   int max_count, int B, int F, int V, int G, void* stream);
int rih_two_hand_sample(const float* phi, const float* vertices, const float* box, const int32_t* weight, float* per_vert,
                        float* ori, float* grad, float* loss, int bs, int V, int G, void* stream);
int rih_two_hand_bwd(const float* grad, const float* box, const float* g_loss, const float* g_pv, const float* g_ori,
                     float* g_vertices, int bs, int V, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MANO parameter head of the reference's `load_new_model` network (common/myhand/decoder_lijun_mano.py:112-160,247-300)
 * nn.Hardswish and scale*tanh (the ParamRegressor MLP, `F.tanh(shape) * 3`): elementwise, n floats. */
int rih_hardswish_fwd(const float* x, float* y, int64_t n, void* stream);
int rih_hardswish_bwd(const float* dy, const float* x, float* dx, int64_t n, void* stream);
int rih_tanh_scale_fwd(const float* x, float* y, int64_t n, float scale, void* stream);
int rih_tanh_scale_bwd(const float* dy, const float* y, float* dx, int64_t n, float scale, void* stream);
/* x [n][6] (viewed (3,2): two column vectors) -> Gram-Schmidt rotation matrix R [n][3][3] (decoder_lijun_mano.py:118-125)
 * and its axis-angle vector aa [n][3] through the quaternion (common/myhand/utils/comm.py:176-324, NaN -> 0).
 * Backward: dx = J_R^T dR + J_aa^T daa (either gradient may be NULL), exact (forward-mode dual numbers). */
int rih_rot6d_fwd(const float* x, float* R, float* aa, int n, void* stream);
int rih_rot6d_bwd(const float* x, const float* dR, const float* daa, float* dx, int n, void* stream);
/* axis-angle [n][3] -> rotation matrix [n][3][3], angle = |axis| + 1e-8 (common/utils/manolayer.py:32-48) */
int rih_rodrigues_fwd(const float* a, float* R, int n, void* stream);
int rih_rodrigues_bwd(const float* a, const float* dR, float* da, int n, void* stream);
/* vout = (v - j[root]) * s, s = target / |j[ja] - j[jb]| per mesh (decoder_lijun_mano.py:262-267: root-centred,
 * bone-length-normalised MANO mesh, target 0.095 m); sout [B].  Backward: dv [B][V][3], dj [B][NJ][3] from dvout and
 * (may be NULL) dsout. */
int rih_center_scale_fwd(const float* v, const float* j, int B, int V, int NJ, int root, int ja, int jb, float target,
                         float* vout, float* sout, void* stream);
int rih_center_scale_bwd(const float* v, const float* j, const float* dvout, const float* dsout, int B, int V, int NJ,
                         int root, int ja, int jb, float target, float* dv, float* dj, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluation metrics of one hand (apps/eval_interhand.py:334-415, common/utils/intag_eval.py:92-143,217-283):
 * joints = Jreg [NJ][V] x vertices unless given (j_pred / j_gt may be NULL), both point sets made relative to joint
 * `root_idx`, prediction rescaled by |gt bone| / |pred bone| (bone = joints bone_a, bone_b);
 *   j_err_ori [B][NJ], v_err_ori [B][V]   |pred - gt| before rescaling      (any of the four may be NULL)
 *   j_err     [B][NJ], v_err     [B][V]   |pred * scale - gt|
 *   pa        [B][2]                      Procrustes-aligned mean joint / vertex error (PA-MPJPE, PA-MPVPE): optimal
 *                                         similarity transform of the root-relative prediction onto the ground truth
 *   j_pred_out [B][NJ][3] (may be NULL)   the joints regressed from v_pred
 * V <= 1024, NJ <= 32.  One workgroup per image; no workspace. */
int rih_hand_metrics(const float* v_pred, const float* v_gt, const float* j_pred, const float* j_gt, const float* Jreg,
                     int B, int V, int NJ, int root_idx, int bone_a, int bone_b, float* j_err_ori, float* v_err_ori,
                     float* j_err, float* v_err, float* pa, float* j_pred_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Hard mesh rasteriser and shader (csrc/rih_render.hip) -- the two-hand renderer of utils/vis_utils.py:39-289, which the
 * reference builds on pytorch3d 0.7.2 (MeshRasterizer blur_radius 0 / faces_per_pixel 1, HardPhongShader, hard_rgb_blend);
 * the semantics are written out in renderih_amd/render.py.  verts [B][V][3] world space, faces [F][3] int32 shared by the
 * batch (indices in [0, V): checked by the caller), cams [B][16] = R (3x3 row-major, view = X R + T), T (3), focal (2),
 * principal point (2) in NDC; cam_kind RIH_CAM_*.  Square images only: 1 <= H = W <= 4096; B <= 65535, B*F < 2^31.
 *   rih_render_setup: face_rec [B][F][16] (may be NULL) = screen bounding box, screen vertices, view z, 1/(area + 1e-8), skip
 *     flag; vnormals [B][V][3] (may be NULL, not both) = Meshes.verts_normals, gathered through the vertex -> (face, corner)
 *     CSR vf_ptr [Vc+1] / vf_list (entries 3 f + corner, ascending per vertex; 1 <= Vc <= V, vertices >= Vc belong to no
 *     face and get the normal 0).
 *   rih_render_raster: pix_to_face [B][H][W] int32 = b F + f of the nearest covering face (ties: lower f) or -1; zbuf
 *     [B][H][W] view z or -1; bary [B][H][W][3] (perspective-corrected under RIH_CAM_PERSPECTIVE) or -1.  Deterministic.
 *   rih_render_shade: rgba [B][H][W][4] = hard_rgb_blend of the light_kind shading (RIH_LIGHT_POINT: PointLights at
 *     (0, 0, -1), needs verts / vnormals / cams; RIH_LIGHT_AMBIENT: the texel) of colors [B][V][3] on a white background. */
#define RIH_CAM_ORTHOGRAPHIC 0
#define RIH_CAM_PERSPECTIVE 1
#define RIH_LIGHT_POINT 0
#define RIH_LIGHT_AMBIENT 1
int rih_render_setup(const float* verts, const int32_t* faces, const int32_t* vf_ptr, const int32_t* vf_list,
                     const float* cams, int cam_kind, int B, int V, int Vc, int F, float* face_rec, float* vnormals,
                     void* stream);
int rih_render_raster(const float* face_rec, int B, int F, int H, int W, int cam_kind, int32_t* pix_to_face, float* zbuf,
                      float* bary, void* stream);
int rih_render_shade(const int32_t* pix_to_face, const float* bary, const float* verts, const int32_t* faces,
                     const float* vnormals, const float* colors, const float* cams, int light_kind, int B, int V, int F,
                     int H, int W, float* rgba, void* stream);

/* Silhouette IoU of two meshes from ONE set of face records (csrc/rih_render.hip, next to rih_render_raster): the reference's
 * utils/compute_maskiou.py:263-270 (two silhouette renders, a threshold, a host copy, np.count_nonzero) as a coverage-only
 * pass (ABI 33; renderih_amd.mask_iou).  face_rec [B][F][16] is what rih_render_setup wrote for the vertices cat(first, second) and one face table whose
 * faces 0 .. F_left-1 belong to the first mesh and the rest to the second (0 <= F_left <= F).  A pixel is covered by a mesh
 * exactly when rih_render_raster of that mesh's faces alone gives pix_to_face >= 0.
 *   counts [B][3] int32 = pixels covered by the first mesh, by the second, by both; zeroed here on the stream, then summed
 *     with integer atomics: bit-identical from run to run.
 *   iou [B] (may be NULL) = both / (first + second - both) in fp32, 0 where the union is empty.
 *   mask [B][H][W] uint8 (may be NULL): bit 0 first mesh, bit 1 second mesh.
 * No host read, no floating-point atomics; capturable in a graph.  Sizes as rih_render_raster. */
int rih_mask_iou(const float* face_rec, int B, int F, int F_left, int H, int W, int cam_kind, int32_t* counts, float* iou,
                 uint8_t* mask, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pose-data conversion, augmentation and validity around the pose optimiser (pose_data_optimize/scripts/HandPoseConverter.py,
 * scripts/HandPoseArguer.py, Ver2Code/NatureJudge/PoseArgue.py, Ver2Code/ValidJudge/ValidJudger.py; csrc/rih_pose_convert.hip,
 * ABI 34; renderih_amd.pose_convert).  ONE launch, one thread per (sample, joint), every form built from one kernel body:
 *   in_fmt   0 axis-angle [N][16][3] (hands_mean is added on the finger joints)   1 Euler degrees [N][16][3], scipy's
 *            extrinsic 'xyz': E = Rz(c) Ry(b) Rx(a)   2 quaternion [N][16][4] (w, x, y, z), any norm > 0, 16-byte aligned
 *   mid      0 nothing (A must be 1)   1 augmentation, u = (rih_hash(seed, (((row0 + m) * 16 + j) * 2 + which)) >> 8) * 2^-24
 *            2 augmentation, u = uniforms[m][j][which]   (which: 0 bend, 1 splay)
 *            d = (pos - neg) * u + neg with pos = max(min(cap, hi - angle), 0), neg = min(max(-cap, lo - angle), 0) from the
 *            sample's ORIGINAL Euler bend (c) resp. splay (b); E' = E Rz(d_bend) Ry(d_splay).  Output row m = n * A + a
 *            reads input row n = m / A; M = N * A output rows.
 *   out_fmt  0 Euler degrees [M][16][3] (c = 0 at gimbal lock)   1 unit quaternion [M][16][4] with w >= 0, 16-byte aligned
 *            2 axis-angle [M][16][3], angle in [0, pi], minus hands_mean   3 validity residual in radians: out[m][hands]
 * tables [hands][16][RIH_POSE_TAB]: per joint invM_U_n_0 (9, row-major), invU_M_n_1 (9), the zero frame invM_U_n_0^T
 * invU_M_n_1^T (9), hands_mean (3; 0 for the root), augmentation bend lo / hi / cap and splay lo / hi / cap (cap = 0: the
 * joint does not move), validity bend lo / hi and splay lo / hi (-inf / +inf: no limit), the side's sign (+1 right, -1 left:
 * the left hand's y, z flip of the quaternion and diag(1, -1, -1) on its root matrix), padding.
 * in_second: NULL, or the second hand's quaternions for out_fmt = 3 (then out is [M][2], tables hold two hands).
 * Results depend on (row0 + m, j) only, never on the launch geometry; inputs are not written.
 * RIH_EINVAL: a null pointer, M < 1 or > 2^27, A < 1, A != 1 without augmentation, row0 < 0, a format out of range, mid = 2
 * without uniforms, in_second with another out_fmt than 3. */
#define RIH_POSE_TAB 44
int rih_pose_convert(const float* in, const float* in_second, float* out, const float* tables, const float* uniforms,
                     uint64_t seed, int64_t row0, int64_t M, int A, int in_fmt, int mid, int out_fmt, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The auxiliary heads of the encoders: heat-map labels, the aux loss and the heat-map decoder (dataset/heatmap.py:11-39,
 * core/Loss.py:180-198, dataset/inference.py:113-127; csrc/rih_aux.hip, ABI 35; renderih_amd.aux_heads).  Every tensor is fp32,
 * contiguous NCHW.  No atomics (two runs give the same bits), no host read, every call capturable in a graph; inputs are not
 * written.  16-byte loads and stores where the plane size is a multiple of 4 and every pointer is 16-byte aligned, dwords
 * otherwise.
 *
 * rih_heatmaps: joints [maps][C] (C = 2: x, y; C = 3: x, y, v) -> hms [maps][R][R],
 *   hms[m][y][x] = exp(-((x - jx)^2 + (y - jy)^2) / (2 sigma^2)); the whole map is 0 when C = 3 and v <= 0, or when jx < 0,
 *   jy < 0, jx >= R or jy >= R (a joint exactly at 0 is drawn, one exactly at R is not).  sigma is the generator's
 *   sigma * scale.  RIH_EINVAL: a null pointer, maps < 1 or > 2^31, C not 2 or 3, R < 1 or > 4096, sigma <= 0.
 *
 * rih_aux_loss: calc_aux_loss and the gradient of its total in ONE pass: every operand read once, every gradient written once.
 *   predictions p_hms [B][Jh][S][S], p_mask [B][2][S][S], p_dense [B][6][S][S]; labels t_mask [B][2][S][S], t_dense
 *   [B][3][S][S], and for the heat maps EITHER t_hms [B][Jh][S][S] OR t_joints [B][Jh][C] with sigma (exactly one non-null):
 *   the target pixel is then produced in the kernel by the device function rih_heatmaps uses and no target tensor is read.
 *   With sl1 = SmoothL1(beta), mean over all elements, and mse = mean squared error:
 *     mask  = sl1(p_mask - t_mask)
 *     dense = 1/2 [ sl1(p_dense[:, 0:3] m0 - t_dense m0) + sl1(p_dense[:, 3:6] m1 - t_dense m1) ],  m0 = t_mask[:, 0:1],
 *             m1 = t_mask[:, 1:2] as FLOAT factors: the gradient is sl1'(d) m / count for any m
 *     hms   = mse(p_hms - t_hms)
 *     total = weights[0] mask + weights[1] dense + weights[2] hms
 *   weights [3] is a DEVICE array read at run time (a captured graph follows a change).  A term whose prediction pointer is NULL
 *   is absent: its value is 0 and its gradient is not written (its label and gradient pointers are ignored).
 *   Writes g_hms, g_mask, g_dense (d total / d prediction, shaped as the predictions) and partial [nblk][4] raw sums per
 *   workgroup, nblk = rih_aux_loss_blocks(B, Jh, S, p_hms != NULL, p_mask != NULL || p_dense != NULL) <= 2048 (0 for sizes
 *   the kernel refuses).
 * rih_aux_loss_final: ONE workgroup adds the partial sums in a fixed order: out [4] = total, mask, dense, hms.
 *   RIH_EINVAL: weights, partial or out NULL, every prediction NULL, B < 1 or > 2^20, S < 1 or > 4096, Jh < 1 or > 4096 with p_hms,
 *   beta <= 0, both or neither of t_hms / t_joints with p_hms, t_joints with C not 2 or 3 or sigma <= 0, a present term
 *   without its label or gradient pointer.
 *
 * rih_hms_decode: get_final_preds2.  hm [maps][H][W] -> preds [maps][2] (x, y), maxvals [maps]; one workgroup per map, the map
 *   in LDS (H * W * 4 <= 65536 bytes).  (1) arg-max of the raw map, the first flat index on ties, x = idx % W, y = idx / W;
 *   preds = (0, 0) when the maximum is <= 0.  (2) kernel > 1: zero-padded separable blur with OpenCV's fixed taps for
 *   sigma = 0 -- 3: (1, 2, 1)/4, 5: (1, 4, 6, 4, 1)/16, 7: (1, 3.5, 7, 9, 7, 3.5, 1)/32 -- then times raw_max / blurred_max.
 *   (3) log(max(., 1e-10)).  (4) only when 1 < x < W - 2 and 1 < y < H - 2: the five finite differences of
 *   inference.py:57-61 and offset = -Hessian^-1 gradient when dxx dyy - dxy^2 != 0 (the two products rounded separately).
 *   A map whose maximum is not positive gives preds = (0, 0) and maxvals = the maximum, never a NaN.  A map with a positive
 *   maximum whose BLURRED maximum is <= 0 (kernel > 1: an isolated positive pixel among large negatives) is rescaled by
 *   raw_max / blurred_max as the reference does, and its coordinates can then be inf or NaN, as the reference's.
 *   RIH_EINVAL: a null pointer, maps < 1 or > 2^31, H or W < 1, H * W > 16384, kernel not 1, 3, 5 or 7. */
int rih_heatmaps(const float* joints, float* hms, int64_t maps, int C, int R, float sigma, void* stream);
int rih_aux_loss_blocks(int B, int Jh, int S, int has_hms, int has_mask_or_dense);
int rih_aux_loss(const float* p_hms, const float* p_mask, const float* p_dense, const float* t_hms, const float* t_joints,
                 const float* t_mask, const float* t_dense, const float* weights, int B, int Jh, int S, int C, float sigma,
                 float beta, float* g_hms, float* g_mask, float* g_dense, float* partial, void* stream);
int rih_aux_loss_final(const float* partial, const float* weights, int B, int Jh, int S, int has_hms, int has_mask_or_dense,
                       float* out, void* stream);
int rih_hms_decode(const float* hm, float* preds, float* maxvals, int64_t maps, int H, int W, int kernel, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The image-to-overlay path of the demo (core/test_utils.py:46-128 `InterRender`, apps/demo.py:103-128; csrc/rih_demo.hip,
 * ABI 36; renderih_amd.demo).  uint8 BGR in, uint8 BGR out; one launch per call, no atomics, no host read, capturable.
 *
 * A ragged image batch is one packed uint8 buffer `src` of `src_bytes` bytes and a DEVICE table desc [B][RIH_DEMO_DESC] of
 * int64 rows: byte offset, H, W, pad_top, pad_left, PH, PW, reserved, ytab, xtab.  The padded image is
 * P[r][c] = I[r - pad_top][c - pad_left] inside the H x W x 3 image and 0 outside; PH x PW is its size.  A row whose image does
 * not lie inside [0, src_bytes), or whose H or W is outside 1 .. 32767, reads as black: no row can make the kernel read out of
 * bounds.  The 8-bit resize of P to Sy x Sx:
 *   PH == Sy and PW == Sx: copy.   PH == 2 Sy and PW == 2 Sx: (P[2y][2x] + P[2y][2x+1] + P[2y+1][2x] + P[2y+1][2x+1] + 2) >> 2.
 *   otherwise the taps come from `tabs`, a 16-byte aligned DEVICE array of tab_entries x 4 int32 (s, s', a0, a1): entries
 *   ytab .. ytab + Sy - 1 for the rows and xtab .. xtab + Sx - 1 for the columns (a range outside the array: black),
 *   T_r = P[r][s] a0 + P[r][s'] a1,  out = clamp((((b0 (T_s >> 4)) >> 16) + ((b1 (T_s' >> 4)) >> 16) + 2) >> 2, 0, 255)
 *   with (s, s', b0, b1) of the row entry.  The tables are built on the host (renderih_amd.demo.axis_table): integer work only
 *   on the device.  This restates cv::resize (CV_8U, INTER_LINEAR); conformity with an OpenCV build is unverified.
 *
 * rih_demo_resize: out [B][Sy][Sx][3] uint8.
 * rih_demo_prepare: `process_img` (pad2squre, resize, BGR -> RGB, / 255, (x - mean) / std in fp32 as rih_prepare_images) to
 *   S x S; each output may be NULL (not all): norm [B][3][S][S] fp32, norm_h8 [B][S][S][8] fp16 (16-byte aligned, lanes 3..7
 *   zero), out_u8 [B][S][S][3] the resized BGR image.
 * rih_demo_compose: out [B][R][R][3] uint8 = trunc(fl(fl(rgb 255) mask) + fl(back fl(1 - mask))), every operation rounded to
 *   fp32, saturated to 0 .. 255 (NaN -> 0; numpy wraps instead).  rgb: pixel i channel c at rgb[i rgb_ld + c], mask at
 *   mask[i mask_ld], i = (b R + y) R + x.  back = the image of row b of bg_desc resized to R x R, or 255 when bg is NULL.
 *   Channels are not swapped.
 * rih_demo_other_view: out [B][2V][3] = cat(v_left - c, v_right - c) Rot, c = (mean(v_left) + mean(v_right)) / 2 per sample;
 *   rot_host: 9 floats (row-major) in HOST memory, read before the launch.  Fixed summation order.
 * rih_demo_smooth: rows_host [E][6] int64 in HOST memory, E <= RIH_DEMO_SMOOTH_MAX: p, out, last, last_v, acc (device fp32
 *   pointers, n elements each; out may be p) and n.  stage = frames seen before: >= 3: out = 0.7 p + 0.3 (last + last_v + 0.5 acc),
 *   else out = p; then (stage >= 1) v = out - last, (stage >= 2) acc = v - last_v, last_v = v; last = out.
 * RIH_EINVAL: a null pointer, a size out of range (B 1 .. 65536, S / R 1 .. 32767), misaligned tabs or norm_h8. */
#define RIH_DEMO_DESC 10
#define RIH_DEMO_SMOOTH_MAX 16
int rih_demo_resize(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int32_t* tabs, int64_t tab_entries, int B,
                    int Sy, int Sx, uint8_t* out, void* stream);
int rih_demo_prepare(const uint8_t* src, int64_t src_bytes, const int64_t* desc, const int32_t* tabs, int64_t tab_entries, int B,
                     int S, float* norm, void* norm_h8, uint8_t* out_u8, void* stream);
int rih_demo_compose(const float* rgb, int64_t rgb_ld, const float* mask, int64_t mask_ld, const uint8_t* bg, int64_t bg_bytes,
                     const int64_t* bg_desc, const int32_t* tabs, int64_t tab_entries, int B, int R, uint8_t* out, void* stream);
int rih_demo_other_view(const float* v_left, const float* v_right, const float* rot_host, int B, int V, float* out,
                        void* stream);
int rih_demo_smooth(const int64_t* rows_host, int E, int stage, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RENDERIH_AMD_H */
