"""Test infrastructure: a numpy/torch-CPU emulation of the C ABI (include/renderih_amd.h) on host memory.

There is no GPU in the build container, so the host-side logic of `renderih_amd.ops` / the module tree (descriptor
geometry, strides, packing, split-K, backward formulas wiring, dropout seeds) is exercised on CPU by swapping the
loaded library for this object: every entry point is restated from the header's contract, reading and writing the
caller's tensors through their raw pointers.  It is NOT a product fallback -- only tests install it
(`with emulated_abi(): ...`), and the kernels themselves are still only proven by the `-m gpu` tests.
"""
import contextlib
import ctypes as C
import os
import numpy as np
import torch
import torch.nn.functional as F


def _f(ptr, n):
    return np.ctypeslib.as_array((C.c_float * int(n)).from_address(int(ptr)))


def _i32(ptr, n):
    return np.ctypeslib.as_array((C.c_int32 * int(n)).from_address(int(ptr)))


def _i8(ptr, n):
    return np.ctypeslib.as_array((C.c_int8 * int(n)).from_address(int(ptr)))


def hash_np(seed, idx):
    """numpy mirror of rih_hash (csrc/rih_hash.h): the lowbias32 finalizer of lo32(idx) ^ hi32(idx) * 0x85EBCA6B ^ keyA(seed) with
    keyB(seed) added between its two multiplies."""
    M32 = np.uint64(0xFFFFFFFF)

    def mix(x, kb=None):
        x = x.astype(np.uint64) & M32
        x ^= x >> np.uint64(16)
        x = (x * np.uint64(0x7feb352d)) & M32
        x ^= x >> np.uint64(15)
        if kb is not None:
            x = (x + kb) & M32
        x = (x * np.uint64(0x846ca68b)) & M32
        x ^= x >> np.uint64(16)
        return x
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo_s, hi_s = seed & 0xFFFFFFFF, seed >> 32
    ka = mix(np.array([lo_s], np.uint64)) ^ mix(np.array([hi_s ^ 0x9E3779B9], np.uint64))
    kb = (mix(np.array([lo_s ^ 0x85EBCA6B], np.uint64)) + mix(np.array([(hi_s + 0xC2B2AE35) & 0xFFFFFFFF], np.uint64))) & M32
    idx = np.asarray(idx).astype(np.uint64)
    lo, hi = idx & M32, idx >> np.uint64(32)
    return mix(lo ^ ka[0] ^ ((hi * np.uint64(0x85EBCA6B)) & M32), kb[0])


def keep_mask(seed, n, p):
    if p <= 0:
        return np.ones(n, np.float32)
    thr = np.uint64(min(int(float(np.float32(p)) * 4294967296.0), 4294967295))
    return (hash_np(seed, np.arange(n)) >= thr).astype(np.float32) / np.float32(1.0 - p)




class EmulatedLib:
    @staticmethod
    def _seed(seed, seed_dev):
        """seed + *seed_dev (mod 2^64), the device-side seed word being host memory under emulation."""
        if seed_dev:
            seed = (int(seed) + int(np.ctypeslib.as_array((C.c_uint64 * 1).from_address(int(seed_dev)))[0])) % (1 << 64)
        return seed

    # ------------------------------------------------------------------ GEMM family
    def _gather(self, base, idx, valid):
        n = int(idx[valid].max()) + 1 if valid.any() else 1
        mem = _f(base, n)
        out = np.zeros(idx.shape, np.float32)
        out[valid] = mem[idx[valid]]
        return out

    def rih_gemm(self, dref, stream):
        d = dref._obj
        M, N, K = d.M, d.N, d.K
        taps = d.KH * d.KW
        assert d.splitk >= 1 and (taps == 1 or d.Cin % 4 == 0)
        if d.a_seg[0] and (d.engine < 1 or d.tile > 2 or d.a_mode != 0 or d.b_mode != 1 or d.nb1 * d.nb2 != 1 or d.splitk != 1):
            return -1           # RIH_EINVAL: only the split engines' fast path reads a segmented A (csrc/rih_gemm.hip gemm_impl)
        if d.a_mode not in (0, 1) or d.b_mode not in (0, 1):
            return -1           # RIH_EINVAL (gemm_impl): fp32 operands only, row-major either way
        for b1 in range(d.nb1):
            for b2 in range(d.nb2):
                Ab = d.A + 4 * (b1 * d.sA1 + b2 * d.sA2)
                Bb = d.B + 4 * (b1 * d.sB1 + b2 * d.sB2)
                Cb = d.C + 4 * (b1 * d.sC1 + b2 * d.sC2)
                plain = (taps == 1 and d.strideA == 1 and d.upS == 1 and d.padH == 0 and d.padW == 0 and d.H == d.Ho
                         and d.W == d.Wo)
                A = None
                if d.a_seg[0]:
                    # segmented A: [A | a_seg[0] | a_seg[1] | a_seg[2]] along K, plain row-major pieces
                    assert plain and d.a_mode == 0 and d.b_mode == 1 and d.nb1 * d.nb2 == 1 and d.splitk == 1
                    starts = [0] + [d.k_seg[i] for i in range(3) if d.a_seg[i]] + [K]
                    bases = [Ab] + [d.a_seg[i] for i in range(3) if d.a_seg[i]]
                    ldas = [d.lda] + [d.lda_seg[i] for i in range(3) if d.a_seg[i]]
                    A = np.empty((M, K), np.float32)
                    for base, ld, k0, k1 in zip(bases, ldas, starts[:-1], starts[1:]):
                        assert k0 % 32 == 0 and k1 > k0
                        A[:, k0:k1] = np.lib.stride_tricks.as_strided(_f(base, (M - 1) * ld + (k1 - k0)), (M, k1 - k0), (4 * ld, 4))
                elif plain and d.a_mode == 0 and K > 0:
                    # fast path (the emulation's only optimisation): dense rows, no gather -- A[m, k] = mem[m * lda + k]
                    A = np.lib.stride_tricks.as_strided(_f(Ab, (M - 1) * d.lda + K), (M, K), (4 * d.lda, 4)).copy()
                elif plain and d.a_mode == 1 and K > 0:
                    rows = d.ones_row if d.ones_row > 0 else M          # A[m, k] = mem[k * lda + m]; rows >= ones_row are not read
                    A = np.zeros((M, K), np.float32)
                    A[:rows] = np.lib.stride_tricks.as_strided(_f(Ab, (K - 1) * d.lda + rows), (rows, K), (4, 4 * d.lda))
                if A is not None:
                    pass
                elif d.a_mode != 1:
                    m = np.arange(M)
                    wo, t = m % d.Wo, m // d.Wo
                    ho, img = t % d.Ho, t // d.Ho
                    k = np.arange(K)
                    tap, ci = k // d.Cin, k % d.Cin
                    kh, kw = tap // d.KW, tap % d.KW
                    hi = (ho * d.strideA - d.padH)[:, None] + kh[None, :]
                    wi = (wo * d.strideA - d.padW)[:, None] + kw[None, :]
                    valid = (hi >= 0) & (wi >= 0) & (hi % d.upS == 0) & (wi % d.upS == 0) & (tap < taps)[None, :]
                    hi, wi = hi // d.upS, wi // d.upS
                    valid &= (hi < d.H) & (wi < d.W)
                    idx = ((img[:, None] * d.H + hi) * d.W + wi) * d.lda + ci[None, :]
                else:
                    m = np.arange(M)
                    tap, ci = m // d.Cin, m % d.Cin
                    kh, kw = tap // d.KW, tap % d.KW
                    k = np.arange(K)
                    wo, t = k % d.Wo, k // d.Wo
                    ho, img = t % d.Ho, t // d.Ho
                    hi = (ho * d.strideA - d.padH)[None, :] + kh[:, None]
                    wi = (wo * d.strideA - d.padW)[None, :] + kw[:, None]
                    valid = (hi >= 0) & (wi >= 0) & (hi < d.H) & (wi < d.W) & (tap < taps)[:, None]
                    idx = ((img[None, :] * d.H + hi) * d.W + wi) * d.lda + ci[:, None]
                    if d.ones_row > 0:      # rows >= ones_row are not read from memory
                        valid[d.ones_row:] = False
                if A is None:
                    idx = np.where(valid, idx, 0)
                    A = self._gather(Ab, idx, valid)
                if d.a_mode == 1 and d.ones_row > 0:
                    A[d.ones_row, :] = 1.0
                if K == 0:
                    Bm = np.zeros((0, N), np.float32)
                elif d.b_mode == 0:     # B[k, n] = mem[k * ldb + n]
                    Bm = np.lib.stride_tricks.as_strided(_f(Bb, (K - 1) * d.ldb + N), (K, N), (4 * d.ldb, 4))
                else:                   # B[k, n] = mem[n * ldb + k]
                    Bm = np.lib.stride_tricks.as_strided(_f(Bb, (N - 1) * d.ldb + K), (K, N), (4, 4 * d.ldb))
                crow = np.arange(M)
                if d.cS > 1:        # strided output rows (parity class of a strided-conv data gradient)
                    assert d.a_mode != 1 and d.splitk == 1 and not d.R
                    cj, ct = crow % d.Wo, crow // d.Wo
                    ci_, cimg = ct % d.Ho, ct // d.Ho
                    crow = (cimg * d.cH + ci_ * d.cS + d.cOH) * d.cW + cj * d.cS + d.cOW
                def c_window(base):     # the [M][N] window of C as a writable strided view (dense rows) or via row indices
                    if d.cS > 1:
                        return None
                    return np.lib.stride_tricks.as_strided(_f(base, (M - 1) * d.ldc + N), (M, N), (4 * d.ldc, 4))
                if d.splitk > 1:
                    assert d.kchunk % 32 == 0
                    for s in range(d.splitk):
                        k0, k1 = s * d.kchunk, min(K, (s + 1) * d.kchunk)
                        c_window(Cb + 4 * s * d.sCsplit)[:] = A[:, k0:k1] @ Bm[k0:k1]
                    continue
                out = np.float32(d.alpha) * (A @ Bm)
                if d.bias:
                    out = out + _f(d.bias + 4 * b1 * d.sBias1, N)[None, :]
                if d.drop_p != 0:        # dropout epilogue: act -> mask stream over the output (offset from d.C) -> + R
                    assert self.rih_gemm_dropout_ok(dref) == 1 and not (d.relu and d.R), 'descriptor without the dropout path'
                    if d.relu:
                        out = np.maximum(out, 0)
                    e = ((Cb - d.C) // 4 + np.arange(M)[:, None] * d.ldc + np.arange(N)[None, :]).astype(np.uint64)
                    seed = (int(d.drop_seed) + (int(np.ctypeslib.as_array((C.c_uint64 * 1).from_address(int(d.drop_seed_dev)))[0])
                                                if d.drop_seed_dev else 0)) & 0xFFFFFFFFFFFFFFFF
                    pf = np.float32(d.drop_p)
                    thr = np.uint64(min(int(float(pf) * 4294967296.0), 4294967295))
                    keep = hash_np(seed, e.ravel()).reshape(M, N) >= thr
                    out = np.where(keep, out.astype(np.float32) * (np.float32(1.0) / (np.float32(1.0) - pf)), np.float32(0))
                if d.R:
                    out = out + np.lib.stride_tricks.as_strided(_f(d.R + 4 * b1 * d.sR1, (M - 1) * d.ldr + N), (M, N),
                                                                (4 * d.ldr, 4))
                if d.relu and d.drop_p == 0:
                    out = np.maximum(out, 0)
                win = c_window(Cb)
                if win is not None:
                    win[:] = out
                else:
                    cm, cn = np.meshgrid(crow, np.arange(N), indexing='ij')
                    mem = _f(Cb, int(crow.max()) * d.ldc + N)
                    mem[(cm * d.ldc + cn).ravel()] = out.astype(np.float32).ravel()
                if d.stats:         # statistics epilogue: column sums / sums of squares per block of stats_rows GEMM rows
                    rp = self.rih_gemm_stats_rows(dref)
                    assert rp > 0, 'stats requested on a descriptor without the statistics path'
                    T = -(-M // rp)
                    st = _f(d.stats, T * 2 * N).reshape(T, 2, N)
                    o32 = out.astype(np.float32)
                    for t in range(T):
                        blk = o32[t * rp:(t + 1) * rp].astype(np.float64)
                        st[t, 0], st[t, 1] = blk.mean(0), ((blk - blk.mean(0)) ** 2).sum(0)
        return 0

    # grouped launch (rih_gemm_multi_*): the contract restated -- weight-gradient descriptors of one variant, a table in "device"
    # memory that stands for the packed problems, one launch that runs them all
    def rih_gemm_multi_variant(self, dref):
        d = dref._obj if hasattr(dref, '_obj') else dref
        plain = (d.KH == 1 and d.KW == 1 and d.strideA == 1 and d.padH == 0 and d.padW == 0 and d.H == d.Ho and d.W == d.Wo)
        ok = (d.engine in (1, 2) and (d.tile in (0, 2) or (d.tile == 1 and d.engine == 2)) and d.a_mode == 1 and d.b_mode == 0 and d.upS == 1 and d.K % 4 == 0
              and d.K >= 1 and d.A % 16 == 0 and d.B % 16 == 0 and d.lda % 4 == 0 and d.ldb % 4 == 0 and d.sA1 % 4 == 0
              and d.sB1 % 4 == 0 and d.sA2 % 4 == 0 and d.sB2 % 4 == 0 and d.M % 4 == 0 and d.N % 4 == 0 and not d.stats)
        if not plain:
            ok = ok and d.Wo % 4 == 0 and d.Cin % 4 == 0
        return (d.tile * 8 + 4 + (1 if plain else 0) + (64 if d.engine == 2 else 0)) if ok else -1

    def rih_gemm_engine(self, dref):
        """The header's contract, restated: engine 2 exists on the fast path of tiles 0..2 only, engine 1 runs otherwise."""
        d = dref._obj if hasattr(dref, '_obj') else dref
        if d.engine == 0 or d.tile == 3:
            return 0
        plain = (d.KH == 1 and d.KW == 1 and d.strideA == 1 and d.padH == 0 and d.padW == 0 and d.H == d.Ho and d.W == d.Wo)
        fast = (d.tile in (0, 1, 2) and d.upS == 1 and d.K % 4 == 0 and d.K >= 1 and d.A % 16 == 0 and d.B % 16 == 0
                and d.lda % 4 == 0 and d.ldb % 4 == 0 and d.sA1 % 4 == 0 and d.sB1 % 4 == 0 and d.sA2 % 4 == 0 and d.sB2 % 4 == 0)
        if d.a_mode != 1 and not plain:
            fast = fast and d.Cin % 32 == 0 and d.KH * d.KW <= 32
        if d.a_mode == 1:
            fast = fast and d.M % 4 == 0 and (plain or (d.Wo % 4 == 0 and d.Cin % 4 == 0))
        if d.b_mode == 0:
            fast = fast and d.N % 4 == 0
        return 2 if (d.engine == 2 and fast) else 1

    def rih_absmax_multi(self, descs, n, stream):
        for i in range(n):
            self.rih_absmax(descs[i].x, descs[i].n, descs[i].out, stream)
        return 0

    def rih_absmax(self, x, n, out, stream):
        if n > 0:
            o = _f(out, 1)
            v = np.abs(_f(x, n))
            v = v[~np.isnan(v)]
            if v.size:
                o[0] = max(float(o[0]), float(v.max()))
        return 0

    def rih_gemm_multi_table_bytes(self, descs, n):
        return 64 + 8 * n if n >= 1 else 0

    def rih_gemm_multi_pack(self, descs, n, host_table, total_blocks):
        vs = {self.rih_gemm_multi_variant(descs[i]) for i in range(n)}
        if len(vs) != 1 or -1 in vs:
            return -1
        copies = []
        for i in range(n):
            c = type(descs[i])()
            C.memmove(C.byref(c), C.byref(descs[i]), C.sizeof(c))
            copies.append(c)
        reg = self.__dict__.setdefault('_multi', {})
        key = len(reg) + 1
        reg[key] = copies
        np.ctypeslib.as_array((C.c_int64 * 1).from_address(int(host_table)))[0] = key
        total_blocks._obj.value = 8 * n
        return vs.pop()

    def rih_gemm_multi_launch(self, table, variant, total_blocks, stream):
        key = int(np.ctypeslib.as_array((C.c_int64 * 1).from_address(int(table)))[0])
        for c in self._multi[key]:
            assert self.rih_gemm_multi_variant(c) == variant
            self.rih_gemm(C.byref(c), stream)
        return 0

    def rih_gemm_stats_rows(self, dref):
        """The header's contract, restated: split engine's fast path, forward-type, no split-K, no batch, dense rows."""
        d = dref._obj
        plain = (d.KH == 1 and d.KW == 1 and d.strideA == 1 and d.padH == 0 and d.padW == 0 and d.H == d.Ho and d.W == d.Wo)
        ok = (d.engine in (1, 2) and d.tile in (0, 1, 2) and d.a_mode == 0
              and d.b_mode in (0, 1) and d.splitk == 1
              and d.nb1 * d.nb2 == 1 and d.cS <= 1 and d.upS == 1 and d.K % 4 == 0 and d.K >= 1
              and d.A % 16 == 0 and d.B % 16 == 0 and d.lda % 4 == 0 and d.ldb % 4 == 0)
        if not plain:
            ok = ok and d.Cin % 32 == 0 and d.KH * d.KW <= 32
        if d.b_mode == 0:
            ok = ok and d.N % 4 == 0
        return (64 if d.tile in (0, 1) else 32) if ok else 0

    def rih_gemm_dropout_ok(self, dref):
        """The header's contract, restated: split engine's fast path, plain row-major A, no split-K, no stats, dense rows."""
        d = dref._obj if hasattr(dref, '_obj') else dref
        plain = (d.KH == 1 and d.KW == 1 and d.strideA == 1 and d.padH == 0 and d.padW == 0 and d.H == d.Ho and d.W == d.Wo)
        ok = (d.engine in (1, 2) and d.tile in (0, 1, 2) and d.a_mode == 0 and d.b_mode in (0, 1) and d.splitk == 1 and plain
              and d.cS <= 1 and d.upS == 1 and d.K % 4 == 0 and d.K >= 1 and d.A % 16 == 0 and d.B % 16 == 0
              and d.lda % 4 == 0 and d.ldb % 4 == 0 and d.sA1 % 4 == 0 and d.sB1 % 4 == 0 and d.sA2 % 4 == 0 and d.sB2 % 4 == 0
              and not (d.relu and d.R))
        if d.b_mode == 0:
            ok = ok and d.N % 4 == 0
        return 1 if ok else 0

    def rih_bn_stats_from_blocks(self, part, T, Cc, rows, rpb, eps, momentum, mean, invstd, rmean, rvar, stream):
        p = _f(part, T * 2 * Cc).reshape(T, 2, Cc).astype(np.float64)
        nk = np.full(T, rpb, np.float64)
        nk[-1] = rows - (T - 1) * rpb
        m = (nk[:, None] * p[:, 0]).sum(0) / rows
        var = np.maximum((p[:, 1].sum(0) + (nk[:, None] * p[:, 0] ** 2).sum(0) - rows * m * m) / rows, 0.0)
        _f(mean, Cc)[:] = m
        _f(invstd, Cc)[:] = 1.0 / np.sqrt(var + eps)
        if rmean:
            unb = var * rows / (rows - 1.0) if rows > 1 else var
            _f(rmean, Cc)[:] = (1.0 - momentum) * _f(rmean, Cc) + momentum * m
            _f(rvar, Cc)[:] = (1.0 - momentum) * _f(rvar, Cc) + momentum * unb
        return 0

    @staticmethod
    def _e2_scale(amax):
        """The power of two rih_gemm engine 2 derives from a bound block: s * bound in [2^14, 2^15)."""
        if not amax:
            return np.float32(1.0)
        a = float(_f(amax, 2048)[::32].max())
        if not (a > 0 and np.isfinite(a)):
            return np.float32(1.0)
        e = int(np.floor(np.log2(a)))
        if e < -126:
            return np.float32(1.0)
        return np.float32(2.0 ** min(14 - e, 126))

    # ------------------------------------------------------------------ halo-resident 3x3 convolution (csrc/rih_conv3.hip)
    def rih_h2_multi(self, descs, n, stream):
        """OIHW weight -> H2 planes dst[n][k / 8][plane][8 halves] (hi = fp16(s w), lo = fp16((s w - hi) 2^11))."""
        for i in range(n):
            d = descs[i]
            if not (d.w and d.dst and d.amax) or d.Kpad % 32 != 0 or d.CinPad < d.Cin:
                return -1
            W = _f(d.w, d.Cout * d.Cin * d.KH * d.KW).reshape(d.Cout, d.Cin, d.KH, d.KW)
            Wp = np.zeros((d.Cout, d.CinPad, d.KH, d.KW), np.float32)
            Wp[:, :d.Cin] = W
            if not d.for_dgrad:
                Bnk = Wp.transpose(0, 2, 3, 1).reshape(d.Cout, d.KH * d.KW * d.CinPad)           # n = co, k = (tap, ci)
            else:
                Bnk = Wp[:, :, ::-1, ::-1].transpose(1, 2, 3, 0).reshape(d.CinPad, d.KH * d.KW * d.Cout)   # n = ci, k = (flipped tap, co)
            N, K = Bnk.shape
            if d.Kpad < K:
                return -1
            x = np.zeros((N, d.Kpad), np.float32)
            x[:, :K] = Bnk
            xs = x * self._e2_scale(d.amax)
            hi = xs.astype(np.float16)
            lo = ((xs - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
            out = np.ctypeslib.as_array((C.c_uint16 * (2 * N * d.Kpad)).from_address(int(d.dst))).reshape(N, d.Kpad // 8, 2, 8)
            out[:, :, 0, :] = hi.view(np.uint16).reshape(N, d.Kpad // 8, 8)
            out[:, :, 1, :] = lo.view(np.uint16).reshape(N, d.Kpad // 8, 8)
        return 0

    @staticmethod
    def _conv3_ok(d):
        return bool(d.x and d.w_h2 and d.y and d.amax_x and d.amax_w and d.imgs >= 1
                    and ((d.H % 8 == 0 and d.W % 32 == 0) or (d.H % 16 == 0 and d.W % 16 == 0)) and d.H >= 8 and d.W >= 16
                    and d.C >= 32 and d.C % 32 == 0 and d.N >= 32 and d.N % 32 == 0 and d.ldx >= d.C
                    and d.ldx % 4 == 0 and d.ldy >= d.N and d.ldy % 4 == 0 and d.Kpad == 9 * d.C
                    and d.x % 16 == 0 and d.w_h2 % 16 == 0 and d.y % 16 == 0 and (not d.stats or d.stats % 16 == 0)
                    and (not d.r or (not d.stats and d.ldr >= d.N and d.ldr % 4 == 0 and d.r % 16 == 0)))

    def rih_conv3x3_ok(self, dref):
        return 1 if self._conv3_ok(dref._obj if hasattr(dref, '_obj') else dref) else 0

    @staticmethod
    def _conv3_geom(d):
        """(patch rows, patch width, channel block) as csrc/rih_conv3.hip chooses them."""
        tw = 32 if (d.H % 8 == 0 and d.W % 32 == 0) else 16
        patches = d.imgs * (d.H // (256 // tw)) * (d.W // tw)
        bn = 128 if (d.N % 128 == 0 and patches * (d.N // 128) >= 256) else 64 if d.N % 64 == 0 else 32
        return 256 // tw, tw, bn

    def rih_conv3x3_stats_rows(self, dref):
        d = dref._obj if hasattr(dref, '_obj') else dref
        if not self._conv3_ok(d):
            return 0
        return 64 if self._conv3_geom(d)[2] >= 64 else 32

    def rih_conv3x3(self, dref, stream):
        d = dref._obj
        if not self._conv3_ok(d):
            return -1
        sw = self._e2_scale(d.amax_w)
        pl = np.ctypeslib.as_array((C.c_uint16 * (2 * d.N * d.Kpad)).from_address(int(d.w_h2))).reshape(d.N, d.Kpad // 8, 2, 8)
        hi = pl[:, :, 0, :].reshape(d.N, d.Kpad).view(np.float16).astype(np.float32)
        lo = pl[:, :, 1, :].reshape(d.N, d.Kpad).view(np.float16).astype(np.float32)
        Wnk = ((hi + lo * np.float32(2.0 ** -11)) / sw).astype(np.float32)           # [N][(tap, c)]
        x = np.lib.stride_tricks.as_strided(_f(d.x, ((d.imgs * d.H * d.W) - 1) * d.ldx + d.C), (d.imgs, d.H, d.W, d.C),
                                            (4 * d.H * d.W * d.ldx, 4 * d.W * d.ldx, 4 * d.ldx, 4))
        xp = np.zeros((d.imgs, d.H + 2, d.W + 2, d.C), np.float32)
        xp[:, 1:-1, 1:-1] = x
        y = np.zeros((d.imgs, d.H, d.W, d.N), np.float32)
        for kh in range(3):
            for kw in range(3):
                t = kh * 3 + kw
                y += xp[:, kh:kh + d.H, kw:kw + d.W].reshape(-1, d.C).dot(Wnk[:, t * d.C:(t + 1) * d.C].T).reshape(y.shape)
        if d.r:             # the residual joins before the ReLU
            y = y + np.lib.stride_tricks.as_strided(_f(d.r, ((d.imgs * d.H * d.W) - 1) * d.ldr + d.N), (d.imgs, d.H, d.W, d.N),
                                                    (4 * d.H * d.W * d.ldr, 4 * d.W * d.ldr, 4 * d.ldr, 4))
        if d.relu:
            y = np.maximum(y, 0)
        out = np.lib.stride_tricks.as_strided(_f(d.y, ((d.imgs * d.H * d.W) - 1) * d.ldy + d.N), (d.imgs, d.H, d.W, d.N),
                                              (4 * d.H * d.W * d.ldy, 4 * d.W * d.ldy, 4 * d.ldy, 4))
        out[...] = y
        if d.stats:
            # blocks = consecutive runs of `rows` pixels of a patch in patch-row-major order: block ((img, ty, tx), wm)
            th, tw, bn = self._conv3_geom(d)
            rows = 64 if bn >= 64 else 32
            T = d.imgs * d.H * d.W // rows
            st = _f(d.stats, T * 2 * d.N).reshape(T, 2, d.N)
            blk = y.reshape(d.imgs, d.H // th, th, d.W // tw, tw, d.N).transpose(0, 1, 3, 2, 4, 5).reshape(T, rows, d.N)
            m = blk.astype(np.float64).mean(1)
            st[:, 0] = m
            st[:, 1] = ((blk - m[:, None]) ** 2).sum(1)
        return 0

    # ------------------------------------------------------------------ stem convolution (csrc/rih_conv3.hip rows_kernel<STEM>)
    @staticmethod
    def _stem_ok(d):
        M = d.imgs * (d.H // 2) * (d.W // 2)
        return bool(d.x and d.w_h2 and d.y and d.amax_x and d.amax_w and d.imgs >= 1 and d.H >= 8 and d.W >= 8 and d.H % 2 == 0
                    and d.W % 2 == 0 and d.C == 4 and d.ldx == 4 and d.N == 64 and d.ldy >= d.N and d.ldy % 4 == 0 and d.Kpad == 224
                    and all(int(v or 0) % 16 == 0 for v in (d.x, d.w_h2, d.y, d.stats)) and M % 256 == 0
                    and d.imgs * d.H * d.W * 16 < (1 << 31) and not d.r)

    def rih_stem_ok(self, dref):
        return 1 if self._stem_ok(dref._obj if hasattr(dref, '_obj') else dref) else 0

    def rih_stem(self, dref, stream):
        d = dref._obj
        if not self._stem_ok(d):
            return -1
        sw = self._e2_scale(d.amax_w)
        pl = np.ctypeslib.as_array((C.c_uint16 * (2 * d.N * d.Kpad)).from_address(int(d.w_h2))).reshape(d.N, d.Kpad // 8, 2, 8)
        hi = pl[:, :, 0, :].reshape(d.N, d.Kpad).view(np.float16).astype(np.float32)
        lo = pl[:, :, 1, :].reshape(d.N, d.Kpad).view(np.float16).astype(np.float32)
        Wnk = ((hi + lo * np.float32(2.0 ** -11)) / sw).astype(np.float32)           # [N][(tap, c)], taps 49..55 zero
        x = _f(d.x, d.imgs * d.H * d.W * 4).reshape(d.imgs, d.H, d.W, 4)
        xp = np.zeros((d.imgs, d.H + 6, d.W + 6, 4), np.float32)
        xp[:, 3:-3, 3:-3] = x
        Ho, Wo = d.H // 2, d.W // 2
        y = np.zeros((d.imgs, Ho, Wo, d.N), np.float32)
        for kh in range(7):
            for kw in range(7):
                t = kh * 7 + kw
                y += xp[:, kh:kh + d.H:2, kw:kw + d.W:2].reshape(-1, 4).dot(Wnk[:, t * 4:(t + 1) * 4].T).reshape(y.shape)
        if d.relu:
            y = np.maximum(y, 0)
        M = d.imgs * Ho * Wo
        np.lib.stride_tricks.as_strided(_f(d.y, (M - 1) * d.ldy + d.N), (M, d.N), (4 * d.ldy, 4))[...] = y.reshape(M, d.N)
        if d.stats:
            T = M // 64
            st = _f(d.stats, T * 2 * d.N).reshape(T, 2, d.N)
            blk = y.reshape(T, 64, d.N)
            m = blk.astype(np.float64).mean(1)
            st[:, 0] = m
            st[:, 1] = ((blk - m[:, None]) ** 2).sum(1)
        return 0

    # ------------------------------------------------------------------ short-K streaming GEMM (csrc/rih_conv3.hip panel_kernel)
    @staticmethod
    def _panel_ok(d):
        return bool(d.a and d.w_h2 and d.c and d.amax_a and d.amax_w and d.K in (64, 128) and d.N >= 64 and d.N % 64 == 0
                    and not (d.K == 128 and d.N % 128 != 0) and d.M >= 128 and d.M % 128 == 0 and d.lda >= d.K and d.lda % 4 == 0
                    and d.ldc >= d.N and d.ldc % 4 == 0 and (not d.r or (d.ldr >= d.N and d.ldr % 4 == 0))
                    and all(int(x or 0) % 16 == 0 for x in (d.a, d.w_h2, d.c, d.r, d.stats)) and not (d.stats and d.r))

    def rih_panel_ok(self, dref):
        return 1 if self._panel_ok(dref._obj if hasattr(dref, '_obj') else dref) else 0

    def rih_panel_stats_rows(self, dref):
        d = dref._obj if hasattr(dref, '_obj') else dref
        if not self._panel_ok(d):
            return 0
        cap = 16384 // d.K
        bn = 256 if (d.N % 256 == 0 and cap >= 256) else 128 if (d.N % 128 == 0 and cap >= 128) else 64
        return (8192 // d.K) // (2 if bn >= 128 else 4)

    def rih_panel(self, dref, stream):
        d = dref._obj
        if not self._panel_ok(d):
            return -1
        return self._panel_like(d, self.rih_panel_stats_rows)

    # ------------------------------------------------------------------ long-K plain-row GEMM (csrc/rih_conv3.hip rows_kernel)
    @staticmethod
    def _rows_ok(d):
        return bool(d.a and d.w_h2 and d.c and d.amax_a and d.amax_w and d.K >= 64 and d.K % 32 == 0 and d.N >= 64 and d.N % 64 == 0
                    and d.M >= 128 and d.M % 128 == 0 and d.lda >= d.K and d.lda % 4 == 0 and d.ldc >= d.N and d.ldc % 4 == 0
                    and (not d.r or (d.ldr >= d.N and d.ldr % 4 == 0)) and 4 * d.M * d.lda < (1 << 31)
                    and all(int(x or 0) % 16 == 0 for x in (d.a, d.w_h2, d.c, d.r, d.stats)) and not (d.stats and d.r))

    @staticmethod
    def _rows_tile(d):
        n128, m256 = d.N % 128 == 0, d.M % 256 == 0
        wgs = lambda m, n: (d.M // m) * (d.N // n)
        if n128 and m256 and wgs(256, 128) >= 256:
            return 256, 128
        if n128 and wgs(128, 128) >= 256:
            return 128, 128
        if m256 and wgs(256, 64) >= 256:
            return 256, 64
        if wgs(128, 64) >= 256 or not n128:
            return 128, 64
        return 128, 128

    def rih_rows_ok(self, dref):
        return 1 if self._rows_ok(dref._obj if hasattr(dref, '_obj') else dref) else 0

    def rih_rows_stats_rows(self, dref):
        d = dref._obj if hasattr(dref, '_obj') else dref
        return self._rows_tile(d)[0] // 4 if self._rows_ok(d) else 0

    def rih_rows(self, dref, stream):
        d = dref._obj
        if not self._rows_ok(d):
            return -1
        return self._panel_like(d, self.rih_rows_stats_rows)

    def rih_rows_tile(self, dref, bm, bn):
        d = dref._obj if hasattr(dref, '_obj') else dref
        if not self._rows_ok(d):
            return 0
        (bm._obj if hasattr(bm, '_obj') else bm).value, (bn._obj if hasattr(bn, '_obj') else bn).value = self._rows_tile(d)
        return 1

    def rih_rows_tiled(self, dref, bm, bn, stream):
        d = dref._obj if hasattr(dref, '_obj') else dref
        if not self._rows_ok(d) or (bm, bn) not in ((256, 128), (128, 128), (256, 64), (128, 64)) or d.M % bm or d.N % bn:
            return -1
        return self._panel_like(d, lambda _d: bm // 4)

    def _panel_like(self, d, stats_rows):
        sw = self._e2_scale(d.amax_w)
        pl = np.ctypeslib.as_array((C.c_uint16 * (2 * d.N * d.K)).from_address(int(d.w_h2))).reshape(d.N, d.K // 8, 2, 8)
        hi = pl[:, :, 0, :].reshape(d.N, d.K).view(np.float16).astype(np.float32)
        lo = pl[:, :, 1, :].reshape(d.N, d.K).view(np.float16).astype(np.float32)
        Wnk = ((hi + lo * np.float32(2.0 ** -11)) / sw).astype(np.float32)
        A = np.lib.stride_tricks.as_strided(_f(d.a, (d.M - 1) * d.lda + d.K), (d.M, d.K), (4 * d.lda, 4))
        y = A.dot(Wnk.T)
        if d.r:
            y = y + np.lib.stride_tricks.as_strided(_f(d.r, (d.M - 1) * d.ldr + d.N), (d.M, d.N), (4 * d.ldr, 4))
        if d.relu:
            y = np.maximum(y, 0)
        np.lib.stride_tricks.as_strided(_f(d.c, (d.M - 1) * d.ldc + d.N), (d.M, d.N), (4 * d.ldc, 4))[...] = y
        if d.stats:
            rows = stats_rows(d)
            T = d.M // rows
            st = _f(d.stats, T * 2 * d.N).reshape(T, 2, d.N)
            blk = y.reshape(T, rows, d.N)
            m = blk.astype(np.float64).mean(1)
            st[:, 0] = m
            st[:, 1] = ((blk - m[:, None]) ** 2).sum(1)
        return 0

    def rih_splitk_reduce(self, P, S, M, N, dst, Cin, taps, CinValid, accumulate, stream):
        return self.rih_splitk_reduce_bias(P, S, M, M, N, dst, Cin, taps, CinValid, accumulate, 0, stream)

    def rih_splitk_reduce_bias_batched(self, P, S, Mp, M, N, dst, Cin, taps, CinValid, accumulate, db, nb, sP, sDst, sDb,
                                       stream):
        for b in range(nb):
            self.rih_splitk_reduce_bias(P + 4 * b * sP, S, Mp, M, N, dst + 4 * b * sDst, Cin, taps, CinValid, accumulate,
                                        db + 4 * b * sDb if db else 0, stream)
        return 0

    def rih_adam_chunk(self):
        return 4096

    def rih_adam_multi(self, table, blk_tensor, blk_chunk, nblocks, lr, beta1, beta2, eps, wd, step, adamw, stream):
        bt, bc = _i32(blk_tensor, nblocks), _i32(blk_chunk, nblocks)
        nt = int(bt.max()) + 1
        tab = np.ctypeslib.as_array((C.c_int64 * (5 * nt)).from_address(int(table))).reshape(nt, 5)
        f = np.float32
        lr, beta1, beta2, eps, wd = f(lr), f(beta1), f(beta2), f(eps), f(wd)
        step_size = f(float(lr) / (1.0 - float(beta1) ** step))
        isb2 = f(1.0 / np.sqrt(1.0 - float(beta2) ** step))
        seen = set()
        for b in range(nblocks):
            t, c = int(bt[b]), int(bc[b])
            assert (t, c) not in seen
            seen.add((t, c))
            pp, gp, mp, vp, n = (int(x) for x in tab[t])
            lo, hi = c * 4096, min(n, (c + 1) * 4096)
            assert lo < hi
            p, g, m, v = _f(pp, n)[lo:hi], _f(gp, n)[lo:hi].copy(), _f(mp, n)[lo:hi], _f(vp, n)[lo:hi]
            if wd != 0:
                if adamw:
                    p *= f(1) - lr * wd
                else:
                    g += wd * p
            m += (g - m) * (f(1) - beta1)
            v[:] = v * beta2 + (f(1) - beta2) * g * g
            p -= step_size * (m / (np.sqrt(v) * isb2 + eps))
        # every chunk of every tensor is covered exactly once
        assert len(seen) == sum((int(n) + 4095) // 4096 for n in tab[:, 4])
        return 0

    def rih_splitk_reduce_multi(self, descs, n, stream):
        for i in range(n):
            d = descs[i]
            self.rih_splitk_reduce_bias(d.P, d.S, d.Mp, d.M, d.N, d.dst, d.Cin, d.taps, d.CinValid, d.accumulate, d.db or 0,
                                        stream, pitch=d.CinPitch)
        return 0

    def rih_splitk_reduce_bias(self, P, S, Mp, M, N, dst, Cin, taps, CinValid, accumulate, db, stream, pitch=0):
        p = _f(P, S * Mp * N).reshape(S, Mp, N).sum(0)
        if db:
            _f(db, N)[:] = p[M]
        p = p[:M]
        pitch = pitch or CinValid           # > CinValid: dst is a column slice of a wider parameter
        out = _f(dst, ((N - 1) * pitch + CinValid) * taps)
        m = np.arange(M)
        tap, ci = m // Cin, m % Cin
        ok = ci < CinValid
        o = ((np.arange(N)[None, :] * pitch + ci[ok][:, None]) * taps + tap[ok][:, None]).ravel()     # [rows ok][N], unique
        v = p[ok].ravel()
        out[o] = (out[o] + v) if accumulate else v
        return 0

    def rih_splitk_finish(self, P, S, M, N, Cp, ldc, bias, R, ldr, alpha, relu, stream):
        out = np.float32(alpha) * _f(P, S * M * N).reshape(S, M, N).sum(0)
        cm, cn = np.meshgrid(np.arange(M), np.arange(N), indexing='ij')
        if bias:
            out = out + _f(bias, N)[None, :]
        if R:
            out = out + _f(R, (M - 1) * ldr + N)[(cm * ldr + cn).ravel()].reshape(M, N)
        if relu:
            out = np.maximum(out, 0)
        _f(Cp, (M - 1) * ldc + N)[(cm * ldc + cn).ravel()] = out.astype(np.float32).ravel()
        return 0

    def rih_pack_conv_weight_multi(self, descs, n, stream):
        for i in range(n):
            d = descs[i]
            if d.mode == 0:
                self.rih_pack_conv_weight(d.w, d.dst, d.Cout, d.Cin, d.KH, d.KW, d.CinPad, 0, stream)
            else:
                self.rih_pack_conv_weight_sub(d.w, d.dst, d.Cout, d.Cin, d.KH, d.KW, d.CinPad, d.kh0, d.kw0, d.step, d.Th,
                                              d.Tw, stream)
        return 0

    def rih_pack_conv_weight(self, w, dst, Cout, Cin, KH, KW, CinPad, for_dgrad, stream):
        W = _f(w, Cout * Cin * KH * KW).reshape(Cout, Cin, KH * KW)
        Wp = np.zeros((Cout, CinPad, KH * KW), np.float32)
        Wp[:, :Cin] = W
        if not for_dgrad:
            out = Wp.transpose(2, 1, 0)                       # [tap][ci][co]
        else:
            out = Wp[:, :, ::-1].transpose(2, 0, 1)           # [tap'][co][ci]
        _f(dst, out.size)[:] = np.ascontiguousarray(out).ravel()
        return 0

    def rih_pack_conv_weight_sub(self, w, dst, Cout, Cin, KH, KW, CinPad, kh0, kw0, step, Th, Tw, stream):
        W = _f(w, Cout * Cin * KH * KW).reshape(Cout, Cin, KH, KW)
        out = np.zeros((Th, Tw, Cout, CinPad), np.float32)
        for th in range(Th):
            for tw in range(Tw):
                out[th, tw, :, :Cin] = W[:, :, kh0 + step * (Th - 1 - th), kw0 + step * (Tw - 1 - tw)]
        _f(dst, out.size)[:] = out.ravel()
        return 0

    # ------------------------------------------------------------------ fused attention forward
    # attention without a score matrix (rih_flash_attention_*): the header's contract restated per (image, head) slice
    def _flash_slices(self, B, heads, S, ld, d):
        cols = np.arange(d)
        return lambda b, h: ((b * S + np.arange(S))[:, None] * ld + h * d + cols[None, :])

    def _flash_probs(self, Qs, Ks, alpha, seed, drop_p, r0, Sq, Sk):
        s = np.float64(alpha) * (Qs.astype(np.float64) @ Ks.astype(np.float64).T)
        mx = s.max(1, keepdims=True)
        e = np.exp(s - mx)
        p = e / e.sum(1, keepdims=True)
        lse2 = (mx[:, 0] + np.log(e.sum(1))) / np.log(2.0)
        keep = np.ones((Sq, Sk))
        if drop_p > 0:
            idx = ((r0 + np.arange(Sq))[:, None] * Sk + np.arange(Sk)[None, :]).ravel()
            thr = np.uint64(min(int(float(np.float32(drop_p)) * 4294967296.0), 4294967295))
            keep = ((hash_np(seed, idx) >= thr).astype(np.float64) / (1.0 - float(np.float32(drop_p)))).reshape(Sq, Sk)
        return p, keep, lse2

    def rih_flash_attention_fwd(self, q, q_ld, k, v, kv_ld, B, heads, Sq, Sk, d, alpha, drop_p, seed, seed_dev, out, ld_out,
                                lse, stream):
        # the refusals of the entry point, before anything is read or written
        if not (q and k and v and out and lse) or B < 1 or heads < 1 or Sq < 1 or Sk < 1 or d not in (16, 32, 64):
            return -1
        if q_ld < d or kv_ld < d or ld_out < heads * d or not 0.0 <= drop_p < 1.0 or B * heads > 65535:
            return -1
        seed = self._seed(seed, seed_dev)
        Q = _f(q, (B * Sq - 1) * q_ld + heads * d)
        Kk = _f(k, (B * Sk - 1) * kv_ld + heads * d)
        Vv = _f(v, (B * Sk - 1) * kv_ld + heads * d)
        O = _f(out, (B * Sq - 1) * ld_out + heads * d)
        L = _f(lse, B * heads * Sq)
        qi, ki, oi = (self._flash_slices(B, heads, Sq, q_ld, d), self._flash_slices(B, heads, Sk, kv_ld, d),
                      self._flash_slices(B, heads, Sq, ld_out, d))
        for b in range(B):
            for h in range(heads):
                r0 = (b * heads + h) * Sq
                p, keep, lse2 = self._flash_probs(Q[qi(b, h)], Kk[ki(b, h)], alpha, seed, drop_p, r0, Sq, Sk)
                O[oi(b, h).ravel()] = ((p * keep) @ Vv[ki(b, h)].astype(np.float64)).astype(np.float32).ravel()
                L[r0:r0 + Sq] = lse2.astype(np.float32)
        return 0

    def rih_flash_attention_bwd(self, dO, do_ld, O, o_ld, q, q_ld, k, v, kv_ld, B, heads, Sq, Sk, d, alpha, drop_p, seed,
                                seed_dev, lse, Dws, dq, dq_ld, dk, dv, dkv_ld, stream):
        if not (dO and O and q and k and v and lse and Dws and dq and dk and dv) or B < 1 or heads < 1 or Sq < 1 or Sk < 1:
            return -1
        if (d not in (16, 32, 64) or q_ld < d or kv_ld < d or do_ld < heads * d or o_ld < heads * d or dq_ld < d or dkv_ld < d
                or not 0.0 <= drop_p < 1.0 or B * heads > 65535):
            return -1
        seed = self._seed(seed, seed_dev)
        G = _f(dO, (B * Sq - 1) * do_ld + heads * d)
        Om = _f(O, (B * Sq - 1) * o_ld + heads * d)
        Q = _f(q, (B * Sq - 1) * q_ld + heads * d)
        Kk = _f(k, (B * Sk - 1) * kv_ld + heads * d)
        Vv = _f(v, (B * Sk - 1) * kv_ld + heads * d)
        dQ = _f(dq, (B * Sq - 1) * dq_ld + heads * d)
        dK = _f(dk, (B * Sk - 1) * dkv_ld + heads * d)
        dV = _f(dv, (B * Sk - 1) * dkv_ld + heads * d)
        Dw = _f(Dws, B * heads * Sq)
        sl = self._flash_slices
        gi, oi, qi, ki = sl(B, heads, Sq, do_ld, d), sl(B, heads, Sq, o_ld, d), sl(B, heads, Sq, q_ld, d), sl(B, heads, Sk, kv_ld, d)
        dqi, dki = sl(B, heads, Sq, dq_ld, d), sl(B, heads, Sk, dkv_ld, d)
        for b in range(B):
            for h in range(heads):
                r0 = (b * heads + h) * Sq
                Qs, Ks, Vs, Gs = (Q[qi(b, h)].astype(np.float64), Kk[ki(b, h)].astype(np.float64), Vv[ki(b, h)].astype(np.float64),
                                  G[gi(b, h)].astype(np.float64))
                p, keep, _ = self._flash_probs(Qs, Ks, alpha, seed, drop_p, r0, Sq, Sk)
                dpd = (Gs @ Vs.T) * keep
                D = (Gs * Om[oi(b, h)].astype(np.float64)).sum(1)
                ds = np.float64(alpha) * p * (dpd - D[:, None])
                Dw[r0:r0 + Sq] = D.astype(np.float32)
                dQ[dqi(b, h).ravel()] = (ds @ Ks).astype(np.float32).ravel()
                dK[dki(b, h).ravel()] = (ds.T @ Qs).astype(np.float32).ravel()
                dV[dki(b, h).ravel()] = ((p * keep).T @ Gs).astype(np.float32).ravel()
        return 0

    def rih_attention_fwd_fused(self, q, q_ld, k, v, kv_ld, B, heads, Sq, Sk, d, alpha, drop_p, seed, seed_dev, P, Pd, ldP,
                                out, ld_out, stream):
        seed = self._seed(seed, seed_dev)
        Q = _f(q, (B * Sq - 1) * q_ld + heads * d)
        Kk = _f(k, (B * Sk - 1) * kv_ld + heads * d)
        Vv = _f(v, (B * Sk - 1) * kv_ld + heads * d)
        Pm, Pdm = _f(P, B * heads * Sq * ldP), _f(Pd, B * heads * Sq * ldP)
        O = _f(out, (B * Sq - 1) * ld_out + heads * d)
        cols = np.arange(d)
        for b in range(B):
            for h in range(heads):
                qi = ((b * Sq + np.arange(Sq))[:, None] * q_ld + h * d + cols[None, :])
                ki = ((b * Sk + np.arange(Sk))[:, None] * kv_ld + h * d + cols[None, :])
                s = np.float32(alpha) * (Q[qi] @ Kk[ki].T)
                e = np.exp(s - s.max(1, keepdims=True))
                p = (e / e.sum(1, keepdims=True)).astype(np.float32)
                r0 = (b * heads + h) * Sq
                pidx = (r0 + np.arange(Sq))[:, None] * ldP + np.arange(Sk)[None, :]
                Pm[pidx.ravel()] = p.ravel()
                pd = p
                if drop_p > 0:
                    idx = ((r0 + np.arange(Sq))[:, None] * Sk + np.arange(Sk)[None, :]).ravel()
                    thr = np.uint64(min(int(float(np.float32(drop_p)) * 4294967296.0), 4294967295))
                    keep = (hash_np(seed, idx) >= thr).astype(np.float32) / np.float32(1.0 - drop_p)
                    pd = (p.ravel() * keep).reshape(Sq, Sk)
                    Pdm[pidx.ravel()] = pd.ravel()
                elif Pd != P:
                    Pdm[pidx.ravel()] = p.ravel()
                oi = ((b * Sq + np.arange(Sq))[:, None] * ld_out + h * d + cols[None, :])
                O[oi.ravel()] = (pd @ Vv[ki]).astype(np.float32).ravel()
        return 0

    def rih_attention_bwd_dq_fused(self, dO, do_ld, k, v, kv_ld, B, heads, Sq, Sk, d, alpha, drop_p, seed, seed_dev, P, dS,
                                   ldP, dq, dq_ld, stream):
        seed = self._seed(seed, seed_dev)
        G = _f(dO, (B * Sq - 1) * do_ld + heads * d)
        Kk = _f(k, (B * Sk - 1) * kv_ld + heads * d)
        Vv = _f(v, (B * Sk - 1) * kv_ld + heads * d)
        Pm, dSm = _f(P, B * heads * Sq * ldP), _f(dS, B * heads * Sq * ldP)
        dQ = _f(dq, (B * Sq - 1) * dq_ld + heads * d)
        cols = np.arange(d)
        for b in range(B):
            for h in range(heads):
                gi = ((b * Sq + np.arange(Sq))[:, None] * do_ld + h * d + cols[None, :])
                ki = ((b * Sk + np.arange(Sk))[:, None] * kv_ld + h * d + cols[None, :])
                r0 = (b * heads + h) * Sq
                pidx = (r0 + np.arange(Sq))[:, None] * ldP + np.arange(Sk)[None, :]
                p = Pm[pidx]
                dp = G[gi] @ Vv[ki].T
                if drop_p > 0:
                    idx = ((r0 + np.arange(Sq))[:, None] * Sk + np.arange(Sk)[None, :]).ravel()
                    thr = np.uint64(min(int(float(np.float32(drop_p)) * 4294967296.0), 4294967295))
                    keep = (hash_np(seed, idx) >= thr).astype(np.float32) / np.float32(1.0 - drop_p)
                    dp = dp * keep.reshape(Sq, Sk)
                ds = (np.float32(alpha) * p * (dp - (dp * p).sum(1, keepdims=True))).astype(np.float32)
                dSm[pidx.ravel()] = ds.ravel()
                qi = ((b * Sq + np.arange(Sq))[:, None] * dq_ld + h * d + cols[None, :])
                dQ[qi.ravel()] = (ds @ Kk[ki]).astype(np.float32).ravel()
        return 0

    def rih_attention_bwd_dkv_fused(self, dO, do_ld, q, q_ld, B, heads, Sq, Sk, d, Pd, dS, ldP, dk, dv, dkv_ld, stream):
        G = _f(dO, (B * Sq - 1) * do_ld + heads * d)
        Q = _f(q, (B * Sq - 1) * q_ld + heads * d)
        Pm, Sm = _f(Pd, B * heads * Sq * ldP), _f(dS, B * heads * Sq * ldP)
        DK, DV = _f(dk, (B * Sk - 1) * dkv_ld + heads * d), _f(dv, (B * Sk - 1) * dkv_ld + heads * d)
        cols = np.arange(d)
        for b in range(B):
            for h in range(heads):
                gi = ((b * Sq + np.arange(Sq))[:, None] * do_ld + h * d + cols[None, :])
                qi = ((b * Sq + np.arange(Sq))[:, None] * q_ld + h * d + cols[None, :])
                pidx = ((b * heads + h) * Sq + np.arange(Sq))[:, None] * ldP + np.arange(Sk)[None, :]
                oi = ((b * Sk + np.arange(Sk))[:, None] * dkv_ld + h * d + cols[None, :])
                DV[oi.ravel()] = (Pm[pidx].T @ G[gi]).astype(np.float32).ravel()
                DK[oi.ravel()] = (Sm[pidx].T @ Q[qi]).astype(np.float32).ravel()
        return 0

    def rih_cdev(self, pred_left, pred_right, gt_left, gt_right, B, V, contact, out, stream):
        from oracle import metrics_oracle
        t = lambda ptr: torch.from_numpy(_f(ptr, B * V * 3).reshape(B, V, 3).copy())
        _f(out, B)[:] = metrics_oracle.compute_cdev(t(pred_left), t(pred_right), t(gt_left), t(gt_right), contact).numpy()
        return 0

    # ------------------------------------------------------------------ fp16 inference backbone (csrc/rih_half.hip)
    @staticmethod
    def _h(ptr, n):
        return np.ctypeslib.as_array((C.c_uint16 * int(n)).from_address(int(ptr))).view(np.float16)

    def _hview(self, ptr, pixels, ld, Cn):
        """[pixels][ld] fp16 memory -> strided view [pixels][Cn] (the last row holds only Cn elements)."""
        flat = self._h(ptr, (pixels - 1) * ld + Cn)
        return np.lib.stride_tricks.as_strided(flat, (pixels, Cn), (2 * ld, 2))

    def rih_hconv(self, dref, stream):
        d = dref._obj
        K = d.KH * d.KW * d.Cin
        assert d.Cin % 8 == 0 and d.Kpad % 64 == 0 and d.Kpad >= K and d.ldx % 8 == 0 and d.zero
        x = self._hview(d.x, d.N * d.H * d.W, d.ldx, d.Cin).astype(np.float32).reshape(d.N, d.H, d.W, d.Cin)
        w = self._h(d.w, d.Cout * d.Kpad).reshape(d.Cout, d.Kpad)[:, :K].astype(np.float32)
        w = torch.from_numpy(w.reshape(d.Cout, d.KH, d.KW, d.Cin).transpose(0, 3, 1, 2).copy())
        y = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), w, None, d.stride, d.pad).permute(0, 2, 3, 1).numpy()
        assert y.shape[1:3] == (d.Ho, d.Wo)
        y = y.reshape(-1, d.Cout).astype(np.float32)
        pixels = y.shape[0]
        if d.res:
            y = y + self._hview(d.res, pixels, d.ldr, d.Cout).astype(np.float32)
        if d.bias:
            y = y + _f(d.bias, d.Cout)[None, :]
        if d.relu:
            y = np.maximum(y, 0)
        if d.post_scale:
            y = y * _f(d.post_scale, d.Cout)[None, :] + _f(d.post_shift, d.Cout)[None, :]
        if d.out_f32:
            flat = _f(d.y, (pixels - 1) * d.ldy + d.Cout)
            np.lib.stride_tricks.as_strided(flat, (pixels, d.Cout), (4 * d.ldy, 4))[:] = y
        else:
            self._hview(d.y, pixels, d.ldy, d.Cout)[:] = np.clip(y, -65504, 65504).astype(np.float16)
        return 0

    def rih_hconv_plan(self, dref):
        """The kernel choice of rih_hconv restated (RIH_HCONV_PLAN_* of the header): base 0x10, halo 1, 16 x 16 patches 2, 128
        output channels per workgroup 4, register staging 8; -1 where the entry point refuses."""
        d = dref._obj
        al16 = lambda p: p is not None and p % 16 == 0
        if not (d.x and d.w and d.y and d.zero):
            return -1
        if d.N < 1 or d.H < 1 or d.W < 1 or d.Cin < 8 or d.Cin % 8 or d.Cout < 1 or d.KH < 1 or d.KW < 1:
            return -1
        if d.stride < 1 or d.pad < 0 or d.Ho < 1 or d.Wo < 1:
            return -1
        if d.Ho != (d.H + 2 * d.pad - d.KH) // d.stride + 1 or d.Wo != (d.W + 2 * d.pad - d.KW) // d.stride + 1:
            return -1
        if d.Kpad % 64 or d.Kpad < d.KH * d.KW * d.Cin:
            return -1
        if d.ldx < d.Cin or d.ldx % 8 or d.ldy < d.Cout or not (al16(d.x) and al16(d.w) and al16(d.zero)):
            return -1
        if (d.res and d.ldr < d.Cout) or bool(d.post_scale) != bool(d.post_shift):
            return -1
        M = d.N * d.Ho * d.Wo
        if M > 0x7fffffff or d.N * d.H * d.W > 0x7fffffff:
            return -1
        env = lambda k: os.environ.get(k, '')
        tw = 0
        if (not env('RIH_HCONV_HALO').startswith('0') and (d.KH, d.KW, d.stride, d.pad) == (3, 3, 1, 1) and not d.res
                and d.Cin % 64 == 0 and d.Cout % 64 == 0 and d.ldy % (4 if d.out_f32 else 8) == 0 and al16(d.y)):
            tw = 32 if (d.H % 8 == 0 and d.W % 32 == 0) else 16 if (d.H % 16 == 0 and d.W % 16 == 0) else 0
        if tw:
            patches = d.N * (d.H // (256 // tw)) * (d.W // tw)
            bn = 128 if (d.Cout % 128 == 0 and patches * (d.Cout // 128) >= 256) else 64
            if patches * (d.Cout // bn) > 0x7fffffff:
                return -1
            return 0x10 | 1 | (2 if tw == 16 else 0) | (4 if bn == 128 else 0)
        force = env('RIH_HCONV_BN')
        narrow = force == '64' or (force != '128' and d.Kpad <= 64)
        bn = 128 if (d.Cout > 64 and not narrow) else 64
        if -(-M // 128) * (-(-d.Cout // bn)) > 0x7fffffff:
            return -1
        return 0x10 | (4 if bn == 128 else 0) | (8 if env('RIH_HCONV_GLDS').startswith('0') else 0)

    def rih_hpack_conv_weight(self, w, scale, dst, Cout, Cin, KH, KW, CinPad, Kpad, stream):
        W = _f(w, Cout * Cin * KH * KW).reshape(Cout, Cin, KH, KW).copy()
        if scale:
            with np.errstate(over='ignore'):          # beyond fp32: inf, clipped below as the kernel clips it
                W = W * _f(scale, Cout)[:, None, None, None]
        out = np.zeros((Cout, Kpad), np.float16)
        packed = np.zeros((Cout, KH, KW, CinPad), np.float32)
        packed[..., :Cin] = W.transpose(0, 2, 3, 1)
        out[:, :KH * KW * CinPad] = np.clip(packed.reshape(Cout, -1), -65504, 65504).astype(np.float16)
        self._h(dst, Cout * Kpad)[:] = out.ravel()
        return 0

    def rih_hbn_fold(self, gamma, beta, mean, var, conv_bias, eps, scale, shift, Cn, stream):
        g = _f(gamma, Cn) if gamma else np.ones(Cn, np.float32)
        b = _f(beta, Cn) if beta else np.zeros(Cn, np.float32)
        s = (g / np.sqrt(_f(var, Cn) + np.float32(eps))).astype(np.float32)
        _f(scale, Cn)[:] = s
        _f(shift, Cn)[:] = b - _f(mean, Cn) * s + (_f(conv_bias, Cn) * s if conv_bias else 0)
        return 0

    def rih_himage_nchw_to_nhwc8(self, img, out, N, Cn, H, W, stream):
        x = _f(img, N * Cn * H * W).reshape(N, Cn, H, W)
        o = np.zeros((N, H, W, 8), np.float16)
        o[..., :Cn] = np.clip(x.transpose(0, 2, 3, 1), -65504, 65504).astype(np.float16)     # saturates, as the kernel does
        self._h(out, o.size)[:] = o.ravel()
        return 0

    def rih_hmaxpool3x3s2(self, x, y, N, H, W, Cn, ldx, ldy, stream):
        X = torch.from_numpy(self._hview(x, N * H * W, ldx, Cn).astype(np.float32).reshape(N, H, W, Cn)).permute(0, 3, 1, 2)
        Y = F.max_pool2d(X, 3, 2, 1).permute(0, 2, 3, 1).numpy()
        self._hview(y, N * Y.shape[1] * Y.shape[2], ldy, Cn)[:] = Y.reshape(-1, Cn).astype(np.float16)
        return 0

    def rih_hupsample2x(self, x, y, N, H, W, Cn, ldx, ldy, stream):
        X = torch.from_numpy(self._hview(x, N * H * W, ldx, Cn).astype(np.float32).reshape(N, H, W, Cn)).permute(0, 3, 1, 2)
        Y = F.interpolate(X, scale_factor=2, mode='bilinear', align_corners=True).permute(0, 2, 3, 1).numpy()
        self._hview(y, N * 4 * H * W, ldy, Cn)[:] = Y.reshape(-1, Cn).astype(np.float16)
        return 0

    def rih_havgpool(self, x, y, N, HW, Cn, ldx, stream):
        X = self._hview(x, N * HW, ldx, Cn).astype(np.float32).reshape(N, HW, Cn)
        _f(y, N * Cn)[:] = X.mean(1).ravel()
        return 0

    # ------------------------------------------------------------------ input preparation (through oracle/input_oracle.py)
    def rih_prepare_images(self, src, B, S, minv, bright, flip, aug_u8, ori, norm, norm_h8, stream):
        from oracle import input_oracle as IO
        u8 = lambda ptr, n: np.ctypeslib.as_array((C.c_uint8 * int(n)).from_address(int(ptr)))
        f64 = lambda ptr, n: np.ctypeslib.as_array((C.c_double * int(n)).from_address(int(ptr)))
        imgs = u8(src, B * S * S * 3).reshape(B, S, S, 3)
        for b in range(B):
            im = imgs[b]
            if minv:
                im = IO.warp_with_inverse(im, f64(minv, 6 * B)[6 * b:6 * b + 6], (S, S))
            if bright:
                br = f64(bright, 4 * B)[4 * b:4 * b + 4]
                im = IO.add_brightness(im, br[:3], br[3])
            if flip and u8(flip, B)[b]:
                im = im[:, ::-1]
            o, n = IO.image_tensors(np.ascontiguousarray(im))
            if aug_u8:
                u8(aug_u8, B * S * S * 3).reshape(B, S, S, 3)[b] = im
            if ori:
                _f(ori, B * 3 * S * S).reshape(B, 3, S, S)[b] = o
            if norm:
                _f(norm, B * 3 * S * S).reshape(B, 3, S, S)[b] = n
            if norm_h8:
                h = self._h(norm_h8, B * S * S * 8).reshape(B, S, S, 8)
                h[b] = 0
                h[b, ..., :3] = n.transpose(1, 2, 0).astype(np.float16)
        return 0

    def rih_prepare_labels(self, p2, p3, B, NV, NJ, A, R, flip, bone_length, root_joint, img_size, o2, o3, root_rel, stream):
        NH = NV + NJ
        NP = 2 * NH
        P2, P3 = _f(p2, B * NP * 2).reshape(B, NP, 2), _f(p3, B * NP * 3).reshape(B, NP, 3)
        O2, O3, RR = _f(o2, B * NP * 2).reshape(B, NP, 2), _f(o3, B * NP * 3).reshape(B, NP, 3), _f(root_rel, 3 * B).reshape(B, 3)
        fl = np.ctypeslib.as_array((C.c_uint8 * int(B)).from_address(int(flip))) if flip else np.zeros(B, np.uint8)
        for b in range(B):
            q2, q3 = P2[b].copy(), P3[b].copy()
            if A:
                a = _f(A, 6 * B)[6 * b:6 * b + 6].reshape(2, 3)
                q2 = (q2 @ a[:, :2].T + a[:, 2][None, :]).astype(np.float32)
            if R:
                q3 = (q3 @ _f(R, 9 * B)[9 * b:9 * b + 9].reshape(3, 3).T).astype(np.float32)
            rl, rr = q3[NV + root_joint].copy(), q3[NH + NV + root_joint].copy()
            rel = rr - rl
            q3[:NH] -= rl
            q3[NH:] -= rr
            if bone_length > 0:
                length = (np.linalg.norm(q3[NV + root_joint] - q3[NV]) + np.linalg.norm(q3[NH + NV + root_joint] - q3[NH + NV])) / 2
                sc = np.float32(bone_length) / np.float32(length)
                q3 = q3 * sc
                rel = rel * sc
            if fl[b]:
                rel[1:] = -rel[1:]
                q2[:, 0] = np.float32(img_size) - q2[:, 0]
                q3[:, 0] = -q3[:, 0]
                q2 = np.concatenate([q2[NH:], q2[:NH]])
                q3 = np.concatenate([q3[NH:], q3[:NH]])
            O2[b], O3[b], RR[b] = q2, q3, rel
        return 0

    # ------------------------------------------------------------------ SDF voxeliser (through oracle/sdf_oracle.py)
    def rih_sdf(self, phi, faces, vertices, B, F, V, G, stream):
        from oracle import sdf_oracle
        fc = _i32(faces, 3 * F).reshape(F, 3)
        vt = _f(vertices, B * V * 3).reshape(B, V, 3)
        _f(phi, B * G * G * G)[:] = sdf_oracle.sdf(fc, vt, G).ravel()
        return 0

    # ------------------------------------------------------------------ MANO layer (through oracle/mano_oracle.py)
    @staticmethod
    def _mano_consts(mref):
        m = mref._obj
        t = lambda ptr, *shape: torch.from_numpy(_f(ptr, int(np.prod(shape))).reshape(shape).copy())
        return {'hands_components': t(m.comps, 45, 45), 'hands_mean': t(m.hands_mean, 45),
                'shapedirs': t(m.shapedirs, 778, 3, 10), 'posedirs': t(m.posedirs, 778, 3, 135),
                'v_template': t(m.v_template, 778, 3), 'J_regressor': t(m.J_reg, 16, 778), 'weights': t(m.weights, 778, 16),
                'parent': [int(m.parent[i]) for i in range(16)]}

    def _mano_run(self, mref, root, pose, ncomp, shape, trans, scale, cidx, new_skel, B, grad=False):
        from oracle import mano_oracle
        c = self._mano_consts(mref)
        g = lambda ptr, *sh: torch.from_numpy(_f(ptr, int(np.prod(sh))).reshape(sh).copy()).requires_grad_(grad)
        ins = {'root': g(root, B, 3, 3), 'pose': g(pose, B, ncomp) if ncomp > 0 else g(pose, B, 15, 3, 3),
               'shape': g(shape, B, 10), 'trans': g(trans, B, 3) if trans else None, 'scale': g(scale, B) if scale else None}
        v, j = mano_oracle.mano_forward(c, ins['root'], ins['pose'], ins['shape'], ins['trans'], ins['scale'],
                                        center_idx=None if cidx < 0 else cidx, use_pca=ncomp > 0, new_skel=bool(new_skel))
        return ins, v, j

    def rih_mano_ws_floats(self, B):
        return 16 * B

    def rih_mano_bwd_ws_floats(self, B):
        return B * (2496 + 240 + 13 * 256)

    def rih_mano_pack_floats(self):
        return 148 * 2496 + 528 + 148 * 48

    def rih_mano_pack(self, mref, packed, stream):
        return 0            # the emulator evaluates the layer from the model buffers directly

    def rih_mano_fwd(self, mref, packed, root, pose, ncomp, shape, trans, scale, cidx, new_skel, v, j, ws, B, variant, stream):
        with torch.no_grad():
            _, vv, jj = self._mano_run(mref, root, pose, ncomp, shape, trans, scale, cidx, new_skel, B)
        _f(v, B * 778 * 3)[:] = vv.numpy().ravel()
        _f(j, B * 21 * 3)[:] = jj.numpy().ravel()
        return 0

    def rih_mano_bwd(self, mref, packed, root, pose, ncomp, shape, trans, scale, cidx, new_skel, dv, dj, ws, d_root, d_pose,
                     d_shape, d_trans, d_scale, ws_bwd, B, stream):
        with torch.enable_grad():
            ins, vv, jj = self._mano_run(mref, root, pose, ncomp, shape, trans, scale, cidx, new_skel, B, grad=True)
            ((vv * torch.from_numpy(_f(dv, B * 778 * 3).reshape(B, 778, 3).copy())).sum() +
             (jj * torch.from_numpy(_f(dj, B * 21 * 3).reshape(B, 21, 3).copy())).sum()).backward()
        for name, ptr in (('root', d_root), ('pose', d_pose), ('shape', d_shape), ('trans', d_trans), ('scale', d_scale)):
            if ptr and ins[name] is not None:
                gr = ins[name].grad
                _f(ptr, gr.numel())[:] = gr.numpy().ravel()
        return 0

    # ------------------------------------------------------------------ MANO parameter head (rih_pose.hip)
    def rih_hardswish_fwd(self, x, y, n, stream):
        _f(y, n)[:] = F.hardswish(torch.from_numpy(_f(x, n).copy())).numpy()
        return 0

    @torch.enable_grad()
    def rih_hardswish_bwd(self, dy, x, dx, n, stream):
        t = torch.from_numpy(_f(x, n).copy()).requires_grad_(True)
        F.hardswish(t).backward(torch.from_numpy(_f(dy, n).copy()))
        _f(dx, n)[:] = t.grad.numpy()
        return 0

    def rih_tanh_scale_fwd(self, x, y, n, scale, stream):
        _f(y, n)[:] = np.float32(scale) * np.tanh(_f(x, n))
        return 0

    def rih_tanh_scale_bwd(self, dy, y, dx, n, scale, stream):
        t = _f(y, n) / np.float32(scale)
        _f(dx, n)[:] = _f(dy, n) * np.float32(scale) * (1 - t * t)
        return 0

    def rih_rot6d_fwd(self, x, R, aa, n, stream):
        from oracle import pose_oracle as po
        Rm = po.rot6d_to_rotmat(torch.from_numpy(_f(x, n * 6).copy()).view(n, 6))
        _f(R, n * 9)[:] = Rm.numpy().ravel()
        _f(aa, n * 3)[:] = po.rotation_matrix_to_angle_axis(Rm).numpy().ravel()
        return 0

    @torch.enable_grad()
    def rih_rot6d_bwd(self, x, dR, daa, dx, n, stream):
        from oracle import pose_oracle as po
        t = torch.from_numpy(_f(x, n * 6).copy()).view(n, 6).requires_grad_(True)
        Rm = po.rot6d_to_rotmat(t)
        a = po.rotation_matrix_to_angle_axis(Rm)
        loss = 0
        if dR:
            loss = loss + (Rm * torch.from_numpy(_f(dR, n * 9).copy()).view(n, 3, 3)).sum()
        if daa:
            loss = loss + (a * torch.from_numpy(_f(daa, n * 3).copy()).view(n, 3)).sum()
        loss.backward()
        _f(dx, n * 6)[:] = t.grad.numpy().ravel()
        return 0

    def rih_rodrigues_fwd(self, a, R, n, stream):
        from oracle import pose_oracle as po
        _f(R, n * 9)[:] = po.rodrigues_batch(torch.from_numpy(_f(a, n * 3).copy()).view(n, 3)).numpy().ravel()
        return 0

    @torch.enable_grad()
    def rih_rodrigues_bwd(self, a, dR, da, n, stream):
        from oracle import pose_oracle as po
        t = torch.from_numpy(_f(a, n * 3).copy()).view(n, 3).requires_grad_(True)
        (po.rodrigues_batch(t) * torch.from_numpy(_f(dR, n * 9).copy()).view(n, 3, 3)).sum().backward()
        _f(da, n * 3)[:] = t.grad.numpy().ravel()
        return 0

    @staticmethod
    def _center_scale(v, j, root, ja, jb, target):
        s = target / torch.linalg.norm(j[:, ja] - j[:, jb], dim=-1)
        return (v - j[:, root:root + 1]) * s.view(-1, 1, 1), s

    def rih_center_scale_fwd(self, v, j, B, V, NJ, root, ja, jb, target, vout, sout, stream):
        o, s = self._center_scale(torch.from_numpy(_f(v, B * V * 3).copy()).view(B, V, 3),
                                  torch.from_numpy(_f(j, B * NJ * 3).copy()).view(B, NJ, 3), root, ja, jb, target)
        _f(vout, B * V * 3)[:] = o.numpy().ravel()
        _f(sout, B)[:] = s.numpy()
        return 0

    @torch.enable_grad()
    def rih_center_scale_bwd(self, v, j, dvout, dsout, B, V, NJ, root, ja, jb, target, dv, dj, stream):
        tv = torch.from_numpy(_f(v, B * V * 3).copy()).view(B, V, 3).requires_grad_(True)
        tj = torch.from_numpy(_f(j, B * NJ * 3).copy()).view(B, NJ, 3).requires_grad_(True)
        o, s = self._center_scale(tv, tj, root, ja, jb, target)
        loss = (o * torch.from_numpy(_f(dvout, B * V * 3).copy()).view(B, V, 3)).sum()
        if dsout:
            loss = loss + (s * torch.from_numpy(_f(dsout, B).copy())).sum()
        loss.backward()
        _f(dv, B * V * 3)[:] = tv.grad.numpy().ravel()
        _f(dj, B * NJ * 3)[:] = tj.grad.numpy().ravel()
        return 0

    # ------------------------------------------------------------------ evaluation metrics
    def rih_hand_metrics(self, v_pred, v_gt, j_pred, j_gt, Jreg, B, V, NJ, root_idx, bone_a, bone_b, j_err_ori, v_err_ori,
                         j_err, v_err, pa, j_pred_out, stream):
        vp = _f(v_pred, B * V * 3).reshape(B, V, 3).astype(np.float64)
        vg = _f(v_gt, B * V * 3).reshape(B, V, 3).astype(np.float64)
        J = _f(Jreg, NJ * V).reshape(NJ, V).astype(np.float64) if Jreg else None
        jp = _f(j_pred, B * NJ * 3).reshape(B, NJ, 3).astype(np.float64) if j_pred else J @ vp
        jg = _f(j_gt, B * NJ * 3).reshape(B, NJ, 3).astype(np.float64) if j_gt else J @ vg
        if j_pred_out:
            _f(j_pred_out, B * NJ * 3)[:] = jp.ravel()
        rp, rg = jp[:, root_idx:root_idx + 1], jg[:, root_idx:root_idx + 1]
        sc = (np.linalg.norm(jg[:, bone_a] - jg[:, bone_b], axis=-1) /
              np.linalg.norm(jp[:, bone_a] - jp[:, bone_b], axis=-1)).reshape(B, 1, 1)
        P = _f(pa, B * 2).reshape(B, 2)
        for k, (x1, x2, eo, es) in enumerate(((jp - rp, jg - rg, j_err_ori, j_err), (vp - rp, vg - rg, v_err_ori, v_err))):
            n = x1.shape[1]
            if eo:
                _f(eo, B * n)[:] = np.linalg.norm(x1 - x2, axis=-1).ravel()
            if es:
                _f(es, B * n)[:] = np.linalg.norm(x1 * sc - x2, axis=-1).ravel()
            for b in range(B):          # Procrustes through the SVD (the kernel takes Horn's quaternion route)
                a, g = x1[b].T, x2[b].T
                mu1, mu2 = a.mean(1, keepdims=True), g.mean(1, keepdims=True)
                X1, X2 = a - mu1, g - mu2
                K = X1 @ X2.T
                U, _, Vh = np.linalg.svd(K)
                Z = np.eye(3)
                Z[2, 2] = np.sign(np.linalg.det(U @ Vh))
                R = Vh.T @ Z @ U.T
                s = np.trace(R @ K) / (X1 ** 2).sum()
                hat = s * (R @ a) + (mu2 - s * (R @ mu1))
                P[b, k] = np.linalg.norm(hat - g, axis=0).mean()
        return 0

    # ------------------------------------------------------------------ fused mesh loss
    def rih_mesh_loss(self, tp, v3p, v2p, c3p, c2p, v3g, v2g, shift, w, img, g3, g2, gc3, gc2, partial, B, stream):
        tp = tp._obj
        V, Fn, NJ, Vc, pool = tp.V, tp.F, tp.NJ, tp.Vc, tp.pool
        faces = torch.from_numpy(_i32(tp.faces, Fn * 3).reshape(Fn, 3).astype(np.int64))
        J = torch.from_numpy(_f(tp.J, NJ * V).reshape(NJ, V).copy())
        perm = torch.from_numpy(_i32(tp.perm, Vc * pool).astype(np.int64))
        w = [float(x) for x in _f(w, 7)]
        P3 = torch.from_numpy(_f(v3p, B * V * 3).reshape(B, V, 3).copy()).requires_grad_(True)
        P2 = torch.from_numpy(_f(v2p, B * V * 2).reshape(B, V, 2).copy()).requires_grad_(True)
        C3 = torch.from_numpy(_f(c3p, B * Vc * 3).reshape(B, Vc, 3).copy()).requires_grad_(True)
        C2 = torch.from_numpy(_f(c2p, B * Vc * 2).reshape(B, Vc, 2).copy()).requires_grad_(True)
        G3 = torch.from_numpy(_f(v3g, B * V * 3).reshape(B, V, 3).copy())
        G2 = torch.from_numpy(_f(v2g, B * V * 2).reshape(B, V, 2).copy())
        if shift:
            G3 = G3 + torch.from_numpy(_f(shift, B * 3).reshape(B, 1, 3).copy())

        def edges(v):
            t_ = v[:, faces]
            return torch.stack([t_[:, :, 0] - t_[:, :, 1], t_[:, :, 1] - t_[:, :, 2], t_[:, :, 2] - t_[:, :, 0]], 2)

        def sl1(x):
            return torch.where(x.abs() < 1, 0.5 * x * x, x.abs() - 0.5)
        with torch.enable_grad():
            s2 = 2.0 / img
            ep, eg = edges(P3), edges(G3)
            n = F.normalize(torch.cross(eg[:, :, 0], eg[:, :, 1], dim=-1), dim=-1).unsqueeze(2)
            g3c, g2c = G3[:, perm], G2[:, perm]
            p = pool
            while p > 1:
                g3c = g3c.reshape(B, -1, 2, 3).mean(2)
                g2c = g2c.reshape(B, -1, 2, 2).mean(2)
                p //= 2
            terms = [((P2 * s2 - 1) - (G2 * s2 - 1)).pow(2).sum((1, 2)), sl1(P3 - G3).sum((1, 2)),
                     sl1(torch.matmul(J, P3) - torch.matmul(J, G3)).sum((1, 2)),
                     sl1((F.normalize(ep, dim=-1) * n).sum(-1)).sum((1, 2)),
                     sl1(torch.linalg.norm(ep, dim=-1) - torch.linalg.norm(eg, dim=-1)).sum((1, 2)),
                     sl1(C3 - g3c).sum((1, 2)), ((C2 * s2 - 1) - (g2c * s2 - 1)).pow(2).sum((1, 2))]
            total = sum(wi * ti.sum() for wi, ti in zip(w, terms))
            total.backward()
        for ptr, tns in ((g3, P3), (g2, P2), (gc3, C3), (gc2, C2)):
            _f(ptr, tns.numel())[:] = tns.grad.numpy().ravel()
        out = _f(partial, B * 8).reshape(B, 8)
        for i, ti in enumerate(terms):
            out[:, i] = ti.detach().numpy()
        return 0

    def rih_mesh_loss_final(self, pl, pr, B, w, cnt, out, stream):
        s = _f(pl, B * 8).reshape(B, 8).sum(0) + _f(pr, B * 8).reshape(B, 8).sum(0)
        o = _f(out, 8)
        w, cnt = _f(w, 7), _f(cnt, 7)
        o[0] = sum(float(w[i]) * float(s[i]) for i in range(7))
        for i in range(7):
            o[1 + i] = 0.5 * float(s[i]) / float(cnt[i])
        return 0

    # ------------------------------------------------------------------ layout / pooling
    def rih_nchw_to_nhwc(self, x, y, N, Cc, H, W, Cpad, stream):
        X = _f(x, N * Cc * H * W).reshape(N, Cc, H, W)
        Y = np.zeros((N, H, W, Cpad), np.float32)
        Y[..., :Cc] = X.transpose(0, 2, 3, 1)
        _f(y, Y.size)[:] = Y.ravel()
        return 0

    def rih_nhwc_to_nchw(self, x, y, N, Cc, H, W, ldx, stream):
        X = _f(x, (N * H * W - 1) * ldx + Cc)
        idx = (np.arange(N * H * W)[:, None] * ldx + np.arange(Cc)[None, :])
        _f(y, N * Cc * H * W)[:] = X[idx].reshape(N, H, W, Cc).transpose(0, 3, 1, 2).ravel()
        return 0

    def rih_maxpool3x3s2_fwd(self, x, y, arg, N, H, W, Cc, stream):
        X = torch.from_numpy(_f(x, N * H * W * Cc).reshape(N, H, W, Cc).copy()).permute(0, 3, 1, 2)
        Y, idx = F.max_pool2d(X, 3, 2, 1, return_indices=True)
        Ho, Wo = Y.shape[2:]
        hi, wi = idx // W, idx % W
        ho = torch.arange(Ho).view(1, 1, Ho, 1)
        wo = torch.arange(Wo).view(1, 1, 1, Wo)
        a = (hi - (ho * 2 - 1)) * 3 + (wi - (wo * 2 - 1))
        _f(y, Y.numel())[:] = Y.permute(0, 2, 3, 1).contiguous().numpy().ravel()
        _i8(arg, Y.numel())[:] = a.permute(0, 2, 3, 1).contiguous().numpy().astype(np.int8).ravel()
        return 0

    def rih_maxpool3x3s2_bwd(self, dy, arg, dx, N, H, W, Cc, stream):
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        DY = _f(dy, N * Ho * Wo * Cc).reshape(N, Ho, Wo, Cc)
        A = _i8(arg, N * Ho * Wo * Cc).reshape(N, Ho, Wo, Cc).astype(np.int64)
        DX = np.zeros((N, H, W, Cc), np.float32)
        n, ho, wo, c = np.meshgrid(np.arange(N), np.arange(Ho), np.arange(Wo), np.arange(Cc), indexing='ij')
        hi, wi = ho * 2 - 1 + A // 3, wo * 2 - 1 + A % 3
        np.add.at(DX, (n, hi, wi, c), DY)
        _f(dx, DX.size)[:] = DX.ravel()
        return 0

    def rih_avgpool_fwd(self, x, y, N, HW, Cc, stream):
        _f(y, N * Cc)[:] = _f(x, N * HW * Cc).reshape(N, HW, Cc).mean(1).ravel()
        return 0

    def rih_avgpool_bwd(self, dy, dx, N, HW, Cc, stream):
        d = _f(dy, N * Cc).reshape(N, 1, Cc) / np.float32(HW)
        _f(dx, N * HW * Cc)[:] = np.broadcast_to(d, (N, HW, Cc)).ravel()
        return 0

    def rih_upsample_bilinear_fwd(self, x, y, N, H, W, Cc, f, stream):
        X = torch.from_numpy(_f(x, N * H * W * Cc).reshape(N, H, W, Cc).copy()).permute(0, 3, 1, 2)
        Y = F.interpolate(X, scale_factor=f, mode='bilinear', align_corners=True)
        _f(y, Y.numel())[:] = Y.permute(0, 2, 3, 1).contiguous().numpy().ravel()
        return 0

    def rih_upsample_bilinear_bwd(self, dy, dx, N, H, W, Cc, f, stream):
        with torch.enable_grad():
            X = torch.zeros(N, Cc, H, W, requires_grad=True)
            Y = F.interpolate(X, scale_factor=f, mode='bilinear', align_corners=True)
            G = torch.from_numpy(_f(dy, N * f * f * H * W * Cc).reshape(N, f * H, f * W, Cc).copy()).permute(0, 3, 1, 2)
            Y.backward(G)
        _f(dx, N * H * W * Cc)[:] = X.grad.permute(0, 2, 3, 1).contiguous().numpy().ravel()
        return 0

    def rih_upsample2x_fwd(self, x, y, N, H, W, Cc, stream):
        return self.rih_upsample_bilinear_fwd(x, y, N, H, W, Cc, 2, stream)

    def rih_upsample2x_bwd(self, dy, dx, N, H, W, Cc, stream):
        return self.rih_upsample_bilinear_bwd(dy, dx, N, H, W, Cc, 2, stream)

    def rih_nearest_up_add_fwd(self, x, add, y, N, H, W, Cc, f, stream):
        X = _f(x, N * H * W * Cc).reshape(N, H, W, Cc)
        Y = np.repeat(np.repeat(X, f, axis=1), f, axis=2)
        if add:
            Y = Y + _f(add, N * f * f * H * W * Cc).reshape(N, f * H, f * W, Cc)
        _f(y, Y.size)[:] = Y.ravel()
        return 0

    def rih_nearest_up_bwd(self, dy, dx, N, H, W, Cc, f, stream):
        G = _f(dy, N * f * f * H * W * Cc).reshape(N, H, f, W, f, Cc)
        _f(dx, N * H * W * Cc)[:] = G.sum(axis=(2, 4)).ravel()
        return 0

    # ------------------------------------------------------------------ batch norm
    def rih_bn_ws_floats(self, rows, Cc):
        return 8

    def rih_bn_stats(self, x, rows, Cc, eps, momentum, mean, invstd, rmean, rvar, ws, stream):
        X = _f(x, rows * Cc).reshape(rows, Cc).astype(np.float64)
        m, v = X.mean(0), X.var(0)
        _f(mean, Cc)[:] = m
        _f(invstd, Cc)[:] = 1.0 / np.sqrt(v + eps)
        if rmean:
            rm, rv = _f(rmean, Cc), _f(rvar, Cc)
            rm[:] = (1 - momentum) * rm + momentum * m
            rv[:] = (1 - momentum) * rv + momentum * v * rows / max(rows - 1, 1)
        return 0

    def rih_bn_eval_stats(self, rmean, rvar, Cc, eps, mean, invstd, stream):
        _f(mean, Cc)[:] = _f(rmean, Cc)
        _f(invstd, Cc)[:] = 1.0 / np.sqrt(_f(rvar, Cc) + np.float32(eps))
        return 0

    @staticmethod
    def _u8view(ptr, n):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n,))

    @staticmethod
    def _amax_into(slot, values):
        if slot:
            o = _f(slot, 1)
            o[0] = max(float(o[0]), float(np.abs(values).max()))

    def rih_bn_apply(self, x, mean, invstd, gamma, beta, res, y, rows, Cc, relu, mask, amax, stream):
        X = _f(x, rows * Cc).reshape(rows, Cc)
        o = (X - _f(mean, Cc)) * (_f(invstd, Cc) * _f(gamma, Cc)) + _f(beta, Cc)
        if res:
            o = o + _f(res, rows * Cc).reshape(rows, Cc)
        if relu:
            if mask:            # one byte per quad of consecutive elements: bit e = element e of the quad is positive
                bits = (o.reshape(-1, 4) > 0).astype(np.uint8)
                self._u8view(mask, rows * Cc // 4)[:] = bits[:, 0] | (bits[:, 1] << 1) | (bits[:, 2] << 2) | (bits[:, 3] << 3)
            o = np.maximum(o, 0)
        _f(y, rows * Cc)[:] = o.ravel()
        self._amax_into(amax, o)
        return 0

    def rih_bn_bwd(self, dy, x, y, mean, invstd, gamma, dx, dres, dgamma, dbeta, rows, Cc, relu, frozen, ws, mask, amax_dx, stream):
        D = _f(dy, rows * Cc).reshape(rows, Cc).copy()
        if relu and mask:
            m = self._u8view(mask, rows * Cc // 4)
            keep = np.stack([(m >> e) & 1 for e in range(4)], 1).reshape(rows, Cc).astype(bool)
            D[~keep] = 0
        elif relu:
            D[_f(y, rows * Cc).reshape(rows, Cc) <= 0] = 0
        X = _f(x, rows * Cc).reshape(rows, Cc)
        xh = (X - _f(mean, Cc)) * _f(invstd, Cc)
        s1, s2 = D.sum(0, dtype=np.float64), (D * xh).sum(0, dtype=np.float64)
        _f(dbeta, Cc)[:] = s1
        _f(dgamma, Cc)[:] = s2
        sc = _f(invstd, Cc) * _f(gamma, Cc)
        if frozen & 1:
            o = D * sc
        else:
            o = (D - (s1 / rows).astype(np.float32) - xh * (s2 / rows).astype(np.float32)) * sc
        if frozen & 2:          # the input is a ReLU output: dx gated by x > 0
            o = np.where(X > 0, o, 0)
        _f(dx, rows * Cc)[:] = o.ravel()
        self._amax_into(amax_dx, o)
        if dres:
            _f(dres, rows * Cc)[:] = D.ravel()
        return 0

    def rih_ln_nblk(self, rows):
        return 1

    def rih_layernorm_fwd(self, x, x2, g, b, y, mean, rstd, rows, D, eps, relu, stream):
        X = _f(x, rows * D).reshape(rows, D).copy()
        if x2:
            X += _f(x2, rows * D).reshape(rows, D)
        m = X.mean(1, keepdims=True)
        v = ((X - m) ** 2).mean(1, keepdims=True)
        rs = 1.0 / np.sqrt(v + np.float32(eps))
        o = (X - m) * rs * _f(g, D) + _f(b, D)
        if relu:
            o = np.maximum(o, 0)
        _f(y, rows * D)[:] = o.ravel()
        _f(mean, rows)[:] = m.ravel()
        _f(rstd, rows)[:] = rs.ravel()
        return 0

    def rih_layernorm_fwd_grouped(self, x, x2, g, b, y, mean, rstd, groups, rows, D, sG, sB, eps, relu, stream):
        for q in range(groups):
            o = 4 * q * rows * D
            self.rih_layernorm_fwd(x + o, x2 + o if x2 else 0, g + 4 * q * sG, b + 4 * q * sB, y + o,
                                   mean + 4 * q * rows, rstd + 4 * q * rows, rows, D, eps, relu, stream)
        return 0

    def rih_layernorm_bwd_grouped(self, dy, x, x2, y, g, mean, rstd, dres, dx, dg, db, groups, rows, D, sG, relu, ws,
                                  stream):
        for q in range(groups):
            o = 4 * q * rows * D
            self.rih_layernorm_bwd(dy + o, x + o, x2 + o if x2 else 0, y + o if y else 0, g + 4 * q * sG,
                                   mean + 4 * q * rows, rstd + 4 * q * rows, dres + o if dres else 0, dx + o,
                                   dg + 4 * q * D if dg else 0, db + 4 * q * D if db else 0, rows, D, relu,
                                   ws + 4 * q * self.rih_ln_nblk(rows) * 2 * D, stream)
        return 0

    def rih_ln_param_final_multi(self, descs, n, stream):
        for i in range(n):
            d = descs[i]
            w = _f(d.ws, d.nblk * 2 * d.D).reshape(d.nblk, 2, d.D)
            _f(d.dg, d.D)[:] = w[:, 0].sum(0)
            _f(d.db, d.D)[:] = w[:, 1].sum(0)
        return 0

    def rih_layernorm_bwd(self, dy, x, x2, y, g, mean, rstd, dres, dx, dg, db, rows, D, relu, ws, stream):
        Dy = _f(dy, rows * D).reshape(rows, D).copy()
        if relu:
            Dy[_f(y, rows * D).reshape(rows, D) <= 0] = 0
        X = _f(x, rows * D).reshape(rows, D).copy()
        if x2:
            X += _f(x2, rows * D).reshape(rows, D)
        m, rs = _f(mean, rows).reshape(rows, 1), _f(rstd, rows).reshape(rows, 1)
        xh = (X - m) * rs
        gd = Dy * _f(g, D)
        c1, c2 = gd.mean(1, keepdims=True), (gd * xh).mean(1, keepdims=True)
        out = rs * (gd - c1 - xh * c2)
        if dres:
            out = out + _f(dres, rows * D).reshape(rows, D)
        _f(dx, rows * D)[:] = out.ravel()
        if dg:
            _f(dg, D)[:] = (Dy * xh).sum(0)
            _f(db, D)[:] = Dy.sum(0)
        else:       # deferred: partials [nblk][2][D] for rih_ln_param_final_multi (everything in block 0)
            w = _f(ws, self.rih_ln_nblk(rows) * 2 * D).reshape(-1, 2, D)
            w[:] = 0
            w[0, 0], w[0, 1] = (Dy * xh).sum(0), Dy.sum(0)
        return 0

    def rih_softmax_fwd(self, S, P, Pd, rows, cols, ld, drop_p, seed, seed_dev, stream):
        seed = self._seed(seed, seed_dev)
        idx = np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
        s = _f(S, (rows - 1) * ld + cols)[idx]
        e = np.exp(s - s.max(1, keepdims=True))
        p = (e / e.sum(1, keepdims=True)).astype(np.float32)
        _f(P, (rows - 1) * ld + cols)[idx.ravel()] = p.ravel()
        if drop_p > 0:
            _f(Pd, (rows - 1) * ld + cols)[idx.ravel()] = p.ravel() * keep_mask(seed, rows * cols, drop_p)
        elif Pd != P:
            _f(Pd, (rows - 1) * ld + cols)[idx.ravel()] = p.ravel()
        return 0

    def rih_softmax_bwd(self, P, dPd, rows, cols, ld, drop_p, seed, seed_dev, alpha, stream):
        seed = self._seed(seed, seed_dev)
        idx = np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]
        p = _f(P, (rows - 1) * ld + cols)[idx]
        mem = _f(dPd, (rows - 1) * ld + cols)
        d = mem[idx] * keep_mask(seed, rows * cols, drop_p).reshape(rows, cols)
        dot = (d * p).sum(1, keepdims=True)
        mem[idx.ravel()] = (np.float32(alpha) * p * (d - dot)).ravel()
        return 0

    # ------------------------------------------------------------------ elementwise / gathers
    def rih_add_dropout(self, a, b, y, n, D, bcast_rows, drop_p, seed, seed_dev, stream):
        seed = self._seed(seed, seed_dev)
        bm = bcast_rows * D
        bv = _f(b, bm if bm > 0 else n)
        bv = bv[np.arange(n) % bm] if bm > 0 else bv.copy()
        bv = bv * keep_mask(seed, n, drop_p)
        _f(y, n)[:] = (_f(a, n) if a else 0) + bv
        return 0

    def rih_dropout_bwd(self, dy, dx, n, drop_p, seed, seed_dev, stream):
        seed = self._seed(seed, seed_dev)
        _f(dx, n)[:] = _f(dy, n) * keep_mask(seed, n, drop_p)
        return 0

    def rih_relu_fwd(self, x, y, n, stream):
        _f(y, n)[:] = np.maximum(_f(x, n), 0)
        return 0

    def rih_relu_bwd(self, dy, y, dx, n, stream):
        _f(dx, n)[:] = np.where(_f(y, n) > 0, _f(dy, n), 0)
        return 0

    def rih_colsum_ws_floats(self, rows, Cc):
        return 8

    def rih_colsum(self, x, rows, Cc, ldx, out, accumulate, ws, stream):
        idx = np.arange(rows)[:, None] * ldx + np.arange(Cc)[None, :]
        s = _f(x, (rows - 1) * ldx + Cc)[idx].sum(0, dtype=np.float64)
        o = _f(out, Cc)
        o[:] = (o if accumulate else 0) + s
        return 0

    def rih_gather_rows(self, x, idx, y, B, Vin, Vout, D, stream):
        X = _f(x, B * Vin * D).reshape(B, Vin, D)
        _f(y, B * Vout * D)[:] = X[:, _i32(idx, Vout)].ravel()
        return 0

    def rih_scatter_rows_add(self, dy, inv_ptr, inv_idx, dx, B, Vin, Vout, D, stream):
        DY = _f(dy, B * Vout * D).reshape(B, Vout, D)
        ptr, lst = _i32(inv_ptr, Vin + 1), _i32(inv_idx, Vout)
        DX = np.zeros((B, Vin, D), np.float32)
        for v in range(Vin):
            for k in range(ptr[v], ptr[v + 1]):
                DX[:, v] += DY[:, lst[k]]
        _f(dx, DX.size)[:] = DX.ravel()
        return 0

    def _csr(self, indptr, indices, vals, V):
        import scipy.sparse as sp
        ip = _i32(indptr, V + 1).copy()
        return sp.csr_matrix((_f(vals, ip[-1]).copy(), _i32(indices, ip[-1]).copy(), ip), shape=(V, V))

    def rih_cheby_fwd(self, x, indptr, indices, vals, y, B, V, Fd, stream):
        L = self._csr(indptr, indices, vals, V)
        X = _f(x, B * V * Fd).reshape(B, V, Fd)
        LX = np.stack([L @ X[b] for b in range(B)])
        _f(y, B * V * 2 * Fd)[:] = np.stack((X, LX), -1).reshape(B, V, 2 * Fd).ravel()
        return 0

    def rih_cheby_bwd(self, dy, indptr, indices, vals, dx, B, V, Fd, stream):
        Lt = self._csr(indptr, indices, vals, V)
        DY = _f(dy, B * V * 2 * Fd).reshape(B, V, Fd, 2)
        out = DY[..., 0] + np.stack([Lt @ DY[b, :, :, 1] for b in range(B)])
        _f(dx, B * V * Fd)[:] = out.ravel()
        return 0

    def rih_project_fwd(self, v, scale, trans, out, B, V, img, stream):
        Vv = _f(v, B * V * 3).reshape(B, V, 3)
        s = (_f(scale, B) * np.float32(img)).reshape(B, 1, 1)
        t = (_f(trans, B * 2).reshape(B, 1, 2) * np.float32(img) / 2 + np.float32(img) / 2)
        _f(out, B * V * 2)[:] = (s * Vv[..., :2] + t).ravel()
        return 0

    def rih_project_bwd(self, dout, v, scale, dv, dscale, dtrans, B, V, img, stream):
        D = _f(dout, B * V * 2).reshape(B, V, 2)
        Vv = _f(v, B * V * 3).reshape(B, V, 3)
        s = (_f(scale, B) * np.float32(img)).reshape(B, 1, 1)
        o = np.zeros((B, V, 3), np.float32)
        o[..., :2] = s * D
        _f(dv, B * V * 3)[:] = o.ravel()
        _f(dscale, B)[:] = (D * Vv[..., :2]).sum((1, 2)) * np.float32(img)
        _f(dtrans, B * 2)[:] = (D.sum(1) * np.float32(img) / 2).ravel()
        return 0

    def rih_version(self):
        return 1

    def rih_arch(self):
        return b'emulated'


@contextlib.contextmanager
def emulated_abi():
    """Route renderih_amd.ops through the emulation on CPU tensors (tests only)."""
    from renderih_amd import _lib, ops

    class _FakeStream:
        cuda_stream = 0

    saved = (_lib._lib, ops._chk, ops._stream)
    _lib._lib = EmulatedLib()
    ops._chk = lambda *a, **k: None
    ops._stream = lambda: 0
    try:
        yield
    finally:
        _lib._lib, ops._chk, ops._stream = saved
