"""GPU parity tests of each HIP operator against plain PyTorch fp32 (CPU) of the same op -- forward and backward.
Tolerance (fp32 bar of BASELINE.json): |a-b| <= 1e-4*|b| + 1e-5*max|b| for outputs, 1e-3 / 1e-4 for gradients."""
import math
import os
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from renderih_amd.testing import assert_close, is_null_gradient

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def scaled(t, s):
    """t * s, and t itself at s == 1: the keyword scales xs / ws / gs of the engine-2 test bodies (activations, weights, upstream
    gradients; tests/test_gpu_e2_range.py) leave the default data bit for bit as it was."""
    return t if s == 1.0 else t * s


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


CONV_CASES = [
    # N, H, W, Cin, Cout, k, stride, pad, bias, relu
    (2, 16, 16, 64, 64, 1, 1, 0, False, False),
    (2, 16, 16, 64, 128, 3, 1, 1, False, False),
    (2, 16, 16, 128, 128, 3, 2, 1, False, False),
    (3, 17, 15, 32, 48, 3, 1, 1, False, True),
    (2, 16, 16, 256, 512, 1, 2, 0, False, False),
    (2, 32, 32, 3, 64, 7, 2, 3, False, False),
    (2, 16, 16, 256, 128, 2, 2, 0, True, True),
    (2, 32, 32, 256, 64, 4, 4, 0, True, True),
    (2, 8, 8, 128, 42, 1, 1, 0, True, False),
    (2, 8, 8, 128, 8, 1, 1, 0, True, False),
    (5, 9, 9, 72, 200, 3, 1, 1, False, False),
    (1, 64, 64, 64, 256, 1, 1, 0, False, True),
    (2, 15, 17, 64, 96, 3, 2, 1, False, False),      # odd sizes: the parity classes of the strided dgrad differ in size
    (2, 13, 13, 32, 64, 1, 2, 0, False, False),
    (2, 32, 32, 32, 32, 3, 1, 1, False, False),       # 17..32 output channels: half-empty split-engine tiles (HRNet's 32-channel branch)
    (1, 9, 9, 64, 30, 1, 1, 0, True, True),           # ... and a column count that is not a multiple of 4 (general kernel)
    (16, 64, 64, 32, 24, 3, 1, 1, True, False),       # many rows, K >= 128: the 128x64 tile
]


@pytest.mark.parametrize('case', CONV_CASES)
def test_conv2d(case, xs=1.0, ws=1.0, gs=1.0):
    from renderih_amd import ops
    N, H, W, Cin, Cout, k, s, p, bias, relu = case
    x = scaled(rnd(N, Cin, H, W, seed=1), xs)
    w = scaled(rnd(Cout, Cin, k, k, seed=2, scale=1.0 / math.sqrt(Cin * k * k)), ws)
    b = scaled(rnd(Cout, seed=3), xs * ws) if bias else None
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    yr = F.conv2d(xr, wr, br, stride=s, padding=p)
    if relu:
        yr = F.relu(yr)
    gy = scaled(rnd(*yr.shape, seed=4), gs)
    yr.backward(gy)

    d = dev()
    cpad = 4 if Cin == 3 else Cin
    xg = torch.zeros(N, H, W, cpad)
    xg[..., :Cin] = nhwc(x)
    xg = xg.to(d).requires_grad_(Cin != 3)
    wg = w.to(d).requires_grad_(True)
    bg = b.to(d).requires_grad_(True) if bias else None
    yg = ops.conv2d(xg, wg, bg, stride=s, pad=p, relu=relu)
    assert_close(nchw(yg), yr, what='conv y %s' % (case,))
    yg.backward(nhwc(gy).to(d))
    assert_close(wg.grad, wr.grad, 1e-3, 1e-4, 'conv dw %s' % (case,))
    if Cin != 3:
        assert_close(nchw(xg.grad), xr.grad, 1e-3, 1e-4, 'conv dx %s' % (case,))
    if bias:
        assert_close(bg.grad, br.grad, 1e-3, 1e-4, 'conv db %s' % (case,))


@pytest.mark.parametrize('engine', [0, 1, 2])
@pytest.mark.parametrize('case', [(2, 16, 16, (128, 128, 256), 256, True), (3, 9, 7, (32, 64), 40, False),
                                  (2, 8, 8, (128, 128, 1024, 32), 256, True), (1, 33, 5, (64, 32, 96), 128, False),
                                  (2, 8, 8, (64, 32), 64, 'ungated'), (1, 6, 6, (32, 40), 32, True)])
def test_conv1x1_cat(case, engine, monkeypatch=None, xs=1.0, ws=1.0, gs=1.0):
    """ops.conv1x1_cat (segmented GEMM operand, rih_gemm_desc.a_seg): the 1x1 convolution of a channel concatenation read in place
    -- output, the statistics epilogue, every part's gradient and the weight gradient (written as column slices by the reduction)
    against F.conv2d on the materialised concatenation; engines 1 and 2, two to four parts, ragged row counts, N tails.  Engine 0
    (rih_gemm reads no segmented operand there) and a channel count that is not a multiple of 32 take the concatenation
    fall-back (round-4 advisor finding: the documented RIH_GEMM_ENGINE=0 broke the mid convolutions).  relu == 'ungated': a
    consumer that does NOT pre-gate the gradient (grad_masked=False) -- the backward applies the ReLU gate itself."""
    from renderih_amd import ops
    N, H, W, Cs, Cout, relu = case
    ungated = relu == 'ungated'
    relu = bool(relu)
    saved = ops.ENGINE
    ops.ENGINE = engine
    try:
        parts = [scaled(rnd(N, c, H, W, seed=11 + i) * (1.0 + 3.0 * i), xs) for i, c in enumerate(Cs)]
        Cin = sum(Cs)
        w = scaled(rnd(Cout, Cin, 1, 1, seed=2, scale=1.0 / math.sqrt(Cin)), ws)
        pr = [t.clone().requires_grad_(True) for t in parts]
        wr = w.clone().requires_grad_(True)
        yr = F.conv2d(torch.cat(pr, dim=1), wr)
        if relu:
            yr = F.relu(yr)
        gy = scaled(rnd(*yr.shape, seed=4), gs)
        if relu and not ungated:
            gy = gy * (yr > 0).float()          # the consumer (BatchNorm with input_relu) hands back a gradient gated by y > 0
        yr.backward(gy)
        d = dev()
        pg = [nhwc(t).contiguous().to(d).requires_grad_(True) for t in parts]
        wg = w.to(d).requires_grad_(True)
        holder = ops.StatsHolder()
        yg = ops.conv1x1_cat(pg, wg, relu=relu, stats=holder, grad_masked=(False if ungated else None))
        assert_close(nchw(yg), yr, what='cat conv y %s' % (case,))
        if holder.part is not None:             # per-block (mean, M2) -> mean / variance per channel
            M = N * H * W
            part = holder.part.double().cpu()
            n = torch.full((holder.T,), float(holder.rows), dtype=torch.float64)
            n[-1] = M - holder.rows * (holder.T - 1)
            mean = (part[:, 0] * n[:, None]).sum(0) / M
            var = (part[:, 1] + n[:, None] * (part[:, 0] - mean) ** 2).sum(0) / M
            y2 = nhwc(yr.detach()).reshape(M, Cout).double()
            assert_close(mean, y2.mean(0), 1e-4, 1e-5, 'cat conv stats mean')
            assert_close(var, y2.var(0, unbiased=False), 1e-3, 1e-5, 'cat conv stats var')
        yg.backward(nhwc(gy).contiguous().to(d))
        assert_close(wg.grad, wr.grad, 1e-3, 1e-4, 'cat conv dw %s' % (case,))
        for i, (a, b) in enumerate(zip(pg, pr)):
            assert_close(nchw(a.grad), b.grad, 1e-3, 1e-4, 'cat conv dx%d %s' % (i, case))
    finally:
        ops.ENGINE = saved


HALO_CASES = [(2, 16, 32, 64, 128, False, True), (1, 8, 64, 32, 64, True, True), (3, 8, 32, 96, 192, False, False),
              (2, 64, 64, 128, 128, True, True), (1, 32, 32, 64, 64, False, True),
              (2, 16, 16, 64, 128, True, True), (1, 32, 16, 32, 64, False, True),           # 16 x 16 patches (W % 32 != 0)
              (2, 16, 32, 32, 32, False, True), (1, 16, 16, 64, 96, True, True),            # 32-channel blocks
              (64, 16, 16, 32, 128, False, False)]                                        # 128-wide blocks on 16 x 16 patches


@pytest.mark.parametrize('case', HALO_CASES)
def test_conv3x3_halo(case, monkeypatch=None, xs=1.0, ws=1.0, gs=1.0):
    """csrc/rih_conv3.hip through ops.conv2d (ops.HALO3, engine 2): stride-1 3x3 convolution with the input halo resident in LDS
    and pre-split (H2) weights -- output (+ ReLU), the BatchNorm statistics of its epilogue, the data gradient (the same kernel on
    flipped weights) and the weight gradient (rih_gemm) against F.conv2d in fp64; and equal to the tap-by-tap implicit GEMM
    (HALO3 off) to fp32 round-off.  (N, H, W, Cin, Cout, relu, stats)."""
    from renderih_amd import ops
    N, H, W, Cin, Cout, relu, want_stats = case
    saved = (ops.ENGINE, ops.HALO3)
    ops.ENGINE = 2
    try:
        x = scaled(rnd(N, Cin, H, W, seed=21) * 3.0, xs)
        w = scaled(rnd(Cout, Cin, 3, 3, seed=22, scale=1.0 / math.sqrt(9 * Cin)), ws)
        xr, wr = x.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
        yr = F.conv2d(xr, wr, padding=1)
        if relu:
            yr = F.relu(yr)
        gy = scaled(rnd(*yr.shape, seed=23), gs)
        yr.backward(gy.double())
        d = dev()
        outs = {}
        for halo in (True, False):
            ops.HALO3 = halo
            xg = nhwc(x).contiguous().to(d).requires_grad_(True)
            wg = w.clone().to(d).requires_grad_(True)        # (a fresh leaf per pass: on the CPU harness .to() is the identity)
            holder = ops.StatsHolder() if want_stats else None
            yg = ops.conv2d(xg, wg, None, stride=1, pad=1, relu=relu, stats=holder)
            yg.backward(nhwc(gy).contiguous().to(d))
            outs[halo] = (nchw(yg).detach().cpu(), nchw(xg.grad).cpu(), wg.grad.cpu())
            assert_close(outs[halo][0], yr.float(), 1e-4, 1e-5, 'halo %s y %s' % (halo, case,))
            assert_close(outs[halo][1], xr.grad.float(), 1e-4, 1e-5, 'halo %s dx %s' % (halo, case,))
            assert_close(outs[halo][2], wr.grad.float(), 1e-4, 1e-5, 'halo %s dw %s' % (halo, case,))
            if halo and want_stats:
                assert holder.part is not None and holder.rows in (32, 64) and holder.T == N * H * W // holder.rows
                M = N * H * W
                part = holder.part.double().cpu()
                mean = part[:, 0].mean(0)
                var = (part[:, 1] + float(holder.rows) * (part[:, 0] - mean) ** 2).sum(0) / M
                y2 = nhwc(yr.detach()).reshape(M, Cout)
                assert_close(mean, y2.mean(0), 1e-4, 1e-5, 'halo stats mean')
                assert_close(var, y2.var(0, unbiased=False), 1e-3, 1e-5, 'halo stats var')
        for a, b, what in zip(outs[True], outs[False], ('y', 'dx', 'dw')):
            assert_close(a, b, 1e-4, 1e-5, 'halo vs implicit GEMM ' + what)
    finally:
        ops.ENGINE, ops.HALO3 = saved


HALO_SKIP_CASES = [(2, 8, 32, 32, 32), (1, 16, 16, 64, 64), (2, 16, 32, 128, 128), (1, 32, 32, 64, 32), (3, 16, 16, 32, 96),
                   (64, 32, 32, 32, 128), (256, 16, 16, 32, 128)]      # >= 256 patches: the 128-wide channel blocks (8 x 32 / 16 x 16 patches)


@pytest.mark.parametrize('case', HALO_SKIP_CASES)
def test_conv3x3_halo_with_skip_gradient(case, xs=1.0, ws=1.0, gs=1.0):
    """The data gradient of a residual block's FIRST 3x3 convolution (HRNet's BasicBlock.conv1 through ops.conv2d_skip): the skip
    path's gradient joins in the halo kernel's epilogue (rih_conv3_desc.r, ABI 19; ops.HALO3_RES) -- dx, dw and the forward against
    fp64 with the skip contribution, and against the tiled kernel's residual epilogue (HALO3_RES off).  The launch really is the halo
    kernel's: counted through ops.conv3x3_halo.  (N, H, W, Cin, Cout)."""
    from renderih_amd import ops
    N, H, W, Cin, Cout = case
    saved = (ops.ENGINE, ops.HALO3, ops.HALO3_RES, ops.conv3x3_halo)
    ops.ENGINE, ops.HALO3 = 2, True
    taken = []
    real = ops.conv3x3_halo

    def spy(*a, **k):
        ok = real(*a, **k)
        taken.append((a[3], k.get('R') is not None, ok))
        return ok
    ops.conv3x3_halo = spy
    try:
        x = scaled(rnd(N, Cin, H, W, seed=51) * 2.0, xs)
        w = scaled(rnd(Cout, Cin, 3, 3, seed=52, scale=1.0 / math.sqrt(9 * Cin)), ws)
        xr, wr = x.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
        yr = F.conv2d(xr, wr, padding=1)
        gy, gk = scaled(rnd(*yr.shape, seed=53), gs), scaled(rnd(*x.shape, seed=54), gs)
        (yr * gy.double()).sum().add((xr * gk.double()).sum()).backward()     # the skip path contributes gk to dx
        d = dev()
        outs = {}
        for res in (True, False):
            ops.HALO3_RES = res
            del taken[:]
            xg = nhwc(x).contiguous().to(d).requires_grad_(True)
            wg = w.clone().to(d).requires_grad_(True)
            yg, idt = ops.conv2d_skip(xg, wg, None, stride=1, pad=1, relu=False)
            ((yg * nhwc(gy).contiguous().to(d)).sum() + (idt * nhwc(gk).contiguous().to(d)).sum()).backward()
            outs[res] = (nchw(yg).detach().cpu(), nchw(xg.grad).cpu(), wg.grad.cpu())
            assert_close(outs[res][0], yr.float(), 1e-4, 1e-5, 'halo skip %s y %s' % (res, case,))
            assert_close(outs[res][1], xr.grad.float(), 1e-4, 1e-5, 'halo skip %s dx %s' % (res, case,))
            assert_close(outs[res][2], wr.grad.float(), 1e-4, 1e-5, 'halo skip %s dw %s' % (res, case,))
            dgrad = [t for t in taken if t[0]]
            assert (dgrad == [(True, True, True)]) if res else (dgrad == []), (res, taken)
        for a_, b_, what in zip(outs[True], outs[False], ('y', 'dx', 'dw')):
            assert_close(a_, b_, 1e-4, 1e-5, 'halo residual vs tiled residual ' + what)
    finally:
        ops.ENGINE, ops.HALO3, ops.HALO3_RES, ops.conv3x3_halo = saved


def test_conv3x3_residual_preconditions():
    """rih_conv3x3_ok with a residual: refused together with statistics, with a pitch below N or a misaligned pointer; rih_stem
    takes none."""
    import ctypes as C
    from renderih_amd import ops
    from renderih_amd._lib import Conv3Desc
    d = dev()
    x = torch.zeros(1, 8, 32, 32, device=d)
    pd = Conv3Desc()
    pd.x = pd.w_h2 = pd.y = pd.amax_x = pd.amax_w = x.data_ptr()
    pd.imgs, pd.H, pd.W, pd.C, pd.N, pd.ldx, pd.ldy, pd.Kpad, pd.relu = 1, 8, 32, 32, 32, 32, 32, 288, 0
    L = ops._L()
    assert int(L.rih_conv3x3_ok(C.byref(pd))) == 1
    pd.r, pd.ldr = x.data_ptr(), 32
    assert int(L.rih_conv3x3_ok(C.byref(pd))) == 1
    pd.ldr = 16
    assert int(L.rih_conv3x3_ok(C.byref(pd))) == 0
    pd.ldr, pd.r = 32, x.data_ptr() + 4
    assert int(L.rih_conv3x3_ok(C.byref(pd))) == 0
    pd.r, pd.stats = x.data_ptr(), x.data_ptr()
    assert int(L.rih_conv3x3_ok(C.byref(pd))) == 0


PANEL_CASES = [(2, 64, 64, 64, 256, False, True), (1, 64, 64, 128, 512, False, True), (2, 64, 32, 64, 64, True, True),
               (2, 64, 64, 64, 128, False, False), (4, 64, 64, 128, 128, True, True)]


@pytest.mark.parametrize('case', PANEL_CASES)
def test_panel_1x1(case, monkeypatch=None, xs=1.0, ws=1.0, gs=1.0):
    """csrc/rih_conv3.hip panel_kernel through ops.conv2d / ops.conv2d_skip (ops.PANEL, engine 2): 1x1 convolutions with K = 64 / 128
    as persistent streaming workgroups -- forward (+ ReLU, + BatchNorm statistics), the data gradient WITH the skip path's gradient
    as residual (conv2d_skip: Bottleneck.conv1), the weight gradient (rih_gemm) -- against fp64, and against the tiled kernels
    (PANEL off).  (N, H, W, Cin, Cout, relu, stats); the planning threshold (>= 256 work items) is lifted for the small shapes."""
    from renderih_amd import ops
    N, H, W, Cin, Cout, relu, want_stats = case
    saved = (ops.ENGINE, ops.PANEL, ops._panel_ok)
    ops.ENGINE = 2
    ok0 = ops._panel_ok

    def ok_small(rows, K, Nn, lda, a, bias=None):            # the kernel's own preconditions without the fill-the-chip rule
        return (ops.PANEL and bias is None and K in (64, 128) and Nn % 64 == 0 and not (K == 128 and Nn % 128 != 0) and rows % 128 == 0
                and lda % 4 == 0)
    ops._panel_ok = ok_small
    try:
        x = scaled(rnd(N, Cin, H, W, seed=31) * 2.0, xs)
        w = scaled(rnd(Cout, Cin, 1, 1, seed=32, scale=1.0 / math.sqrt(Cin)), ws)
        xr, wr = x.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
        yr = F.conv2d(xr, wr)
        if relu:
            yr = F.relu(yr)
        gy, gk = scaled(rnd(*yr.shape, seed=33), gs), scaled(rnd(*x.shape, seed=34), gs)
        (yr * gy.double()).sum().add((xr * gk.double()).sum()).backward()     # the skip path contributes gk to dx
        d = dev()
        outs = {}
        for panel in (True, False):
            ops.PANEL = panel
            xg = nhwc(x).contiguous().to(d).requires_grad_(True)
            wg = w.clone().to(d).requires_grad_(True)
            holder = ops.StatsHolder() if want_stats else None
            yg, idt = ops.conv2d_skip(xg, wg, None, stride=1, pad=0, relu=relu, stats=holder)
            ((yg * nhwc(gy).contiguous().to(d)).sum() + (idt * nhwc(gk).contiguous().to(d)).sum()).backward()
            outs[panel] = (nchw(yg).detach().cpu(), nchw(xg.grad).cpu(), wg.grad.cpu())
            assert_close(outs[panel][0], yr.float(), 1e-4, 1e-5, 'panel %s y %s' % (panel, case,))
            assert_close(outs[panel][1], xr.grad.float(), 1e-4, 1e-5, 'panel %s dx %s' % (panel, case,))
            assert_close(outs[panel][2], wr.grad.float(), 1e-4, 1e-5, 'panel %s dw %s' % (panel, case,))
            if panel and want_stats:
                assert holder.part is not None and holder.rows in (32, 64)
                M = N * H * W
                part = holder.part.double().cpu()
                mean = part[:, 0].mean(0)
                var = (part[:, 1] + float(holder.rows) * (part[:, 0] - mean) ** 2).sum(0) / M
                y2 = nhwc(yr.detach()).reshape(M, Cout)
                assert_close(mean, y2.mean(0), 1e-4, 1e-5, 'panel stats mean')
                assert_close(var, y2.var(0, unbiased=False), 1e-3, 1e-5, 'panel stats var')
        for a, b, what in zip(outs[True], outs[False], ('y', 'dx', 'dw')):
            assert_close(a, b, 1e-4, 1e-5, 'panel vs tiled GEMM ' + what)
    finally:
        ops.ENGINE, ops.PANEL, ops._panel_ok = saved


# (N, H, W, Cin, Cout, relu, stats): rih_rows as Conv2dFn reaches it.  With at most 768 rows rows_tile() gives these launches
# rows_kernel<128, 64> (Cout or, for the data gradient, Cin not a multiple of 128) or <128, 128>, never a 256-row tile (those need
# >= 256 workgroups; tests/test_gpu_rows_tiles.py names the tile instead and covers all four) -- K from one k-tile pair to 1024, K
# not a multiple of 64, residual and statistics epilogues
ROWS_CASES = [(2, 16, 16, 256, 64, False, True), (1, 16, 8, 96, 128, True, True), (2, 8, 8, 512, 192, False, False),
              (1, 16, 16, 1024, 64, True, True), (1, 8, 16, 64, 256, False, True), (3, 16, 8, 160, 320, True, False)]


@pytest.mark.parametrize('case', ROWS_CASES)
def test_rows_1x1(case, monkeypatch=None, xs=1.0, ws=1.0, gs=1.0):
    """csrc/rih_conv3.hip rows_kernel through ops.conv2d / ops.conv2d_skip (ops.ROWS, engine 2): 1x1 convolutions with a long reduction
    as 512-thread workgroups with three LDS-DMA-staged stages of H2 weight planes, two A stages in LDS and the A prefetch in registers -- forward (+ ReLU, + BatchNorm statistics), the
    data gradient WITH the skip path's gradient as residual (conv2d_skip: Bottleneck.conv1), the weight gradient (rih_gemm) --
    against fp64 (gradients at rtol 1e-4 + 1e-5 max: north_star's bar), and against the tiled kernels (ROWS off).  The planning
    thresholds (K >= 256, N >= 128, >= 128 workgroups) are lifted for the small shapes; the panel kernel is off so that K = 64 / 128 come here.
    The tile is the library's choice, at these sizes 128 x 64 or 128 x 128 only, and the statistics are checked after merging the
    blocks; tests/test_gpu_rows_tiles.py has every tile and the statistics block by block."""
    from renderih_amd import ops
    N, H, W, Cin, Cout, relu, want_stats = case
    saved = (ops.ENGINE, ops.ROWS, ops.ROWS_MINK, ops.ROWS_MIN_WGS, ops.PANEL, ops.ROWS_MIN_M, ops.ROWS_MIN_N)
    ops.ENGINE, ops.ROWS_MINK, ops.ROWS_MIN_WGS, ops.PANEL, ops.ROWS_MIN_M, ops.ROWS_MIN_N = 2, 64, 1, False, 1, 64
    try:
        x = scaled(rnd(N, Cin, H, W, seed=41) * 2.0, xs)
        w = scaled(rnd(Cout, Cin, 1, 1, seed=42, scale=1.0 / math.sqrt(Cin)), ws)
        xr, wr = x.double().clone().requires_grad_(True), w.double().clone().requires_grad_(True)
        yr = F.conv2d(xr, wr)
        if relu:
            yr = F.relu(yr)
        gy, gk = scaled(rnd(*yr.shape, seed=43), gs), scaled(rnd(*x.shape, seed=44), gs)
        (yr * gy.double()).sum().add((xr * gk.double()).sum()).backward()     # the skip path contributes gk to dx
        d = dev()
        outs = {}
        for rows in (True, False):
            ops.ROWS = rows
            n0 = sum(1 for t in (ops.PROFILE or []) if t[3][6] == 52)
            xg = nhwc(x).contiguous().to(d).requires_grad_(True)
            wg = w.clone().to(d).requires_grad_(True)
            holder = ops.StatsHolder() if want_stats else None
            yg, idt = ops.conv2d_skip(xg, wg, None, stride=1, pad=0, relu=relu, stats=holder)
            ((yg * nhwc(gy).contiguous().to(d)).sum() + (idt * nhwc(gk).contiguous().to(d)).sum()).backward()
            outs[rows] = (nchw(yg).detach().cpu(), nchw(xg.grad).cpu(), wg.grad.cpu())
            assert_close(outs[rows][0], yr.float(), 1e-4, 1e-5, 'rows %s y %s' % (rows, case,))
            assert_close(outs[rows][1], xr.grad.float(), 1e-4, 1e-5, 'rows %s dx %s' % (rows, case,))
            assert_close(outs[rows][2], wr.grad.float(), 1e-4, 1e-5, 'rows %s dw %s' % (rows, case,))
            if rows and want_stats:
                assert holder.part is not None and holder.rows in (32, 64)
                M = N * H * W
                part = holder.part.double().cpu()
                mean = part[:, 0].mean(0)
                var = (part[:, 1] + float(holder.rows) * (part[:, 0] - mean) ** 2).sum(0) / M
                y2 = nhwc(yr.detach()).reshape(M, Cout)
                assert_close(mean, y2.mean(0), 1e-4, 1e-5, 'rows stats mean')
                assert_close(var, y2.var(0, unbiased=False), 1e-3, 1e-5, 'rows stats var')
        for a, b, what in zip(outs[True], outs[False], ('y', 'dx', 'dw')):
            assert_close(a, b, 1e-4, 1e-5, 'rows vs tiled GEMM ' + what)
    finally:
        ops.ENGINE, ops.ROWS, ops.ROWS_MINK, ops.ROWS_MIN_WGS, ops.PANEL, ops.ROWS_MIN_M, ops.ROWS_MIN_N = saved


def test_rows_and_stem_kernels_are_reproducible_at_bench_size():
    """Sixty launches of rih_rows on the HBM-bound 262144 x 256 -> 64 shapes (forward with statistics, data gradient with residual)
    and twenty of rih_stem at B = 64, every second one on an operand fresh out of a producer kernel, with unrelated traffic behind
    each launch: all outputs bit-identical to the first, and the first rih_rows output of either form (with the forward's statistics,
    block by block) equal to an fp64 matmul on the device at the suite's bar.  Round 6: the kernels issue their requests through inline assembly; a
    COUNTED wait (vmcnt(N), N > 0) across LDS-DMA requests and buffer loads let 6 of 800 such launches convert registers whose
    load had not landed (profiles/r06/rows/c14_*), which no small-shape parity test saw -- the waits are vmcnt(0) since."""
    if dev().type != 'cuda':
        pytest.skip('a timing-dependent hardware hazard: nothing to see on the host harness')
    from renderih_amd import ops
    d = dev()
    M, K, N = 262144, 256, 64
    scratch = torch.empty(32 << 20, device=d)
    torch.manual_seed(3)
    src = torch.randn(M, K, device=d)
    for fwd in (True, False):
        w = (torch.randn(N, K, 1, 1, device=d) if fwd else torch.randn(K, N, 1, 1, device=d)) * (2.0 / K) ** 0.5
        R = None if fwd else torch.randn(M, N, device=d) * 0.1
        a0 = torch.relu(src * 1.3 + 0.2)
        ba, bw = ops.bound_of(a0), ops.bound_of(w)
        first = None
        for rep in range(60):
            a = torch.relu(src * 1.3 + 0.2) if rep % 2 else a0
            c = torch.empty(M, N, device=d)
            holder = ops.StatsHolder() if fwd else None
            assert ops.rows_gemm(a, w, c, M, N, K, K, N, not fwd, stats=holder, R=R, ldr=N, ba=ba, bw=bw)
            scratch.normal_()
            if first is None:
                first = c.clone()
                # ... and the first is RIGHT: fp64 on the device from the same fp32 operands, at the bar of test_rows_1x1
                w2 = w[:, :, 0, 0].double()
                ref = a0.double() @ (w2.t() if fwd else w2)
                if R is not None:
                    ref += R.double()
                what = 'rih_rows at bench size (%s)' % ('fwd' if fwd else 'dgrad')
                assert_close(first, ref, 1e-4, 1e-5, what)
                if fwd:
                    assert holder.rows in (32, 64) and holder.T == M // holder.rows
                    blk = ref.reshape(holder.T, holder.rows, N)
                    mean = blk.mean(1)
                    assert_close(holder.part[:, 0], mean, 1e-4, 1e-5, what + ' block means')
                    assert_close(holder.part[:, 1], ((blk - mean[:, None]) ** 2).sum(1), 1e-3, 1e-5, what + ' block M2')
                del ref
            else:
                assert torch.equal(c, first), 'rih_rows launch %d (%s) differs from the first' % (rep, 'fwd' if fwd else 'dgrad')
    img = torch.randn(64, 256, 256, 4, device=d)
    img[..., 3] = 0
    w7 = torch.randn(64, 3, 7, 7, device=d) * 0.08
    first = None
    for rep in range(20):
        x = img * 1.0 if rep % 2 else img
        y = ops.conv2d(x, w7, None, stride=2, pad=3)
        scratch.normal_()
        if first is None:
            first = y.clone()
        else:
            assert torch.equal(y, first), 'rih_stem launch %d differs from the first' % rep


def test_rows_kernel_is_taken_and_falls_back(monkeypatch):
    """The dispatch of ops.Conv2dFn: a 1x1 convolution with K >= ROWS_MINK lands on rih_rows (forward and data gradient), an output
    view the library refuses (not 16-byte aligned) falls back to rih_gemm instead of raising (the host-side
    preconditions do not know every C-side one)."""
    from renderih_amd import ops
    monkeypatch.setattr(ops, 'ENGINE', 2)
    monkeypatch.setattr(ops, 'ROWS_MIN_WGS', 1)
    monkeypatch.setattr(ops, 'ROWS_MIN_M', 1)
    calls = []
    real = ops.rows_gemm
    monkeypatch.setattr(ops, 'rows_gemm', lambda *a, **k: (calls.append(real(*a, **k)) or calls[-1]))
    d = dev()
    x = nhwc(rnd(1, 256, 16, 16, seed=5)).contiguous().to(d).requires_grad_(True)
    w = rnd(256, 256, 1, 1, seed=6, scale=1 / 16.0).to(d).requires_grad_(True)         # (K = 256 forward AND as a data gradient)
    y = ops.conv2d(x, w, None, stride=1, pad=0)
    y.sum().backward()
    assert calls == [True, True], calls
    ref = F.conv2d(nchw(x.detach()).double().cpu(), w.detach().double().cpu())
    assert_close(nchw(y).detach().cpu(), ref.float(), 1e-4, 1e-5, 'rows dispatch y')
    from renderih_amd._lib import PanelDesc
    import ctypes as C
    pd = PanelDesc()
    pd.a = pd.w_h2 = pd.amax_a = pd.amax_w = x.data_ptr()
    pd.c = x.data_ptr() + 4                         # a misaligned output
    pd.M, pd.N, pd.K, pd.lda, pd.ldc = 256, 64, 256, 256, 64
    assert int(ops._L().rih_rows_ok(C.byref(pd))) == 0
    pd.c = x.data_ptr()
    assert int(ops._L().rih_rows_ok(C.byref(pd))) == 1


def test_grouped_weight_gradients_on_128x64_tiles(monkeypatch, xs=1.0, ws=1.0, gs=1.0):
    """ops.WGRAD_T1 (round 6): weight gradients with 33..64 output channels on a large map ride in the grouped launch on 128 x 64
    tiles of engine 2 (rih_gemm_multi variant 64 + 8 + 4 + plain) -- 3 x 3 and 1 x 1 convolutions, with the 64 x 64-tile path and fp64
    as references; bit-reproducible from run to run."""
    from renderih_amd import ops
    monkeypatch.setattr(ops, 'ENGINE', 2)
    monkeypatch.setattr(ops, 'WGRAD_T1_MINK', 512)
    d = dev()
    xl = [scaled(rnd(2, 64, 16, 32, seed=61), xs), scaled(rnd(2, 128, 16, 32, seed=66), xs)]
    gys = [scaled(rnd(2, 64, 16, 32, seed=62), gs), scaled(rnd(2, 48, 16, 32, seed=63), gs)]
    wl = [scaled(rnd(64, 64, 3, 3, seed=64, scale=0.05), ws), scaled(rnd(48, 128, 1, 1, seed=65, scale=0.1), ws)]
    refs = []
    for x, w, gy, pad in zip(xl, wl, gys, (1, 0)):
        wr = w.double().clone().requires_grad_(True)
        F.conv2d(x.double(), wr, padding=pad).backward(gy.double())
        refs.append(wr.grad.float())
    seen = []
    flush = ops.GroupedGemms.flush

    def spy(self):
        seen.extend(v for v, _, _, _ in self.items)
        return flush(self)
    monkeypatch.setattr(ops.GroupedGemms, 'flush', spy)
    got = {}
    for t1 in (True, False, True):
        monkeypatch.setattr(ops, 'WGRAD_T1', t1)
        del seen[:]
        xg = [nhwc(x).contiguous().to(d) for x in xl]
        wg = [w.clone().to(d).requires_grad_(True) for w in wl]
        with ops.deferred_reductions():
            ys = [ops.conv2d(xg[0], wg[0], None, stride=1, pad=1), ops.conv2d(xg[1], wg[1], None, stride=1, pad=0)]
            g = torch.autograd.grad([(y * nhwc(gy).contiguous().to(d)).sum() for y, gy in zip(ys, gys)], wg)
        g = [t.cpu() for t in g]
        if t1:
            assert sorted(seen) == [64 + 8 + 4 + 0, 64 + 8 + 4 + 1], seen
            if True in got:
                assert all(torch.equal(a, b) for a, b in zip(g, got[True])), 'grouped 128x64 launch is not reproducible'
        else:
            assert all((v & 63) >> 3 == 2 for v in seen), seen
        got[t1] = g
        for a, r in zip(g, refs):
            assert_close(a, r, 1e-4, 1e-5, 'wgrad T1=%s vs fp64' % t1)


@pytest.mark.parametrize('case', [(2, 32, 32, True, True), (16, 24, 40, False, True), (4, 16, 16, True, False)])
def test_stem_conv(case, monkeypatch=None, xs=1.0, ws=1.0, gs=1.0):
    """csrc/rih_conv3.hip rows_kernel<STEM> through ops.conv2d (ops.STEM, engine 2): encoder.resnet.conv1 -- 7 x 7 / stride 2 / padding 3
    on the 4-channel padded image -- with the im2col loader (one tap of one output pixel = one float4; zero padding and the K = 196 ->
    224 tail by predication): output (+ ReLU), the BatchNorm statistics of its epilogue, the weight gradient (rih_gemm) against
    F.conv2d in fp64, and equal to rih_gemm's general kernel (STEM off) to fp32 round-off.  (N, H, W, relu, stats)."""
    from renderih_amd import ops
    N, H, W, relu, want_stats = case
    saved = (ops.ENGINE, ops.STEM)
    ops.ENGINE = 2
    try:
        x = scaled(rnd(N, 3, H, W, seed=51) * 2.0, xs)
        w = scaled(rnd(64, 3, 7, 7, seed=52, scale=1.0 / math.sqrt(147.0)), ws)
        xr, wr = x.double(), w.double().clone().requires_grad_(True)
        yr = F.conv2d(xr, wr, stride=2, padding=3)
        if relu:
            yr = F.relu(yr)
        gy = scaled(rnd(*yr.shape, seed=53), gs)
        yr.backward(gy.double())
        d = dev()
        outs = {}
        for stem in (True, False):
            ops.STEM = stem
            xg = torch.zeros(N, H, W, 4)
            xg[..., :3] = nhwc(x)
            xg = xg.to(d)
            wg = w.clone().to(d).requires_grad_(True)
            holder = ops.StatsHolder() if want_stats else None
            yg = ops.conv2d(xg, wg, None, stride=2, pad=3, relu=relu, stats=holder)
            yg.backward(nhwc(gy).contiguous().to(d))
            outs[stem] = (nchw(yg).detach().cpu(), wg.grad.cpu())
            assert_close(outs[stem][0], yr.float(), 1e-4, 1e-5, 'stem %s y %s' % (stem, case,))
            assert_close(outs[stem][1], wr.grad.float(), 1e-4, 1e-5, 'stem %s dw %s' % (stem, case,))
            if stem and want_stats:
                M = N * (H // 2) * (W // 2)
                assert holder.part is not None and holder.rows == 64 and holder.T == M // 64
                part = holder.part.double().cpu()
                mean = part[:, 0].mean(0)
                var = (part[:, 1] + 64.0 * (part[:, 0] - mean) ** 2).sum(0) / M
                y2 = nhwc(yr.detach()).reshape(M, 64)
                assert_close(mean, y2.mean(0), 1e-4, 1e-5, 'stem stats mean')
                assert_close(var, y2.var(0, unbiased=False), 1e-3, 1e-5, 'stem stats var')
        assert_close(outs[True][0], outs[False][0], 1e-4, 1e-5, 'stem kernel vs general GEMM y')
    finally:
        ops.ENGINE, ops.STEM = saved


LIN_CASES = [(126, 512, 256, True, False, False), (126, 2048, 509, True, False, False), (100, 64, 3, True, False, False),
             (128, 252, 1, True, False, False), (6, 252, 778, False, False, False), (4032, 128, 128, True, True, True),
             (300, 256, 256, True, False, True), (8064, 64, 64, True, True, False)]


@pytest.mark.parametrize('case', LIN_CASES)
def test_linear(case):
    from renderih_amd import ops
    M, K, N, bias, relu, res = case
    x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K))
    b = rnd(N, seed=3) if bias else None
    r = rnd(M, N, seed=5) if res else None
    ts = [t.clone().requires_grad_(True) if t is not None else None for t in (x, w, b, r)]
    yr = F.linear(ts[0], ts[1], ts[2])
    if res:
        yr = yr + ts[3]
    if relu:
        yr = F.relu(yr)
    gy = rnd(M, N, seed=4)
    yr.backward(gy)
    d = dev()
    tg = [t.to(d).requires_grad_(True) if t is not None else None for t in (x, w, b, r)]
    yg = ops.linear(tg[0], tg[1], tg[2], residual=tg[3], relu=relu)
    assert_close(yg, yr, what='linear y %s' % (case,))
    yg.backward(gy.to(d))
    for name, a, bb in zip(('dx', 'dw', 'db', 'dres'), tg, ts):
        if a is not None:
            assert_close(a.grad, bb.grad, 1e-3, 1e-4, 'linear %s %s' % (name, case))


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('relu,res', [(True, True), (True, False), (False, False)])
@pytest.mark.parametrize('shape', [(2, 16, 16, 64), (3, 7, 9, 256), (2, 4, 4, 2048), (1, 64, 64, 128)])
def test_batchnorm(training, relu, res, shape):
    from renderih_amd import ops
    N, H, W, Cc = shape
    x = rnd(N, Cc, H, W, seed=1) * 2 + 0.5
    r = rnd(N, Cc, H, W, seed=2) if res else None
    g, b = torch.rand(Cc) + 0.5, rnd(Cc, seed=3) * 0.1
    rm, rv = rnd(Cc, seed=4) * 0.1, torch.rand(Cc) + 0.5
    xr, gr, br = x.clone().requires_grad_(True), g.clone().requires_grad_(True), b.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if res else None
    rm_r, rv_r = rm.clone(), rv.clone()
    yr = F.batch_norm(xr, rm_r, rv_r, gr, br, training, 0.1, 1e-5)
    if res:
        yr = yr + rr
    if relu:
        yr = F.relu(yr)
    gy = rnd(*yr.shape, seed=5)
    yr.backward(gy)
    d = dev()
    xg = nhwc(x).to(d).requires_grad_(True)
    gg, bg = g.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    rg = nhwc(r).to(d).requires_grad_(True) if res else None
    rm_g, rv_g = rm.to(d), rv.to(d)
    yg = ops.batchnorm(xg, gg, bg, rm_g, rv_g, residual=rg, training=training, relu=relu)
    assert_close(nchw(yg), yr, what='bn y')
    yg.backward(nhwc(gy).to(d))
    assert_close(nchw(xg.grad), xr.grad, 1e-3, 1e-4, 'bn dx')
    assert_close(gg.grad, gr.grad, 1e-3, 1e-4, 'bn dgamma')
    assert_close(bg.grad, br.grad, 1e-3, 1e-4, 'bn dbeta')
    if res:
        assert_close(nchw(rg.grad), rr.grad, 1e-3, 1e-4, 'bn dres')
    assert_close(rm_g, rm_r, 1e-4, 1e-5, 'bn running_mean')
    assert_close(rv_g, rv_r, 1e-4, 1e-5, 'bn running_var')


def check_linear_dropout_epilogue(rows, K, Nf, relu, res, pair=False, p=0.3, expect_fused=True):
    """rih_gemm_desc.drop_p (ops.linear / ops.linear_pair with drop=): dropout in the GEMM's epilogue against the GEMM followed by
    rih_add_dropout -- the same mask stream, so the output and every gradient are bit-identical; shapes the epilogue does not
    take (ragged K) fall back to the two launches inside ops."""
    from renderih_amd import ops
    import torch.nn as nn
    d = dev()
    lead = (2, rows) if pair else (rows,)
    x = rnd(*lead, K, seed=21).to(d)
    r = rnd(*lead, Nf, seed=22).to(d) if res else None
    gy = rnd(*lead, Nf, seed=23).to(d)
    mods = [nn.Linear(K, Nf) for _ in range(2 if pair else 1)]
    for i, m in enumerate(mods):
        m.weight.data = rnd(Nf, K, seed=24 + i) * 0.2
        m.bias.data = rnd(Nf, seed=26 + i) * 0.1
        m.to(d)
    seed = 0x1234567 + rows
    took = []
    orig = ops._finish_dropout

    def recording(fused, *a):
        took.append(bool(fused))
        return orig(fused, *a)

    def run(fuse):
        xs = x.clone().requires_grad_(True)
        rs = r.clone().requires_grad_(True) if res else None
        for m in mods:
            m.zero_grad(set_to_none=True)
        if fuse:
            y = (ops.linear_pair(xs, mods[0], mods[1], residual=rs, relu=relu, drop=(p, seed)) if pair else
                 ops.linear(xs, mods[0].weight, mods[0].bias, residual=rs, relu=relu, drop=(p, seed)))
        else:
            t = (ops.linear_pair(xs, mods[0], mods[1], relu=relu) if pair else
                 ops.linear(xs, mods[0].weight, mods[0].bias, relu=relu))
            y = ops.add_dropout(rs, t, p, seed)
        y.backward(gy)
        grads = [xs.grad] + [g for m in mods for g in (m.weight.grad.clone(), m.bias.grad.clone())] + ([rs.grad] if res else [])
        return y.detach(), grads
    y0, g0 = run(False)
    ops._finish_dropout = recording
    try:
        y1, g1 = run(True)
    finally:
        ops._finish_dropout = orig
    assert took == [expect_fused], (took, expect_fused)
    assert torch.equal(y0, y1)
    zeros = float((y1 == (r if res else 0)).float().mean())
    assert (0.5 * p < zeros < 1.0) if not relu else zeros > 0.5 * p        # the mask is really there
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)


@pytest.mark.parametrize('case', [(8064, 256, 256, False, True, True), (40448, 64, 64, True, False, True),
                                  (8128, 128, 128, False, True, False), (300, 64, 509, False, True, False),
                                  (126, 30, 64, True, False, False, 0.3, False)])
def test_linear_dropout_epilogue_is_bit_identical(case):
    check_linear_dropout_epilogue(*case)


@pytest.mark.parametrize('rows,D,x2,relu', [(126, 64, False, False), (4, 509, False, False), (300, 256, True, True),
                                             (1000, 128, True, False), (64, 512, False, True), (7, 1024, True, True),
                                             (131, 64, True, True), (5, 128, False, False), (3, 200, True, True)])
def test_layernorm(rows, D, x2, relu):
    from renderih_amd import ops
    x, y2 = rnd(rows, D, seed=1) * 2 + 0.3, (rnd(rows, D, seed=2) if x2 else None)
    g, b = torch.rand(D) + 0.5, rnd(D, seed=3) * 0.1
    ts = [t.clone().requires_grad_(True) if t is not None else None for t in (x, y2, g, b)]
    inp = ts[0] + ts[1] if x2 else ts[0]
    yr = F.layer_norm(inp, (D,), ts[2], ts[3], 1e-6)
    if relu:
        yr = F.relu(yr)
    gy = rnd(rows, D, seed=4)
    yr.backward(gy)
    d = dev()
    tg = [t.to(d).requires_grad_(True) if t is not None else None for t in (x, y2, g, b)]
    yg = ops.layernorm(tg[0], tg[2], tg[3], eps=1e-6, x2=tg[1], relu=relu)
    assert_close(yg, yr, what='ln y')
    yg.backward(gy.to(d))
    for name, a, bb in zip(('dx', 'dx2', 'dg', 'db'), tg, ts):
        if a is not None:
            assert_close(a.grad, bb.grad, 1e-3, 1e-4, 'ln ' + name)


def _mha_ref(q, k, v, h):
    B, Sq, D = q.shape
    d = D // h
    qq = q.view(B, Sq, h, d).transpose(1, 2)
    kk = k.view(B, -1, h, d).transpose(1, 2)
    vv = v.view(B, -1, h, d).transpose(1, 2)
    a = torch.softmax(qq @ kk.transpose(-1, -2) / d ** 0.5, -1)
    return (a @ vv).transpose(1, 2).contiguous().view(B, Sq, D), a


@pytest.mark.parametrize('B,Sq,Sk,D,h', [(2, 64, 64, 256, 4), (2, 127, 127, 256, 4), (2, 190, 190, 128, 4),
                                          (3, 316, 316, 64, 4), (2, 63, 63, 256, 4), (2, 126, 252, 128, 4)])
def test_attention(B, Sq, Sk, D, h):
    from renderih_amd import ops
    q, k, v = rnd(B, Sq, D, seed=1), rnd(B, Sk, D, seed=2), rnd(B, Sk, D, seed=3)
    ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
    yr, _ = _mha_ref(*ts, h)
    gy = rnd(B, Sq, D, seed=4)
    yr.backward(gy)
    d = dev()
    tg = [t.to(d).requires_grad_(True) for t in (q, k, v)]
    yg = ops.attention(tg[0], tg[1], tg[2], h)
    assert_close(yg, yr, what='attn out')
    yg.backward(gy.to(d))
    for name, a, bb in zip(('dq', 'dk', 'dv'), tg, ts):
        assert_close(a.grad, bb.grad, 1e-3, 1e-4, 'attn ' + name)


@pytest.mark.parametrize('B,Sq,Sk,D,h,p', [(2, 127, 127, 256, 4, 0.0), (1, 190, 190, 128, 4, 0.1), (1, 316, 316, 64, 4, 0.05),
                                          (2, 63, 252, 128, 4, 0.0), (1, 33, 5, 64, 4, 0.2), (3, 1, 129, 32, 2, 0.0)])
def test_flash_attention_equals_three_kernel_path(B, Sq, Sk, D, h, p):
    """rih_flash_attention_* (no score matrix in memory: online softmax on transposed score tiles, probabilities recomputed in
    the backward from one log-sum-exp word per row) against the three-kernel sequence (batched QK^T GEMM, softmax, batched PV
    GEMM) it replaces, on the decoder's shapes -- head widths 64 / 32 / 16, ragged query and key counts, cross attention with
    Sq != Sk, a single query row -- with the SAME dropout mask (same hash, same element index): outputs and dq / dk / dv."""
    from renderih_amd import ops
    d = dev()
    q, k, v, gy = rnd(B, Sq, D, seed=1), rnd(B, Sk, D, seed=2) * 1.5, rnd(B, Sk, D, seed=3), rnd(B, Sq, D, seed=4)
    res = []
    saved = ops.FLASH_ATTN
    try:
        for flash in (False, True):
            ops.FLASH_ATTN = flash
            # (fresh leaves per path: where dev() is the CPU, .to() alone returns q, k, v themselves and both paths would add
            # into the same .grad tensors, which the comparison below would then hold against themselves)
            tg = [t.clone().to(d).requires_grad_(True) for t in (q, k, v)]
            y = ops.attention(tg[0], tg[1], tg[2], h, p, 987654321)
            y.backward(gy.to(d))
            res.append([y.detach()] + [t.grad for t in tg])
    finally:
        ops.FLASH_ATTN = saved
    for name, a, b in zip(('out', 'dq', 'dk', 'dv'), res[1], res[0]):
        assert_close(a, b, 2e-4, 2e-5, 'flash attention ' + name)


def _hash_np(seed, idx):
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


def test_attention_dropout_matches_hash_mask():
    from renderih_amd import ops
    B, S, D, h, p, seed = 2, 100, 64, 4, 0.25, 123456789
    q, k, v = rnd(B, S, D, seed=1), rnd(B, S, D, seed=2), rnd(B, S, D, seed=3)
    with np.errstate(over='ignore'):
        keep = _hash_np(seed, np.arange(B * h * S * S)) >= np.uint64(int(p * 2 ** 32))
    keep = torch.from_numpy(keep.reshape(B, h, S, S))
    assert abs(keep.float().mean().item() - (1 - p)) < 0.01
    ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
    _, a = _mha_ref(*ts, h)
    a = a * keep / (1 - p)
    vv = ts[2].view(B, S, h, D // h).transpose(1, 2)
    yr = (a @ vv).transpose(1, 2).contiguous().view(B, S, D)
    gy = rnd(B, S, D, seed=4)
    yr.backward(gy)
    d = dev()
    tg = [t.to(d).requires_grad_(True) for t in (q, k, v)]
    yg = ops.attention(tg[0], tg[1], tg[2], h, p, seed)
    assert_close(yg, yr, what='attn+dropout out')
    yg.backward(gy.to(d))
    for name, a_, bb in zip(('dq', 'dk', 'dv'), tg, ts):
        assert_close(a_.grad, bb.grad, 1e-3, 1e-4, 'attn+dropout ' + name)


def test_add_dropout_and_bcast():
    from renderih_amd import ops
    d = dev()
    a, b = rnd(4, 63, 128, seed=1), rnd(4, 63, 128, seed=2)
    ag, bg = a.to(d).requires_grad_(True), b.to(d).requires_grad_(True)
    y = ops.add_dropout(ag, bg, 0.0, 0)
    assert_close(y, a + b, what='add')
    p, seed = 0.3, 42
    y = ops.add_dropout(ag, bg, p, seed)
    with np.errstate(over='ignore'):
        keep = torch.from_numpy((_hash_np(seed, np.arange(a.numel())) >= np.uint64(int(p * 2 ** 32))).reshape(a.shape))
    assert_close(y, a + b * keep / (1 - p), what='add_dropout')
    gy = rnd(*a.shape, seed=3)
    y.backward(gy.to(d))
    assert_close(ag.grad, gy, what='add_dropout da')
    assert_close(bg.grad, gy * keep / (1 - p), what='add_dropout db')
    e = rnd(63, 128, seed=5)
    eg = e.to(d).requires_grad_(True)
    ag.grad = None
    y = ops.add_rows_bcast(ag, eg)
    assert_close(y, a + e, what='bcast add')
    y.backward(gy.to(d))
    assert_close(eg.grad, gy.sum(0), 1e-4, 1e-5, 'bcast de')


def test_pool_upsample_layout():
    from renderih_amd import ops
    d = dev()
    for Cc in (64, 6):          # 16-byte (channel-quad) kernels and the scalar ones (C % 4 != 0)
        x = rnd(2, Cc, 18, 18, seed=1)
        xr = x.clone().requires_grad_(True)
        yr = F.max_pool2d(xr, 3, 2, 1)
        gy = rnd(*yr.shape, seed=2)
        yr.backward(gy)
        xg = nhwc(x).to(d).requires_grad_(True)
        yg = ops.maxpool3x3s2(xg)
        assert_close(nchw(yg), yr, what='maxpool C=%d' % Cc)
        yg.backward(nhwc(gy).to(d))
        assert_close(nchw(xg.grad), xr.grad, what='maxpool dx C=%d' % Cc)

    for H, Cc in ((8, 128), (16, 128), (5, 128), (7, 10)):
        x = rnd(2, Cc, H, H + 1, seed=3)
        xr = x.clone().requires_grad_(True)
        yr = F.interpolate(xr, scale_factor=2, mode='bilinear', align_corners=True)
        gy = rnd(*yr.shape, seed=4)
        yr.backward(gy)
        xg = nhwc(x).to(d).requires_grad_(True)
        yg = ops.upsample_bilinear2x(xg)
        assert_close(nchw(yg), yr, what='upsample %d' % H)
        yg.backward(nhwc(gy).to(d))
        assert_close(nchw(xg.grad), xr.grad, 1e-4, 1e-5, 'upsample dx %d' % H)

    x = rnd(3, 2048, 8, 8, seed=5)
    xr = x.clone().requires_grad_(True)
    yr = F.adaptive_avg_pool2d(xr, 1).flatten(1)
    gy = rnd(3, 2048, seed=6)
    yr.backward(gy)
    xg = nhwc(x).to(d).requires_grad_(True)
    yg = ops.global_avgpool(xg)
    assert_close(yg, yr, what='avgpool')
    yg.backward(gy.to(d))
    assert_close(nchw(xg.grad), xr.grad, what='avgpool dx')

    img = rnd(2, 3, 32, 32, seed=7)
    y = ops.nchw_to_nhwc(img.to(d), cpad=4)
    assert torch.equal(y[..., :3].cpu(), nhwc(img)) and float(y[..., 3].abs().max()) == 0.0
    t = rnd(2, 16, 16, 8, seed=8)
    tg = t.to(d).requires_grad_(True)
    a, b = ops.nhwc_to_nchw(tg, 0, 2), ops.nhwc_to_nchw(tg, 2, 8)
    assert torch.equal(a.cpu(), nchw(t)[:, :2]) and torch.equal(b.cpu(), nchw(t)[:, 2:])
    (a.sum() + 2 * b.sum()).backward()
    want = torch.ones_like(t)
    want[..., 2:] = 2
    assert torch.equal(tg.grad.cpu(), want)


@pytest.mark.parametrize('f,H,W,C', [(2, 8, 8, 64), (4, 16, 16, 128), (8, 8, 8, 256), (4, 5, 7, 32)])
def test_resample_hrnet(f, H, W, C):
    """Bilinear x2/x4/x8 (align_corners, HRNet heads) and the fused nearest-upsample + add of the HRNet fuse layers."""
    from renderih_amd import ops
    d = dev()
    x = rnd(2, C, H, W, seed=11)
    xr = x.clone().requires_grad_(True)
    yr = F.interpolate(xr, size=(f * H, f * W), mode='bilinear', align_corners=True)
    gy = rnd(*yr.shape, seed=12)
    yr.backward(gy)
    xg = nhwc(x).to(d).requires_grad_(True)
    yg = ops.upsample_bilinear(xg, f)
    assert_close(nchw(yg), yr, what='bilinear x%d' % f)
    yg.backward(nhwc(gy).to(d))
    assert_close(nchw(xg.grad), xr.grad, 1e-4, 1e-5, 'bilinear x%d dx' % f)

    acc = rnd(2, C, f * H, f * W, seed=13)
    xr = x.clone().requires_grad_(True)
    ar = acc.clone().requires_grad_(True)
    yr = ar + F.interpolate(xr, scale_factor=f, mode='nearest')
    yr.backward(gy)
    xg = nhwc(x).to(d).requires_grad_(True)
    ag = nhwc(acc).to(d).requires_grad_(True)
    yg = ops.nearest_up_add(xg, ag, f)
    assert_close(nchw(yg), yr, what='nearest x%d + add' % f)
    yg.backward(nhwc(gy).to(d))
    assert_close(nchw(xg.grad), xr.grad, 1e-4, 1e-5, 'nearest x%d dx' % f)
    assert_close(nchw(ag.grad), ar.grad, what='nearest add grad')
    y0 = ops.nearest_up_add(nhwc(x).to(d), None, f)
    assert_close(nchw(y0), F.interpolate(x, scale_factor=f, mode='nearest'), what='nearest x%d' % f)


def test_cheby_gather_project():
    from renderih_amd import ops, assets
    from renderih_amd.attn import GraphCSR
    d = dev()
    # (graph level, F): LDS-staged kernels (V <= 256; F = 24: a partial channel slice), the gather kernels (504 vertices) and
    # the scalar ones (F % 4 != 0)
    for level, Fc in ((3, 64), (2, 256), (4, 24), (1, 32), (3, 6)):
        L = assets.load_graph_dict('left')['coarsen_graphs_L'][level]
        V = L.shape[0]
        Ld = torch.from_numpy(np.asarray(L.todense(), dtype=np.float32))
        csr, csr_t = GraphCSR(Ld.numpy()).on(d)
        x = rnd(3, V, Fc, seed=1)
        xr = x.clone().requires_grad_(True)
        yr = torch.stack((xr, torch.matmul(Ld, xr)), -1).flatten(-2)
        gy = rnd(*yr.shape, seed=2)
        yr.backward(gy)
        xg = x.to(d).requires_grad_(True)
        yg = ops.cheby_features(xg, csr, csr_t)
        assert_close(yg, yr, what='cheby V=%d F=%d' % (V, Fc))
        yg.backward(gy.to(d))
        assert_close(xg.grad, xr.grad, 1e-4, 1e-5, 'cheby dx V=%d F=%d' % (V, Fc))

    idx = np.random.RandomState(0).randint(0, 50, size=120)
    g = ops.RowIndex(idx, 50, d)
    x = rnd(2, 50, 3, seed=3)
    xr = x.clone().requires_grad_(True)
    yr = xr[:, torch.from_numpy(idx)]
    gy = rnd(*yr.shape, seed=4)
    yr.backward(gy)
    xg = x.to(d).requires_grad_(True)
    yg = g(xg)
    assert torch.equal(yg.cpu(), yr.detach())
    yg.backward(gy.to(d))
    assert_close(xg.grad, xr.grad, 1e-5, 1e-6, 'gather dx')

    v, s, t = rnd(4, 778, 3, seed=5) * 0.1, torch.rand(4) + 0.5, rnd(4, 2, seed=6) * 0.2
    ts = [a.clone().requires_grad_(True) for a in (v, s, t)]
    yr = (ts[1] * 256).view(-1, 1, 1) * ts[0][..., :2] + (ts[2] * 128 + 128).unsqueeze(1)
    gy = rnd(4, 778, 2, seed=7)
    yr.backward(gy)
    tg = [a.to(d).requires_grad_(True) for a in (v, s, t)]
    yg = ops.projection_batch(tg[1], tg[2], tg[0], 256)
    assert_close(yg, yr, what='project')
    yg.backward(gy.to(d))
    for name, a, b in zip(('dv', 'dscale', 'dtrans'), tg, ts):
        assert_close(a.grad, b.grad, 1e-4, 1e-5, 'project ' + name)


@pytest.mark.parametrize('B,S,D,h', [(2, 64, 256, 4), (2, 190, 128, 4), (2, 316, 64, 4)])
def test_self_attention_packed(B, S, D, h):
    from renderih_amd import ops
    qkv = rnd(B, S, 3 * D, seed=1)
    t = qkv.clone().requires_grad_(True)
    yr, _ = _mha_ref(t[..., :D].contiguous(), t[..., D:2 * D].contiguous(), t[..., 2 * D:].contiguous(), h)
    gy = rnd(B, S, D, seed=2)
    yr.backward(gy)
    d = dev()
    g = qkv.to(d).clone().requires_grad_(True)
    yg = ops.self_attention_packed(g, h)
    assert_close(yg, yr, what='packed self-attn out')
    yg.backward(gy.to(d))
    assert_close(g.grad, t.grad, 1e-3, 1e-4, 'packed self-attn dqkv')


@pytest.mark.parametrize('B,V,D,h', [(2, 63, 256, 4), (2, 252, 64, 4)])
def test_cross_attention_packed(B, V, D, h):
    from renderih_amd import ops
    L, R = rnd(B, V, 3 * D, seed=1), rnd(B, V, 3 * D, seed=2)
    tl, tr = L.clone().requires_grad_(True), R.clone().requires_grad_(True)
    sl = lambda t, i: t[..., i * D:(i + 1) * D].contiguous()
    r2l, _ = _mha_ref(sl(tl, 0), sl(tr, 1), sl(tr, 2), h)
    l2r, _ = _mha_ref(sl(tr, 0), sl(tl, 1), sl(tl, 2), h)
    g1, g2 = rnd(B, V, D, seed=3), rnd(B, V, D, seed=4)
    ((r2l * g1).sum() + (l2r * g2).sum()).backward()
    d = dev()
    gl, gr = L.to(d).clone().requires_grad_(True), R.to(d).clone().requires_grad_(True)
    a, b = ops.cross_attention_packed(gl, gr, h)
    assert_close(a, r2l, what='cross R2L')
    assert_close(b, l2r, what='cross L2R')
    ((a * g1.to(d)).sum() + (b * g2.to(d)).sum()).backward()
    assert_close(gl.grad, tl.grad, 1e-3, 1e-4, 'cross dL')
    assert_close(gr.grad, tr.grad, 1e-3, 1e-4, 'cross dR')


def _tile4_engine2(case, d):
    from renderih_amd import ops
    N, H, W, Cin, Cout, k, s, p = case
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = (rnd(N, H, W, Cin, seed=31) * 37.0).to(d)               # magnitudes away from 1: the operand scales matter
    wp = (rnd(k * k * Cin, Cout, seed=32) * 1e-3).to(d)
    M, K = N * Ho * Wo, k * k * Cin
    geom = (H, W, Cin, Ho, Wo, k, k, s, 1, p, p)
    bx, bw = ops.bound_of(x), ops.bound_of(wp)
    ys, sts = [], []
    for t in (0, 4):
        y = torch.empty(N, Ho, Wo, Cout, device=d)
        h = ops.StatsHolder()
        ops.gemm(x, wp, y, M, Cout, K, Cin, Cout, Cout, a_mode=0, b_mode=0, geom=geom, tile=t, engine=2, amax_a=bx, amax_b=bw, stats=h)
        assert h.part is not None and h.rows == (64 if t == 0 else 128), (t, h.rows)
        ys.append(y)
        # per-block (mean, M2) -> whole-tensor mean / variance per channel (Chan's merge, in double on the host)
        part = h.part.double().cpu()
        n = torch.full((h.T,), float(h.rows), dtype=torch.float64)
        n[-1] = M - h.rows * (h.T - 1)
        mean = (part[:, 0] * n[:, None]).sum(0) / M
        var = (part[:, 1] + n[:, None] * (part[:, 0] - mean) ** 2).sum(0) / M
        sts.append((mean, var))
    ref = (x.view(M, -1).double().cpu() if k == 1 else None)
    assert_close(ys[1], ys[0], 1e-5, 1e-6, 'tile4 e2 conv fwd')
    assert_close(sts[1][0], sts[0][0], 1e-5, 1e-6, 'tile4 e2 stats mean')
    assert_close(sts[1][1], sts[0][1], 1e-4, 1e-6, 'tile4 e2 stats var')
    y2 = ys[1].double().view(M, Cout).cpu()
    assert_close(sts[1][0], y2.mean(0), 1e-5, 1e-6, 'tile4 e2 stats mean vs output')
    assert_close(sts[1][1], y2.var(0, unbiased=False), 1e-4, 1e-6, 'tile4 e2 stats var vs output')
    if ref is not None:
        assert_close(ys[1].view(M, Cout), (ref @ wp.double().cpu()).float(), 1e-5, 1e-6, 'tile4 e2 conv vs fp64')
    dy = (rnd(N, Ho, Wo, Cout, seed=33) * 1e-4).to(d)
    bdy = ops.bound_of(dy)
    sk, kc = 2, -(-(-(-M // 2)) // 32) * 32
    parts = []
    for t in (0, 4):
        part = torch.zeros(sk, K, Cout, device=d)
        ops.gemm(x, dy, part, K, Cout, M, Cin, Cout, Cout, a_mode=1, b_mode=0, splitk=sk, kchunk=kc, sCsplit=K * Cout,
                 geom=geom, tile=t, engine=2, amax_a=bx, amax_b=bdy)
        parts.append(part.sum(0))
    assert_close(parts[1], parts[0], 1e-5, 1e-6, 'tile4 e2 wgrad')
    a, b = x.view(M if k == 1 else N * H * W, Cin), (rnd(Cout, Cin, seed=34) * 0.02).to(d)
    bb = ops.bound_of(b)
    zs = []
    for t in (0, 4):
        z = torch.empty(a.shape[0], Cout, device=d)
        ops.gemm(a, b, z, a.shape[0], Cout, Cin, Cin, Cin, Cout, a_mode=0, b_mode=1, tile=t, engine=2, amax_a=bx, amax_b=bb)
        zs.append(z)
    assert_close(zs[1], zs[0], 1e-5, 1e-6, 'tile4 e2 linear')
    assert_close(zs[1], (a.double() @ b.double().t()).float(), 1e-5, 1e-6, 'tile4 e2 linear vs fp64')


# ------------------------------------------------------------------------------- hands-stacked (paired) layers
def _leaf(t, d):
    return t.detach().clone().to(d).requires_grad_(True)


@pytest.mark.parametrize('M,K,N,relu,res,stacked', [(126, 256, 128, False, True, False), (380, 64, 192, False, False, True),
                                                    (64, 512, 64, True, False, False), (33, 12, 6, False, True, False)])
def test_linear_pair(M, K, N, relu, res, stacked):
    """Both hands' nn.Linear in one launch (bias / weight / residual walk by per-slice strides) vs two F.linear."""
    from renderih_amd import ops
    d = dev()
    x = rnd(2, 3, M, K, seed=1)
    w = rnd(2, N, K, seed=2, scale=1 / math.sqrt(K))
    b = rnd(2, N, seed=3)
    r = rnd(2, 3, M, N, seed=4) if res else None
    gy = rnd(2, 3, M, N, seed=5)
    ts = [t.clone().requires_grad_(True) if t is not None else None for t in (x, w, b, r)]
    yr = torch.stack([F.linear(ts[0][h], ts[1][h], ts[2][h]) for h in (0, 1)])
    if res:
        yr = yr + ts[3]
    if relu:
        yr = F.relu(yr)
    yr.backward(gy)
    xg = _leaf(x, d)
    rg = _leaf(r, d) if res else None
    if stacked:
        wg, bg = _leaf(w, d), _leaf(b, d)
        yg = ops.LinearPairFn.apply(xg, wg, None, bg, None, rg, relu)
    else:
        pad = torch.zeros(7 * 4, device=d)          # separately allocated parameters: arbitrary distance in memory
        wl, wr_, bl, br_ = _leaf(w[0], d), _leaf(w[1], d), _leaf(b[0], d), _leaf(b[1], d)
        assert pad.numel() == 28
        yg = ops.LinearPairFn.apply(xg, wl, wr_, bl, br_, rg, relu)
    assert_close(yg, yr, what='linear_pair y')
    yg.backward(gy.to(d))
    assert_close(xg.grad, ts[0].grad, 1e-3, 1e-4, 'linear_pair dx')
    if stacked:
        assert_close(wg.grad, ts[1].grad, 1e-3, 1e-4, 'linear_pair dw')
        assert_close(bg.grad, ts[2].grad, 1e-3, 1e-4, 'linear_pair db')
    else:
        for h, (a, bb) in enumerate(((wl, bl), (wr_, br_))):
            assert_close(a.grad, ts[1].grad[h], 1e-3, 1e-4, 'linear_pair dw%d' % h)
            assert_close(bb.grad, ts[2].grad[h], 1e-3, 1e-4, 'linear_pair db%d' % h)
    if res:
        assert_close(rg.grad, ts[3].grad, 1e-3, 1e-4, 'linear_pair dres')


@pytest.mark.parametrize('decoupled,wd', [(False, 0.0), (False, 1e-2), (True, 1e-2)])
def test_adam_one_launch_matches_torch(decoupled, wd):
    """renderih_amd.optim.Adam / AdamW (rih_adam_multi: every tensor of a parameter group in one launch) against
    torch.optim.Adam / AdamW on the CPU over 4 steps: odd sizes (scalar tail, one element, exactly one chunk, chunk + 1),
    a parameter without gradient, a gradient tensor rebound between steps (table rebuild), then a state_dict round trip into
    the torch optimizer."""
    from renderih_amd import optim
    d = dev()
    sizes = [(1,), (5,), (64, 3, 7, 7), (4096,), (4097,), (300, 257), (2048,)]
    ref = [rnd(*s, seed=i).requires_grad_(True) for i, s in enumerate(sizes)] + [rnd(9, seed=50).requires_grad_(True)]
    got = [t.detach().clone().to(d).requires_grad_(True) for t in ref]
    kw = dict(lr=3e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=wd)
    o_ref = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ref, **kw)
    o_got = (optim.AdamW if decoupled else optim.Adam)(got, **kw)
    for step in range(4):
        for i, (a, b) in enumerate(zip(ref[:-1], got[:-1])):
            g = rnd(*a.shape, seed=100 * step + i) * (10.0 ** (i - 3))
            a.grad = g.clone()
            if step == 2 or b.grad is None:
                b.grad = g.clone().to(d)             # new tensor: the pointer table must follow
            else:
                b.grad.copy_(g)
        o_ref.step()
        o_got.step()
        for i, (a, b) in enumerate(zip(ref, got)):
            assert_close(b.detach(), a.detach(), 2e-6, 1e-7, 'adam step %d tensor %d' % (step, i))
    assert torch.equal(got[-1].detach().cpu(), ref[-1].detach())            # no gradient: untouched, no state
    assert got[-1] not in o_got.state or len(o_got.state[got[-1]]) == 0
    # checkpoints are interchangeable with torch's optimizer
    sd = o_got.state_dict()
    o_t = (torch.optim.AdamW if decoupled else torch.optim.Adam)([t.detach().clone().requires_grad_(True) for t in got], **kw)
    o_t.load_state_dict(sd)
    st = o_t.state[o_t.param_groups[0]['params'][3]]
    assert int(st['step']) == 4
    assert_close(st['exp_avg'], o_ref.state[ref[3]]['exp_avg'], 1e-5, 1e-6, 'exp_avg after round trip')
    assert_close(st['exp_avg_sq'], o_ref.state[ref[3]]['exp_avg_sq'], 1e-5, 1e-6, 'exp_avg_sq after round trip')
    # ... and the loaded optimizer keeps STEPPING like the reference one: every parameter owns its step counter (one shared
    # counter object would be advanced once per parameter by torch's loop, i.e. the bias corrections would run 7x too fast)
    tp = o_t.param_groups[0]['params']
    for i, (a, b) in enumerate(zip(ref[:-1], tp[:-1])):
        g = rnd(*a.shape, seed=900 + i) * (10.0 ** (i - 3))
        a.grad, b.grad = g.clone(), g.clone().to(b.device)
    o_ref.step()
    o_t.step()
    for i, (a, b) in enumerate(zip(ref[:-1], tp[:-1])):
        assert int(o_t.state[b]['step']) == 5, 'step counter of tensor %d after one torch step: %s' % (i, o_t.state[b]['step'])
        assert_close(b.detach(), a.detach(), 2e-6, 1e-7, 'torch step after loading our state, tensor %d' % i)
    # the other direction: torch's state (incl. a checkpoint of an old torch with Python-number steps) into this optimizer
    sd_t = o_t.state_dict()
    for k, st_ in sd_t['state'].items():
        if k % 2 == 0:
            st_['step'] = float(st_['step'])
    o_back = (optim.AdamW if decoupled else optim.Adam)([t.detach().clone().to(d).requires_grad_(True) for t in tp], **kw)
    o_back.load_state_dict(sd_t)
    bp = o_back.param_groups[0]['params']
    for step in range(2):
        for i, (a, b) in enumerate(zip(ref[:-1], bp[:-1])):
            g = rnd(*a.shape, seed=950 + 10 * step + i) * (10.0 ** (i - 3))
            a.grad, b.grad = g.clone(), g.clone().to(d)
        o_ref.step()
        o_back.step()
    for i, (a, b) in enumerate(zip(ref[:-1], bp[:-1])):
        assert int(o_back.state[b]['step']) == 7
        assert_close(b.detach(), a.detach(), 3e-6, 1e-7, 'our step after loading torch state, tensor %d' % i)


def test_deferred_reductions_equal_immediate():
    """ops.deferred_reductions (rih_splitk_reduce_multi: the split-K partial slabs of many weight gradients summed by one
    launch at the end of a backward stage) leaves bit-identical gradients: a strided 3x3 conv with bias, a 1x1 conv, an
    nn.Linear with bias and a paired (left/right) Linear -- > 60 descriptors in total, so the packing splits launches."""
    from renderih_amd import ops
    d = dev()
    x = nhwc(rnd(2, 32, 12, 12, seed=1)).to(d)
    ws = [(rnd(48, 32, 3, 3, seed=2, scale=0.1).to(d).requires_grad_(True), rnd(48, seed=3).to(d).requires_grad_(True), 2, 1),
          (rnd(24, 32, 1, 1, seed=4, scale=0.2).to(d).requires_grad_(True), None, 1, 0)]
    xl = rnd(2, 5, 70, 40, seed=5).to(d)
    wl, bl = rnd(2, 36, 40, seed=6, scale=0.2).to(d).requires_grad_(True), rnd(2, 36, seed=7).to(d).requires_grad_(True)
    wm = [rnd(20, 40, seed=8 + i, scale=0.2).to(d).requires_grad_(True) for i in range(64)]
    lns = [((rnd(40, seed=90 + i) + 1).to(d).requires_grad_(True), rnd(40, seed=95 + i).to(d).requires_grad_(True))
           for i in range(5)]              # LayerNorm parameter gradients ride in the same deferral (rih_ln_param_final_multi)

    def loss():
        t = sum(ops.conv2d(x, w, b, stride=s, pad=p).sum() * (i + 1) for i, (w, b, s, p) in enumerate(ws))
        t = t + (ops.LinearPairFn.apply(xl, wl, None, bl, None, None, False) ** 2).sum()
        for i, w in enumerate(wm):
            t = t + (ops.linear(xl[0], w) * (0.5 + i)).sum()
        for i, (g, b) in enumerate(lns[:3]):            # (every parameter is used ONCE: autograd must not sum two uses early)
            t = t + (ops.layernorm(xl[1], g, b) * (1 + i)).sum()
        t = t + (ops.LayerNormPairFn.apply(xl, None, lns[3][0], lns[4][0], lns[3][1], lns[4][1], 1e-6, True, False) ** 2).sum()
        return t

    params = [w for w, _, _, _ in ws] + [ws[0][1], wl, bl] + wm + [p for gb in lns for p in gb]
    want = torch.autograd.grad([loss()], params)
    saved = ops.GROUP_WGRAD
    ops.GROUP_WGRAD = 0             # same split-K plan as the immediate path: bit-identical sums (grouping: the test below)
    try:
        with ops.deferred_reductions():
            got = torch.autograd.grad([loss()], params)
    finally:
        ops.GROUP_WGRAD = saved
    assert ops._DEFERRED is None and ops._DEFERRED_LN is None and ops._DEFERRED_GEMM is None
    for a, b in zip(got, want):
        assert bool(torch.isfinite(b).all()) and torch.equal(a, b)


@pytest.mark.parametrize('level', [1, 2])
def test_grouped_weight_gradients(level, xs=1.0, ws=1.0, gs=1.0):
    """ops.GROUP_WGRAD: inside deferred_reductions() the weight-gradient GEMMs themselves are collected and run as ONE
    rih_gemm_multi launch per kernel variant at the end of the block, with fewer split-K slices per problem (the problems fill the
    chip together).  Decoder-like shapes -- paired nn.Linear (nb1 = 2, bias row), single nn.Linear, 3x3 / 1x1 convolutions with
    and without bias, a gradient large enough for the 128x128 tile -- against the immediate path: equal to split-K round-off,
    and bit-reproducible from run to run."""
    from renderih_amd import ops
    d = dev()
    leaf = lambda t, s: scaled(t, s).to(d).requires_grad_(True)
    x = nhwc(scaled(rnd(2, 32, 8, 8, seed=1), xs)).to(d)
    x64 = nhwc(scaled(rnd(2, 64, 8, 8, seed=21), xs)).to(d)
    convs = [(x, leaf(rnd(64, 32, 3, 3, seed=2, scale=0.1), ws), leaf(rnd(64, seed=3), xs * ws), 1, 1),
             (x, leaf(rnd(40, 32, 1, 1, seed=4, scale=0.2), ws), None, 1, 0),
             (x64, leaf(rnd(136, 64, 3, 3, seed=22, scale=0.1), ws), None, 1, 1)]        # 576 x 136: 128x128 tiles
    xl = scaled(rnd(2, 4, 66, 40, seed=5), xs).to(d)       # 264 rows per hand
    wl, bl = leaf(rnd(2, 72, 40, seed=6, scale=0.2), ws), leaf(rnd(2, 72, seed=7), xs * ws)
    wm = [leaf(rnd(36 + 4 * i, 40, seed=8 + i, scale=0.2), ws) for i in range(5)]
    bm = [leaf(rnd(36 + 4 * i, seed=40 + i), xs * ws) for i in range(5)]

    def loss():
        t = sum(ops.conv2d(xx, w, b, stride=s, pad=p).sum() * (i + 1) for i, (xx, w, b, s, p) in enumerate(convs))
        t = t + (ops.LinearPairFn.apply(xl, wl, None, bl, None, None, False) ** 2).sum()
        for i, (w, b) in enumerate(zip(wm, bm)):
            t = t + (ops.linear(xl[i % 2], w, b) * (0.5 + i)).sum()
        return scaled(t, gs)

    params = [w for _, w, _, _, _ in convs] + [convs[0][2], wl, bl] + wm + bm
    want = torch.autograd.grad([loss()], params)
    seen = []
    flush = ops.GroupedGemms.flush

    def spy(self):
        seen.extend(v for v, _, _, _ in self.items)
        return flush(self)
    saved = ops.GROUP_WGRAD
    ops.GROUP_WGRAD = level
    ops.GroupedGemms.flush = spy
    try:
        runs = []
        for _ in range(2):
            with ops.deferred_reductions():
                runs.append(torch.autograd.grad([loss()], params))
    finally:
        ops.GROUP_WGRAD = saved
        ops.GroupedGemms.flush = flush
    if ops.ENGINE == 1:
        # paired + 5 single Linears + the 3x3 / 1x1 convolutions rode in grouped launches; level 2 adds the 128x128-tile one
        assert seen.count(2 * 8 + 4 + 1) >= 2 * 6 and seen.count(2 * 8 + 4 + 0) >= 2, seen
        assert (seen.count(0 * 8 + 4 + 0) >= 2) == (level == 2), seen
    for a, a2, b in zip(runs[0], runs[1], want):
        assert torch.equal(a, a2)
        assert_close(a, b, 2e-5, 2e-5, 'grouped weight gradient')


@pytest.mark.parametrize('rows,D,relu,x2,skip', [(190, 128, False, False, True), (126, 256, True, True, False),
                                                 (5, 509, False, False, False), (67, 64, True, False, True),
                                                 (40, 64, False, True, False)])
def test_layernorm_pair(rows, D, relu, x2, skip):
    from renderih_amd import ops
    d = dev()
    x, xb = rnd(2, rows, D, seed=1) * 2 + 0.3, (rnd(2, rows, D, seed=2) if x2 else None)
    g, b = rnd(2, D, seed=3) + 1, rnd(2, D, seed=4)
    gy, gs = rnd(2, rows, D, seed=5), rnd(2, rows, D, seed=6)
    ts = [t.clone().requires_grad_(True) if t is not None else None for t in (x, xb, g, b)]
    xin = ts[0] + ts[1] if x2 else ts[0]
    yr = torch.stack([F.layer_norm(xin[h], (D,), ts[2][h], ts[3][h], 1e-6) for h in (0, 1)])
    if relu:
        yr = F.relu(yr)
    ((yr * gy).sum() + ((ts[0] * gs).sum() if skip else 0)).backward()
    xg = _leaf(x, d)
    x2g = _leaf(xb, d) if x2 else None
    ps = [_leaf(t, d) for t in (g[0], g[1], b[0], b[1])]
    out = ops.LayerNormPairFn.apply(xg, x2g, ps[0], ps[1], ps[2], ps[3], 1e-6, relu, skip)
    yg = out[0] if skip else out
    assert_close(yg, yr, what='layernorm_pair y')
    ((yg * gy.to(d)).sum() + ((out[1] * gs.to(d)).sum() if skip else 0)).backward()
    assert_close(xg.grad, ts[0].grad, 1e-3, 1e-4, 'layernorm_pair dx')
    if x2:
        assert_close(x2g.grad, ts[1].grad, 1e-3, 1e-4, 'layernorm_pair dx2')
    for h in (0, 1):
        assert_close(ps[h].grad, ts[2].grad[h], 1e-3, 1e-4, 'layernorm_pair dg%d' % h)
        assert_close(ps[2 + h].grad, ts[3].grad[h], 1e-3, 1e-4, 'layernorm_pair db%d' % h)


@pytest.mark.parametrize('N,H,Cin,Cout,p', [(2, 16, 256, 128, 2), (2, 32, 64, 64, 4), (3, 8, 32, 48, 1),
                                            (2, 16, 64, 48, 4)])     # the last one: K = 1024, two tiles -> forward split-K
def test_patch_conv_pair(N, H, Cin, Cout, p):
    """relu(conv(x, w_h) + b_h), kernel = stride = patch, for both hands on one shared map; the data gradient is the
    un-patchified GEMM, summed over the hands."""
    from renderih_amd import ops
    d = dev()
    x = rnd(N, Cin, H, H, seed=1)
    w = rnd(2, Cout, Cin, p, p, seed=2, scale=1 / math.sqrt(Cin * p * p))
    b = rnd(2, Cout, seed=3)
    g = H // p
    gy = rnd(2, N, g, g, Cout, seed=4)
    ts = [t.clone().requires_grad_(True) for t in (x, w, b)]
    yr = torch.stack([nhwc(F.relu(F.conv2d(ts[0], ts[1][h], ts[2][h], stride=p))) for h in (0, 1)])
    yr.backward(gy)
    xg = _leaf(nhwc(x), d)
    ps = [_leaf(t, d) for t in (w[0], w[1], b[0], b[1])]
    yg = ops.PatchConvPairFn.apply(xg, *ps)
    assert_close(yg, yr, what='patch_conv_pair y')
    yg.backward(gy.to(d))
    assert_close(nchw(xg.grad), ts[0].grad, 1e-3, 1e-4, 'patch_conv_pair dx')
    for h in (0, 1):
        assert_close(ps[h].grad, ts[1].grad[h], 1e-3, 1e-4, 'patch_conv_pair dw%d' % h)
        assert_close(ps[2 + h].grad, ts[2].grad[h], 1e-3, 1e-4, 'patch_conv_pair db%d' % h)


def test_cross_attention_stacked_and_rows_pair():
    from renderih_amd import ops
    d = dev()
    B, V, D, h = 2, 63, 128, 4
    qkv = rnd(2, B, V, 3 * D, seed=1)
    g1 = rnd(2, B, V, D, seed=2)
    a = _leaf(qkv, d)
    o = ops.cross_attention_stacked(a, h)
    b0, b1 = _leaf(qkv[0], d), _leaf(qkv[1], d)
    r2l, l2r = ops.cross_attention_packed(b0, b1, h)
    assert torch.equal(o[0], r2l) and torch.equal(o[1], l2r)
    o.backward(g1.to(d))
    (r2l * g1[0].to(d)).sum().backward(retain_graph=True)
    (l2r * g1[1].to(d)).sum().backward()
    assert_close(a.grad[0], b0.grad, 1e-5, 1e-6, 'cross stacked dL')
    assert_close(a.grad[1], b1.grad, 1e-5, 1e-6, 'cross stacked dR')

    x, e = rnd(2, 3, 64, 32, seed=3), rnd(2, 64, 32, seed=4)
    xr, er = x.clone().requires_grad_(True), e.clone().requires_grad_(True)
    yr = xr + er[:, None]
    gy = rnd(2, 3, 64, 32, seed=5)
    yr.backward(gy)
    xg, el, er_ = _leaf(x, d), _leaf(e[0], d), _leaf(e[1], d)
    yg = ops.add_rows_pair(xg, el, er_)
    assert_close(yg, yr, what='add_rows_pair')
    yg.backward(gy.to(d))
    assert_close(xg.grad, xr.grad, 1e-5, 1e-6, 'add_rows_pair dx')
    assert_close(el.grad, er.grad[0], 1e-4, 1e-5, 'add_rows_pair de0')
    assert_close(er_.grad, er.grad[1], 1e-4, 1e-5, 'add_rows_pair de1')


def test_pack_cache_one_launch_equals_per_call_packs():
    """ops.PackCache (rih_pack_conv_weight_multi): after the recording pass, refresh() repacks every operand in one launch
    from the CURRENT weights, and the convolutions (forward, strided and dense data gradients) give bit-identical results to
    the per-call packs; a weight update between steps is picked up by the next refresh."""
    from renderih_amd import ops
    d = dev()
    x = nhwc(rnd(2, 8, 13, 11, seed=1)).to(d).requires_grad_(True)
    ws = [rnd(16, 8, 3, 3, seed=2, scale=0.2).to(d).requires_grad_(True), rnd(12, 16, 3, 3, seed=3, scale=0.2).to(d).requires_grad_(True),
          rnd(8, 12, 2, 2, seed=4, scale=0.3).to(d).requires_grad_(True)]

    def run():
        h = ops.conv2d(x, ws[0], None, stride=1, pad=1)
        h = ops.conv2d(h, ws[1], None, stride=2, pad=1)
        h = ops.conv2d(h, ws[2], None, stride=2, pad=0)
        return [h] + list(torch.autograd.grad([(h * h).sum()], [x] + ws))

    want = run()
    pc = ops.PackCache()
    try:
        ops._PACK = pc
        first = run()                       # recording pass: packs on the spot
        assert len(pc.entries) >= 5         # 3 forward operands + the dense and the parity-class data-gradient operands
        pc.refresh()
        second = run()                      # everything from the one-launch refresh
        with torch.no_grad():
            for w in ws:
                w.mul_(1.5)
        pc.stale()
        ops._PACK = None
        want2 = run()
        ops._PACK = pc
        pc.refresh()
        third = run()
    finally:
        ops._PACK = None
    for a, b, c in zip(want, first, second):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b in zip(want2, third):
        assert torch.equal(a, b)
    assert not torch.equal(want[0], want2[0])


@pytest.mark.parametrize('case', [(2, 16, 16, 64, 128, 3, 1, 1, False), (3, 9, 7, 32, 72, 3, 2, 1, True),
                                  (2, 16, 16, 64, 256, 1, 1, 0, False), (40, 32, 32, 64, 64, 1, 1, 0, True),
                                  (1, 10, 10, 64, 36, 1, 1, 0, False), (2, 8, 8, 256, 256, 3, 1, 1, False)])
def test_conv_bn_statistics_from_the_gemm_epilogue(case):
    """encoder.conv_bn in training mode: the BatchNorm statistics come out of the convolution's GEMM epilogue (raw column sums
    per wave row block, rih_gemm_desc.stats -> rih_bn_stats_from_blocks) -- output, running buffers and all gradients equal the
    separate statistics pass to fp32 round-off, and torch.  Cases: one tile, ragged M / N with a strided 3x3, 1x1 on the 128x128
    tile, 40960 rows (640 row blocks -> the two-launch finish), N = 36 (ragged column tile), and a forward split-K
    convolution (8x8, K = 2304: no statistics path -> the separate pass)."""
    import torch.nn as nn
    from renderih_amd import ops, encoder
    N, H, W, Cin, Cout, k, s, p, conv_relu = case
    d = dev()
    x = rnd(N, Cin, H, W, seed=1)
    cm = nn.Conv2d(Cin, Cout, k, s, p, bias=False)
    bn = nn.BatchNorm2d(Cout)
    with torch.no_grad():
        cm.weight.copy_(rnd(Cout, Cin, k, k, seed=2, scale=1.0 / math.sqrt(Cin * k * k)))
        bn.weight.copy_(torch.rand(Cout, generator=torch.Generator().manual_seed(3)) + 0.5)
        bn.bias.copy_(rnd(Cout, seed=4) * 0.1)
    # torch reference (Conv -> [ReLU] -> BN -> ReLU)
    xr = x.clone().requires_grad_(True)
    import copy
    cm_r, bn_r = copy.deepcopy(cm), copy.deepcopy(bn)
    t = cm_r(xr)
    if conv_relu:
        t = F.relu(t)
    yr = F.relu(bn_r(t))
    gy = rnd(*yr.shape, seed=5)
    yr.backward(gy)
    outs = []
    for use_stats in (True, False):
        cm_g, bn_g = copy.deepcopy(cm).to(d), copy.deepcopy(bn).to(d)
        xg = nhwc(x).to(d).requires_grad_(True)
        old = ops.GEMM_STATS
        ops.GEMM_STATS = use_stats
        try:
            holder_seen = []
            orig = ops.StatsHolder
            if use_stats:
                class Spy(orig):
                    def __init__(self):
                        super().__init__()
                        holder_seen.append(self)
                ops.StatsHolder = Spy
            yg = encoder.conv_bn(cm_g, bn_g, xg, relu=True, conv_relu=conv_relu)
        finally:
            ops.GEMM_STATS = old
            ops.StatsHolder = orig
        if use_stats:
            took = holder_seen and holder_seen[0].part is not None
            assert bool(took) == (case != (2, 8, 8, 256, 256, 3, 1, 1, False)), 'statistics epilogue taken: %s' % took
        yg.backward(nhwc(gy).to(d))
        outs.append((yg.detach(), xg.grad, cm_g.weight.grad, bn_g.weight.grad, bn_g.bias.grad, bn_g.running_mean, bn_g.running_var))
        assert_close(nchw(yg), yr, what='conv_bn y (stats=%s)' % use_stats)
        assert_close(nchw(xg.grad), xr.grad, 1e-3, 1e-4, 'conv_bn dx')
        assert_close(cm_g.weight.grad, cm_r.weight.grad, 1e-3, 1e-4, 'conv_bn dw')
        assert_close(bn_g.weight.grad, bn_r.weight.grad, 1e-3, 1e-4, 'conv_bn dgamma')
        assert_close(bn_g.running_mean, bn_r.running_mean, 1e-4, 1e-5, 'running_mean')
        assert_close(bn_g.running_var, bn_r.running_var, 1e-4, 1e-5, 'running_var')
    for a, b in zip(*outs):
        assert_close(a, b, 1e-4, 1e-5, 'epilogue statistics vs separate pass')


def test_conv_bn_epilogue_statistics_survive_a_large_mean():
    """Convolution outputs with |mean| / std ~ 2000: E[x^2] - mean^2 in fp32 would lose the variance entirely; the epilogue's
    shifted sums + Chan merges (and the double-precision block merge) keep it: batch variance within 1e-3 of the fp64 value,
    like the separate statistics pass."""
    import copy
    import torch.nn as nn
    from renderih_amd import ops, encoder
    d = dev()
    g = torch.Generator().manual_seed(11)
    x = 40.0 + 0.02 * torch.randn(2, 64, 16, 16, generator=g)
    cm = nn.Conv2d(64, 128, 1, bias=False)
    bn = nn.BatchNorm2d(128, momentum=1.0)           # running_var = this batch's (unbiased) variance
    with torch.no_grad():
        cm.weight.copy_((1.0 + 0.1 * torch.randn(128, 64, 1, 1, generator=g)) / 64.0)
    y64 = F.conv2d(x.double(), cm.weight.double())
    var64 = y64.var((0, 2, 3), unbiased=False).detach()
    assert float((y64.mean((0, 2, 3)).abs() / var64.sqrt()).min().detach()) > 500
    for use_stats in (True, False):
        cm_g, bn_g = copy.deepcopy(cm).to(d), copy.deepcopy(bn).to(d)
        old = ops.GEMM_STATS
        ops.GEMM_STATS = use_stats
        try:
            with torch.no_grad():
                encoder.conv_bn(cm_g, bn_g, nhwc(x).to(d))
        finally:
            ops.GEMM_STATS = old
        n = x.numel() // 64
        got_var = bn_g.running_var.cpu().double() * (n - 1) / n             # undo the unbiasing
        # (the fp32 convolution output itself carries ~1e-6 * 40 of round-off per element against a std of 2.5e-3)
        assert float(((got_var - var64).abs() / var64).max()) < 1e-2, (use_stats, float(((got_var - var64).abs() / var64).max()))


def _torch_attention_block(mods, x, heads, cross):
    """Plain-torch restatement (no dropout) of SelfAttn.forward_pair / the cross-hand half of inter_attn.forward_pair on the
    hands-stacked x [2, B, S, D] -- models/model_attn/self_attn.py:56-85, inter_attn.py:75-125."""
    def ln(m, t):
        return F.layer_norm(t, (t.shape[-1],), m.weight, m.bias, m.eps)

    def mha(q, k, v):
        B, S, D = q.shape
        d = D // heads
        sp = lambda t: t.view(B, -1, heads, d).transpose(1, 2)
        a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(d), -1)
        return (a @ sp(v)).transpose(1, 2).reshape(B, S, D)

    out = []
    if not cross:
        for h, m in enumerate(mods):
            y = ln(m.layer_norm, x[h])
            o = mha(F.linear(y, m.w_qs.weight, m.w_qs.bias), F.linear(y, m.w_ks.weight, m.w_ks.bias),
                    F.linear(y, m.w_vs.weight, m.w_vs.bias))
            x1 = x[h] + F.linear(o, m.fc.weight, m.fc.bias)
            y2 = ln(m.ff.layer_norm, x1)
            out.append(x1 + F.linear(F.relu(F.linear(y2, m.ff.fc1.weight, m.ff.fc1.bias)), m.ff.fc2.weight, m.ff.fc2.bias))
    else:
        m = mods
        y = [ln(m.layer_norm1, x[0]), ln(m.layer_norm2, x[1])]
        q = [F.linear(t, m.w_qs.weight, m.w_qs.bias) for t in y]
        k = [F.linear(t, m.w_ks.weight, m.w_ks.bias) for t in y]
        v = [F.linear(t, m.w_vs.weight, m.w_vs.bias) for t in y]
        feat = [mha(q[0], k[1], v[1]), mha(q[1], k[0], v[0])]
        for h, ff in enumerate((m.ffL, m.ffR)):
            x1 = x[h] + F.linear(feat[h], m.fc.weight, m.fc.bias)
            y2 = ln(ff.layer_norm, x1)
            out.append(x1 + F.linear(F.relu(F.linear(y2, ff.fc1.weight, ff.fc1.bias)), ff.fc2.weight, ff.fc2.bias))
    return torch.stack(out)

