"""Engine 2 (csrc/rih_e2.h: fp32 from three fp16 MFMA products of a scaled two-term split) away from unit scale, kernel family by
kernel family.  Part B runs the parity bodies of tests/test_gpu_ops.py with their activations, weights and upstream gradients
multiplied by the magnitudes of the project's descriptor fuzz: the scale clamp of e2_scale, `at_least_one` of the weight
gradient's all-ones row and the order in which RIH_E2_STAGE undoes the two operand scales only act there.  Part C gives one
operand an in-tensor spread -- one hot pixel row at 2^13, every seventh at 2^-10, output channels at 1 or 2^-8 -- so that most
rows live far down the fp16 planes, and checks every output row at ITS OWN magnitude.  The assertions are the suite's bar against
fp64, |a - b| <= 1e-4 |b| + 1e-5 max|b|, which is scale invariant; every measured error is printed before it is asserted."""
import math
import pytest
import torch
import torch.nn.functional as F

import test_gpu_ops as G
from renderih_amd.testing import assert_close, rel_err

pytestmark = pytest.mark.gpu

# (activations, weights, upstream gradients): tests/test_kernels_on_cpu.py, test_gemm_descriptor_fuzz_against_emulator -- no fp32
# product of them is denormal or overflows
MAGNITUDES = [(1e-6, 1e-9, 1e-6), (1e7, 2e5, 1e4), (3e4, 1e-3, 1.0), (1.0, 1.0, 1e-6)]


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _grouped(monkeypatch, **k):
    G.test_grouped_weight_gradients_on_128x64_tiles(monkeypatch, **k)
    G.test_grouped_weight_gradients(2, **k)


# the smallest case of each family that the host harness runs too
FAMILIES = {
    'halo': lambda mp, **k: G.test_conv3x3_halo((1, 8, 32, 32, 64, False, True), **k),
    'halo_residual': lambda mp, **k: G.test_conv3x3_halo_with_skip_gradient((1, 8, 32, 32, 32), **k),
    'panel': lambda mp, **k: G.test_panel_1x1((1, 16, 16, 64, 256, False, True), **k),
    'rows': lambda mp, **k: G.test_rows_1x1((1, 16, 8, 96, 128, True, True), **k),
    'stem': lambda mp, **k: G.test_stem_conv((2, 32, 32, True, True), **k),
    'segmented_a': lambda mp, **k: G.test_conv1x1_cat((3, 9, 7, (32, 64), 40, False), 2, **k),
    'gemm': lambda mp, **k: G.test_conv2d((3, 17, 15, 32, 48, 3, 1, 1, False, True), **k),
    'gemm_strided': lambda mp, **k: G.test_conv2d((2, 15, 17, 64, 96, 3, 2, 1, False, False), **k),
    'grouped_wgrad': _grouped,
}


def run_family(family, mag, monkeypatch):
    from renderih_amd import ops
    monkeypatch.setattr(ops, 'ENGINE', 2)
    real = G.assert_close

    def measured(a, b, rtol=1e-4, atol_frac=1e-5, what=''):
        print('e2_range %s xs=%g ws=%g gs=%g | %s | rtol %g atol %g | max err / max|ref| = %.3g'
              % ((family,) + tuple(mag) + (what, rtol, atol_frac, rel_err(a, b))))
        return real(a, b, rtol, atol_frac, what)
    monkeypatch.setattr(G, 'assert_close', measured)
    xs, ws, gs = mag
    FAMILIES[family](monkeypatch, xs=xs, ws=ws, gs=gs)


@pytest.mark.parametrize('mag', MAGNITUDES, ids=lambda m: '%g_%g_%g' % m)
@pytest.mark.parametrize('family', sorted(FAMILIES))
def test_family_off_unit_scale(family, mag, monkeypatch):
    run_family(family, mag, monkeypatch)


# ------------------------------------------------------------------------------------------------ C: one hot row
def row_scales(M, shift=0):
    """Powers of two per pixel row: 1, every seventh 2^-10, one (not a seventh) 2^13; `shift` rotates the pattern."""
    r = torch.ones(M)
    r[::7] = 2.0 ** -10
    hot = M // 2 + (1 if (M // 2) % 7 == 0 else 0)
    r[hot] = 2.0 ** 13
    return torch.roll(r, shift)


def col_scales(N):
    c = torch.ones(N)
    c[1::3] = 2.0 ** -8
    return c


def neighbourhood(r, N, H, W, k):
    """The magnitude of a k x k convolution's output row: the largest row scale under its window (r itself for k = 1)."""
    if k == 1:
        return r
    return F.max_pool2d(r.view(N, 1, H, W), k, 1, k // 2).reshape(-1)


def close_per_row(got, ref, rows, cols, what):
    """got, ref [M, n]: both divided exactly (powers of two) by the row's and the column's scale, then the suite's bar."""
    div = rows.double()[:, None] * (cols.double()[None, :] if cols is not None else 1.0)
    a, b = got.double().cpu() / div, ref.double().cpu() / div
    print('e2_range hot row | %s | max err / max|ref| per row scale = %.3g' % (what, rel_err(a, b)))
    assert_close(a, b, 1e-4, 1e-5, what)


def merged_stats(holder, M):
    part = holder.part.double().cpu()
    n = torch.full((holder.T,), float(holder.rows), dtype=torch.float64)
    n[-1] = M - holder.rows * (holder.T - 1)
    mean = (part[:, 0] * n[:, None]).sum(0) / M
    var = (part[:, 1] + n[:, None] * (part[:, 0] - mean) ** 2).sum(0) / M
    return mean, var


def hot_data(N, H, W, Cin, Cout, k, seed):
    """x [N, H, W, Cin] with row scales, w [Cout, Cin, k, k] with output-channel scales, gy [N, H, W, Cout] with the rotated row
    scales, and the fp64 results of the stride-1 convolution: y, dx, dw as [M, .] / weight-shaped tensors."""
    M = N * H * W
    g = torch.Generator().manual_seed(seed)
    r, rg, c = row_scales(M), row_scales(M, 5), col_scales(Cout)
    x = torch.randn(M, Cin, generator=g) * r[:, None]
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k) * c[:, None, None, None]
    gy = torch.randn(M, Cout, generator=g) * rg[:, None]
    xr = G.nchw(x.view(N, H, W, Cin)).double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    yr = F.conv2d(xr, wr, padding=k // 2)
    yr.backward(G.nchw(gy.view(N, H, W, Cout)).double())
    ref = (G.nhwc(yr.detach()).reshape(M, Cout), G.nhwc(xr.grad).reshape(M, Cin), wr.grad)
    return x.view(N, H, W, Cin), w, gy.view(N, H, W, Cout), neighbourhood(r, N, H, W, k), neighbourhood(rg, N, H, W, k), c, ref


def check_hot_conv(name, y, dx, dw, holder, ro, rgo, c, ref):
    M = ro.numel()
    yr, dxr, dwr = ref
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dw).all()), name
    close_per_row(y.reshape(M, -1), yr, ro, c, name + ' y')
    close_per_row(dx.reshape(M, -1), dxr, rgo, None, name + ' dx')
    print('e2_range hot row | %s dw | max err / max|ref| = %.3g' % (name, rel_err(dw, dwr)))
    assert_close(dw, dwr, 1e-4, 1e-5, name + ' dw')
    if holder is not None:
        assert holder.part is not None, name + ': no statistics epilogue'
        mean, var = merged_stats(holder, M)
        assert_close(mean, yr.mean(0), 1e-4, 1e-5, name + ' stats mean')
        assert_close(var, yr.var(0, unbiased=False), 1e-3, 1e-5, name + ' stats var')


def hot_halo():
    from renderih_amd import ops
    N, H, W, Cin, Cout = 1, 8, 32, 32, 64
    x, w, gy, ro, rgo, c, ref = hot_data(N, H, W, Cin, Cout, 3, 101)
    saved = (ops.ENGINE, ops.HALO3, ops.conv3x3_halo)
    ops.ENGINE, ops.HALO3 = 2, True
    taken, real = [], ops.conv3x3_halo
    ops.conv3x3_halo = lambda *a, **k: (taken.append(real(*a, **k)), taken[-1])[1]
    try:
        d = dev()
        xg, wg = x.to(d).requires_grad_(True), w.clone().to(d).requires_grad_(True)
        holder = ops.StatsHolder()
        y = ops.conv2d(xg, wg, None, stride=1, pad=1, stats=holder)
        y.backward(gy.to(d))
        assert taken == [True, True], taken             # forward and data gradient on the halo kernel
        check_hot_conv('halo', y.detach().cpu(), xg.grad.cpu(), wg.grad.cpu(), holder, ro, rgo, c, ref)
    finally:
        ops.ENGINE, ops.HALO3, ops.conv3x3_halo = saved


def hot_1x1(name):
    """panel: (1, 16, 16, 64, 64) with the fill-the-chip rule lifted; rows: (1, 16, 16, 128, 128), thresholds lifted, panel off --
    the settings of G.test_panel_1x1 / G.test_rows_1x1, at shapes whose data gradient (K = Cout, N = Cin) the kernel takes too."""
    from renderih_amd import ops
    N, H, W, Cin, Cout = (1, 16, 16, 64, 64) if name == 'panel' else (1, 16, 16, 128, 128)
    x, w, gy, ro, rgo, c, ref = hot_data(N, H, W, Cin, Cout, 1, 102)
    names = ('ENGINE', 'PANEL', '_panel_ok', 'panel_gemm', 'ROWS', 'rows_gemm', 'ROWS_MINK', 'ROWS_MIN_WGS', 'ROWS_MIN_M', 'ROWS_MIN_N')
    saved = [getattr(ops, n) for n in names]
    taken = []
    real = ops.panel_gemm if name == 'panel' else ops.rows_gemm
    spy = lambda *a, **k: (taken.append((bool(a[8]), bool(real(*a, **k)))), taken[-1][1])[1]      # (for_dgrad, taken)
    ops.ENGINE = 2
    if name == 'panel':
        ops.PANEL, ops.panel_gemm = True, spy
        ops._panel_ok = lambda rows, K, Nn, lda, a, bias=None: (bias is None and K in (64, 128) and Nn % 64 == 0
                                                                and not (K == 128 and Nn % 128 != 0) and rows % 128 == 0 and lda % 4 == 0)
    else:
        ops.PANEL, ops.ROWS, ops.rows_gemm = False, True, spy
        ops.ROWS_MINK, ops.ROWS_MIN_WGS, ops.ROWS_MIN_M, ops.ROWS_MIN_N = 64, 1, 1, 64
    try:
        d = dev()
        xg, wg = x.to(d).requires_grad_(True), w.clone().to(d).requires_grad_(True)
        holder = ops.StatsHolder()
        y = ops.conv2d(xg, wg, None, stride=1, pad=0, stats=holder)
        y.backward(gy.to(d))
        assert taken == [(False, True), (True, True)], (name, taken)    # forward and data gradient ran on the kernel under test
        check_hot_conv(name, y.detach().cpu(), xg.grad.cpu(), wg.grad.cpu(), holder, ro, rgo, c, ref)
    finally:
        for n, v in zip(names, saved):
            setattr(ops, n, v)


def hot_segmented_a():
    from renderih_amd import ops
    N, H, W, Cs, Cout = 3, 9, 7, (32, 64), 40
    x, w, gy, ro, rgo, c, ref = hot_data(N, H, W, sum(Cs), Cout, 1, 103)
    saved = ops.ENGINE
    ops.ENGINE = 2
    L = ops._L()
    real = L.rih_gemm
    ran = []            # (engine, pieces of a segmented A operand) of every rih_gemm launch
    L.rih_gemm = lambda dref, s: (ran.append((int(L.rih_gemm_engine(dref)), sum(1 for p in dref._obj.a_seg if p))), real(dref, s))[1]
    try:
        d = dev()
        parts = [t.contiguous().to(d).requires_grad_(True) for t in torch.split(x, Cs, dim=-1)]
        wg = w.clone().to(d).requires_grad_(True)
        holder = ops.StatsHolder()
        y = ops.conv1x1_cat(parts, wg, relu=False, stats=holder)
        assert ran == [(2, len(Cs) - 1)], ran           # one forward launch, engine 2, A read piece by piece
        y.backward(gy.to(d))
        assert ran[1:1 + len(Cs)] == [(2, 0)] * len(Cs), ran        # one data-gradient launch per part, engine 2 (then the weight gradients)
        dx = torch.cat([p.grad.cpu() for p in parts], dim=-1)
        check_hot_conv('segmented A', y.detach().cpu(), dx, wg.grad.cpu(), holder, ro, rgo, c, ref)
    finally:
        ops.ENGINE = saved
        L.rih_gemm = real


def hot_gemm_tile(tile):
    """rih_gemm's split kernels on a named tile (0: 128 x 128, 1: 128 x 64, 2: 64 x 64), engine 2, ragged M and N: forward
    (B = w [N][K]), data gradient (B = w as [K'][N']) and weight gradient (transposed-gather A) of a 1x1 convolution."""
    import ctypes as C
    from renderih_amd import ops
    M, K, Nn = 200, 96, 72
    x, w, gy, ro, rgo, c, ref = hot_data(1, 1, M, K, Nn, 1, 104 + tile)
    L = ops._L()
    real = L.rih_gemm
    ran = []
    L.rih_gemm = lambda dref, s: (ran.append((int(L.rih_gemm_engine(dref)), int(dref._obj.tile))), real(dref, s))[1]
    try:
        d = dev()
        xg, wg, gg = x.reshape(M, K).to(d), w.reshape(Nn, K).to(d), gy.reshape(M, Nn).to(d)
        bx, bw, bg = ops.bound_of(xg), ops.bound_of(wg), ops.bound_of(gg)
        y, dx, dwt = torch.empty(M, Nn, device=d), torch.empty(M, K, device=d), torch.empty(K, Nn, device=d)
        ops.gemm(xg, wg, y, M, Nn, K, K, K, Nn, a_mode=0, b_mode=1, tile=tile, engine=2, amax_a=bx, amax_b=bw)
        ops.gemm(gg, wg, dx, M, K, Nn, Nn, K, K, a_mode=0, b_mode=0, tile=tile, engine=2, amax_a=bg, amax_b=bw)
        ops.gemm(xg, gg, dwt, K, Nn, M, K, Nn, Nn, a_mode=1, b_mode=0, tile=tile, engine=2, amax_a=bx, amax_b=bg)
        assert ran == [(2, tile)] * 3, ran
        check_hot_conv('rih_gemm tile %d' % tile, y.cpu(), dx.cpu(), dwt.cpu().t().reshape(Nn, K, 1, 1), None, ro, rgo, c, ref)
    finally:
        L.rih_gemm = real


HOT = {'halo': hot_halo, 'panel': lambda: hot_1x1('panel'), 'rows': lambda: hot_1x1('rows'), 'segmented_a': hot_segmented_a,
       'gemm_tile0': lambda: hot_gemm_tile(0), 'gemm_tile1': lambda: hot_gemm_tile(1), 'gemm_tile2': lambda: hot_gemm_tile(2)}


@pytest.mark.parametrize('family', sorted(HOT))
def test_one_hot_row(family):
    HOT[family]()
