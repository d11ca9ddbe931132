"""csrc/rih_conv3.hip rows_kernel, every tile and every epilogue, at shapes of a few workgroups.

rih_rows chooses its tile from the size of the grid (rows_tile(): a 256-row tile only with >= 256 workgroups), so no small shape
reaches rows_kernel<256, *> through it.  rih_rows_tiled (ABI 26, ops.rows_gemm(tile=...)) is the same launch on a tile the caller
names; these tests walk tile x epilogue x k-tile count x grid x pitches through it and compare every launch with an fp64
`A @ W^T (+ R)` (then ReLU) computed on the CPU from the same fp32 inputs, at the suite's bar (renderih_amd.testing.assert_close:
1e-4 |ref| + 1e-5 max|ref| for outputs and block means, 1e-3 / 1e-5 for the blocks' second moments, as test_rows_1x1).  The
statistics are compared block by block, before any merge: a partial in the wrong slot fails.

The helpers (check_rows_tile, check_refusals) also run on the host-compiled kernels (tests/test_kernels_on_cpu.py) and on the
emulated ABI (tests/test_cpu_emulated.py), which replace dev()."""
import ctypes as C
import functools
import math

import pytest
import torch

from renderih_amd.testing import assert_close

pytestmark = pytest.mark.gpu

RIH_EINVAL = -1
TILES = [(256, 128), (128, 128), (256, 64), (128, 64)]
EPILOGUES = ['plain', 'relu', 'stats', 'stats_relu', 'res', 'res_relu']
NAN_BITS = 0x7fc00abc       # a quiet NaN with a payload of our own


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _problem_uncached(M, N, K, for_dgrad):
    """fp32 inputs on the CPU and the fp64 product: (A [M][K], OIHW 1x1 weight, R [M][N], A @ W^T in fp64).  The weight is
    [N][K][1][1] for the forward form and [K][N][1][1] for the data-gradient form (W[n][k] = w[k][n])."""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + (7 if for_dgrad else 0))
    A = torch.randn(M, K, generator=g) * 2.0
    w = torch.randn((K, N, 1, 1) if for_dgrad else (N, K, 1, 1), generator=g) / math.sqrt(K)
    R = torch.randn(M, N, generator=g)
    Wnk = w[:, :, 0, 0].t() if for_dgrad else w[:, :, 0, 0]
    return A, w, R, A.double() @ Wnk.double().t()


_problem = functools.lru_cache(maxsize=None)(_problem_uncached)     # shared by the epilogues of a shape; nobody writes to it


def reference(lin, R, epi):
    y = lin + R.double() if epi.startswith('res') else lin
    return torch.relu(y) if epi.endswith('relu') else y


def check_block_statistics(holder, ref, bm, what):
    """holder.part[t] against the fp64 mean and centred sum of squares of rows [t bm/4, (t + 1) bm/4) of the reference."""
    M, N = ref.shape
    assert holder.part is not None, what
    assert holder.rows == bm // 4 and holder.T == M // holder.rows, (what, holder.rows, holder.T)
    part = holder.part.double().cpu()
    assert tuple(part.shape) == (holder.T, 2, N), (what, part.shape)
    blk = ref.reshape(holder.T, holder.rows, N)
    mean = blk.mean(1)
    m2 = ((blk - mean[:, None]) ** 2).sum(1)
    assert_close(part[:, 0], mean, 1e-4, 1e-5, what + ' block means')
    assert_close(part[:, 1], m2, 1e-3, 1e-5, what + ' block M2')


def launch(A, w, R, M, N, K, epi, for_dgrad, tile, pitched=False):
    """One ops.rows_gemm launch on dev().  Returns (C [M][N] on the CPU, StatsHolder or None, untouched: whether every float of C's
    buffer outside the [M][N] window -- padding columns and the rows behind -- still holds its NaN pattern)."""
    from renderih_amd import ops
    d = dev()
    lda, ldc, ldr = (K + 12, N + 4, N + 8) if pitched else (K, N, N)
    guard = 3                                           # rows of C's buffer behind the output
    a_buf = torch.full((M, lda), 1e30, dtype=torch.float32)
    a_buf[:, :K] = A
    r_buf = torch.full((M, ldr), 1e30, dtype=torch.float32)
    r_buf[:, :N] = R
    c_bits = torch.full((M + guard, ldc), NAN_BITS, dtype=torch.int32)
    a_buf, r_buf, c_buf = a_buf.to(d), r_buf.to(d), c_bits.view(torch.float32).to(d)
    a, c = a_buf[:, :K], c_buf[:M, :N]
    res = epi.startswith('res')
    wd = w.to(d)
    holder = ops.StatsHolder() if epi.startswith('stats') else None
    # the bound of A's values, not of its buffer: the padding holds 1e30
    ok = ops.rows_gemm(a, wd, c, M, N, K, lda, ldc, for_dgrad, relu=epi.endswith('relu'), stats=holder,
                       R=r_buf[:, :N] if res else None, ldr=ldr if res else 0, ba=ops.bound_of(A.to(d)), bw=ops.bound_of(wd), tile=tile)
    assert ok, 'the library refused the descriptor'
    out_bits = c_buf.cpu().view(torch.int32)
    outside = torch.ones(M + guard, ldc, dtype=torch.bool)
    outside[:M, :N] = False
    return c.cpu(), holder, bool((out_bits[outside] == NAN_BITS).all())


def check_rows_tile(tile, grid, K, epi, for_dgrad=False, pitched=False):
    """rows_kernel<bm, bn, epilogue of `epi`> on a grid of grid[0] x grid[1] workgroups with K / 32 k-tiles against fp64."""
    bm, bn = tile
    M, N = grid[0] * bm, grid[1] * bn
    what = 'rows %dx%d grid %dx%d K %d %s%s%s' % (bm, bn, grid[0], grid[1], K, epi, ' dgrad' if for_dgrad else '', ' pitched' if pitched else '')
    A, w, R, lin = _problem(M, N, K, for_dgrad)
    ref = reference(lin, R, epi)
    got, holder, untouched = launch(A, w, R, M, N, K, epi, for_dgrad, tile, pitched)
    assert untouched, what + ': wrote outside the [M][N] window of C'
    assert_close(got, ref, 1e-4, 1e-5, what)
    if holder is not None:
        check_block_statistics(holder, ref, bm, what)


def _desc(a, w_h2, c, M, N, K, r=None, stats=None):
    from renderih_amd._lib import PanelDesc
    pd = PanelDesc()
    pd.a, pd.w_h2, pd.c = a.data_ptr(), w_h2.data_ptr(), c.data_ptr()
    pd.amax_a = pd.amax_w = a.data_ptr()
    pd.r = r.data_ptr() if r is not None else None
    pd.stats = stats.data_ptr() if stats is not None else None
    pd.M, pd.N, pd.K, pd.lda, pd.ldc, pd.ldr, pd.relu = M, N, K, K, N, (N if r is not None else 0), 0
    return pd


def planned_tile(M, N, K):
    """What rih_rows_tile answers for a dense M x N x K descriptor (only the shape and the alignment are looked at)."""
    from renderih_amd import ops
    t = torch.zeros(64, device=dev())
    bm, bn = C.c_int(-1), C.c_int(-1)
    assert int(ops._L().rih_rows_tile(C.byref(_desc(t, t, t, M, N, K)), C.byref(bm), C.byref(bn))) == 1
    return bm.value, bn.value


def check_refusals():
    """rih_rows_tiled answers RIH_EINVAL -- before any launch -- for a tile that does not divide the problem, a tile that is none
    of the four, and statistics together with a residual; rih_rows_tile answers 0 and leaves its outputs alone for the last."""
    from renderih_amd import ops
    d, L = dev(), ops._L()
    M, N, K = 384, 256, 64
    # (operands of the right size all the same: a refusal that failed would then still launch inside them)
    a, wp, c = torch.zeros(M, K, device=d), torch.zeros(N, K, device=d), torch.zeros(2 * M, N, device=d)
    r, st = torch.zeros(M, N, device=d), torch.zeros(M // 32, 2, N, device=d)
    tiled = lambda pd, bm, bn: int(L.rih_rows_tiled(C.byref(pd), bm, bn, ops._stream()))
    pd = _desc(a, wp, c, M, N, K)
    assert int(L.rih_rows_ok(C.byref(pd))) == 1
    assert tiled(pd, 256, 128) == RIH_EINVAL            # M = 384 is not a multiple of 256
    assert tiled(pd, 256, 64) == RIH_EINVAL
    assert tiled(pd, 64, 64) == RIH_EINVAL              # bm = 64
    assert tiled(pd, 128, 32) == RIH_EINVAL and tiled(pd, 128, 256) == RIH_EINVAL and tiled(pd, 0, 0) == RIH_EINVAL
    pd = _desc(a, wp, c, M, 192, K)
    assert int(L.rih_rows_ok(C.byref(pd))) == 1
    assert tiled(pd, 128, 128) == RIH_EINVAL            # N = 192 is not a multiple of 128
    pd = _desc(a, wp, c, M, N, K, r=r, stats=st)
    assert int(L.rih_rows_ok(C.byref(pd))) == 0
    assert tiled(pd, 128, 128) == RIH_EINVAL            # statistics together with a residual
    bm, bn = C.c_int(-7), C.c_int(-9)
    assert int(L.rih_rows_tile(C.byref(pd), C.byref(bm), C.byref(bn))) == 0 and (bm.value, bn.value) == (-7, -9)
    assert not bool(c.any())                            # nothing ran


# ---------------------------------------------------------------------------------------------------------------- the GPU tests
def _tid(t):
    return '%dx%d' % t


@pytest.mark.parametrize('epi', EPILOGUES)
@pytest.mark.parametrize('K', [64, 96, 256])            # two k-tiles (the minimum), three (odd), eight
@pytest.mark.parametrize('tile', TILES, ids=_tid)
def test_tile_epilogue_trip_count(tile, K, epi):
    """Forward weight form, 3 x 2 = 6 workgroups (not a multiple of 8: the remainder branch of xcd_remap)."""
    check_rows_tile(tile, (3, 2), K, epi)


@pytest.mark.parametrize('epi', ['res', 'res_relu'])
@pytest.mark.parametrize('K', [64, 96, 256])
@pytest.mark.parametrize('tile', TILES, ids=_tid)
def test_tile_data_gradient_with_residual(tile, K, epi):
    """The data-gradient weight form (for_dgrad: n = ci, k = co) with the skip path's gradient as residual."""
    check_rows_tile(tile, (3, 2), K, epi, for_dgrad=True)


@pytest.mark.parametrize('epi', ['stats', 'res'])
@pytest.mark.parametrize('K', [160, 1056])              # five k-tiles; 33: odd and long
@pytest.mark.parametrize('tile', TILES, ids=_tid)
def test_tile_more_trip_counts(tile, K, epi):
    check_rows_tile(tile, (3, 2), K, epi)


@pytest.mark.parametrize('epi', ['stats', 'res'])
@pytest.mark.parametrize('grid', [(1, 1), (5, 2)], ids=_tid)    # a single workgroup; ten: q = 1, r = 2 in xcd_remap
@pytest.mark.parametrize('tile', TILES, ids=_tid)
def test_tile_more_grids(tile, grid, epi):
    check_rows_tile(tile, grid, 96, epi)


@pytest.mark.parametrize('tile', TILES, ids=_tid)
def test_tile_pitches(tile):
    """lda = K + 12, ldc = N + 4, ldr = N + 8 on views into larger buffers: A's and R's padding holds 1e30 (a read past the pitch
    shows in the result), C's padding columns and the rows behind C hold a NaN pattern that must survive bit for bit."""
    check_rows_tile(tile, (3, 2), 96, 'res', pitched=True)


# the smallest shapes at which rih_rows itself takes each tile (>= 256 workgroups), K = 96
PLANNER_CASES = [(8192, 1024, (256, 128), 'stats'), (16512, 256, (128, 128), 'res'), (22016, 192, (256, 64), 'stats_relu'),
                 (11136, 192, (128, 64), 'res_relu')]


@pytest.mark.parametrize('M,N,tile,epi', PLANNER_CASES, ids=lambda v: _tid(v) if isinstance(v, tuple) else str(v))
def test_planner_choice_is_the_forced_tile(M, N, tile, epi):
    """rih_rows_tile answers the tile of the table; rih_rows meets the fp64 bar and is bit-identical to rih_rows_tiled on that tile
    (the same instantiation on the same grid: equality follows from determinism)."""
    K = 96
    assert planned_tile(M, N, K) == tile
    A, w, R, lin = _problem_uncached(M, N, K, False)
    ref = reference(lin, R, epi)
    what = 'rih_rows %d x %d x %d %s' % (M, N, K, epi)
    own, h_own, _ = launch(A, w, R, M, N, K, epi, False, None)
    assert_close(own, ref, 1e-4, 1e-5, what)
    forced, h_forced, _ = launch(A, w, R, M, N, K, epi, False, tile)
    assert torch.equal(own, forced), what + ': rih_rows differs from rih_rows_tiled on its own tile'
    if h_own is not None:
        check_block_statistics(h_own, ref, tile[0], what)
        assert torch.equal(h_own.part, h_forced.part)


def test_tiled_refusals():
    check_refusals()
