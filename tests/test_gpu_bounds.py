"""The producers of engine 2's operand bounds (csrc/rih_e2.h: e2_scale reads one bound block per operand; any upper bound is
right, one that is too small overflows the fp16 planes): rih_absmax, rih_absmax_multi, the `amax` outputs of rih_bn_apply /
rih_bn_bwd and ops.inherit_bound -- every bound against max|t| of the tensor it describes, BIT FOR BIT (a maximum rounds
nothing, so there is no tolerance), and two producer -> consumer chains against fp64 at the suite's bar."""
import math
import pytest
import torch
import torch.nn.functional as F

from renderih_amd.testing import assert_close

pytestmark = pytest.mark.gpu

BF = 2048                   # floats of a bound block: 64 slot words, one per 128-byte line
SENTINEL = -3.0             # what the 31 other words of every line hold before a launch
EINVAL = -1


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def bound(block):
    return block.view(64, 32)[:, 0].max().cpu()


def new_blocks(n=1):
    """n bound blocks: slot words zero, every other word a sentinel."""
    b = torch.full((n, 64, 32), SENTINEL)
    b[:, :, 0] = 0.0
    return b.reshape(n, BF).to(dev())


def assert_rest_untouched(blocks, what=''):
    rest = blocks.view(-1, 64, 32)[:, :, 1:].cpu()
    assert bool((rest == SENTINEL).all()), 'words outside the 64 slots were written ' + str(what)


def absmax(t, block):
    from renderih_amd import ops
    assert t.is_contiguous() and block.is_contiguous()
    return int(ops._L().rih_absmax(t.data_ptr(), t.numel(), block.data_ptr(), ops._stream()))


# n: 1, 3 (scalar tail only), 4 (one float4), 5 (float4 + tail), 1023, 4097 (a second workgroup, n % 4 = 1), 16*256*64 + 7 (65
# workgroups: the slots wrap), 16*256*300 (slots wrap four times)
ABSMAX_N = [1, 3, 4, 5, 1023, 4097, 16 * 256 * 64 + 7, 16 * 256 * 300]


def check_absmax_n(n):
    """The single largest magnitude at element 0, at element n - 1 (the scalar tail when n % 4 != 0) and in the middle with a
    negative sign -- through a 16-byte-aligned pointer (float4 path) and through one offset by one float (scalar path)."""
    g = torch.Generator().manual_seed(n)
    base = (torch.rand(n + 1, generator=g) * 2 - 1)          # |.| < 1
    buf = base.to(dev())
    for off in (0, 1):
        t = buf[off:off + n]
        assert (t.data_ptr() % 16 == 0) == (off == 0)
        for pos, peak in ((0, 5.5), (n - 1, 6.25), (n // 2, -7.125)):
            keep = t[pos].clone()
            t[pos] = peak
            blk = new_blocks()
            assert absmax(t, blk[0]) == 0
            want = t.cpu().abs().max()
            assert float(want) == abs(peak)
            assert torch.equal(bound(blk[0]), want), ('rih_absmax', n, off, pos, float(bound(blk[0])), float(want))
            assert_rest_untouched(blk, ('rih_absmax', n, off, pos))
            t[pos] = keep


@pytest.mark.parametrize('n', ABSMAX_N)
def test_absmax_equals_the_maximum(n):
    check_absmax_n(n)


def test_absmax_zero_nan_and_merge():
    """An all-zero tensor leaves the block all zero; NaNs are ignored (in a float4 with the maximum, in the tail, an all-NaN
    tensor); a block that already holds a larger value keeps it, a smaller one is raised."""
    d = dev()
    blk = new_blocks()
    assert absmax(torch.zeros(4099, device=d), blk[0]) == 0
    assert bool((blk.view(64, 32)[:, 0].cpu() == 0).all())
    assert_rest_untouched(blk, 'zeros')
    for off in (0, 1):
        x = torch.rand(4104) * 2 - 1
        x[8], x[9], x[10] = float('nan'), -3.5, float('nan')
        x[4095 + off], x[4096 + off] = float('nan'), float('nan')           # the last element of the tensor read below
        t = x.to(d)[off:off + 4097]
        blk = new_blocks()
        assert absmax(t, blk[0]) == 0
        tc = t.cpu()
        want = tc[~tc.isnan()].abs().max()
        assert float(want) == 3.5 and torch.equal(bound(blk[0]), want), ('NaN ignored', off, float(bound(blk[0])))
    blk = new_blocks()
    assert absmax(torch.full((37,), float('nan'), device=d), blk[0]) == 0
    assert bool((blk.view(64, 32)[:, 0].cpu() == 0).all()), 'an all-NaN tensor must leave the block alone'
    # merge, not overwrite: 70 workgroups, so every slot is visited
    t = (torch.rand(16 * 256 * 70) * 2 - 1).to(d)
    t[12345] = -2.5
    for held, want in ((9.75, 9.75), (0.5, 2.5)):
        blk = new_blocks()
        v = blk.view(64, 32)
        v[:, 0] = held
        assert absmax(t, blk[0]) == 0
        assert float(bound(blk[0])) == want, (held, float(bound(blk[0])))
        assert bool((v[:, 0].cpu() >= held).all()), 'a slot lost the value it held'
        assert_rest_untouched(blk, 'merge')


MULTI_SIZES = [1, 2, 3, 4, 5, 7, 64, 255, 1023, 4097, 9001]
MULTI_BIG = 256 * 16 * 256 + 4099       # more blocks than the 256-block cap: the grid stride covers the rest


def check_absmax_multi(count, with_big):
    """`count` tensors of ragged sizes at ragged alignments inside one buffer, each with its own maximum (at the first, the last
    or a middle element, either sign): every block receives its own tensor's maximum, and a spare block none."""
    from renderih_amd import ops
    from renderih_amd._lib import AbsmaxDesc
    sizes = [MULTI_SIZES[(5 * i + i // 11) % len(MULTI_SIZES)] for i in range(count)]
    if with_big:
        sizes[count // 2] = MULTI_BIG
    offs, total = [], 0
    for i, n in enumerate(sizes):
        total += i % 3                  # a gap of 0 / 1 / 2 floats: aligned and unaligned starts
        offs.append(total)
        total += n
    g = torch.Generator().manual_seed(count)
    buf = torch.rand(total + 8, generator=g) * 2 - 1
    peaks = []
    for i, (o, n) in enumerate(zip(offs, sizes)):
        peak = (2.0 + i / 256.0) * (-1.0 if i % 2 else 1.0)
        pos = (n - 1, 0, n // 2)[i % 3] if n != MULTI_BIG else n - 1
        buf[o + pos] = peak
        peaks.append(abs(peak))
    bufd = buf.to(dev())
    blks = new_blocks(count + 1)
    arr = (AbsmaxDesc * count)()
    for i, (a, o, n) in enumerate(zip(arr, offs, sizes)):
        a.x, a.out, a.n = bufd.data_ptr() + 4 * o, blks[i].data_ptr(), n
    assert int(ops._L().rih_absmax_multi(arr, count, ops._stream())) == 0
    got = blks.view(count + 1, 64, 32)[:, :, 0].max(1).values.cpu()
    want = torch.stack([buf[o:o + n].abs().max() for o, n in zip(offs, sizes)])
    assert want.tolist() == peaks
    bad = [(i, sizes[i], float(got[i]), float(want[i])) for i in range(count) if got[i] != want[i]]
    assert not bad, ('rih_absmax_multi', count, bad[:8])
    assert float(got[count]) == 0.0, 'a block of no tensor was written'
    assert_rest_untouched(blks, ('rih_absmax_multi', count))


@pytest.mark.parametrize('count,with_big', [(1, True), (119, False), (120, False), (121, True), (241, False)])
def test_absmax_multi_gives_every_tensor_its_own_maximum(count, with_big):
    check_absmax_multi(count, with_big)


def test_absmax_multi_refuses_empty_and_null():
    from renderih_amd import ops
    from renderih_amd._lib import AbsmaxDesc
    L = ops._L()
    x = torch.ones(8, device=dev())
    blks = new_blocks(3)
    for bad in ('n', 'x', 'out'):
        arr = (AbsmaxDesc * 3)()
        for i, a in enumerate(arr):
            a.x, a.out, a.n = x.data_ptr(), blks[i].data_ptr(), 8
        if bad == 'n':
            arr[1].n = 0
        elif bad == 'x':
            arr[2].x = None
        else:
            arr[0].out = None
        assert int(L.rih_absmax_multi(arr, 3, ops._stream())) == EINVAL, bad
    assert float(blks.view(3, 64, 32)[:, :, 0].max().cpu()) == 0.0, 'a refused list must not be run in part'
    assert int(L.rih_absmax_multi(None, 1, ops._stream())) == EINVAL


# ------------------------------------------------------------------------------------------------ BatchNorm kernels
BN_SHAPES = [(3, 7, 9, 256), (2, 4, 4, 2048), (1, 5, 1, 4)]


def bn_forward(x, gamma, beta, rm, rv, res, training, relu, want_mask=True):
    """rih_bn_stats / rih_bn_eval_stats + rih_bn_apply as BatchNormFn.forward calls them; x [rows, C] on the device."""
    from renderih_amd import ops
    L, s = ops._L(), ops._stream()
    rows, Cc = x.shape
    d = x.device
    mean, invstd = torch.empty(Cc, device=d), torch.empty(Cc, device=d)
    ws = torch.empty(int(L.rih_bn_ws_floats(rows, Cc)), device=d)
    if training:
        assert int(L.rih_bn_stats(x.data_ptr(), rows, Cc, 1e-5, 0.1, mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(),
                                  rv.data_ptr(), ws.data_ptr(), s)) == 0
    else:
        assert int(L.rih_bn_eval_stats(rm.data_ptr(), rv.data_ptr(), Cc, 1e-5, mean.data_ptr(), invstd.data_ptr(), s)) == 0
    y = torch.empty_like(x)
    mask = torch.empty(x.numel() // 4, device=d, dtype=torch.uint8) if (relu and want_mask) else None
    blk = new_blocks()
    assert int(L.rih_bn_apply(x.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                              ops._p(res), y.data_ptr(), rows, Cc, 1 if relu else 0, ops._p(mask), blk[0].data_ptr(), s)) == 0
    return y, mask, mean, invstd, blk


def bn_data(shape, res, outlier):
    """x ~ 2 randn + 0.5, gamma in [0.5, 1.5) but 8 on the last channel.  outlier: the last element of x is far out, so that the
    largest output is the last one; otherwise the last row is the mean of the others (x-hat = 0 there, so that a large dy in the last
    row gives the largest dx)."""
    N, H, W, Cc = shape
    rows = N * H * W
    g = torch.Generator().manual_seed(rows + Cc)
    x = torch.randn(rows, Cc, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    rm, rv = torch.randn(Cc, generator=g) * 0.1 + 0.5, torch.rand(Cc, generator=g) + 3.5
    r = torch.randn(rows, Cc, generator=g) if res else None
    gamma[-1] = 8.0
    if outlier:
        x[-1, -1], beta[-1] = 50.0, 1.0
    else:
        x[:, -1] = x[:, -1].abs() + 0.1         # (positive: the input_relu flag of the backward gates dx by x > 0)
        x[-1, :], beta[-1] = x[:-1].mean(0), 2.0
    if res:
        r[-1, -1] = 3.0
    return x, gamma, beta, rm, rv, r


def check_bn_apply_bound(shape, training, relu, res):
    d = dev()
    x, gamma, beta, rm, rv, r = (t.to(d) if t is not None else None for t in bn_data(shape, res, True))
    y, _, _, _, blk = bn_forward(x, gamma, beta, rm, rv, r, training, relu)
    yc = y.cpu()
    what = ('rih_bn_apply', shape, training, relu, res)
    assert bool(torch.isfinite(yc).all()), what
    assert int(yc.abs().flatten().argmax()) >= yc.numel() - 4, ('the largest output is not in the last quad', what)
    assert torch.equal(bound(blk[0]), yc.abs().max()), (what, float(bound(blk[0])), float(yc.abs().max()))
    assert_rest_untouched(blk, what)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('relu,res', [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize('shape', BN_SHAPES)
def test_bn_apply_bound_is_max_abs_y(shape, relu, res, training):
    check_bn_apply_bound(shape, training, relu, res)


@pytest.mark.parametrize('relu', [False, True])
def test_bn_apply_bound_with_a_negative_peak(relu):
    """The largest pre-activation magnitude is negative.  Without ReLU the bound is that magnitude (the kernel must take |y|);
    with ReLU it is the maximum of the post-ReLU y, far below it."""
    d = dev()
    shape = (3, 7, 9, 256)
    x, gamma, beta, rm, rv, _ = bn_data(shape, False, False)
    gamma[-1], gamma[17] = 1.0, 1.5
    x[5, 17] = -90.0
    pre = (x.double() - rm.double()) / (rv.double() + 1e-5).sqrt() * gamma.double() + beta.double()
    assert float(-pre.min()) > 4 * float(pre.max())
    x, gamma, beta, rm, rv = (t.to(d) for t in (x, gamma, beta, rm, rv))
    y, _, _, _, blk = bn_forward(x, gamma, beta, rm, rv, None, False, relu)
    yc = y.cpu()
    assert torch.equal(bound(blk[0]), yc.abs().max()), (relu, float(bound(blk[0])), float(yc.abs().max()))
    assert (float(yc.abs().max()) > 30.0) == (not relu)


def bwd_inputs(shape, training, relu, res, use_mask, d):
    """What a forward pass leaves for the backward."""
    x, gamma, beta, rm, rv, r = (t.to(d) if t is not None else None for t in bn_data(shape, res, False))
    y, mask, mean, invstd, _ = bn_forward(x, gamma, beta, rm, rv, r, training, relu, want_mask=use_mask)
    return x, gamma, y, mask, mean, invstd


def check_bn_bwd_bound(shape, flags, relu, res, use_mask):
    """rih_bn_bwd as BatchNormFn.backward calls it (relu_mask) and with the y fall-back: bound == max|dx|, the largest dx in the
    last quad.  flags: bit 0 = frozen statistics, bit 1 = the input is a ReLU output."""
    from renderih_amd import ops
    L, s = ops._L(), ops._stream()
    d = dev()
    x, gamma, y, mask, mean, invstd = bwd_inputs(shape, not (flags & 1), relu, res, use_mask, d)
    rows, Cc = x.shape
    g = torch.Generator().manual_seed(7 + flags)
    dy = torch.randn(rows, Cc, generator=g)
    dy[-1, -1] = 100.0
    dy = dy.to(d)
    dx, dres = torch.empty_like(x), (torch.empty_like(x) if res else None)
    dg, db = torch.empty(Cc, device=d), torch.empty(Cc, device=d)
    ws = torch.empty(int(L.rih_bn_ws_floats(rows, Cc)), device=d)
    blk = new_blocks()
    assert int(L.rih_bn_bwd(dy.data_ptr(), x.data_ptr(), (0 if (use_mask or not relu) else y.data_ptr()), mean.data_ptr(),
                            invstd.data_ptr(), gamma.data_ptr(), dx.data_ptr(), ops._p(dres), dg.data_ptr(), db.data_ptr(), rows,
                            Cc, 1 if relu else 0, flags, ws.data_ptr(), ops._p(mask), blk[0].data_ptr(), s)) == 0
    dxc = dx.cpu()
    what = ('rih_bn_bwd', shape, flags, relu, res, use_mask)
    assert bool(torch.isfinite(dxc).all()), what
    assert int(dxc.abs().flatten().argmax()) >= dxc.numel() - 4, ('the largest dx is not in the last quad', what)
    assert torch.equal(bound(blk[0]), dxc.abs().max()), (what, float(bound(blk[0])), float(dxc.abs().max()))
    assert_rest_untouched(blk, what)
    if res:             # dres = the (gated) dy: it has its own, different maximum, which the block must not have taken
        assert float(dres.cpu().abs().max()) != float(dxc.abs().max())


@pytest.mark.parametrize('flags', [0, 1, 2, 3])
@pytest.mark.parametrize('relu,res,use_mask', [(False, False, True), (True, False, True), (True, True, True), (True, False, False),
                                               (False, True, True), (True, True, False)])
@pytest.mark.parametrize('shape', BN_SHAPES)
def test_bn_bwd_bound_is_max_abs_dx(shape, relu, res, use_mask, flags):
    check_bn_bwd_bound(shape, flags, relu, res, use_mask)


# ------------------------------------------------------------------------------------------------ ops layer
def test_ops_batchnorm_leaves_the_kernels_bound_on_y_and_dx():
    """ops.batchnorm: cached_bound(y) is the block rih_bn_apply wrote (== max|y|); an in-place change torch can see makes bound_of
    measure again; in the backward dx carries max|dx| and dres carries no bound."""
    from renderih_amd import ops
    d = dev()
    saved = ops.ENGINE
    ops.ENGINE = 2
    try:
        x, gamma, beta, rm, rv, r = (t.to(d) for t in bn_data((3, 7, 9, 256), True, True))
        x = x.view(3, 7, 9, 256).requires_grad_(True)
        r = r.view(3, 7, 9, 256).requires_grad_(True)
        xin, rin = x * 1.0, r * 1.0                 # non-leaf: their hooks see the tensors BatchNormFn.backward returns
        seen = {}
        xin.register_hook(lambda g_: seen.__setitem__('dx', (g_, ops.cached_bound(g_))))
        rin.register_hook(lambda g_: seen.__setitem__('dres', (g_, ops.cached_bound(g_))))
        y = ops.batchnorm(xin, gamma, beta, rm, rv, residual=rin, training=True, relu=True)
        blk = ops.cached_bound(y)
        assert blk is not None and blk.numel() == BF
        assert ops.bound_of(y) is blk
        assert torch.equal(bound(blk), y.detach().cpu().abs().max())
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(3)).to(d)
        y.backward(gy)
        dx, bdx = seen['dx']
        assert bdx is not None and torch.equal(bound(bdx), dx.cpu().abs().max())
        assert seen['dres'][1] is None, 'dres carries a bound'
        with torch.no_grad():
            y.mul_(-2.5)
        assert ops.cached_bound(y) is None
        blk2 = ops.bound_of(y)
        assert blk2 is not blk and torch.equal(bound(blk2), y.detach().cpu().abs().max())
    finally:
        ops.ENGINE = saved


def test_inherited_bounds():
    """ops.cat_channels / maxpool3x3s2 / upsample_bilinear: the inherited bound is >= max|y| and equals the largest input bound
    (selections) or that bound times 1 + 2^-20 (the bilinear samples, which round); a part without a bound leaves y without
    one."""
    from renderih_amd import ops
    d = dev()
    saved = ops.ENGINE
    ops.ENGINE = 2
    try:
        g = torch.Generator().manual_seed(5)
        parts = [(torch.randn(2, 9, 7, c, generator=g) * s_).to(d) for c, s_ in ((32, 1.0), (64, 40.0), (32, 0.01))]
        parts[1][1, 8, 6, 63] = -4321.5
        bs = [ops.bound_of(p) for p in parts]
        for p, b in zip(parts, bs):
            assert torch.equal(bound(b), p.cpu().abs().max())
        big = max(float(bound(b)) for b in bs)
        assert big == 4321.5
        y = ops.cat_channels(parts)
        by = ops.cached_bound(y)
        assert by is not None and float(bound(by)) == big and big >= float(y.cpu().abs().max())
        z = ops.maxpool3x3s2(parts[1])
        bz = ops.cached_bound(z)
        assert bz is not None and float(bound(bz)) == big and big >= float(z.cpu().abs().max())
        # a bilinear sample rounds (ops.BILINEAR_SLACK): the bound handed on is the input's times 1 + 2^-20 in fp32, no more
        wide = float(torch.tensor(big, dtype=torch.float32) * (1.0 + 2.0 ** -20))
        assert big < wide <= big * (1.0 + 2.0 ** -19)
        for fn in (lambda t: ops.upsample_bilinear(t, 2), ops.upsample_bilinear2x, lambda t: ops.upsample_bilinear(t, 4)):
            z = fn(parts[1])
            bz = ops.cached_bound(z)
            assert bz is not None and float(bound(bz)) == wide
            assert wide >= float(z.cpu().abs().max())
        # a map that holds its maximum everywhere: the samples round ABOVE it (0.1 -> 0.10000001), the bound must still hold
        flat = torch.full((1, 5, 6, 32), 0.1, device=d)
        bf = ops.bound_of(flat)
        assert torch.equal(bound(bf), flat.cpu().abs().max())
        for f in (2, 4):
            z = ops.upsample_bilinear(flat, f)
            bz = bound(ops.cached_bound(z))
            assert torch.equal(bz, bound(bf) * (1.0 + 2.0 ** -20)), f
            assert float(bz) >= float(z.cpu().abs().max()), f
        fresh = torch.randn(2, 9, 7, 32, generator=g).to(d)           # no bound yet
        assert ops.cached_bound(fresh) is None
        assert ops.cached_bound(ops.cat_channels([parts[0], fresh, parts[2]])) is None
        assert ops.cached_bound(ops.maxpool3x3s2(fresh)) is None
        assert ops.cached_bound(ops.upsample_bilinear(fresh, 2)) is None
    finally:
        ops.ENGINE = saved


# ------------------------------------------------------------------------------------------------ producer -> consumer
def test_bn_bound_feeds_the_halo_kernel_at_3e4():
    """BatchNorm (+ residual, ReLU) -> 3x3 convolution on the halo kernel with y ~ 3e4 randn: the convolution scales its A operand
    by the bound rih_bn_apply wrote and by nothing else (no rih_absmax launch); finite, and against fp64 from the y the kernel
    wrote at the suite's bar."""
    from renderih_amd import ops
    d = dev()
    saved = (ops.ENGINE, ops.HALO3, ops.conv3x3_halo)
    ops.ENGINE, ops.HALO3 = 2, True
    taken = []
    real = ops.conv3x3_halo

    def spy(*a, **k):
        ok = real(*a, **k)
        taken.append(ok)
        return ok
    ops.conv3x3_halo = spy
    L = ops._L()
    real_absmax = L.rih_absmax
    measured = []
    try:
        N, H, W, Cin, Cout = 1, 8, 32, 32, 64
        g = torch.Generator().manual_seed(77)
        x = (torch.randn(N, H, W, Cin, generator=g) * 2 + 0.5).to(d)
        gamma, beta = ((torch.rand(Cin, generator=g) + 0.5) * 3e4).to(d), (torch.randn(Cin, generator=g) * 3e3).to(d)
        rm, rv = torch.zeros(Cin).to(d), torch.ones(Cin).to(d)
        r = (torch.randn(N, H, W, Cin, generator=g) * 3e4).to(d)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(d)
        ops.bound_of(w)                 # (cached on w: a plain tensor's bound is trusted)
        y = ops.batchnorm(x, gamma, beta, rm, rv, residual=r, training=True, relu=True)
        yc = y.cpu()
        assert 5e4 < float(yc.abs().max()) < 1e6
        assert torch.equal(bound(ops.cached_bound(y)), yc.abs().max())
        L.rih_absmax = lambda *a: (measured.append(a[1]), real_absmax(*a))[1]
        z = ops.conv2d(y, w, None, stride=1, pad=1)
        L.rih_absmax = real_absmax
        assert taken == [True], taken
        assert measured == [], 'the convolution measured an operand that carried a bound'
        zc = nchw(z).cpu()
        assert bool(torch.isfinite(zc).all())
        ref = F.conv2d(nchw(yc).double(), w.cpu().double(), padding=1)
        assert_close(zc, ref, 1e-4, 1e-5, 'BatchNorm -> halo conv at 3e4')
    finally:
        L.rih_absmax = real_absmax
        ops.ENGINE, ops.HALO3, ops.conv3x3_halo = saved


@pytest.mark.parametrize('gscale', [1e4, 1e-6])
def test_bn_bwd_bound_feeds_the_conv_backward(gscale):
    """conv 3x3 -> BatchNorm (training) with the upstream gradient x 1e4 / x 1e-6: the convolution's data gradient (halo kernel)
    and weight gradient read the BatchNorm's dx with the bound rih_bn_bwd wrote -- against fp64 from that same dx."""
    from renderih_amd import ops
    d = dev()
    saved = (ops.ENGINE, ops.HALO3)
    ops.ENGINE, ops.HALO3 = 2, True
    try:
        N, H, W, Cin, Cout = 1, 8, 32, 32, 64
        g = torch.Generator().manual_seed(78)
        x = (torch.randn(N, H, W, Cin, generator=g) * 2).to(d).requires_grad_(True)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(9 * Cin)).to(d).requires_grad_(True)
        gamma, beta = (torch.rand(Cout, generator=g) + 0.5).to(d), (torch.randn(Cout, generator=g) * 0.1).to(d)
        rm, rv = torch.zeros(Cout).to(d), torch.ones(Cout).to(d)
        gy = (torch.randn(N, H, W, Cout, generator=g) * gscale).to(d)
        c = ops.conv2d(x, w, None, stride=1, pad=1)
        seen = []
        c.register_hook(lambda g_: seen.append((g_, ops.cached_bound(g_))))
        y = ops.batchnorm(c, gamma, beta, rm, rv, training=True, relu=False)
        y.backward(gy)
        (dc, bdc), = seen
        dcc = dc.cpu()
        assert bdc is not None and torch.equal(bound(bdc), dcc.abs().max())
        xr = nchw(x.detach().cpu()).double().requires_grad_(True)
        wr = w.detach().cpu().double().requires_grad_(True)
        F.conv2d(xr, wr, padding=1).backward(nchw(dcc).double())
        assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(w.grad).all())
        assert_close(nchw(x.grad.cpu()), xr.grad, 1e-4, 1e-5, 'conv dx behind BatchNorm, gradient x %g' % gscale)
        assert_close(w.grad.cpu(), wr.grad, 1e-4, 1e-5, 'conv dw behind BatchNorm, gradient x %g' % gscale)
    finally:
        ops.ENGINE, ops.HALO3 = saved
