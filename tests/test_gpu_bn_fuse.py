"""The fused BatchNorm kernels against the call sequences they replace, on the same inputs:
  * the pair y = act(BN_a(xa) + BN_b(xb)) -- rih_bn_apply2 / rih_bn_bwd2 -- against rih_bn_apply(b) -> rih_bn_apply(a, residual)
    and rih_bn_bwd(a, dres) -> rih_bn_bwd(b, dy = dres);
  * the stem maxpool3x3s2(relu(BN(x))) -- rih_bn_pool_fwd / rih_bn_pool_bwd -- against rih_bn_apply(relu, mask) ->
    rih_maxpool3x3s2_fwd and rih_maxpool3x3s2_bwd -> rih_bn_bwd;
  * the two gates of rih_bn_bwd behind a ReLU, the forward's sign bytes and y > 0, against each other.

Every comparison is BITWISE, on int32 views; no tolerances.  One thing is not a property of either source and is taken out of the
comparison: the sign and payload bits of a NaN.  IEEE 754 leaves them open when several operands of one operation are NaN; this
hardware takes them from the first NaN operand, and the compiler orders the factors of a contracted product, and places a negation
among them, per kernel -- per instantiation even of one source line: bn_bwd_apply_kernel and bn_bwd2_apply_kernel both take
`t - xhat * (s2 / rows)` from bn_bwd_dx, and it has been compiled to fma(-xhat, s2 / rows, t) in the one and to
fma(-(s2 / rows), xhat, t) in the other.  With the bits of NaNs compared too, exactly the 'nan' regime failed, on dxa / dxb
under training statistics, at every shape (first: (1, 4, relu 0, frozen 0 0)); all other regimes, +-inf included, were equal.  So
every NaN is mapped to one pattern before the comparison: NaNs must sit at the same places, everything else must have the same bits.

Every output buffer lies between two stretches of a poison value that must survive.  Operand bounds are compared as the maximum
over the 64 slots of a bound block: which slot a workgroup publishes to depends on the launch grid, the maximum does not.

Data regimes: random; constant inputs (ties: the first tap of a window must win); beta so negative that the ReLU closes
everywhere; gamma = 0; one NaN; one +inf and one -inf.  Each under training statistics (rih_bn_stats of the inputs) and under
frozen ones (rih_bn_eval_stats) -- for the pair independently for the two BatchNorms, with and without the ReLU.

The check_* functions also run on the host-compiled kernels (tests/test_bn_fuse_on_cpu.py), which replace dev()."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = -7.25e30
POISON_BYTE = 0xA5
GUARD = 64                  # elements of poison in front of and behind every output (a multiple of 16 bytes)
PAIR_SHAPES = ((1, 4), (7, 8), (130, 12), (512, 64), (1030, 256), (65, 2048))       # (rows, C): one row, odd row counts, more
#                       than one chunk of col_geom (130 x 12: 3 quads on 2 quad-threads; 512 x 64, 1030 x 256), more than one column block
REGIMES = ('random', 'constant', 'beta_neg', 'gamma0', 'nan', 'inf')
BOUND_FLOATS = 2048


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _lib():
    from renderih_amd import ops
    return ops._L(), ops._stream()


def _sync():
    if dev().type == 'cuda':
        torch.cuda.synchronize()


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev()).clone()


class Out:
    """an output buffer of n elements between two poisoned guards"""

    def __init__(self, n, dtype=torch.float32):
        fill = POISON if dtype == torch.float32 else POISON_BYTE if dtype == torch.uint8 else POISON_BYTE - 256
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype).to(dev())
        self.fill, self.n = fill, n

    @property
    def t(self):
        return self.buf[GUARD:GUARD + self.n]

    def ptr(self):
        return self.t.data_ptr()

    def bits(self):
        """the payload as integers, after checking that the guards survived"""
        b = self.buf.cpu()
        want = torch.full((GUARD,), self.fill, dtype=b.dtype)
        assert torch.equal(b[:GUARD], want) and torch.equal(b[GUARD + self.n:], want), 'poison around an output was overwritten'
        p = b[GUARD:GUARD + self.n]
        if p.dtype != torch.float32:
            return p
        return torch.where(torch.isnan(p), torch.full_like(p, float('nan')), p).view(torch.int32)     # see the module docstring


def _bound():
    return torch.zeros(BOUND_FLOATS, dtype=torch.float32).to(dev())


def _same(a, b, what, case):
    assert torch.equal(a.bits(), b.bits()), '%s differs: %s' % (what, case)


def pair_problem(rows, Cc, regime, seed):
    rs = np.random.RandomState(seed)
    f = np.float32
    p = {'xa': (rs.randn(rows, Cc) * 3.0 + 0.5).astype(f), 'xb': (rs.randn(rows, Cc) * 0.7 - 0.25).astype(f),
         'dy': rs.randn(rows, Cc).astype(f)}
    for s in 'ab':
        p['gamma_' + s] = (rs.rand(Cc) + 0.5).astype(f) * rs.choice([-1, 1], Cc).astype(f)
        p['beta_' + s] = (rs.randn(Cc) * 0.5).astype(f)
        p['rmean_' + s] = (rs.randn(Cc) * 0.3).astype(f)
        p['rvar_' + s] = (rs.rand(Cc) + 0.25).astype(f)
    i = rs.randint(rows * Cc)
    j = rs.randint(rows * Cc)
    if regime == 'constant':
        p['xa'][:] = f(1.75)
        p['xb'][:] = f(-0.5)
    elif regime == 'beta_neg':
        p['beta_a'][:] = f(-1e3)
        p['beta_b'][:] = f(-1e3)
    elif regime == 'gamma0':
        p['gamma_a'][:] = 0
        p['gamma_b'][:] = 0
    elif regime == 'nan':
        p['xa'].reshape(-1)[i] = np.nan
        p['dy'].reshape(-1)[j] = np.nan
    elif regime == 'inf':
        p['xb'].reshape(-1)[i] = np.inf
        p['dy'].reshape(-1)[j] = -np.inf
    return {k: _up(v) for k, v in p.items()}


def _statistics(lib, st, p, s, rows, Cc, frozen):
    """mean / invstd of BatchNorm s as the model obtains them: batch statistics of the input, or the running ones"""
    mean, invstd = torch.empty(Cc).to(dev()), torch.empty(Cc).to(dev())
    if frozen:
        assert lib.rih_bn_eval_stats(p['rmean_' + s].data_ptr(), p['rvar_' + s].data_ptr(), Cc, 1e-5, mean.data_ptr(),
                                     invstd.data_ptr(), st) == 0
    else:
        ws = torch.empty(int(lib.rih_bn_ws_floats(rows, Cc))).to(dev())
        assert lib.rih_bn_stats(p['x' + s].data_ptr(), rows, Cc, 1e-5, 0.1, mean.data_ptr(), invstd.data_ptr(), 0, 0,
                                ws.data_ptr(), st) == 0
    return mean, invstd


def check_pair(rows, Cc, relu, frozen_a, frozen_b, regime, seed=0):
    lib, st = _lib()
    case = (rows, Cc, relu, frozen_a, frozen_b, regime)
    p = pair_problem(rows, Cc, regime, seed)
    n = rows * Cc
    ma, ia = _statistics(lib, st, p, 'a', rows, Cc, frozen_a)
    mb, ib = _statistics(lib, st, p, 'b', rows, Cc, frozen_b)
    P = lambda t: t.data_ptr()

    # forward, today's sequence: the branch's BatchNorm, then the block's with it as the residual
    idt, y0, y1 = Out(n), Out(n), Out(n)
    m0, m1 = Out(n // 4, torch.uint8), Out(n // 4, torch.uint8)
    b0, b1 = _bound(), _bound()
    assert lib.rih_bn_apply(P(p['xb']), P(mb), P(ib), P(p['gamma_b']), P(p['beta_b']), 0, idt.ptr(), rows, Cc, 0, 0, 0, st) == 0
    assert lib.rih_bn_apply(P(p['xa']), P(ma), P(ia), P(p['gamma_a']), P(p['beta_a']), idt.ptr(), y0.ptr(), rows, Cc, relu,
                            m0.ptr() if relu else 0, P(b0), st) == 0
    assert lib.rih_bn_apply2(P(p['xa']), P(ma), P(ia), P(p['gamma_a']), P(p['beta_a']), P(p['xb']), P(mb), P(ib), P(p['gamma_b']),
                             P(p['beta_b']), y1.ptr(), rows, Cc, relu, m1.ptr() if relu else 0, P(b1), st) == 0
    _sync()
    _same(y0, y1, 'y', case)
    _same(m0, m1, 'relu mask', case)        # without the ReLU neither may touch it: both still poison
    assert torch.equal(b0.max().cpu(), b1.max().cpu()), 'bound of y differs: %s' % (case,)

    # backward, today's sequence: the block's BatchNorm leaves the gated dy in dres, the branch's BatchNorm reads it as its dy
    dxa0, dxb0, dres, dxa1, dxb1 = (Out(n) for _ in range(5))
    small = [[Out(Cc) for _ in range(4)] for _ in range(2)]     # dgamma_a, dbeta_a, dgamma_b, dbeta_b of each route
    ba0, bb0, ba1, bb1 = (_bound() for _ in range(4))
    ws = torch.empty(int(lib.rih_bn_ws_floats(rows, Cc))).to(dev())
    ws2 = Out(int(lib.rih_bn_ws2_floats(rows, Cc)))
    mask = m0.ptr() if relu else 0
    assert lib.rih_bn_bwd(P(p['dy']), P(p['xa']), 0, P(ma), P(ia), P(p['gamma_a']), dxa0.ptr(), dres.ptr(), small[0][0].ptr(),
                          small[0][1].ptr(), rows, Cc, relu, frozen_a, P(ws), mask, P(ba0), st) == 0
    assert lib.rih_bn_bwd(dres.ptr(), P(p['xb']), 0, P(mb), P(ib), P(p['gamma_b']), dxb0.ptr(), 0, small[0][2].ptr(),
                          small[0][3].ptr(), rows, Cc, 0, frozen_b, P(ws), 0, P(bb0), st) == 0
    assert lib.rih_bn_bwd2(P(p['dy']), P(p['xa']), P(ma), P(ia), P(p['gamma_a']), P(p['xb']), P(mb), P(ib), P(p['gamma_b']),
                           dxa1.ptr(), dxb1.ptr(), small[1][0].ptr(), small[1][1].ptr(), small[1][2].ptr(), small[1][3].ptr(),
                           rows, Cc, relu, frozen_a, frozen_b, ws2.ptr(), mask, P(ba1), P(bb1), st) == 0
    _sync()
    _same(dxa0, dxa1, 'dxa', case)
    _same(dxb0, dxb1, 'dxb', case)
    for k, name in enumerate(('dgamma_a', 'dbeta_a', 'dgamma_b', 'dbeta_b')):      # the two dbeta each against its own reference
        _same(small[0][k], small[1][k], name, case)
    ws2.bits()              # the workspace's guards: rih_bn_ws2_floats is enough
    assert torch.equal(ba0.max().cpu(), ba1.max().cpu()), 'bound of dxa differs: %s' % (case,)
    assert torch.equal(bb0.max().cpu(), bb1.max().cpu()), 'bound of dxb differs: %s' % (case,)


def pair_flags():
    return list(itertools.product((1, 0), (0, 1), (0, 1)))      # relu, frozen_a, frozen_b


def check_pair_shape(rows, Cc):
    """every regime x ReLU x frozen_a x frozen_b at one shape"""
    k = 0
    for (relu, fa, fb), regime in itertools.product(pair_flags(), REGIMES):
        check_pair(rows, Cc, relu, fa, fb, regime, seed=k)
        k += 1
    return k


@pytest.mark.parametrize('rows,Cc', PAIR_SHAPES)
def test_pair_is_bitwise_the_two_call_sequence(rows, Cc):
    assert check_pair_shape(rows, Cc) == 48


def test_pair_refuses_what_it_cannot_do():
    lib, st = _lib()
    t = torch.zeros(64).to(dev())
    P = t.data_ptr()
    assert lib.rih_bn_ws2_floats(4, 6) == 0 and lib.rih_bn_ws2_floats(0, 8) == 0
    assert lib.rih_bn_apply2(P, P, P, P, P, P, P, P, P, P, P, 2, 6, 1, 0, 0, st) != 0            # C % 4
    assert lib.rih_bn_apply2(P, P, P, P, P, 0, P, P, P, P, P, 2, 8, 1, 0, 0, st) != 0            # no xb
    assert lib.rih_bn_bwd2(P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, 2, 8, 1, 0, 0, P, 0, 0, 0, st) != 0      # ReLU without its mask


# ------------------------------------------------------------------------------------------------ the two gates of rih_bn_bwd
MASK_Y_SHAPES = PAIR_SHAPES[:4]     # one row; a tail shorter than four rows per thread; more than one chunk; more than one quad per thread
MASK_Y_REGIMES = ('random', 'beta_neg', 'nan')


def check_bwd_mask_equals_y(rows, Cc, frozen, with_dres, regime, seed=0):
    """rih_bn_bwd behind a ReLU gates dy by the forward's sign bytes or, without them, by y > 0: one rih_bn_apply(relu) leaves
    both, and the two backward routes must leave the same bits.  `frozen`: the two bits of frozen_stats."""
    lib, st = _lib()
    case = (rows, Cc, frozen, with_dres, regime)
    p = pair_problem(rows, Cc, regime, seed)
    n = rows * Cc
    mean, invstd = _statistics(lib, st, p, 'a', rows, Cc, frozen & 1)
    P = lambda t: t.data_ptr()
    y, mask = Out(n), Out(n // 4, torch.uint8)
    assert lib.rih_bn_apply(P(p['xa']), P(mean), P(invstd), P(p['gamma_a']), P(p['beta_a']), 0, y.ptr(), rows, Cc, 1, mask.ptr(), 0,
                            st) == 0
    routes = []
    for by_mask in (True, False):
        o = {'dx': Out(n), 'dres': Out(n), 'dgamma': Out(Cc), 'dbeta': Out(Cc), 'ws': Out(int(lib.rih_bn_ws_floats(rows, Cc)))}
        bound = _bound()
        assert lib.rih_bn_bwd(P(p['dy']), P(p['xa']), 0 if by_mask else y.ptr(), P(mean), P(invstd), P(p['gamma_a']), o['dx'].ptr(),
                              o['dres'].ptr() if with_dres else 0, o['dgamma'].ptr(), o['dbeta'].ptr(), rows, Cc, 1, frozen,
                              o['ws'].ptr(), mask.ptr() if by_mask else 0, P(bound), st) == 0
        routes.append((o, bound))
    _sync()
    (a, ba), (b, bb) = routes
    for name in ('dx', 'dres', 'dgamma', 'dbeta'):      # dres not asked for: both still poison
        _same(a[name], b[name], name, case)
    a['ws'].bits(), b['ws'].bits()
    assert torch.equal(ba.max().cpu(), bb.max().cpu()), 'bound of dx differs: %s' % (case,)


def mask_y_flags():
    return list(itertools.product((0, 1, 2, 3), (True, False)))      # frozen_stats, with dres


def check_bwd_mask_equals_y_shape(rows, Cc):
    k = 0
    for (frozen, with_dres), regime in itertools.product(mask_y_flags(), MASK_Y_REGIMES):
        check_bwd_mask_equals_y(rows, Cc, frozen, with_dres, regime, seed=k)
        k += 1
    return k


@pytest.mark.parametrize('rows,Cc', MASK_Y_SHAPES)
def test_bwd_gated_by_mask_is_bitwise_gated_by_y(rows, Cc):
    assert check_bwd_mask_equals_y_shape(rows, Cc) == 24


# ------------------------------------------------------------------------------------------------ the stem
POOL_SHAPES = ((1, 1, 1, 4), (1, 2, 3, 4), (2, 5, 7, 8), (3, 9, 6, 12), (1, 8, 8, 64), (2, 16, 16, 64), (1, 40, 40, 4))
#   (N, H, W, C): odd sizes reach every border rule; (2, 16, 16, 64) and (1, 40, 40, 4) give col_geom more than one chunk


def pool_problem(N, H, W, Cc, regime, seed):
    rs = np.random.RandomState(seed)
    f = np.float32
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = {'xa': (rs.randn(N * H * W, Cc) * 2.0 + 0.3).astype(f), 'dy': rs.randn(N * Ho * Wo, Cc).astype(f),
         'gamma_a': ((rs.rand(Cc) + 0.5) * rs.choice([-1, 1], Cc)).astype(f), 'beta_a': (rs.randn(Cc) * 0.5).astype(f),
         'rmean_a': (rs.randn(Cc) * 0.3).astype(f), 'rvar_a': (rs.rand(Cc) + 0.25).astype(f)}
    i, j = rs.randint(N * H * W * Cc), rs.randint(N * Ho * Wo * Cc)
    if regime == 'constant':
        p['xa'][:] = f(1.75)
        p['beta_a'][:] = np.abs(p['beta_a']) + f(0.1)      # under training statistics bn(x) = beta: every tap ties above zero
    elif regime == 'beta_neg':
        p['beta_a'][:] = f(-1e3)
    elif regime == 'gamma0':
        p['gamma_a'][:] = 0
    elif regime == 'nan':
        p['xa'].reshape(-1)[i] = np.nan
        p['dy'].reshape(-1)[j] = np.nan
    elif regime == 'inf':
        p['xa'].reshape(-1)[i] = np.inf if seed % 2 else -np.inf
        p['dy'].reshape(-1)[j] = -np.inf if seed % 2 else np.inf
    return {k: _up(v) for k, v in p.items()}


def check_pool(N, H, W, Cc, frozen, regime, seed=0):
    lib, st = _lib()
    case = (N, H, W, Cc, frozen, regime)
    p = pool_problem(N, H, W, Cc, regime, seed)
    rows = N * H * W
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    n, npool = rows * Cc, N * Ho * Wo * Cc
    mean, invstd = _statistics(lib, st, p, 'a', rows, Cc, frozen)
    P = lambda t: t.data_ptr()
    x, ga, be = P(p['xa']), P(p['gamma_a']), P(p['beta_a'])

    # forward, today's sequence: BatchNorm + ReLU (with its sign mask), then the pool
    y, mask = Out(n), Out(n // 4, torch.uint8)
    yp0, yp1 = Out(npool), Out(npool)
    arg0, arg1 = Out(npool, torch.int8), Out(npool, torch.int8)
    b0, b1 = _bound(), _bound()
    assert lib.rih_bn_apply(x, P(mean), P(invstd), ga, be, 0, y.ptr(), rows, Cc, 1, mask.ptr(), P(b0), st) == 0
    assert lib.rih_maxpool3x3s2_fwd(y.ptr(), yp0.ptr(), arg0.ptr(), N, H, W, Cc, st) == 0
    assert lib.rih_bn_pool_fwd(x, P(mean), P(invstd), ga, be, yp1.ptr(), arg1.ptr(), N, H, W, Cc, P(b1), st) == 0
    _sync()
    _same(yp0, yp1, 'pooled y', case)
    _same(arg0, arg1, 'arg', case)
    assert torch.equal(b0.max().cpu(), b1.max().cpu()), 'bound of the pooled y differs: %s' % (case,)
    if regime == 'constant' and not frozen:
        a = arg1.bits().reshape(N, Ho, Wo, Cc)       # all taps tie: the first one inside the map wins
        assert bool((a[:, 1:, 1:] == 0).all()) and bool((a[:, 0, 0] == 4).all()) and bool((a[:, 1:, 0] == 1).all())

    # backward, today's sequence: the pool's backward writes the full-resolution gradient, the BatchNorm's backward reads it twice
    dfull, dx0, dx1 = Out(n), Out(n), Out(n)
    small = [[Out(Cc) for _ in range(2)] for _ in range(2)]
    bb0, bb1 = _bound(), _bound()
    ws = torch.empty(int(lib.rih_bn_ws_floats(rows, Cc))).to(dev())
    ws1 = Out(int(lib.rih_bn_ws_floats(rows, Cc)))
    assert lib.rih_maxpool3x3s2_bwd(P(p['dy']), arg0.ptr(), dfull.ptr(), N, H, W, Cc, st) == 0
    assert lib.rih_bn_bwd(dfull.ptr(), x, 0, P(mean), P(invstd), ga, dx0.ptr(), 0, small[0][0].ptr(), small[0][1].ptr(), rows, Cc,
                          1, frozen, P(ws), mask.ptr(), P(bb0), st) == 0
    assert lib.rih_bn_pool_bwd(P(p['dy']), arg0.ptr(), x, P(mean), P(invstd), ga, be, dx1.ptr(), small[1][0].ptr(),
                               small[1][1].ptr(), N, H, W, Cc, frozen, ws1.ptr(), P(bb1), st) == 0
    _sync()
    _same(dx0, dx1, 'dx', case)
    _same(small[0][0], small[1][0], 'dgamma', case)
    _same(small[0][1], small[1][1], 'dbeta', case)
    ws1.bits()
    assert torch.equal(bb0.max().cpu(), bb1.max().cpu()), 'bound of dx differs: %s' % (case,)


def check_pool_shape(N, H, W, Cc):
    k = 0
    for frozen, regime in itertools.product((0, 1), REGIMES):
        check_pool(N, H, W, Cc, frozen, regime, seed=k)
        k += 1
    return k


@pytest.mark.parametrize('N,H,W,Cc', POOL_SHAPES)
def test_stem_is_bitwise_the_four_call_sequence(N, H, W, Cc):
    assert check_pool_shape(N, H, W, Cc) == 12


def test_stem_refuses_what_it_cannot_do():
    lib, st = _lib()
    t = torch.zeros(256).to(dev())
    P = t.data_ptr()
    assert lib.rih_bn_pool_fwd(P, P, P, P, P, P, P, 1, 2, 2, 6, 0, st) != 0          # C % 4
    assert lib.rih_bn_pool_fwd(P, P, P, P, P, P + 4, P, 1, 2, 2, 8, 0, st) != 0      # an output off 16 bytes
    assert lib.rih_bn_pool_bwd(P, P, P, P, P, P, P, P, P, P, 1, 2, 2, 8, 0, 0, 0, st) != 0       # no workspace


# ------------------------------------------------------------------------------------------------ through the model
def mini_trunk():
    """stem, a Bottleneck with a downsample branch (stride 2), an identity Bottleneck"""
    import torch.nn as nn
    from renderih_amd import encoder as E

    class Mini(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)      # the image arrives padded to 4 channels, as in ResNetTrunk
            self.bn1 = nn.BatchNorm2d(64)
            ds = nn.Sequential(nn.Conv2d(64, 64, 1, 2, bias=False), nn.BatchNorm2d(64))
            self.b0 = E.Bottleneck(64, 16, 2, ds)
            self.b1 = E.Bottleneck(64, 16)

        def forward(self, x):
            x = E.stem_pool(self.conv1, self.bn1, x)
            y = self.b1(self.b0(x))
            E.flush_batches_tracked()
            return y
    return Mini()


def run_mini(state, x, w, train, fuse):
    """(output, parameter gradients, buffers) of one forward + backward of mini_trunk from `state`"""
    from renderih_amd import ops
    saved = ops.BN_PAIR_FUSE, ops.BN_POOL_FUSE
    ops.BN_PAIR_FUSE = ops.BN_POOL_FUSE = fuse
    try:
        m = mini_trunk()
        m.load_state_dict(state)
        m = m.to(dev())
        m.train(train)
        ops.bounds_reset()
        y = m(x.to(dev()))
        (y * w.to(dev())).sum().backward()
        _sync()
    finally:
        ops.BN_PAIR_FUSE, ops.BN_POOL_FUSE = saved
    out = {'y': y.detach().cpu()}
    out.update({'grad.' + k: v.grad.cpu() for k, v in m.named_parameters()})
    out.update({'buf.' + k: v.cpu() for k, v in m.named_buffers()})
    return out


def mini_inputs():
    g = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    state = {k: v.clone() for k, v in mini_trunk().state_dict().items()}
    for k, v in state.items():
        if k.endswith('running_mean') or k.endswith('bias'):
            v.copy_(torch.randn(v.shape, generator=g) * 0.2)
        elif k.endswith('running_var') or (k.endswith('weight') and v.dim() == 1):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
    x = torch.randn(2, 32, 32, 4, generator=g)
    x[..., 3] = 0
    return state, x, torch.randn(2, 4, 4, 64, generator=g)


def check_model(train):
    from renderih_amd import ops
    assert ops.bn_pair_fused() and ops.bn_pool_fused(), 'the library under test has no fused kernels'
    state, x, w = mini_inputs()
    a, b = run_mini(state, x, w, train, True), run_mini(state, x, w, train, False)
    assert set(a) == set(b) and len(a) > 40
    for k in a:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(
            torch.int32) if b[k].dtype == torch.float32 else b[k]), k
    assert all(torch.isfinite(v).all() for v in a.values())
    if train:
        assert int(a['buf.b0.downsample.1.num_batches_tracked']) == 1 and not torch.equal(a['buf.b0.bn3.running_mean'],
                                                                                          state['b0.bn3.running_mean'])


@pytest.mark.parametrize('train', (True, False))
def test_model_is_bitwise_the_same_with_both_switches_on_and_off(train):
    check_model(train)
