"""csrc/rih_flash.hip against multi-head attention in torch.float64 at the edges of its tiling, of its operand layouts and of
its logit range.  Case tables, reference and the bar: tests/flash_cases.py.

What the rest of the suite leaves open: test_flash_attention_equals_three_kernel_path compares flash with the project's own
three-kernel path (a shared mistake passes), test_attention compares it with torch fp32 at unit scale, where softmax is far
from saturation and the online-softmax machinery -- corr = exp2f(m - m_new), the -inf of padded keys, the fp32 lse word both
backward kernels recompute every probability from -- has little to do.  Nothing checked lse itself, nothing called
rih_flash_attention_* directly: the scalar (vec == 0) branches of issue_tiles / store_T and the RIH_EINVAL lines of the two
entry points never ran.

The check_* helpers also run on the host-compiled kernels (tests/test_kernels_on_cpu.py), which replaces dev()."""
import contextlib

import pytest
import torch

import flash_cases as FC

pytestmark = pytest.mark.gpu

RIH_EINVAL = -1
SENT = -7.25                # fills pitch gaps, guard bands and outputs before a launch
GUARD = 64                  # floats in front of and behind every slab


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@contextlib.contextmanager
def flash_path(on):
    """ops.FLASH_ATTN for the duration of a check; also asserts below that the path meant took the case."""
    from renderih_amd import ops
    saved = ops.FLASH_ATTN
    ops.FLASH_ATTN = on
    try:
        yield ops
    finally:
        ops.FLASH_ATTN = saved


def _what(shape, regime, tag=''):
    return FC.case_id((shape, regime)) + tag


def leaf(t):
    """A fresh leaf on the device under test (the inputs of a case are shared: on the host build .to() alone would hand them out)."""
    return t.detach().clone().to(dev()).requires_grad_(True)


def run_attention(q, k, v, gy, heads, p=0.0, seed=0):
    from renderih_amd import ops
    d = dev()
    tg = [leaf(t) for t in (q, k, v)]
    y = ops.attention(tg[0], tg[1], tg[2], heads, p, seed)
    y.backward(gy.to(d))
    return [y.detach()] + [t.grad for t in tg]


def check_vs_fp64(shape, regime, flash=True, p=0.0, seed=0):
    B, Sq, Sk, D, heads = shape
    inp, ref = FC.inputs(shape, regime), FC.reference(shape, regime, p, seed)
    with flash_path(flash) as ops:
        assert ops._flash_ok(D // heads, B, heads) == flash          # the path meant, not its sibling
        got = run_attention(*inp, heads, p, seed)
    FC.check_bar(got, ref, _what(shape, regime, (' flash' if flash else ' three-kernel') + (' p%g' % p if p else '')), inp, heads)
    if regime == 'zero':                                            # all logits equal: the output is the mean of v
        mean = inp[2].double().mean(1, keepdim=True).expand(B, Sq, D)
        err = float((got[0].double().cpu() - mean).abs().max())
        print('FLASH-EDGE %s out vs mean(v) %.3e bound %.3e' % (_what(shape, regime), err, Sk * FC.U))
        assert err <= Sk * FC.U, (shape, err)
    return got


# ------------------------------------------------------------------------------------------------------------- the C ABI, directly
class Slab:
    """[rows][width] floats at row pitch ld, starting `off` floats past a 16-byte boundary, inside ONE allocation whose every
    other float (pitch gaps, GUARD floats in front and behind) holds SENT."""

    def __init__(self, rows, width, ld=None, off=0, values=None):
        d = dev()
        ld = width if ld is None else ld
        self.rows, self.width, self.ld = rows, width, ld
        n = (rows - 1) * ld + width
        self.flat = torch.full((GUARD + 4 + n + GUARD,), SENT, device=d)
        base = self.flat.data_ptr()
        assert base % 4 == 0
        start = GUARD + (-(base // 4 + GUARD)) % 4 + off
        assert (base + 4 * start) % 16 == 4 * off
        self.idx = ((torch.arange(rows)[:, None] * ld + torch.arange(width)[None, :]).reshape(-1) + start).to(d)
        self.ptr = base + 4 * start
        if values is not None:
            self.flat[self.idx] = values.reshape(-1).to(d)

    def values(self):
        return self.flat[self.idx].reshape(self.rows, self.width).cpu()

    def untouched(self):
        """every float outside the [rows][width] window still holds the sentinel"""
        m = torch.ones_like(self.flat, dtype=torch.bool)
        m[self.idx] = False
        return bool((self.flat[m] == SENT).all())

    def all_untouched(self):
        return bool((self.flat == SENT).all())


def abi_forward(shape, inp, off=0, pitches=(0, 0), p=0.0, seed=0):
    """rih_flash_attention_fwd on slabs: q and out at pitch D + pitches[0], k and v at D + pitches[1], all `off` floats off a
    16-byte boundary.  Returns the slabs."""
    from renderih_amd import ops
    B, Sq, Sk, D, heads = shape
    d = D // heads
    q, k, v, _ = inp
    s = dict(q=Slab(B * Sq, D, D + pitches[0], off, q), k=Slab(B * Sk, D, D + pitches[1], off, k),
             v=Slab(B * Sk, D, D + pitches[1], off, v), out=Slab(B * Sq, D, D + pitches[0], off),
             lse=Slab(1, B * heads * Sq))
    rc = ops._L().rih_flash_attention_fwd(s['q'].ptr, s['q'].ld, s['k'].ptr, s['v'].ptr, s['k'].ld, B, heads, Sq, Sk, d,
                                          1.0 / d ** 0.5, p, seed, 0, s['out'].ptr, s['out'].ld, s['lse'].ptr, ops._stream())
    assert rc == 0, rc
    return s


def abi_backward(shape, inp, fwd, off=0, pitches=(0, 0), p=0.0, seed=0):
    """rih_flash_attention_bwd on the slabs of abi_forward: dO and dq at pitch D + pitches[1], dk and dv at D + pitches[0]."""
    from renderih_amd import ops
    B, Sq, Sk, D, heads = shape
    d = D // heads
    s = dict(fwd, do=Slab(B * Sq, D, D + pitches[1], off, inp[3]), D=Slab(1, B * heads * Sq),
             dq=Slab(B * Sq, D, D + pitches[1], off), dk=Slab(B * Sk, D, D + pitches[0], off),
             dv=Slab(B * Sk, D, D + pitches[0], off))
    rc = ops._L().rih_flash_attention_bwd(s['do'].ptr, s['do'].ld, s['out'].ptr, s['out'].ld, s['q'].ptr, s['q'].ld, s['k'].ptr,
                                          s['v'].ptr, s['k'].ld, B, heads, Sq, Sk, d, 1.0 / d ** 0.5, p, seed, 0, s['lse'].ptr,
                                          s['D'].ptr, s['dq'].ptr, s['dq'].ld, s['dk'].ptr, s['dv'].ptr, s['dk'].ld,
                                          ops._stream())
    assert rc == 0, rc
    return s


def check_lse_word(shape, regime):
    """The lse word of the forward -- the only state the backward keeps -- and the extent of what the forward writes: [B, heads,
    Sq] words and [B Sq][D] outputs, nothing for the rows of the last wavefront past Sq."""
    B, Sq, Sk, D, heads = shape
    inp, ref = FC.inputs(shape, regime), FC.reference(shape, regime)
    s = abi_forward(shape, inp)
    FC.check_lse(s['lse'].values().reshape(B, heads, Sq), ref, _what(shape, regime))
    FC.check_bar([s['out'].values().reshape(B, Sq, D)], ref, _what(shape, regime, ' abi'), names=('out',))
    for name in ('lse', 'out'):
        assert s[name].untouched(), (shape, regime, name, 'written past its extent')
    for name, t in zip('qkv', inp):
        assert s[name].untouched() and torch.equal(s[name].values().reshape(t.shape), t), (shape, regime, name, 'input overwritten')


def check_forward_at_full_lift(shape, order):
    """'last' / 'first' with the dominating key 40 above the rest (corr = e^-40 on the final tile; every later probability
    e^-40): out and lse against fp64.  The gradients of such rows are beyond fp32 (flash_cases.LIFT) and are not looked at."""
    B, Sq, Sk, D, heads = shape
    (q, k, v), ref = FC.forward_reference(shape, order)
    s = abi_forward(shape, (q, k, v, None))
    what = _what(shape, order, ' lift %g' % FC.FWD_LIFT)
    FC.check_lse(s['lse'].values().reshape(B, heads, Sq), ref, what)
    FC.check_bar([s['out'].values().reshape(B, Sq, D)], ref, what, names=('out',))


def check_unaligned_bit_identical(shape, p=0.0, seed=0):
    """The same values through 16-byte-aligned contiguous operands (float4 loads and stores) and through views one float off
    alignment with row pitches heads d + 1 and heads d + 3 (the scalar branches of issue_tiles and store_T): the vec flags
    change the load width only, so every result is bit-identical; pitch gaps and guard bands keep their sentinel."""
    B, Sq, Sk, D, heads = shape
    inp, ref = FC.inputs(shape, 'qk1'), FC.reference(shape, 'qk1', p, seed)
    res = []
    for off, pitches in ((0, (0, 0)), (1, (1, 3))):
        s = abi_backward(shape, inp, abi_forward(shape, inp, off, pitches, p, seed), off, pitches, p, seed)
        for name, slab in s.items():
            assert slab.untouched(), (shape, off, name, 'a pitch gap or guard band was written')
        res.append({n: s[n].values() for n in ('out', 'lse', 'dq', 'dk', 'dv')})
    for n in res[0]:
        assert torch.equal(res[0][n], res[1][n]), (shape, n, float((res[0][n] - res[1][n]).abs().max()))
    got = [res[1][n].reshape(getattr(ref, n).shape) for n in FC.NAMES]
    FC.check_bar(got, ref, _what(shape, 'qk1', ' unaligned abi'), inp, heads)
    FC.check_lse(res[1]['lse'].reshape(B, heads, Sq), ref, _what(shape, 'qk1', ' unaligned abi'))


def check_refusals():
    """Both entry points answer RIH_EINVAL -- before any launch -- and leave their outputs alone.  (Operands of a valid call's size
    wherever the refused argument allows it: a refusal that failed would then still run inside them.)"""
    from renderih_amd import ops
    L = ops._L()
    B, heads, Sq, Sk, d = 2, 2, 5, 7, 16
    D = heads * d
    q, do, o = (Slab(B * Sq, D, values=torch.ones(B * Sq, D)) for _ in range(3))
    k, v = (Slab(B * Sk, D, values=torch.ones(B * Sk, D)) for _ in range(2))
    lse_in = Slab(1, B * heads * Sq, values=torch.zeros(1, B * heads * Sq))
    outs = dict(out=Slab(B * Sq, D), lse=Slab(1, B * heads * Sq), D=Slab(1, B * heads * Sq), dq=Slab(B * Sq, D),
                dk=Slab(B * Sk, D), dv=Slab(B * Sk, D))
    fwd_ok = dict(q=q.ptr, q_ld=D, k=k.ptr, v=v.ptr, kv_ld=D, B=B, heads=heads, Sq=Sq, Sk=Sk, d=d, alpha=0.25, drop_p=0.0,
                  seed=1, seed_dev=0, out=outs['out'].ptr, ld_out=D, lse=outs['lse'].ptr, stream=ops._stream())
    bwd_ok = dict(dO=do.ptr, do_ld=D, O=o.ptr, o_ld=D, q=q.ptr, q_ld=D, k=k.ptr, v=v.ptr, kv_ld=D, B=B, heads=heads, Sq=Sq,
                  Sk=Sk, d=d, alpha=0.25, drop_p=0.0, seed=1, seed_dev=0, lse=lse_in.ptr, Dws=outs['D'].ptr, dq=outs['dq'].ptr,
                  dq_ld=D, dk=outs['dk'].ptr, dv=outs['dv'].ptr, dkv_ld=D, stream=ops._stream())
    common = [dict(d=8), dict(d=48), dict(d=128), dict(d=0), dict(q_ld=d - 1), dict(kv_ld=d - 1), dict(drop_p=-0.125),
              dict(drop_p=1.0), dict(drop_p=1.5), dict(B=65536 // heads), dict(B=0), dict(heads=0), dict(Sq=0), dict(Sq=-3),
              dict(Sk=0), dict(Sk=-1), dict(q=0), dict(k=0), dict(v=0)]
    fwd_bad = common + [dict(ld_out=D - 1), dict(out=0), dict(lse=0)]
    bwd_bad = common + [dict(do_ld=D - 1), dict(o_ld=D - 1), dict(dq_ld=d - 1), dict(dkv_ld=d - 1), dict(dO=0), dict(O=0),
                        dict(lse=0), dict(Dws=0), dict(dq=0), dict(dk=0), dict(dv=0)]
    for fn, ok, bad in ((L.rih_flash_attention_fwd, fwd_ok, fwd_bad), (L.rih_flash_attention_bwd, bwd_ok, bwd_bad)):
        for change in bad:
            assert set(change) <= set(ok), change
            rc = fn(*dict(ok, **change).values())
            assert rc == RIH_EINVAL, (fn.__name__ if hasattr(fn, '__name__') else fn, change, rc)
    if dev().type == 'cuda':
        torch.cuda.synchronize()
    for name, slab in outs.items():
        assert slab.all_untouched(), (name, 'written by a refused call')


# ---------------------------------------------------------------------------------------------------- the packed entry points
def _packed(B, S, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, S, 3 * D, generator=g)


def _direction_ref(qsrc, ksrc, vsrc, gy, heads, p, seed):
    B, S, D3 = qsrc.shape
    D = D3 // 3
    q, k, v = qsrc[..., :D].contiguous(), ksrc[..., D:2 * D].contiguous(), vsrc[..., 2 * D:].contiguous()
    keep = FC.keep_mask(B, heads, S, S, p, seed) if p > 0 else None
    return (q, k, v, gy), FC.make_ref(q, k, v, gy, heads, keep, p)


def check_entry_points(S, p):
    """self_attention_packed, cross_attention_packed and cross_attention_stacked (own_keys False / True) read head slices in place
    from [B, S, 3D] projections and write dq / dk / dv of two launches into ONE packed gradient buffer: every slot of it against
    the fp64 gradient of the direction that owns it (a slot written twice or never fails its direction's bar)."""
    B, D, heads = 2, 64, 4
    d = dev()
    s1, s2 = 1234567, 7654321
    L, R = _packed(B, S, D, 11 + S), _packed(B, S, D, 13 + S)
    g = torch.Generator().manual_seed(17 + S)
    g1, g2 = torch.randn(B, S, D, generator=g), torch.randn(B, S, D, generator=g)
    slots = lambda t: (t[..., :D], t[..., D:2 * D], t[..., 2 * D:])
    tag = ' S%d p%g' % (S, p)
    with flash_path(True) as ops:
        assert ops._flash_ok(D // heads, B, heads)
        # self attention
        x = leaf(L)
        y = ops.self_attention_packed(x, heads, p, s1)
        y.backward(g1.to(d))
        inp, ref = _direction_ref(L, L, L, g1, heads, p, s1)
        FC.check_bar([y, *slots(x.grad)], ref, 'self_attention_packed' + tag, inp, heads)
        # the cross pair on two packed projections
        xl, xr = leaf(L), leaf(R)
        y1, y2 = ops.cross_attention_packed(xl, xr, heads, p, s1, s2)
        (y1 * g1.to(d)).sum().add((y2 * g2.to(d)).sum()).backward()
        inp1, r2l = _direction_ref(L, R, R, g1, heads, p, s1)        # left queries over right keys / values
        inp2, l2r = _direction_ref(R, L, L, g2, heads, p, s2)
        gl, gr = slots(xl.grad), slots(xr.grad)
        FC.check_bar([y1, gl[0], gr[1], gr[2]], r2l, 'cross_attention_packed r2l' + tag, inp1, heads)
        FC.check_bar([y2, gr[0], gl[1], gl[2]], l2r, 'cross_attention_packed l2r' + tag, inp2, heads)
        # ... and on the hands-stacked projection, with the other hand's keys or each hand's own
        for own in (False, True):
            x = leaf(torch.stack([L, R]))
            y = ops.cross_attention_stacked(x, heads, p, s1, s2, own_keys=own)
            y.backward(torch.stack([g1, g2]).to(d))
            gl, gr = slots(x.grad[0]), slots(x.grad[1])
            name = 'cross_attention_stacked own_keys=%s ' % own
            if own:
                inp1, ra = _direction_ref(L, L, R, g1, heads, p, s1)     # softmax(Lq Lk^T) Rv
                inp2, rb = _direction_ref(R, R, L, g2, heads, p, s2)
                FC.check_bar([y[0], gl[0], gl[1], gr[2]], ra, name + 'slice 0' + tag, inp1, heads)
                FC.check_bar([y[1], gr[0], gr[1], gl[2]], rb, name + 'slice 1' + tag, inp2, heads)
            else:
                FC.check_bar([y[0], gl[0], gr[1], gr[2]], r2l, name + 'r2l' + tag, inp1, heads)
                FC.check_bar([y[1], gr[0], gl[1], gl[2]], l2r, name + 'l2r' + tag, inp2, heads)


def check_dropout(shape):
    B, Sq, Sk, D, heads = shape
    p, seed = 0.25, 24680
    ref = FC.reference(shape, 'qk1', p, seed)
    frac = float(ref.keep.float().mean())
    print('FLASH-EDGE %s keep fraction %.4f' % (_what(shape, 'qk1', ' p%g' % p), frac))
    assert abs(frac - (1 - p)) <= 0.02, frac
    a = check_vs_fp64(shape, 'qk1', True, p, seed)
    b = check_vs_fp64(shape, 'qk1', True, p, seed)
    for name, x, y in zip(FC.NAMES, a, b):
        assert torch.equal(x, y), (shape, name, 'two runs differ')


# ---------------------------------------------------------------------------------------------------------------- the GPU tests
@pytest.mark.parametrize('case', FC.CASES, ids=FC.case_id)
def test_flash_vs_fp64(case):
    check_vs_fp64(*case)


@pytest.mark.parametrize('case', FC.THREE_KERNEL_CASES, ids=FC.case_id)
def test_three_kernel_path_vs_fp64(case):
    """The sibling test_flash_attention_equals_three_kernel_path leans on, anchored to fp64 as well."""
    check_vs_fp64(*case, flash=False)


LSE_CASES = [c for c in FC.CASES if c[0] in ((1, 33, 31, 64, 4), (1, 129, 33, 64, 4))]


@pytest.mark.parametrize('case', LSE_CASES, ids=FC.case_id)
def test_flash_lse_word(case):
    check_lse_word(*case)


@pytest.mark.parametrize('case', FC.FWD_CASES, ids=FC.case_id)
def test_flash_forward_at_full_lift(case):
    check_forward_at_full_lift(*case)


@pytest.mark.parametrize('shape', [(1, 129, 33, 64, 4), (2, 65, 97, 256, 4)], ids=lambda s: 'x'.join(map(str, s)))
def test_flash_dropout_vs_fp64(shape):
    check_dropout(shape)


@pytest.mark.parametrize('p', [0.0, 0.25])
@pytest.mark.parametrize('S', [33, 129])
def test_flash_entry_points_vs_fp64(S, p):
    check_entry_points(S, p)


@pytest.mark.parametrize('shape,p', [((1, 33, 31, 64, 4), 0.0), ((1, 129, 33, 256, 4), 0.0), ((1, 33, 31, 64, 4), 0.25)],
                         ids=['d16', 'd64', 'd16-dropout'])
def test_flash_unaligned_operands_are_bit_identical(shape, p):
    check_unaligned_bit_identical(shape, p, 97531)


def test_flash_refusals():
    check_refusals()
