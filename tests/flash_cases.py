"""Case tables, the fp64 reference and the bar of the flash-attention edge tests (tests/test_gpu_flash_edges.py on the GPU,
tests/test_kernels_on_cpu.py on the host build of csrc/rih_flash.hip).  No GPU is touched here.

The bar.  For one case let e(x) = max|x - x64| / max|x64| against multi-head attention in torch.float64
autograd, and e32 = the largest e() of the same arithmetic in torch.float32 on the CPU over (out, dq, dk, dv).  A kernel passes
if each of its four tensors has

    e(got) <= 8 * max(e32, 2^-24 * (1 + Lmax)),        Lmax = max|alpha q.k|.

The first term is measured on the reference, per case.  The second is the rounding of the one fp32 log-sum-exp word per query
the design keeps for the backward (its magnitude is up to Lmax log2 e, and the probabilities are recomputed as
exp2(s alpha2 - lse)); it keeps the bar from collapsing where torch's fp32 happens to be exact.  The factor 8 is the margin
for the roundings flash has and torch has not: one rescale of the accumulator per 32-key tile (at most 10 tiles at 316 keys)
and the lse word.  A dropped tile, a mis-indexed key, a wrong alpha or a stale running maximum are off by 1e-2 or more.

A reference tensor that is identically zero (dq and dk with a single key; dk with q == 0) has no scale to be relative to:
there the kernel's tensor is bounded by 2 d 2^-24 alpha max_ij(sum_c |dO_ic| |v_jc|) max|k| (max|q| for dk), the gamma_d bound
of D = rowsum(dO o O) and dP = dO V^T, which are the same dot product summed in two orders.  That rule is applied ONLY where the
reference is identically zero, never as a floor.

Beyond the asserted range (q, k scale 30, |alpha s| up to about 4e3) flash degrades faster than torch: at scale 100 the
logits reach 1e4 and the probability exp2f(s alpha2 - lse) is the exponential of a difference of two fp32 numbers near 1.4e4,
each rounded to about 1e-3.  That regime is outside the decoder's range; measure() prints it, nothing asserts it."""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

LOG2E = 1.4426950408889634
U = 2.0 ** -24
FACTOR = 8.0

# (B, Sq, Sk, D, heads): the smallest shapes that reach each edge of the tiling -- 32 keys per LDS tile; a forward / dq workgroup
# owns 128 queries as 4 wavefronts x 32; a dkv workgroup owns 128 keys and walks 32-query tiles; head widths 16, 32, 64
SHAPES = [
    (1, 1, 1, 64, 4),           # one query, one key, d = 16
    (1, 130, 1, 64, 4),         # a single key under two query workgroups
    (1, 33, 31, 64, 4),         # one ragged key tile
    (1, 32, 32, 128, 4),        # exactly one tile each way, d = 32
    (1, 31, 33, 256, 4),        # the second key tile holds one key, d = 64
    (1, 128, 64, 32, 2),        # one exactly full query workgroup, d = 16
    (1, 129, 33, 64, 4),        # the second query workgroup holds one row
    (1, 5, 129, 32, 2),         # dkv grid of two, the second workgroup holds one key
    (1, 97, 257, 128, 4),       # dkv grid of three; nine key tiles forward, the last with one key
    (2, 65, 97, 256, 4),        # image stride, d = 64
    (3, 40, 160, 48, 3),        # three heads, d = 16: a head index that is no power of two
]
SCALES = [1e-3, 1.0, 8.0, 30.0]                     # of q and k (randn); nothing beyond 30 is asserted
WIDE_VDO = 'v1e4_do1e-4'                            # v x 1e4, dO x 1e-4 at q, k scale 1: out and dv are linear in these
WIDE_SHAPES = [s for s in SHAPES if s[2] >= 97]
# Orderings of the running maximum: every query is u + 0.1 randn with u a unit vector per head, and c u is added to chosen key
# rows, which lifts their logit by about c alpha.
#   'last'  the dominating key is the last valid one (alone in the padded tail tile where Sk % 32 == 1): corr wipes out the
#           whole accumulator on the final tile
#   'first' it is key 0: every later tile has corr == 1 and probabilities that vanish
#   'rise'  the first key of every tile lies RISE above the one of the tile before: one rescale per tile
#   'zero'  q == 0: all logits equal, the output is the mean of v, dk is exactly zero
# The lift of 'last' and 'first' is LIFT = 12, not 40.  A softmax row saturated to 1 - e^-40 has gradients dq, dk of the order
# e^-40 that NO fp32 arithmetic resolves: torch's fp32 softmax backward returns an exact 0 for the dominating key and misses
# fp64 by e32 = 1.0 on all three shapes (0.1 at a lift of 20, 2.4e-4 at 12, 1e-5 at 8), and the bar is meaningless where fp32
# is.  12 is the largest of those lifts at which torch fp32 keeps e32 <= 1e-3 (measured on the reference alone; over the whole
# table the worst e32 is 6.3e-4, five queries over 129 keys at scale 30); at e^-12 a stale maximum or a missing rescale is
# still an error of order one in `out`.  The forward alone -- out and the lse word, which stay well conditioned (e32 of out: 1e-10)
# -- is checked at the full lift of 40 as well (FWD_LIFT, forward_reference()).  'rise' keeps its +8 per tile (e32 <= 3.5e-4).
ORDERINGS = ['last', 'first', 'rise', 'zero']
ORDER_SHAPES = [(1, 33, 31, 64, 4), (1, 31, 33, 256, 4), (1, 97, 257, 128, 4)]
LIFT = 12.0
RISE = 8.0
FWD_LIFT = 40.0


def scale_id(s):
    return 'qk%g' % s


REGIMES = [scale_id(s) for s in SCALES]
CASES = [(s, r) for s in SHAPES for r in REGIMES] + [(s, WIDE_VDO) for s in WIDE_SHAPES] + \
        [(s, o) for s in ORDER_SHAPES for o in ORDERINGS]
FWD_CASES = [(s, o) for s in ORDER_SHAPES for o in ('last', 'first')]
THREE_KERNEL_CASES = [(s, scale_id(x)) for s in SHAPES[:4] for x in (1.0, 30.0)]


def case_id(case):
    return '%s-%s' % ('x'.join(str(n) for n in case[0]), case[1])


def _unit_queries_and_lifted_keys(g, B, Sq, Sk, D, heads, order, lift, rise):
    d = D // heads
    u = torch.randn(heads, d, generator=g)
    u = (u / u.norm(dim=1, keepdim=True)).reshape(1, 1, D)
    q = u + 0.1 * torch.randn(B, Sq, D, generator=g)
    k = torch.randn(B, Sk, D, generator=g)
    per_logit = math.sqrt(d)                        # c with c alpha = 1
    if order == 'last':
        k[:, Sk - 1] += lift * per_logit * u[0]
    elif order == 'first':
        k[:, 0] += lift * per_logit * u[0]
    elif order == 'rise':
        for t in range((Sk + 31) // 32):
            k[:, 32 * t] += rise * (t + 1) * per_logit * u[0]
    elif order == 'zero':
        q = torch.zeros(B, Sq, D)
    return q.contiguous(), k.contiguous()


@functools.lru_cache(maxsize=None)
def inputs(shape, regime, lift=LIFT, rise=RISE):
    """(q, k, v, dO) of a case: fp32 on the CPU, shared by every test of the case; nobody writes to them."""
    B, Sq, Sk, D, heads = shape
    g = torch.Generator().manual_seed(sum(a * b for a, b in zip(shape, (1000003, 10007, 101, 7, 1))) +
                                       104729 * (REGIMES + [WIDE_VDO] + ORDERINGS).index(regime))
    v = torch.randn(B, Sk, D, generator=g)
    gy = torch.randn(B, Sq, D, generator=g)
    if regime in ORDERINGS:
        q, k = _unit_queries_and_lifted_keys(g, B, Sq, Sk, D, heads, regime, lift, rise)
    else:
        s = 1.0 if regime == WIDE_VDO else SCALES[REGIMES.index(regime)]
        q, k = torch.randn(B, Sq, D, generator=g) * s, torch.randn(B, Sk, D, generator=g) * s
        if regime == WIDE_VDO:
            v, gy = v * 1e4, gy * 1e-4
    return q, k, v, gy


def keep_mask(B, heads, Sq, Sk, p, seed):
    """The boolean [B, heads, Sq, Sk] dropout mask of the kernels: element ((b heads + head) Sq + i) Sk + j of the counter-based
    hash (csrc/rih_hash.h through its numpy mirror) is kept where the word is >= p 2^32."""
    from test_gpu_ops import _hash_np
    with np.errstate(over='ignore'):
        keep = _hash_np(seed, np.arange(B * heads * Sq * Sk)) >= np.uint64(int(p * 2 ** 32))
    return torch.from_numpy(keep.reshape(B, heads, Sq, Sk))


def _mha(dtype, q, k, v, gy, heads, keep, p):
    B, Sq, D = q.shape
    d = D // heads
    ts = [t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v)]
    qq, kk, vv = (t.view(B, -1, heads, d).transpose(1, 2) for t in ts)
    s = (qq @ kk.transpose(-1, -2)) / math.sqrt(d)                  # alpha s
    a = torch.softmax(s, -1)
    if keep is not None:
        a = a * keep.to(dtype) / (1.0 - p)
    out = (a @ vv).transpose(1, 2).reshape(B, Sq, D)
    grads = [None, None, None]
    if gy is not None:
        out.backward(gy.to(dtype))
        grads = [t.grad for t in ts]
    s = s.detach()
    lse2 = torch.logsumexp(s, -1) * LOG2E                           # log2 sum_j 2^(alpha log2e s_ij), [B, heads, Sq]
    return out.detach(), grads[0], grads[1], grads[2], lse2, float(s.abs().max())


def ref64(q, k, v, gy, heads, keep=None, p=0.0):
    """out, dq, dk, dv, lse2, Lmax of multi-head attention in torch.float64 autograd (gy None: forward only)."""
    return _mha(torch.float64, q, k, v, gy, heads, keep, p)


def ref32(q, k, v, gy, heads, keep=None, p=0.0):
    """The same arithmetic in torch.float32 on the CPU: it only sizes the bar."""
    return _mha(torch.float32, q, k, v, gy, heads, keep, p)


NAMES = ('out', 'dq', 'dk', 'dv')
Ref = namedtuple('Ref', 'out dq dk dv lse2 Lmax e32 lse2_32 keep')


def rel_err(x, x64):
    return float((x.double() - x64).abs().max()) / float(x64.abs().max())


def make_ref(q, k, v, gy, heads, keep=None, p=0.0):
    r64 = ref64(q, k, v, gy, heads, keep, p)
    r32 = ref32(q, k, v, gy, heads, keep, p)
    e32 = max([rel_err(a, b) for a, b in zip(r32[:4], r64[:4]) if a is not None and float(b.abs().max()) > 0.0] or [0.0])
    return Ref(*r64, e32, r32[4], keep)


@functools.lru_cache(maxsize=None)
def reference(shape, regime, p=0.0, seed=0):
    """The Ref of a case of the table, computed once."""
    B, Sq, Sk, D, heads = shape
    q, k, v, gy = inputs(shape, regime)
    return make_ref(q, k, v, gy, heads, keep_mask(B, heads, Sq, Sk, p, seed) if p > 0 else None, p)


@functools.lru_cache(maxsize=None)
def forward_reference(shape, order):
    """An ordering at the full lift (FWD_LIFT): inputs and the forward-only Ref (out, lse2)."""
    q, k, v, _ = inputs(shape, order, FWD_LIFT, RISE)
    return (q, k, v), make_ref(q, k, v, None, shape[4])


def bar(ref):
    return FACTOR * max(ref.e32, U * (1.0 + ref.Lmax))


def zero_reference_bound(name, q, k, v, gy, heads):
    """Bound on |dq| (|dk|) where the fp64 reference is identically zero: see the module's docstring."""
    B, Sq, D = q.shape
    d = D // heads
    split = lambda t: t.double().abs().view(B, -1, heads, d).transpose(1, 2)
    dov = float((split(gy) @ split(v).transpose(-1, -2)).max())            # max_ij sum_c |dO_ic| |v_jc|
    other = k if name == 'dq' else q
    return 2.0 * d * U * dov * float(other.abs().max()) / math.sqrt(d)


def check_bar(got, ref, what, inp=None, heads=None, names=NAMES):
    """got: the kernel's tensors in the order of `names`.  Prints e(got), e32, Lmax and e(got) / max(e32, 2^-24 (1 + Lmax)) for each
    of them, then asserts the bar (ratio <= 8), or the zero-reference rule where the reference is identically zero."""
    base = max(ref.e32, U * (1.0 + ref.Lmax))
    bad = []
    for name, a in zip(names, got):
        x64 = getattr(ref, name)
        a = a.detach().double().cpu()
        assert a.shape == x64.shape and bool(torch.isfinite(a).all()), (what, name, tuple(a.shape))
        if float(x64.abs().max()) == 0.0:
            assert name in ('dq', 'dk') and inp is not None, (what, name)
            bound, worst = zero_reference_bound(name, *inp, heads), float(a.abs().max())
            print('FLASH-EDGE %s %s zero-reference max|got| %.3e bound %.3e' % (what, name, worst, bound))
            if not worst <= bound:
                bad.append((name, 'zero reference', worst, bound))
            continue
        e = rel_err(a, x64)
        print('FLASH-EDGE %s %s e %.3e e32 %.3e Lmax %.4g ratio %.3f' % (what, name, e, ref.e32, ref.Lmax, e / base))
        if not e <= FACTOR * base:
            bad.append((name, e, FACTOR * base))
    assert not bad, (what, bad)


def check_lse(lse, ref, what):
    """|lse - lse2| <= 8 max(|lse2_32 - lse2|, 2^-24 max(1, |lse2|)) elementwise; lse2_32 = torch's fp32 value of the same word."""
    lse = lse.detach().double().cpu().reshape(ref.lse2.shape)
    assert bool(torch.isfinite(lse).all()), what
    err = (lse - ref.lse2).abs()
    tol = FACTOR * torch.maximum((ref.lse2_32.double() - ref.lse2).abs(), U * ref.lse2.abs().clamp(min=1.0))
    print('FLASH-EDGE %s lse max err %.3e worst err/tol %.3f max|lse2| %.4g' % (
        what, float(err.max()), float((err / tol).max()), float(ref.lse2.abs().max())))
    assert bool((err <= tol).all()), (what, float((err / tol).max()))


def measure(shape, scale, run):
    """One printed figure outside the asserted range (scale 100): run(q, k, v, gy, heads) -> (out, dq, dk, dv)."""
    B, Sq, Sk, D, heads = shape
    g = torch.Generator().manual_seed(31)
    q, k = torch.randn(B, Sq, D, generator=g) * scale, torch.randn(B, Sk, D, generator=g) * scale
    v, gy = torch.randn(B, Sk, D, generator=g), torch.randn(B, Sq, D, generator=g)
    r64, r32 = ref64(q, k, v, gy, heads), ref32(q, k, v, gy, heads)
    got = run(q, k, v, gy, heads)
    for name, a, b, c in zip(NAMES, got, r32[:4], r64[:4]):
        print('FLASH-RANGE %s qk%g %s e(got) %.3e e(torch fp32) %.3e Lmax %.4g' % (
            'x'.join(map(str, shape)), scale, name, rel_err(a.detach().cpu(), c), rel_err(b, c), r64[5]))
