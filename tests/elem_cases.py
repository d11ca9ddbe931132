"""Case tables, input builders, the fp64 references and the bar of the edge tests of csrc/rih_elem.hip: LayerNorm, softmax
(+ dropout), max and average pooling, the Chebyshev feature build and row gather / scatter (tests/test_gpu_elem_edges.py on
the GPU, tests/test_kernels_on_cpu.py on the host build; tests/test_elem_cases.py checks the tables themselves).  No GPU is
touched here.

The bar.  For one case let e(x) = max|x - x64| / max|x64| per tensor against torch.float64 autograd,
and e32 = the largest e() over the asserted tensors of the same arithmetic in torch.float32 on the CPU.  A kernel tensor
passes if

    e(got) <= 8 * max(e32, 2^-23).

8 is flash_cases.FACTOR, the project's margin for a different summation order; 2^-23 is one rounding of an input plus one of
the output and keeps the bar from collapsing where torch happens to be exact.  Every asserted case has e32 <= CAP = 1.25e-4
(tests/test_elem_cases.py), so the bar never exceeds 1e-3: a dropped element, a wrong neighbour, a wrong divisor or a
mis-indexed tail costs 1e-3 or more.

Not asserted, on purpose: LayerNorm at an offset of 1e4 over unit spread (torch fp32 itself misses fp64 by up to 1e-3: the
variance of numbers near 1e4 has lost 2^-24 * 1e8 = 6 of its value) and the softmax backward at logit scales 30 and 1e3 (rows
saturate, the gradient is a difference of nearly equal numbers: e32 reaches 3e-4 and 1.0).  Those tensors are printed with
their own e32 and never compared.  The softmax forward is asserted at every scale."""
import functools
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from flash_cases import FACTOR

U23 = 2.0 ** -23
CAP = 1.25e-4
EPS = 1e-6                  # of every LayerNorm here (the decoder's)
ALPHA = 0.125               # of the softmax backward: dS = alpha P (dP - sum dP P); a power of two, so it adds no rounding
DROP_P, DROP_SEED = 0.25, 0x1234567


def _gen(family, case):
    return torch.Generator().manual_seed(zlib.crc32(repr((family, case)).encode()))


def rel_err(x, x64):
    return float((x.double() - x64).abs().max()) / float(x64.abs().max())


def case_id(case):
    return '-'.join('x'.join(str(v) for v in p) if isinstance(p, tuple) else ('%g' % p if isinstance(p, float) else str(p))
                    for p in case if p != '')


class Ref:
    """x64: name -> fp64 tensor; e32_each: name -> e() of torch fp32; e32: the largest of them over `asserted`; exact_zero: the
    names whose reference is identically zero and whose kernel value must be exactly zero."""

    def __init__(self, r64, r32, asserted=None, exact_zero=()):
        self.x64 = r64
        self.asserted = tuple(r64) if asserted is None else tuple(asserted)
        self.exact_zero = tuple(exact_zero)
        self.e32_each = {n: (0.0 if float(r64[n].abs().max()) == 0.0 else rel_err(r32[n], r64[n])) for n in r64}
        self.e32 = max([self.e32_each[n] for n in self.asserted] or [0.0])

    def bar(self):
        return FACTOR * max(self.e32, U23)


def make_ref(fn, asserted=None, exact_zero=()):
    """fn(dtype) -> name -> tensor, once in float64 and once in float32 (which only sizes the bar)."""
    return Ref(fn(torch.float64), fn(torch.float32), asserted, exact_zero)


def check_bar(what, got, ref):
    """got: name -> the kernel's tensor.  One ELEM-EDGE line per tensor, then the bar on the asserted ones."""
    base = max(ref.e32, U23)
    bad = []
    for name, x64 in ref.x64.items():
        a = got[name].detach().double().cpu().reshape(x64.shape)
        assert bool(torch.isfinite(a).all()), (what, name, 'not finite')
        if float(x64.abs().max()) == 0.0:
            worst = float(a.abs().max())
            print('ELEM-EDGE %s %s zero-reference max|got| %.3e' % (what, name, worst))
            assert name in ref.exact_zero, (what, name, 'a zero reference the case does not announce')
            if worst != 0.0:
                bad.append((name, 'must be exactly zero', worst))
            continue
        e = rel_err(a, x64)
        if name in ref.asserted:
            print('ELEM-EDGE %s %s e %.3e e32 %.3e ratio %.3f' % (what, name, e, ref.e32, e / base))
            if not e <= FACTOR * base:
                bad.append((name, e, FACTOR * base))
        else:
            print('ELEM-EDGE %s %s e %.3e e32 %.3e (its own) not asserted' % (what, name, e, ref.e32_each[name]))
    assert not bad, (what, bad)


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
# (rows, D).  The 16-byte kernels exist for D = 64 / 128 / 256 / 512 / 1024 and take 4, 2 or 1 rows per wavefront: 1, 5, 17 rows
# leave a ragged last row group.  Everything else is the generic kernel (one row per wavefront, 64 lanes x up to 16 elements).
LN_VEC_SHAPES = [(1, 64), (5, 64), (17, 128), (3, 256), (9, 512), (2, 1024)]
LN_GENERIC_SHAPES = [(1, 3), (4, 65), (5, 200), (2, 1023)]
LN_REGIMES = {'off0': (0.0, 1.0), 'off1e2': (1e2, 1.0), 'off1e3': (1e3, 1.0), 'sp1e-3': (0.0, 1e-3), 'sp1e3': (0.0, 1e3)}
LN_UNASSERTED_REGIMES = {'off1e4': (1e4, 1.0)}
LN_SWITCHES = ['x2', 'relu', 'skip', 'x2+relu+skip']
# a case: (rows, D, regime, switches)
LN_CASES = [(r, d, reg, '') for (r, d) in LN_VEC_SHAPES + LN_GENERIC_SHAPES for reg in LN_REGIMES]
LN_SWITCH_CASES = [(r, d, reg, sw) for (r, d) in ((5, 64), (5, 200)) for sw in LN_SWITCHES for reg in ('off0', 'off1e2')
                   if reg == 'off0' or 'relu' not in sw]
LN_PAIR_CASES = [(5, 64, 'off1e2', 'pair'), (3, 200, 'off1e2', 'pair')]
LN_MISALIGNED_CASES = [(5, 64, 'off1e2', ''), (3, 256, 'off1e3', ''), (5, 64, 'off0', 'x2+relu+skip')]
LN_MEASURED_CASES = [(3, 256, 'off1e4', ''), (5, 200, 'off1e4', '')]          # printed, nothing asserted


@functools.lru_cache(maxsize=None)
def ln_inputs(case):
    """x (and x2), gamma, beta, the gradient of y and the gradient that arrives over the skip connection; for a 'pair' case a
    leading dimension of two hands and [2][D] parameters.  Shared by every test of the case; nobody writes to them."""
    rows, D, regime, sw = case
    off, spread = dict(LN_REGIMES, **LN_UNASSERTED_REGIMES)[regime]
    g = _gen('ln', case)
    lead = (2,) if sw == 'pair' else ()
    rn = lambda *s: torch.randn(*s, generator=g)
    inp = dict(x=rn(*lead, rows, D) * spread + off, x2=None, dres=None,
               g=torch.rand(*lead, D, generator=g) + 0.5, b=rn(*lead, D) * 0.1, gy=rn(*lead, rows, D))
    if 'x2' in sw:
        inp['x2'] = rn(rows, D) * spread * 0.5
    if 'skip' in sw:
        inp['dres'] = rn(rows, D)
    return inp


def _ln_run(dtype, x, x2, g, b, gy, dres, relu):
    xs, gs, bs = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, g, b))
    t = xs if x2 is None else xs + x2.to(dtype)
    y = F.layer_norm(t, (x.shape[-1],), gs, bs, EPS)
    if relu:
        y = torch.relu(y)
    loss = (y * gy.to(dtype)).sum()
    if dres is not None:
        loss = loss + (xs * dres.to(dtype)).sum()
    loss.backward()
    return dict(y=y.detach(), dx=xs.grad, dg=gs.grad, db=bs.grad)


@functools.lru_cache(maxsize=None)
def ln_reference(case):
    inp, sw = ln_inputs(case), case[3]

    def fn(dtype):
        if sw != 'pair':
            return _ln_run(dtype, inp['x'], inp['x2'], inp['g'], inp['b'], inp['gy'], inp['dres'], 'relu' in sw)
        hands = [_ln_run(dtype, inp['x'][h], None, inp['g'][h], inp['b'][h], inp['gy'][h], None, False) for h in (0, 1)]
        return {n: torch.stack([hands[0][n], hands[1][n]]) for n in hands[0]}
    return make_ref(fn, asserted=() if case[2] in LN_UNASSERTED_REGIMES else None)


# --------------------------------------------------------------------------------------------------------------------- softmax
# (rows, cols, ld).  16-byte forms (cols % 4 == 0, ld % 4 == 0): one column quad per lane up to 256 columns, two up to 512, four
# up to 1024; everything else is the generic kernel.  A workgroup owns four rows: with five the second holds one.
SM_SHAPES = [(1, 1, 1), (6, 4, 8), (3, 256, 256), (2, 260, 264), (3, 516, 516), (2, 768, 1024), (5, 1024, 1024), (5, 513, 513),
             (5, 1023, 1024), (5, 127, 128)]
SM_SCALES = [1e-3, 1.0, 8.0, 30.0, 1e3]
SM_BWD_MAX_SCALE = 8.0                                  # the backward is asserted up to here; beyond, see the module docstring
# a case: (rows, cols, ld, scale, drop_p)
SM_CASES = [(r, c, ld, s, 0.0) for (r, c, ld) in SM_SHAPES for s in SM_SCALES]
SM_DROPOUT_CASES = [(3, 516, 516, 1.0, DROP_P), (5, 127, 128, 1.0, DROP_P)]
SM_MASK_TWIN = ((3, 516, 516, 1.0, DROP_P), 517)        # the same rows at an odd pitch: the scalar kernel, the same mask


@functools.lru_cache(maxsize=None)
def sm_inputs(case):
    rows, cols, ld, scale, p = case
    g = _gen('sm', (rows, cols, scale))                 # not the pitch: a twin at another pitch has the same values
    return dict(S=torch.randn(rows, cols, generator=g) * scale, dP=torch.randn(rows, cols, generator=g))


def sm_keep(case):
    """The boolean [rows, cols] dropout mask: element r cols + j of the counter-based hash is kept where the word is >= p 2^32."""
    from test_gpu_ops import _hash_np
    rows, cols, ld, scale, p = case
    with np.errstate(over='ignore'):
        keep = _hash_np(DROP_SEED, np.arange(rows * cols)) >= np.uint64(int(p * 2 ** 32))
    return torch.from_numpy(keep.reshape(rows, cols))


@functools.lru_cache(maxsize=None)
def sm_reference(case):
    rows, cols, ld, scale, p = case
    inp = sm_inputs(case)
    keep = sm_keep(case) if p > 0 else None

    def fn(dtype):
        S = inp['S'].to(dtype).clone().requires_grad_(True)
        P = torch.softmax(S, -1)
        Pd = P if keep is None else P * keep.to(dtype) / (1.0 - p)
        (Pd * inp['dP'].to(dtype)).sum().backward()
        out = dict(P=P.detach(), dS=ALPHA * S.grad)
        if keep is not None:
            out['Pd'] = Pd.detach()
        return out
    names = ['P'] + (['Pd'] if p > 0 else []) + (['dS'] if scale <= SM_BWD_MAX_SCALE else [])
    return make_ref(fn, asserted=names, exact_zero=('dS',) if cols == 1 else ())        # one column: P = 1, dS = 0 exactly


# ------------------------------------------------------------------------------------------------------------------- Chebyshev
# (V, F, B) on a synthetic CSR: row v has v % 10 neighbours with randn weights -- empty rows and rows of 1..9 neighbours, so the
# four-at-a-time loop of the gather form sees every tail.  LDS form: F % 4 == 0 and V <= 256 (V = 256 fills the staging loop
# exactly, F = 20 leaves a partial last slice of channel quads); gather form: V = 257, 300; scalar form: F = 6.
CH_CASES = [(256, 8, 2), (257, 8, 2), (1, 4, 1), (256, 20, 1), (40, 6, 2), (300, 4, 1)]
CH_MISALIGNED_CASE = (40, 8, 2)
CH_TWIN = (2, 4, 65536)         # B > 65535 leaves the LDS form; its two halves of 32768 take it: bit-identical


def ch_matrix(V):
    """The dense [V][V] float32 operator: row v holds v % 10 (at most V) randn weights at distinct random columns."""
    rs = np.random.RandomState(1000 + V)
    M = np.zeros((V, V), np.float32)
    for v in range(V):
        deg = min(v % 10, V)
        M[v, rs.choice(V, size=deg, replace=False)] = rs.randn(deg).astype(np.float32)
    return M


def csr_of(M):
    """(indptr, indices, vals) of a dense matrix, columns ascending, as int32 / int32 / float32 tensors."""
    rows, cols = np.nonzero(M)
    indptr = np.zeros(M.shape[0] + 1, np.int32)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=M.shape[0]))
    return (torch.from_numpy(indptr), torch.from_numpy(cols.astype(np.int32)), torch.from_numpy(M[rows, cols].astype(np.float32)))


@functools.lru_cache(maxsize=None)
def ch_inputs(case):
    V, Fd, B = case
    g = _gen('ch', case)
    M = ch_matrix(V)
    return dict(M=M, csr=csr_of(M), csr_t=csr_of(np.ascontiguousarray(M.T)), x=torch.randn(B, V, Fd, generator=g),
                gy=torch.randn(B, V, 2 * Fd, generator=g))


@functools.lru_cache(maxsize=None)
def ch_reference(case):
    inp = ch_inputs(case)

    def fn(dtype):
        x = inp['x'].to(dtype).clone().requires_grad_(True)
        L = torch.from_numpy(inp['M']).to(dtype)
        y = torch.stack((x, torch.matmul(L, x)), -1).flatten(-2)            # (x, L x) interleaved on the feature dimension
        y.backward(inp['gy'].to(dtype))
        return dict(y=y.detach(), dx=x.grad)
    return make_ref(fn)


def ch_twin_inputs():
    """The bit-identity problem: V = 2 with a dense 2 x 2 operator (two neighbours per row, so every sum has an order)."""
    V, Fd, B = CH_TWIN
    g = _gen('ch', CH_TWIN)
    M = np.array([[0.75, -1.5], [0.3, 2.25]], np.float32)
    return dict(M=M, csr=csr_of(M), csr_t=csr_of(np.ascontiguousarray(M.T)), x=torch.randn(B, V, Fd, generator=g),
                gy=torch.randn(B, V, 2 * Fd, generator=g))


# -------------------------------------------------------------------------------------------------------------- gather / scatter
# (index name, D) at Vin = 7, B = 2.  'crafted': rows 0 and 2 are read three times, rows 1 and 4 never (an empty inv_ptr range).
GS_VIN, GS_B = 7, 2
GS_INDEX = {'crafted': [0, 2, 0, 3, 2, 5, 0, 6, 2, 5], 'one': [3]}
GS_CASES = [(name, D) for name in GS_INDEX for D in (1, 3, 4, 130)]


@functools.lru_cache(maxsize=None)
def gs_inputs(case):
    name, D = case
    g = _gen('gs', case)
    return dict(idx=GS_INDEX[name], x=torch.randn(GS_B, GS_VIN, D, generator=g),
                gy=torch.randn(GS_B, len(GS_INDEX[name]), D, generator=g))


def gs_unread(case):
    return sorted(set(range(GS_VIN)) - set(GS_INDEX[case[0]]))


@functools.lru_cache(maxsize=None)
def gs_reference(case):
    inp = gs_inputs(case)

    def fn(dtype):
        x = inp['x'].to(dtype).clone().requires_grad_(True)
        y = x[:, torch.tensor(inp['idx'])]
        y.backward(inp['gy'].to(dtype))
        return dict(y=y.detach(), dx=x.grad)
    return make_ref(fn)


# --------------------------------------------------------------------------------------------------------------------- pooling
# (N, H, W, C) x input.  3 x 3 windows, stride 2, padding 1; C % 4 == 0 takes the 16-byte form.
MP_SHAPES = [(1, 1, 1, 4), (1, 2, 2, 6), (1, 3, 3, 4), (2, 7, 5, 8), (1, 5, 8, 3)]
MP_INPUTS = ['ties', 'neg', 'const']
MP_CASES = [(s, k) for s in MP_SHAPES for k in MP_INPUTS]
MP_CONST = 0.75
AP_CASES = [(1, 1, 1, 6), (2, 3, 5, 10), (1, 8, 8, 4), (3, 7, 7, 33)]


@functools.lru_cache(maxsize=None)
def mp_inputs(case):
    """x as NCHW and the gradient of the pooled map.  'ties': relu(round(2 x) / 2), what the pool sees behind a ReLU -- many zeros,
    whole windows that tie; 'neg': the same map minus (its maximum + 1), all <= -1 with the
    same ties, so a padding tap that counted as 0 would win every border window; 'const': one value everywhere."""
    (N, H, W, Cc), kind = case
    g = _gen('mp', case[0])                             # per shape: 'neg' is 'ties' shifted
    x = torch.relu(torch.round(torch.randn(N, Cc, H, W, generator=g) * 2) / 2)
    if kind == 'neg':
        x = x - (float(x.max()) + 1.0)
    elif kind == 'const':
        x = torch.full_like(x, MP_CONST)
    return dict(x=x, gy=torch.randn(N, Cc, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=g))


@functools.lru_cache(maxsize=None)
def mp_reference(case):
    inp = mp_inputs(case)

    def fn(dtype):
        x = inp['x'].to(dtype).clone().requires_grad_(True)
        y = F.max_pool2d(x, 3, 2, 1)                    # routes a tie to the first tap in (kh, kw) order, as the kernel must
        y.backward(inp['gy'].to(dtype))
        return dict(y=y.detach(), dx=x.grad)
    return make_ref(fn)


def mp_tied_windows(case):
    """(windows whose maximum is reached by two or more taps, windows) of a case's input."""
    x = mp_inputs(case)['x']
    cols = F.unfold(F.pad(x, (1, 1, 1, 1), value=float('-inf')), 3, stride=2)       # [N, C 9, L]
    cols = cols.view(x.shape[0], x.shape[1], 9, -1)
    tied = (cols == cols.max(2, keepdim=True).values).sum(2) >= 2
    return int(tied.sum()), tied.numel()


@functools.lru_cache(maxsize=None)
def ap_inputs(case):
    N, H, W, Cc = case
    g = _gen('ap', case)
    return dict(x=torch.randn(N, Cc, H, W, generator=g) + 100.0, gy=torch.randn(N, Cc, generator=g))


@functools.lru_cache(maxsize=None)
def ap_reference(case):
    inp = ap_inputs(case)

    def fn(dtype):
        x = inp['x'].to(dtype).clone().requires_grad_(True)
        y = F.adaptive_avg_pool2d(x, 1).flatten(1)
        y.backward(inp['gy'].to(dtype))
        return dict(y=y.detach(), dx=x.grad)
    return make_ref(fn)


FAMILIES = {
    'layernorm': (LN_CASES + LN_SWITCH_CASES + LN_PAIR_CASES + LN_MISALIGNED_CASES + LN_MEASURED_CASES, ln_reference),
    'softmax': (SM_CASES + SM_DROPOUT_CASES, sm_reference),
    'cheby': (CH_CASES + [CH_MISALIGNED_CASE], ch_reference),
    'gather': (GS_CASES, gs_reference),
    'maxpool': (MP_CASES, mp_reference),
    'avgpool': (AP_CASES, ap_reference),
}
