"""The three passes that only move weights or weight gradients -- the split-K slab reduction (rih_splitk_reduce_multi,
rih_splitk_reduce_bias, rih_splitk_reduce_bias_batched), the weight repack (rih_pack_conv_weight_multi) and the H2 weight planes
(rih_h2_multi) -- each on its wide kernel and on its reference kernel (descriptor field `reserved` != 0).

Every comparison is BITWISE.  The reduction is compared with an exact-order float32 restatement of its contract (reduce_numpy:
four accumulators from 0.f, a_j takes k = j mod 4 in increasing k below 4 floor(S / 4), the tail goes into a0,
(a0 + a1) + (a2 + a3), then dst + v when accumulating; the bias row on two accumulators, even / odd k, tail into s0) and with the
reference kernel; the repack with the numpy maps of tests/abi_emulator.py and with the reference kernel; the H2 planes with the
reference kernel.  Every output buffer carries a poison value behind and between its extents, which must survive.

The check_* functions also run on the host-compiled kernels (tests/test_weight_passes_on_cpu.py), which replace dev()."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = np.float32(-7.25e30)
F32 = np.float32
REDUCE_PACK = 56            # descriptors per launch of rih_splitk_reduce_multi / rih_pack_conv_weight_multi
S_VALUES = (1, 2, 3, 4, 5, 8, 9, 13)
S_DEEP = (32, 35, 44, 67)       # from S = 32 the four partial sums of an element sit on four lanes: 1, 1 + 3 and 2 rounds of 8 loads, tails
GEOMETRIES = ((1, 8, 8), (1, 12, 11), (9, 8, 8), (9, 32, 32), (49, 4, 3))      # (taps, Cin, CinValid); M = taps * Cin: 72, 288, ...
N_WIDE, N_FALLBACK = (4, 8, 68, 132), (3, 33)
MAGNITUDES = (1e-3, 1.0, 1e3)


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _lib():
    from renderih_amd import ops
    return ops._L(), ops._stream()


def _sync():
    if dev().type == 'cuda':
        torch.cuda.synchronize()


def _up(a, offset=0):
    """numpy array -> tensor on dev() (a private copy), `offset` floats into a larger allocation when the test wants it unaligned"""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1).copy())
    if offset:
        buf = torch.empty(flat.numel() + offset, dtype=flat.dtype).to(dev())
        buf[offset:] = flat.to(dev())
        return buf[offset:]
    return flat.to(dev()).clone()


def _down(t):
    return t.cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------ split-K reduction
def reduce_numpy(P, M, has_bias):
    """(weight-gradient sums [M][N], bias row [N] or None) of slabs P [S][Mp][N] in the kernels' order, in float32"""
    S = P.shape[0]
    a = [np.zeros(P.shape[1:], F32)[:M] for _ in range(4)]
    s4 = 4 * (S // 4)
    for k in range(s4):
        a[k % 4] = a[k % 4] + P[k, :M]
    for k in range(s4, S):
        a[0] = a[0] + P[k, :M]
    v = (a[0] + a[1]) + (a[2] + a[3])
    b = None
    if has_bias:
        s = [np.zeros(P.shape[2], F32), np.zeros(P.shape[2], F32)]
        s2 = 2 * (S // 2)
        for k in range(s2):
            s[k % 2] = s[k % 2] + P[k, M]
        if s2 < S:
            s[0] = s[0] + P[S - 1, M]
        b = s[0] + s[1]
    assert v.dtype == F32
    return v, b


def reduce_expected(case, P, init):
    """the whole dst buffer after the reduction: parameter layout [N][pitch][taps], first CinValid columns of every n written"""
    S, taps, cin, cv, N, has_bias, acc, pitch = case
    M = taps * cin
    v, b = reduce_numpy(P, M, has_bias)
    out = init.copy()
    p = pitch or cv
    m = np.arange(M)
    tap, ci = m // cin, m % cin
    ok = ci < cv
    o = ((np.arange(N)[None, :] * p + ci[ok][:, None]) * taps + tap[ok][:, None]).ravel()
    out[o] = (out[o] + v[ok].ravel()) if acc else v[ok].ravel()
    return out, b


def reduce_problem(case, seed):
    """slabs, the initial dst buffer (random inside the written extents' rows, POISON between the column slices and behind) and the
    expected results"""
    S, taps, cin, cv, N, has_bias, acc, pitch = case
    rs = np.random.RandomState(seed)
    M = taps * cin
    Mp = M + 4 if has_bias else M
    P = (rs.randn(S, Mp, N) * MAGNITUDES[seed % 3]).astype(F32)
    p = pitch or cv
    init = np.full(N * p * taps + 16, POISON, F32)
    body = init[:N * p * taps].reshape(N, p, taps)
    body[:, :cv, :] = (rs.randn(N, cv, taps) * MAGNITUDES[seed % 3]).astype(F32)
    exp, b = reduce_expected(case, P, init)
    return P, Mp, init, exp, b


def reduce_cases():
    """S x geometry x N in full with the flags (bias row, accumulate, CinPitch) cycling, geometry x N x flags in full with S
    cycling, and S_DEEP x geometry x N with the flags cycling"""
    cases = []
    flags = list(itertools.product((False, True), (0, 1), (False, True)))
    i = 0
    for S, (taps, cin, cv), N in itertools.product(S_VALUES, GEOMETRIES, N_WIDE + N_FALLBACK):
        hb, acc, wide_pitch = flags[i % 8]
        cases.append((S, taps, cin, cv, N, hb, acc, cv + 8 if wide_pitch else 0))
        i += 3
    for (taps, cin, cv), N, (hb, acc, wide_pitch) in itertools.product(GEOMETRIES, N_WIDE + N_FALLBACK, flags):
        cases.append((S_VALUES[i % len(S_VALUES)], taps, cin, cv, N, hb, acc, cv + 8 if wide_pitch else 0))
        i += 1
    for S, (taps, cin, cv), N in itertools.product(S_DEEP, GEOMETRIES, N_WIDE + N_FALLBACK):
        hb, acc, wide_pitch = flags[i % 8]
        cases.append((S, taps, cin, cv, N, hb, acc, cv + 8 if wide_pitch else 0))
        i += 3
    return cases


def run_reduce_multi(cases, problems, reference, misalign=False):
    """one rih_splitk_reduce_multi call over `cases`; returns [(dst buffer, bias gradient incl. its poison tail)]"""
    from renderih_amd._lib import ReduceDesc
    lib, stream = _lib()
    n = len(cases)
    arr = (ReduceDesc * n)()
    keep = []
    for a, case, (P, Mp, init, _, _) in zip(arr, cases, problems):
        S, taps, cin, cv, N, has_bias, acc, pitch = case
        tP, tD, tB = _up(P, 1 if misalign else 0), _up(init), _up(np.full(N + 8, POISON, F32))
        keep.append((tP, tD, tB))
        a.P, a.dst, a.db = tP.data_ptr(), tD.data_ptr(), (tB.data_ptr() if has_bias else 0)
        a.S, a.Mp, a.M, a.N, a.Cin, a.taps, a.CinValid, a.accumulate = S, Mp, taps * cin, N, cin, taps, cv, acc
        a.CinPitch, a.reserved = pitch, (1 if reference else 0)
    assert lib.rih_splitk_reduce_multi(arr, n, stream) == 0
    _sync()
    return [(_down(tD), _down(tB)) for _, tD, tB in keep]


def check_reduce_outputs(cases, problems, outs, what):
    for case, (_, _, _, exp, b), (dst, db) in zip(cases, problems, outs):
        N, has_bias = case[4], case[5]
        assert np.array_equal(dst, exp), (what, case, int((dst != exp).sum()))
        if has_bias:
            assert np.array_equal(db[:N], b), (what, 'bias row', case)
            assert (db[N:] == POISON).all(), (what, 'behind the bias gradient', case)
        else:
            assert (db == POISON).all(), (what, 'bias gradient without a bias row', case)


def check_reduce_multi():
    """all cases, in lists of several packs, on the wide dispatch and forced onto the reference kernel"""
    cases = reduce_cases()
    problems = [reduce_problem(c, i) for i, c in enumerate(cases)]
    for reference in (False, True):
        outs = run_reduce_multi(cases, problems, reference)
        check_reduce_outputs(cases, problems, outs, 'reference kernel' if reference else 'wide dispatch')
    return len(cases)


def check_reduce_list_lengths():
    """descriptor lists of 1, one full pack and one pack + 1: every descriptor of every list is reduced, once"""
    base = [c for c in reduce_cases() if c[0] in (3, 5)][:REDUCE_PACK + 1]
    assert len(base) == REDUCE_PACK + 1
    problems = [reduce_problem(c, 1000 + i) for i, c in enumerate(base)]
    for n in (1, REDUCE_PACK, REDUCE_PACK + 1):
        outs = run_reduce_multi(base[-n:], problems[-n:], False)
        check_reduce_outputs(base[-n:], problems[-n:], outs, 'list of %d' % n)


def check_reduce_unaligned():
    """P one float off a 16-byte boundary at N % 4 == 0: the reference kernel takes it, same bits"""
    cases = [(S, taps, cin, cv, N, hb, acc, pitch) for (S, (taps, cin, cv), N, (hb, acc, pitch)) in
             zip((3, 4, 5, 9, 13), GEOMETRIES, (8, 68, 132, 4, 68), ((True, 0, 0), (False, 1, 19), (True, 1, 0), (False, 0, 40), (True, 0, 11)))]
    problems = [reduce_problem(c, 2000 + i) for i, c in enumerate(cases)]
    outs = run_reduce_multi(cases, problems, False, misalign=True)
    check_reduce_outputs(cases, problems, outs, 'P + 1 float')


def check_reduce_plain_entry_points():
    """rih_splitk_reduce_bias and rih_splitk_reduce_bias_batched (two slices; slab stride a multiple of four floats -> wide kernel,
    one float more -> reference kernel) against the restatement"""
    lib, stream = _lib()
    for i, (S, (taps, cin, cv), N, has_bias, acc) in enumerate(((3, (9, 8, 8), 68, True, 0), (8, (1, 12, 11), 132, False, 1),
                                                                (5, (49, 4, 3), 8, True, 1), (4, (9, 32, 32), 33, True, 0),
                                                                (41, (9, 8, 8), 68, True, 1))):
        case = (S, taps, cin, cv, N, has_bias, acc, 0)
        for gap in (0, 1):
            probs = [reduce_problem(case, 3000 + 10 * i + b) for b in range(2)]
            Mp = probs[0][1]
            sP, sD = S * Mp * N + gap, probs[0][2].size
            slabs = np.full(2 * sP, POISON, F32)
            for b in range(2):
                slabs[b * sP:b * sP + S * Mp * N] = probs[b][0].ravel()
            tP, tD = _up(slabs), _up(np.concatenate([p[2] for p in probs]))
            tB = _up(np.full(2 * (N + 8), POISON, F32))
            assert lib.rih_splitk_reduce_bias_batched(tP.data_ptr(), S, Mp, taps * cin, N, tD.data_ptr(), cin, taps, cv, acc,
                                                      tB.data_ptr() if has_bias else 0, 2, sP, sD, N + 8, stream) == 0
            _sync()
            dst, db = _down(tD).reshape(2, sD), _down(tB).reshape(2, N + 8)
            check_reduce_outputs([case, case], probs, [(dst[b], db[b]) for b in range(2)], 'batched, gap %d' % gap)
        P, Mp, init, exp, b = reduce_problem(case, 3500 + i)
        tP, tD, tB = _up(P), _up(init), _up(np.full(N + 8, POISON, F32))
        assert lib.rih_splitk_reduce_bias(tP.data_ptr(), S, Mp, taps * cin, N, tD.data_ptr(), cin, taps, cv, acc,
                                          tB.data_ptr() if has_bias else 0, stream) == 0
        _sync()
        check_reduce_outputs([case], [(P, Mp, init, exp, b)], [(_down(tD), _down(tB))], 'rih_splitk_reduce_bias')


# ------------------------------------------------------------------------------------------------ weight repack
PACK_SHAPES = ((8, 3, 7), (20, 9, 3), (64, 64, 3), (40, 36, 1), (3, 8, 2))      # (Cout, Cin, K)


def pack_cases():
    """[(Cout, Cin, KH, KW, CinPad, mode, kh0, kw0, step, Th, Tw)]: mode 0, mode 1 in full, mode 1 on every step-2 tap subset"""
    cases = []
    for Cout, Cin, K in PACK_SHAPES:
        cpad = (Cin + 3) // 4 * 4
        cases.append((Cout, Cin, K, K, cpad, 0, 0, 0, 1, K, K))
        cases.append((Cout, Cin, K, K, cpad, 1, 0, 0, 1, K, K))
        for kh0, kw0 in itertools.product((0, 1), (0, 1)):
            Th, Tw = len(range(kh0, K, 2)), len(range(kw0, K, 2))
            if K > 1 and Th > 0 and Tw > 0:
                cases.append((Cout, Cin, K, K, cpad, 1, kh0, kw0, 2, Th, Tw))
    return cases


def pack_size(f):
    Cout, Cin, KH, KW, cpad, mode, kh0, kw0, step, Th, Tw = f
    return KH * KW * cpad * Cout if mode == 0 else Th * Tw * Cout * cpad


def run_pack(cases, weights, reference):
    from renderih_amd._lib import PackDesc
    lib, stream = _lib()
    n = len(cases)
    arr = (PackDesc * n)()
    keep = []
    for a, f, w in zip(arr, cases, weights):
        tw, td = _up(w), _up(np.full(pack_size(f) + 16, POISON, F32))
        keep.append((tw, td))
        a.w, a.dst = tw.data_ptr(), td.data_ptr()
        (a.Cout, a.Cin, a.KH, a.KW, a.CinPad, a.mode, a.kh0, a.kw0, a.step, a.Th, a.Tw) = f
        a.reserved = 1 if reference else 0
    assert lib.rih_pack_conv_weight_multi(arr, n, stream) == 0
    _sync()
    return [_down(td) for _, td in keep]


def pack_expected(f, w):
    from abi_emulator import EmulatedLib
    Cout, Cin, KH, KW, cpad, mode, kh0, kw0, step, Th, Tw = f
    out = np.full(pack_size(f) + 16, POISON, F32)
    w = np.ascontiguousarray(w)
    emu = EmulatedLib()
    if mode == 0:
        emu.rih_pack_conv_weight(w.ctypes.data, out.ctypes.data, Cout, Cin, KH, KW, cpad, 0, None)
    else:
        emu.rih_pack_conv_weight_sub(w.ctypes.data, out.ctypes.data, Cout, Cin, KH, KW, cpad, kh0, kw0, step, Th, Tw, None)
    return out


def check_pack():
    """every case in lists of 1, a full pack and a pack + 1 (the cases repeated in turn), both kernels, against the numpy maps"""
    base = pack_cases()
    rs = np.random.RandomState(5)
    for n in (1, REDUCE_PACK, REDUCE_PACK + 1):
        cases = [base[(i + n) % len(base)] for i in range(n)]
        weights = [rs.randn(f[0], f[1], f[2], f[3]).astype(F32) for f in cases]
        exp = [pack_expected(f, w) for f, w in zip(cases, weights)]
        for reference in (False, True):
            outs = run_pack(cases, weights, reference)
            for f, e, o in zip(cases, exp, outs):
                assert np.array_equal(o, e), ('reference kernel' if reference else 'wide kernel', n, f, int((o != e).sum()))
    assert len(base) >= 2 * len(PACK_SHAPES) + 4


# ------------------------------------------------------------------------------------------------ H2 weight planes
H2_SHAPES = ((64, 3, 7, 4), (64, 64, 3, 64), (96, 32, 1, 32), (32, 96, 1, 96))      # (Cout, Cin, KH = KW, CinPad)
H2_BOUNDS = (1e-3, 1.0, 300.0)


def h2_cases():
    """[(Cout, Cin, K, CinPad, for_dgrad, Kpad, bound)]; Kpad = K rounded up to 32 (the stem: 196 -> 224) and 32 more"""
    cases = []
    for (Cout, Cin, K, cpad), for_dgrad, extra, bound in itertools.product(H2_SHAPES, (0, 1), (0, 32), H2_BOUNDS):
        kk = K * K * (Cout if for_dgrad else cpad)
        cases.append((Cout, Cin, K, cpad, for_dgrad, (kk + 31) // 32 * 32 + extra, bound))
    return cases


def run_h2(cases, weights, reference):
    from renderih_amd._lib import BOUND_FLOATS, H2Desc
    lib, stream = _lib()
    n = len(cases)
    arr = (H2Desc * n)()
    keep = []
    for a, (Cout, Cin, K, cpad, for_dgrad, kpad, bound), w in zip(arr, cases, weights):
        rows = cpad if for_dgrad else Cout
        # the planes are 2 * rows * Kpad halves = rows * Kpad floats' worth of bytes
        tw, td, tb = _up(w), _up(np.full(rows * kpad + 16, POISON, F32)), _up(np.full(BOUND_FLOATS, bound, F32))
        keep.append((tw, td, tb))
        a.w, a.dst, a.amax = tw.data_ptr(), td.data_ptr(), tb.data_ptr()
        a.Cout, a.Cin, a.KH, a.KW, a.CinPad, a.for_dgrad, a.Kpad = Cout, Cin, K, K, cpad, for_dgrad, kpad
        a.reserved = 1 if reference else 0
    assert lib.rih_h2_multi(arr, n, stream) == 0
    _sync()
    return [_down(td) for _, td, _ in keep]


def check_h2():
    cases = h2_cases()
    assert (64, 3, 7, 4, 0, 224, 1.0) in cases
    rs = np.random.RandomState(9)
    # |w| <= bound, with values down to 2^-12 of it
    weights = [(np.clip(rs.randn(c[0], c[1], c[2], c[2]) / 3.0, -1, 1) * c[6] * 2.0 ** -rs.randint(0, 12)).astype(F32) for c in cases]
    wide, ref = run_h2(cases, weights, False), run_h2(cases, weights, True)
    for c, a, b in zip(cases, wide, ref):
        rows = c[3] if c[4] else c[0]
        assert (b[rows * c[5]:] == POISON).all() and (a[rows * c[5]:] == POISON).all(), ('behind the planes', c)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (c, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
        assert not (b[:rows * c[5]] == POISON).any(), ('planes not written', c)
        # the element map, independently of both kernels: hi + lo / 2048 = scale * w with ONE power-of-two scale (1e-3: a wrong
        # element is off by its whole value; this is no precision check)
        planes = b[:rows * c[5]].view(np.float16).reshape(rows, c[5] // 8, 2, 8).astype(np.float64)
        x = (planes[:, :, 0] + planes[:, :, 1] / 2048.0).reshape(rows, c[5])
        W = np.zeros((c[0], c[3], c[2], c[2]))
        W[:, :c[1]] = weights[cases.index(c)]
        if not c[4]:
            want = W.transpose(0, 2, 3, 1).reshape(c[0], -1)
        else:
            want = W[:, :, ::-1, ::-1].transpose(1, 2, 3, 0).reshape(c[3], -1)
        kk = want.shape[1]
        scale = x[:, :kk][want != 0] / want[want != 0]
        assert scale.size and np.allclose(scale, scale.flat[0], rtol=1e-3, atol=0), ('element map', c)
        assert (x[:, :kk][want == 0] == 0).all() and (x[:, kk:] == 0).all(), ('zero rows / padding', c)


# ------------------------------------------------------------------------------------------------ the tests
def test_reduce_multi_is_bitwise_the_contract_on_both_kernels():
    assert check_reduce_multi() == 8 * 5 * 6 + 5 * 6 * 8 + 4 * 5 * 6


def test_reduce_list_lengths_around_the_pack_size():
    check_reduce_list_lengths()


def test_reduce_unaligned_slabs_take_the_reference_kernel():
    check_reduce_unaligned()


def test_reduce_plain_and_batched_entry_points():
    check_reduce_plain_entry_points()


def test_pack_is_bitwise_the_numpy_maps_on_both_kernels():
    check_pack()


def test_h2_planes_are_bitwise_the_reference_kernel():
    check_h2()
