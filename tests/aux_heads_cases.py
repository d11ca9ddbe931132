"""TEST INFRASTRUCTURE: the cases and bars of the auxiliary heads (renderih_amd.aux_heads, csrc/rih_aux.hip), shared by
tests/test_aux_heads.py (CPU: the torch mirror and the host-compiled kernels) and tests/test_gpu_aux_heads.py (GPU), and the
input builders of tests/golden/make_aux_heads_golden.py.

Bars.  For every compared quantity the fp32 mirror was measured against the fp64 mirror on the CPU over the cases below
(`mirror_errors()`); MIRROR_FP32 holds the figures found, BARS is four times them, and a test asserts that the figures written
here are within a factor 2 of what it finds.  The fused kernels (host-compiled and on the GPU) and the fp32 mirror on the device
are held to BARS against the fp64 mirror and against the fixture.  What each figure measures:
  heatmap   max |value - fp64 value| over a map set (values lie in [0, 1])
  loss      max relative error of the four scalars (total, mask, dense, hms)
  grad      max |g - fp64 g| / max |fp64 g|, per gradient tensor, the worst of the three
  decode    max |coordinate - fp64 coordinate| in pixels
`maxvals` of the decoder is a maximum over the inputs: exact, no bar.  The fp64 mirror is held to the fixture at FP64 (the
reference ran in fp64 on the same fp32-representable inputs), the decoder at half an fp32 ulp of the coordinate on top: the
reference returns its coordinates in float32 (inference.py:39)."""
import functools
import os

import numpy as np
import torch

from renderih_amd import aux_heads as ah

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'aux_heads.npz')

# measured on the CPU (profiles/aux_heads/pytest_cpu.log prints them): fp32 mirror against fp64 mirror
MIRROR_FP32 = {'heatmap': 6.1e-8, 'loss': 8.8e-8, 'grad': 1.3e-7, 'decode': 2.2e-6}
BARS = {k: 4 * v for k, v in MIRROR_FP32.items()}
FP64 = 1e-12

F64, F32 = torch.float64, torch.float32


@functools.lru_cache(None)
def fix():
    return dict(np.load(GOLDEN))


def r32(a):
    """fp64 array of fp32-representable values: the fp64 mirror, the fp32 mirror and the kernels see identical inputs."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def t(a, device='cpu', dtype=F64):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def absmax(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------ heat maps
# (R, J, C, generator sigma, scale): R = 4 and 5 (5: the dword path, R * R % 4 != 0), 64; J = 1, 3, 42; both joint forms;
# scale != 1 with sigma * scale representable in fp32 (the kernel takes the product as one float)
HEATMAP_CASES = [(4, 1, 3, 1, 1), (5, 3, 3, -1, 8), (5, 3, 2, 1, 1.5), (4, 42, 3, 2, 0.75), (64, 3, 2, 2, 0.75),
                 (64, 42, 3, -1, 1), (64, 1, 3, 2, 1)]
FIXTURE_HEATMAP_CASES = [0, 1, 2, 3, 4]           # those the fixture holds (the reference's generator ran on them)


def heatmap_joints(R, J, C, seed):
    """[N, J, C] fp32-representable: random joints in [-1, R + 1] and, first, the edges of heatmap.py:33-38: a joint at 0, at
    R - eps, exactly at R, a negative one, third column 0, -1 and 1."""
    rs = np.random.RandomState(seed)
    N = 8 if J == 1 else 2
    j = rs.uniform(-1.0, R + 1.0, size=(N * J, 3))
    j[:, 2] = rs.choice([1.0, 1.0, 1.0, 0.5, 0.0, -1.0], size=N * J)
    eps = 2.0 ** -10
    special = [(0.0, 0.0, 1.0), (R - eps, 1.0, 1.0), (R, 1.0, 1.0), (1.0, R, 1.0), (-0.5, 1.0, 1.0), (1.0, 1.5, 0.0),
               (1.0, 1.5, -1.0), (R - eps, R - eps, 1.0)]
    for i, s in enumerate(special[:N * J]):
        j[i] = s
    return r32(j.reshape(N, J, 3)[..., :C])


def run_heatmaps(fused, device, dtype=F32):
    """Every heat-map case against the fp64 mirror (and the fixture where it holds the case); returns the worst error."""
    worst = 0.0
    for ci, (R, J, C, sigma, scale) in enumerate(HEATMAP_CASES):
        j = heatmap_joints(R, J, C, 10 + ci)
        want = ah.HeatmapGenerator(R, sigma)(t(j), scale)
        if ci in FIXTURE_HEATMAP_CASES:
            ref = fix()['hm%d/out' % ci]
            assert ref.dtype == np.float32 and np.array_equal(fix()['hm%d/joints' % ci], j)
            # the reference stores float32: half an fp32 ulp of a value <= 1
            assert absmax(want, ref) <= 2.0 ** -25 + FP64, ('fp64 mirror against the reference', ci, absmax(want, ref))
            assert np.array_equal(ah.HeatmapGenerator(R, sigma)(j, scale), ref), 'numpy in, numpy float32 out, as the reference'
        gen = (ah.FusedHeatmapGenerator if fused else ah.HeatmapGenerator)(R, sigma)
        jin = t(j, device, dtype)
        keep = jin.clone()
        got = gen(jin, scale)
        assert got.dtype == dtype and tuple(got.shape) == (j.shape[0], J, R, R) and torch.equal(jin, keep)
        e = absmax(got, want)
        print('heat maps case %d (R %d, J %d, C %d, sigma %g x %g): %.3e' % (ci, R, J, C, gen.sigma, scale, e))
        assert e <= (BARS['heatmap'] if dtype == F32 else FP64), (ci, e)
        off = want.reshape(-1, R * R).abs().amax(1) == 0
        assert bool(off.any()) and bool((got.reshape(-1, R * R)[off.to(got.device)] == 0).all()), 'a switched-off map is exactly 0'
        if fused:
            assert torch.equal(gen(jin, scale), got), 'two runs are bit-identical'
            two = gen(jin[0], scale)                                      # the 2-D form [J, C] -> [1, J, R, R]
            assert tuple(two.shape) == (1, J, R, R) and torch.equal(two[0], got[0])
        worst = max(worst, e)
    return worst


# ------------------------------------------------------------------------------------------------ loss
# (B, Jh, S): (1, 1, 4) one item; (1, 3, 5) the dword tail; (2, 42, 8) the fixture's shape; (2, 42, 64) several items a plane
LOSS_SHAPES = [(1, 1, 4), (1, 3, 5), (2, 42, 8), (2, 42, 64)]
FIXTURE_LOSS_SHAPE = (2, 42, 8)


def loss_sigma(S):
    return 2.0 if S >= 64 else 1.0


def loss_inputs(B, Jh, S, seed=0):
    """fp32-representable fp64 arrays.  Differences of exactly 0, +-1, +-beta (the SmoothL1 kink of core/Loss.py:26), large ones,
    float mask values (0.5, 0.25) among the binary ones; joints with switched-off and out-of-range entries."""
    rs = np.random.RandomState(1000 + 7 * S + Jh + seed)
    beta = np.float64(np.float32(ah.SMOOTH_L1_BETA))
    d = {}
    d['t_mask'] = (rs.rand(B, 2, S, S) < 0.5).astype(np.float64)
    fm = d['t_mask'].reshape(-1)
    fm[5::7] = 0.5
    fm[6::11] = 0.25
    fm[:7] = 1.0
    d['t_dense'] = r32(rs.rand(B, 3, S, S))
    d['t_dense'].reshape(-1)[:7] = 0.5           # (dyadic: label + step is exact in fp32)
    d['p_mask'] = r32(d['t_mask'] + 0.08 * rs.randn(B, 2, S, S))
    d['p_dense'] = r32(np.concatenate([d['t_dense'], d['t_dense']], 1) + 0.08 * rs.randn(B, 6, S, S))
    steps = [0.0, 1.0, -1.0, 5.0, beta, -beta, -7.5]
    pm, pd, td = d['p_mask'].reshape(-1), d['p_dense'].reshape(-1), d['t_dense'].reshape(-1)
    for i, s in enumerate(steps[:min(len(steps), S * S)]):
        pm[i] = fm[i] + s                        # (mask 1 there: the dense difference is the step itself)
        pd[i] = td[i] + s
    d['p_mask'], d['p_dense'] = r32(d['p_mask']), r32(d['p_dense'])
    j = rs.uniform(0.0, S, size=(B, Jh, 3))
    j[..., 2] = rs.choice([1.0, 1.0, 1.0, 0.0, -1.0], size=(B, Jh))
    j[0, 0] = (S / 2 + 0.25, S / 2 - 0.5, 1.0)
    if Jh > 2:
        j[0, 1] = (-0.25, 1.0, 1.0)
        j[0, 2] = (1.0, S, 1.0)
    d['joints'] = r32(j)
    hm = ah.heatmaps(t(d['joints']), S, loss_sigma(S)).numpy()
    d['t_hms'] = r32(hm)
    d['p_hms'] = r32(hm + 0.1 * rs.randn(B, Jh, S, S))
    ph = d['p_hms'].reshape(-1)
    ph[0], ph[1] = d['t_hms'].reshape(-1)[0], d['t_hms'].reshape(-1)[1] + 3.0
    return d


def shape_inputs(B, Jh, S):
    if (B, Jh, S) == FIXTURE_LOSS_SHAPE:
        return {k[len('loss/in/'):]: v for k, v in fix().items() if k.startswith('loss/in/')}
    return loss_inputs(B, Jh, S)


TERM_KEYS = ('total_loss', 'mask_loss', 'dense_loss', 'hms_loss')


def eval_loss(loss, d, device, dtype, form='tensor', absent=None, scale=None, joints_cols=3):
    """Run `loss` on the inputs d -> (terms [4] as a tensor, {name: gradient})."""
    pred = {k: t(d['p_' + k], device, dtype).requires_grad_(True) for k in ('mask', 'dense', 'hms') if k != absent}
    kw = dict(hms=t(d['t_hms'], device, dtype)) if form == 'tensor' else \
        dict(joints2d=t(d['joints'][..., :joints_cols], device, dtype), sigma=loss_sigma(d['t_hms'].shape[-1]))
    if absent == 'hms':
        kw = {}
    total, terms = loss(pred, t(d['t_mask'], device, dtype), t(d['t_dense'], device, dtype), **kw)
    assert set(terms) == set(TERM_KEYS) and terms['total_loss'] is total
    (total if scale is None else total * scale).backward()
    return torch.stack([terms[k].detach() for k in TERM_KEYS]), {k: v.grad for k, v in pred.items()}


@functools.lru_cache(None)
def loss_reference(B, Jh, S, form='tensor', absent=None):
    """The fp64 mirror with autograd on the CPU, computed once per case."""
    return eval_loss(ah.AuxLoss(), shape_inputs(B, Jh, S), 'cpu', F64, form, absent)


def loss_errors(got, want):
    terms = float(((got[0].double().cpu() - want[0]).abs() / want[0].abs().clamp_min(1e-300))[want[0] != 0].max())
    assert bool((got[0].cpu()[want[0] == 0] == 0).all()), 'an absent term is exactly 0'
    assert set(got[1]) == set(want[1])
    return terms, max(rel(got[1][k], want[1][k]) for k in want[1])


def run_loss(fused, device, shape, dtype=F32, form='tensor', absent=None):
    """One loss case against the fp64 mirror's autograd; returns (terms error, gradient error)."""
    B, Jh, S = shape
    want = loss_reference(B, Jh, S, form, absent)
    got = eval_loss((ah.FusedAuxLoss if fused else ah.AuxLoss)(), shape_inputs(B, Jh, S), device, dtype, form, absent)
    et, eg = loss_errors(got, want)
    print('loss %s %s absent %s: terms %.3e, gradients %.3e' % (shape, form, absent, et, eg))
    assert et <= (BARS['loss'] if dtype == F32 else FP64), (shape, form, absent, et)
    assert eg <= (BARS['grad'] if dtype == F32 else FP64), (shape, form, absent, eg)
    return et, eg


def run_loss_fixture(fused, device, dtype=F32):
    """The reference's calc_aux_loss (fp64, autograd gradients) on the fixture's inputs."""
    f = fix()
    B, Jh, S = FIXTURE_LOSS_SHAPE
    d = shape_inputs(B, Jh, S)
    assert d['p_hms'].shape == (B, Jh, S, S)
    loss = (ah.FusedAuxLoss if fused else ah.AuxLoss)()
    assert (loss.w['MASK'], loss.w['DENSEPOSE'], loss.w['HMS']) == tuple(f['loss/weights']) and loss.beta == float(f['loss/beta'])
    got = eval_loss(loss, d, device, dtype)
    want = (torch.from_numpy(np.stack([f['loss/' + k] for k in TERM_KEYS])),
            {k: torch.from_numpy(f['loss/grad_' + k]) for k in ('mask', 'dense', 'hms')})
    et, eg = loss_errors(got, want)
    print('loss fixture: terms %.3e, gradients %.3e' % (et, eg))
    assert et <= (BARS['loss'] if dtype == F32 else FP64) and eg <= (BARS['grad'] if dtype == F32 else FP64), (et, eg)
    # the reference's own dict (what calc_aux_loss returns), through the function with its argument order
    pred = {k: t(d['p_' + k], device, dtype) for k in ('mask', 'dense', 'hms')}
    out = ah.calc_aux_loss(loss, None, pred, t(d['t_mask'], device, dtype), t(d['t_dense'], device, dtype),
                           t(d['t_hms'], device, dtype))
    assert set(out) == set(TERM_KEYS) and rel(out['total_loss'], f['loss/total_loss']) <= (BARS['loss'] if dtype == F32 else FP64)


def run_loss_forms_agree(fused, device, shape, dtype=F32):
    """Tensor label against joints label (2- and 3-column joints): the same total and gradients within the bars."""
    B, Jh, S = shape
    d = dict(shape_inputs(B, Jh, S))
    loss = (ah.FusedAuxLoss if fused else ah.AuxLoss)()
    a = eval_loss(loss, d, device, dtype, 'tensor')
    b = eval_loss(loss, d, device, dtype, 'joints')
    et, eg = loss_errors(b, (a[0].double().cpu(), a[1]))
    print('loss %s tensor label against joints label: terms %.3e, gradients %.3e' % (shape, et, eg))
    assert et <= BARS['loss'] and eg <= BARS['grad'], (et, eg)
    d['joints'] = np.where(d['joints'][..., 2:] > 0, d['joints'], -1.0)          # two columns: "off" has to be out of range
    d['t_hms'] = ah.heatmaps(t(d['joints']), S, loss_sigma(S)).numpy()
    want = eval_loss(ah.AuxLoss(), d, 'cpu', F64, 'tensor')
    got = eval_loss(loss, d, device, dtype, 'joints', joints_cols=2)
    et, eg = loss_errors(got, want)
    assert et <= BARS['loss'] and eg <= BARS['grad'], ('two-column joints', et, eg)


def run_loss_properties(fused, device, shape=(1, 3, 5)):
    """A non-unit incoming gradient with retain_graph, two runs bit-identical, inputs untouched, a change of weights."""
    B, Jh, S = shape
    d = shape_inputs(B, Jh, S)
    loss = (ah.FusedAuxLoss if fused else ah.AuxLoss)()
    pred = {k: t(d['p_' + k], device, F32).requires_grad_(True) for k in ('mask', 'dense', 'hms')}
    labels = [t(d[k], device, F32) for k in ('t_mask', 't_dense', 't_hms')]
    keep = [x.detach().clone() for x in list(pred.values()) + labels]
    total, terms = loss(pred, labels[0], labels[1], hms=labels[2])
    g1 = torch.autograd.grad(total * 0.37, list(pred.values()), retain_graph=True)
    g2 = torch.autograd.grad(total, list(pred.values()), retain_graph=True)
    g3 = torch.autograd.grad(total, list(pred.values()))
    want = loss_reference(B, Jh, S)
    for k, a, b, c in zip(pred, g1, g2, g3):
        assert torch.equal(b, c), 'the saved gradients survive a backward (retain_graph)'
        assert rel(a, 0.37 * want[1][k]) <= BARS['grad'] and rel(b, want[1][k]) <= BARS['grad']
    total2, terms2 = loss(pred, labels[0], labels[1], hms=labels[2])
    assert torch.equal(total, total2) and all(torch.equal(terms[k], terms2[k]) for k in terms), 'two runs are bit-identical'
    for x, y in zip(list(pred.values()) + labels, keep):
        assert torch.equal(x.detach(), y), 'inputs are not written'
    loss.set_weights(MASK=2.0, HMS=0.0)
    total3, terms3 = loss(pred, labels[0], labels[1], hms=labels[2])
    want3 = 2.0 * want[0][1] + 30.0 * want[0][2]
    assert rel(total3, want3) <= BARS['loss'] and torch.equal(terms3['mask_loss'], terms['mask_loss'])


def run_loss_refusals(fused, device):
    B, Jh, S = 1, 3, 5
    d = shape_inputs(B, Jh, S)
    loss = (ah.FusedAuxLoss if fused else ah.AuxLoss)()
    pred = {k: t(d['p_' + k], device, F32) for k in ('mask', 'dense', 'hms')}
    m, de, h = (t(d[k], device, F32) for k in ('t_mask', 't_dense', 't_hms'))
    raises = lambda fn, exc=ValueError, match=None: _raises(fn, exc, match)     # noqa: E731
    raises(lambda: loss(dict(pred, mask=pred['mask'][:, :1]), m, de, hms=h), match='HRNet')          # [B, 1, S, S]
    raises(lambda: loss(dict(pred, mask=pred['mask'][:, 0]), m, de, hms=h), match='HRNet')           # [B, S, S], encoder.py:395
    raises(lambda: loss(pred, m, de))                                                                # no heat-map label
    raises(lambda: loss(pred, m, de, hms=h, joints2d=t(d['joints'], device, F32)))                   # both
    raises(lambda: loss(pred, m[:, :1], de, hms=h))
    raises(lambda: loss({}, m, de, hms=h))
    raises(lambda: loss.set_weights(BONE=1.0), KeyError)
    if fused:
        nc = torch.empty(B, 2, S, 2 * S, device=device)[..., ::2].copy_(pred['mask'])
        assert not nc.is_contiguous()
        raises(lambda: loss(dict(pred, mask=nc), m, de, hms=h), match='contiguous')
        raises(lambda: loss(pred, m.double(), de, hms=h), RuntimeError)


def _raises(fn, exc, match):
    import pytest
    with pytest.raises(exc, match=match):
        fn()


# ------------------------------------------------------------------------------------------------ decoder
DECODE_SIZES = [(8, 8), (8, 12), (64, 64)]
DECODE_KERNELS = [1, 3, 5, 7]
KINDS = ['peak', 'col1', 'col2', 'colW-3', 'colW-2', 'row1', 'rowH-2', 'constant', 'zero', 'negative', 'tie', 'flat', 'peak',
         'peak']


def decoder_maps(H, W, n, seed):
    """[n, H, W] float32.  n = 1: one sub-pixel peak.  Otherwise the kinds above in turn: sub-pixel Gaussian peaks with amplitude
    in [0.2, 1] and noise; peaks in columns 1, 2, W - 3, W - 2 and rows 1, H - 2 (either side of the refinement's border); a
    constant, an all-zero and an all-negative map; a two-way tie; a map that is flat after the 1e-10 clamp (determinant 0 in the
    interior).  Every noisy map has a unique maximum, asserted here."""
    rs = np.random.RandomState(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    sg = 2.0 if min(H, W) >= 32 else 1.25
    out, kinds = [], []
    for i in range(n):
        kind = 'peak' if n == 1 else KINDS[i % len(KINDS)]
        cx, cy = rs.uniform(2.6, W - 3.6), rs.uniform(2.6, H - 3.6)
        if kind.startswith('col'):
            cx = {'col1': 1, 'col2': 2, 'colW-3': W - 3, 'colW-2': W - 2}[kind] + rs.uniform(-0.3, 0.3)
        if kind.startswith('row'):
            cy = {'row1': 1, 'rowH-2': H - 2}[kind] + rs.uniform(-0.3, 0.3)
        amp = rs.uniform(0.2, 1.0)
        m = amp * np.exp(-((xs - cx) ** 2 + (ys - cy) ** 2) / (2 * sg * sg)) + 0.01 * amp * rs.uniform(-1, 1, size=(H, W))
        if kind == 'constant':
            m = np.full((H, W), 0.3)
        elif kind == 'zero':
            m = np.zeros((H, W))
        elif kind == 'negative':
            m = -0.1 - np.abs(m)
        elif kind == 'tie':
            m[int(cy), int(cx)] = m[int(cy) + 1, int(cx) - 1] = 1.5 * m.max()
        elif kind == 'flat':
            m = np.full((H, W), 1e-12)
            m[int(cy), int(cx)] = 5e-11
        m = m.astype(np.float32)
        if kind not in ('constant', 'zero', 'tie'):
            assert int((m == m.max()).sum()) == 1, 'a random map needs a unique maximum (%s, seed %d)' % (kind, seed)
        out.append(m)
        kinds.append(kind)
    return np.stack(out), kinds


def decoder_case(H, W, NJ):
    """N * J = 1 or 3 * 42 maps as [N, J, H, W] float32."""
    n, shape = (1, (1, 1)) if NJ == 1 else (126, (3, 42))
    maps, kinds = decoder_maps(H, W, n, 50 + H + 3 * W + NJ)
    return maps.reshape(shape + (H, W)), kinds


def check_special_maps(preds, maxvals, maps, kinds):
    """What is known without arithmetic: non-positive maxima give (0, 0); ties take the first flat index; no NaN anywhere."""
    preds, maxvals = preds.detach().double().cpu().reshape(-1, 2), maxvals.detach().double().cpu().reshape(-1)
    flat = maps.reshape(len(kinds), -1)
    H, W = maps.shape[-2:]
    assert bool(torch.isfinite(preds).all()) and bool(torch.isfinite(maxvals).all())
    assert np.array_equal(maxvals.numpy(), flat.max(1).astype(np.float64)), 'maxvals is the maximum of the map, exactly'
    for i, kind in enumerate(kinds):
        if kind in ('zero', 'negative'):
            assert preds[i].tolist() == [0.0, 0.0], (kind, preds[i])
        if kind == 'constant':
            assert preds[i].tolist() == [0.0, 0.0] and maxvals[i] > 0
        if kind == 'flat':
            idx = int(flat[i].argmax())
            assert preds[i].tolist() == [float(idx % W), float(idx // W)], 'determinant 0: the integer coordinates stay'
        if kind in ('col1', 'colW-2', 'row1', 'rowH-2'):
            idx = int(flat[i].argmax())
            assert preds[i].tolist() == [float(idx % W), float(idx // W)], 'outside 1 < x < W - 2: no refinement'
        if kind in ('col2', 'colW-3', 'peak', 'tie') and min(H, W) >= 5:
            idx = int(flat[i].argmax())                                    # np.argmax: the first flat index
            assert abs(float(preds[i, 0]) - idx % W) < 1.5 and abs(float(preds[i, 1]) - idx // W) < 1.5
            assert preds[i].tolist() != [float(idx % W), float(idx // W)], 'inside the border the peak is refined'


def run_decode(fused, device, size, NJ, kernel, dtype=F32):
    """One decoder case against the fp64 mirror; returns the error in pixels."""
    H, W = size
    maps, kinds = decoder_case(H, W, NJ)
    want = ah.decode_heatmaps(t(maps), kernel)
    hm = t(maps, device, dtype)
    keep = hm.clone()
    got = ah.FusedHeatmapDecoder(kernel)(hm) if fused else ah.decode_heatmaps(hm, kernel)
    assert torch.equal(hm, keep), 'the input is not written'
    assert tuple(got[0].shape) == maps.shape[:2] + (2,) and tuple(got[1].shape) == maps.shape[:2]
    check_special_maps(got[0], got[1], maps, kinds)
    e = absmax(got[0], want[0])
    print('decode %dx%d, %d maps, kernel %d: %.3e px' % (H, W, NJ, kernel, e))
    assert e <= (BARS['decode'] if dtype == F32 else FP64), (size, NJ, kernel, e)
    if fused:
        again = ah.FusedHeatmapDecoder(kernel)(hm)
        assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1]), 'two runs are bit-identical'
    return e


def run_decode_fixture(fused, device, dtype=F32):
    """dataset.inference.get_final_preds2 (run in fp64 on these fp32 maps; coordinates returned in float32)."""
    f = fix()
    for H, W in DECODE_SIZES:
        maps = f['dec%dx%d/maps' % (H, W)]
        mine, kinds = decoder_maps(H, W, maps.shape[1], 900 + H + W)
        assert np.array_equal(mine, maps[0]), 'the fixture was generated from decoder_maps'
        for kernel in DECODE_KERNELS:
            ref_p, ref_m = f['dec%dx%d/k%d/preds' % (H, W, kernel)], f['dec%dx%d/k%d/maxvals' % (H, W, kernel)]
            assert ref_p.dtype == np.float32
            half_ulp = np.spacing(np.abs(ref_p)).astype(np.float64) / 2
            want = ah.decode_heatmaps(t(maps), kernel)
            assert bool(((want[0].numpy() - ref_p).__abs__() <= half_ulp + 1e-9).all()), \
                ('fp64 mirror against the reference', H, W, kernel, np.abs(want[0].numpy() - ref_p).max())
            assert np.array_equal(want[1].numpy()[..., None], ref_m)
            p_np, m_np = ah.get_final_preds2(maps.astype(np.float64), kernel)     # numpy in, numpy out, as the reference
            assert p_np.dtype == np.float32 and np.array_equal(p_np, ref_p) and np.array_equal(m_np, ref_m)
            hm = t(maps, device, dtype)
            got = ah.FusedHeatmapDecoder(kernel)(hm) if fused else ah.decode_heatmaps(hm, kernel)
            check_special_maps(got[0], got[1], maps, kinds)
            err = np.abs(got[0].detach().double().cpu().numpy() - ref_p)
            print('decode fixture %dx%d kernel %d: %.3e px' % (H, W, kernel, err.max()))
            # fp32: the plain bar; fp64: the float32 rounding of the reference's own coordinates
            assert bool((err <= (BARS['decode'] if dtype == F32 else 1e-9 + half_ulp)).all()), (H, W, kernel, err.max())


def run_decode_refusals(fused, device):
    hm = torch.rand(1, 2, 8, 8, device=device)
    if fused:
        for k in (0, 2, 4, 9):
            _raises(lambda: ah.FusedHeatmapDecoder(k), ValueError, 'taps')
        dec = ah.FusedHeatmapDecoder(5)
        _raises(lambda: dec(torch.rand(1, 1, 128, 129, device=device)), ValueError, 'LDS')
        _raises(lambda: dec(hm[..., ::2]), ValueError, 'contiguous')
        _raises(lambda: dec(hm.double()), RuntimeError, None)
        p, m = dec(torch.rand(1, 1, 128, 128, device=device))                # 64 KB exactly: the largest map
        assert bool(torch.isfinite(p).all())
    else:
        for k in (2, 4, 9):
            _raises(lambda: ah.decode_heatmaps(hm, k), ValueError, 'taps')
        a, b = ah.decode_heatmaps(hm, 0), ah.decode_heatmaps(hm, 1)          # `if kernel > 1` (inference.py:117)
        assert torch.equal(a[0], b[0])


def run_einval(lib, buf, stream=0):
    """The C entry points refuse bad sizes and null pointers (RIH_EINVAL) before launching anything."""
    E = -1                                   # RIH_EINVAL
    ok = lib.rih_heatmaps(buf, buf + 4096, 2, 3, 4, 1.0, stream)
    assert ok == 0
    for args in ((0, buf, 2, 3, 4, 1.0), (buf, 0, 2, 3, 4, 1.0), (buf, buf, 0, 3, 4, 1.0), (buf, buf, 2, 4, 4, 1.0),
                 (buf, buf, 2, 3, 0, 1.0), (buf, buf, 2, 3, 5000, 1.0), (buf, buf, 2, 3, 4, 0.0)):
        assert lib.rih_heatmaps(*args, stream) == E, args
    for args in ((0, buf, buf, 1, 8, 8, 5), (buf, 0, buf, 1, 8, 8, 5), (buf, buf, 0, 1, 8, 8, 5), (buf, buf, buf, 0, 8, 8, 5),
                 (buf, buf, buf, 1, 0, 8, 5), (buf, buf, buf, 1, 128, 129, 5), (buf, buf, buf, 1, 8, 8, 2),
                 (buf, buf, buf, 1, 8, 8, 9), (buf, buf, buf, 1, 8, 8, 0)):
        assert lib.rih_hms_decode(*args, stream) == E, args
    b = buf
    good = dict(p_hms=b, p_mask=b, p_dense=b, t_hms=b, t_joints=0, t_mask=b, t_dense=b, w=b, B=1, Jh=1, S=4, C=3, sigma=1.0,
                beta=0.05, g_hms=b, g_mask=b, g_dense=b, partial=b)
    for change in (dict(w=0), dict(partial=0), dict(p_hms=0, p_mask=0, p_dense=0), dict(B=0), dict(S=0), dict(S=5000),
                   dict(Jh=0), dict(beta=0.0), dict(t_joints=b), dict(t_hms=0), dict(t_hms=0, t_joints=b, C=4),
                   dict(t_hms=0, t_joints=b, sigma=0.0), dict(g_hms=0), dict(g_mask=0), dict(g_dense=0), dict(t_mask=0),
                   dict(t_dense=0)):
        a = dict(good, **change)
        assert lib.rih_aux_loss(*[a[k] for k in good], stream) == E, change
    assert lib.rih_aux_loss_blocks(1, 1, 4, 1, 1) == 2 and lib.rih_aux_loss_blocks(64, 42, 64, 1, 1) == 2048
    assert lib.rih_aux_loss_blocks(0, 1, 4, 1, 1) == 0 and lib.rih_aux_loss_blocks(1, 1, 4, 0, 0) == 0
    for args in ((0, b, 1, 1, 4, 1, 1, b), (b, 0, 1, 1, 4, 1, 1, b), (b, b, 1, 1, 4, 1, 1, 0), (b, b, 0, 1, 4, 1, 1, b),
                 (b, b, 1, 1, 4, 0, 0, b)):
        assert lib.rih_aux_loss_final(*args, stream) == E, args


# ------------------------------------------------------------------------------------------------ bars
def mirror_errors():
    """fp32 mirror against fp64 mirror on the CPU, over the cases above: what MIRROR_FP32 was written from."""
    worst = {k: 0.0 for k in MIRROR_FP32}
    for ci, (R, J, C, sigma, scale) in enumerate(HEATMAP_CASES):
        j = heatmap_joints(R, J, C, 10 + ci)
        g = ah.HeatmapGenerator(R, sigma)
        worst['heatmap'] = max(worst['heatmap'], absmax(g(t(j, dtype=F32), scale), g(t(j), scale)))
    for shape in LOSS_SHAPES:
        for form in ('tensor', 'joints'):
            want = loss_reference(*shape, form)
            got = eval_loss(ah.AuxLoss(), shape_inputs(*shape), 'cpu', F32, form)
            et, eg = loss_errors(got, want)
            worst['loss'], worst['grad'] = max(worst['loss'], et), max(worst['grad'], eg)
    for H, W in DECODE_SIZES:
        for NJ in (1, 126):
            maps, _ = decoder_case(H, W, NJ)
            for kernel in DECODE_KERNELS:
                e = absmax(ah.decode_heatmaps(t(maps, dtype=F32), kernel)[0], ah.decode_heatmaps(t(maps), kernel)[0])
                worst['decode'] = max(worst['decode'], e)
    return worst


# ------------------------------------------------------------------------------------------------ labels
def run_labels(device, S):
    """aux_labels against direct render_mask / render_densepose calls: the channel order on a scene with only ONE hand in view,
    the threshold, the flip rule, the heat-map label in both forms."""
    import render_cases as rc
    from renderih_amd import render
    r = render.mano_two_hands_renderer(img_size=S, device=device)
    B = 2
    vl, vr, sl, tl, sr, tr = rc.ortho_scene(B, seed=3)
    vr_cam = rc.right_in_left_camera(vr, sl, tl, sr, tr)
    vr_cam[1, :, 0] += 50.0                                               # image 1: the right hand is out of view
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    cam = dict(scale=tt(sl), trans2d=tt(tl))
    rgb = r.render_mask(v3d_left=tt(vl), v3d_right=tt(vr_cam), **cam)
    dp = r.render_densepose(v3d_left=tt(vl), v3d_right=tt(vr_cam), **cam)[0]
    rs = np.random.RandomState(S)
    j = (np.round(rs.uniform(0, 4 * S, size=(B, 42, 3)) * 4) / 4).astype(np.float32)    # (dyadic: S - 1 - x is exact in fp32)
    j[..., 2] = 1.0
    j[0, 0, 0], j[0, 1, 0] = -0.5 * 4, (S - 0.5) * 4                     # left joints 0, 1 of image 0: x = -0.5 (off) and S - 0.5
    mask, dense, joints = ah.aux_labels(r, tt(vl), tt(vr_cam), joints2d=tt(j), img_size=4 * S, **cam)
    assert tuple(mask.shape) == (B, 2, S, S) and tuple(dense.shape) == (B, 3, S, S) and tuple(joints.shape) == (B, 42, 3)
    assert mask.is_contiguous() and dense.is_contiguous()
    assert set(mask.unique().tolist()) <= {0.0, 1.0}
    # the left hand is painted into colour channel 2, the right hand into channel 1; the loader keeps [1:]: right first
    assert torch.equal(mask[:, 0], (rgb[..., 1] * 255 > 127).to(mask.dtype)) and torch.equal(mask[:, 1], (rgb[..., 2] * 255 > 127).to(mask.dtype))
    assert float(mask[0, 0].sum()) > 0 and float(mask[0, 1].sum()) > 0
    assert float(mask[1, 0].sum()) == 0 and float(mask[1, 1].sum()) > 0, 'only the LEFT hand in view: channel 1 alone is set'
    assert torch.equal(dense, dp.permute(0, 3, 1, 2)) and float(dense.min()) >= 0 and float(dense.max()) <= 1
    assert absmax(joints[..., :2], j[..., :2] / 4.0) <= 1e-6 * S and torch.equal(joints[..., 2], tt(j[..., 2]))
    maps = ah.aux_labels(r, tt(vl), tt(vr_cam), joints2d=tt(j), img_size=4 * S, heatmaps_as='tensor', **cam)[2]
    assert absmax(maps, ah.heatmaps(joints.double().cpu(), S, ah.HEATMAP_SIGMA)) <= BARS['heatmap']
    # flip (loader_ori.py:117-143), per sample: image 0 flipped, image 1 not
    flip = torch.tensor([True, False], device=device)
    fm, fd, fj = ah.aux_labels(r, tt(vl), tt(vr_cam), joints2d=tt(j), img_size=4 * S, flip=flip, **cam)
    assert torch.equal(fm[0], mask[0].flip(-1)[[1, 0]]) and torch.equal(fm[1], mask[1])
    assert torch.equal(fd[0], dense[0].flip(-1)) and torch.equal(fd[1], dense[1])
    assert torch.equal(fj[1], joints[1]) and torch.equal(fj[0, :21, 1:], joints[0, 21:, 1:])
    assert absmax(fj[0, :21, 0], (S - 1) - joints[0, 21:, 0]) == 0 and absmax(fj[0, 23:, 0], (S - 1) - joints[0, 2:21, 0]) == 0
    ft = ah.aux_labels(r, tt(vl), tt(vr_cam), joints2d=tt(j), img_size=4 * S, flip=True, heatmaps_as='tensor', **cam)[2]
    assert torch.equal(ft[:, :21], maps[:, 21:].flip(-1)) and torch.equal(ft[:, 21:], maps[:, :21].flip(-1))
    # the two forms at the generator's edges: a joint that is off (x = -0.5) stays off through the flip in both; every map of
    # the joints form equals the mirrored image, except the one of the joint in the last pixel (x = S - 0.5), the stated deviation
    drawn = ah.heatmaps(fj.double().cpu(), S, ah.HEATMAP_SIGMA)
    assert float(ft[0, 21].abs().max()) == 0 and float(drawn[0, 21].abs().max()) == 0
    assert float(ft[0, 22].abs().max()) > 0 and float(drawn[0, 22].abs().max()) == 0
    x0 = torch.cat([joints[0, 21:, 0], joints[0, :21, 0]]).cpu()            # the unflipped x of each flipped channel
    last = (x0 > S - 1) & (x0 < S)
    assert bool(last[22]) and float(drawn[0, last].abs().max()) == 0
    assert absmax(drawn[0, ~last], ft[0, ~last]) <= BARS['heatmap'], absmax(drawn[0, ~last], ft[0, ~last])
    none = ah.aux_labels(r, tt(vl), tt(vr_cam), **cam)
    assert none[2] is None and torch.equal(none[0], mask)
