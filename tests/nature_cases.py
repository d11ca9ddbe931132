"""Shared by tests/test_nature_loss.py, tests/test_gpu_nature_loss.py and the pose-optimiser tests of the NatureLoss term: seeded
inputs, the evaluation of a module into numpy arrays, the comparison bars.

Tolerances (from the issue and from measurements of the REFERENCE computation, not of the code under test):
  mirror vs golden    max |err| <= 1e-6 max |want| per array (both are fp32 torch on the CPU).
  gradients           the project's operator bar |err| <= 1e-4 |want| + 1e-5 max |want| (renderih_amd.testing.assert_close).
  loss, terms         relative error <= TERM_RTOL = 4 x the largest relative deviation of the fp32 torch MIRROR from the fp64
                      mirror over `deviation_cases()` (the three golden cases and every seeded case the fused tests use), taken
                      on the CPU and on the GPU (profiles/nature_loss/deviation_{cpu,gpu}.log).  The two counts must be equal.
                      Measured: 1.63e-7 on the CPU (golden case a) and 1.04e-7 on an MI355X (golden case c) ->
                      TERM_RTOL = 6.52e-7.  The fused kernels were then found at most 2.2e-7 from the golden and 2.4e-7 from the
                      fp64 mirror (B = 1, H = 512 on the MI355X).  `mirror_fp32_deviation` repeats the measurement; it is not a test, since torch's
                      own fp32 rounding differs between BLAS builds.
Every seeded case is DECIDED: on the fp64 mirror every row has |p1 - 0.6| >= 1e-3 (the mask p1 < 1.5 p0 is p1 < 0.6), so no
rounding of an fp32 evaluation flips a row across the mask, and no LeakyReLU input lies within KINK = 1e-6 of 0: on the wrong
side of 0 the slope of that unit changes a hundredfold, which no tolerance on gradients absorbs.  (These inputs are sums of at
most 512 products with a magnitude of a few tenths; an fp32 evaluation is off by a few 1e-8 in the typical case -- 6e-8 times
the magnitude, the rounding errors of the terms adding like a random walk -- so 1e-6 leaves a factor of ten and more.  A
stricter margin leaves no seed at B = 32, H = 512: 131072 units with a density of about 1.5 per unit length around 0.)  `seeded_case` walks seeds until both hold and
asserts them; they are conditions on the inputs, judged on the fp64 mirror alone.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

from renderih_amd import testing  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'nature_loss.npz')
GOLDEN_CASES = ('a', 'b', 'c')
UPSTREAM = 1.5                            # the scalar the loss is multiplied by before the backward
MARGIN = 1e-3                             # a decided row: |p1 - 0.6| >= MARGIN on the fp64 mirror
KINK = 1e-6                               # a decided unit: |LeakyReLU input| >= KINK on the fp64 mirror
# largest relative deviation of the loss or a term of the fp32 torch mirror from the fp64 mirror over deviation_cases()
MEASURED_CPU = 1.63e-7
MEASURED_GPU = 1.04e-7
TERM_RTOL = 4 * max(MEASURED_CPU, MEASURED_GPU)
# (B, H, pred_scale).  H = 64 keeps the host harness quick, 512 is the reference's width; pred_scale 8 spreads the
# probabilities across the mask, 1 leaves every row masked.  B = 1: fewer rows than a tile; B = 3 (and 5): a tile holds hands
# of both sides and the last tile is partial, for every tile height the library may be built with (rows_cases() checks it)
CPU_CASES = [(1, 64, 8.0), (3, 64, 8.0), (5, 64, 8.0), (3, 64, 1.0), (3, 512, 8.0)]
GPU_CASES = [(1, 512, 8.0), (3, 512, 8.0), (32, 512, 8.0), (32, 512, 1.0)]


def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def random_poses(rs, B):
    """[2,B,16,4] fp64: rotations by up to ~80 degrees with |q| in [0.7, 1.4], as the prior golden draws them."""
    axis = rs.randn(2, B, 16, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * rs.uniform(0.0, 1.4, size=(2, B, 16, 1))
    return np.concatenate([np.cos(half), np.sin(half) * axis], -1) * rs.uniform(0.7, 1.4, size=(2, B, 16, 1))


_MODULES = {}


def module(cls, H, pred_scale, seed=0, bias1=None):
    """One instance per class and weight set; `bias1` replaces layer_pred.bias[1] (a large value empties both masks)."""
    from renderih_amd.nature import synthetic_state_dict
    key = (cls.__name__, H, pred_scale, seed, bias1)
    if key not in _MODULES:
        sd = synthetic_state_dict(seed, H, pred_scale)
        if bias1 is not None:
            sd['layer_pred.bias'][1] = bias1
        _MODULES[key] = cls(sd)
    import copy
    return copy.deepcopy(_MODULES[key])


def mirror_cls():
    from renderih_amd.nature import TwoHandNatureLoss
    return TwoHandNatureLoss


def fused_cls():
    from renderih_amd.nature import FusedTwoHandNatureLoss
    return FusedTwoHandNatureLoss


def evaluate(mod, case, device, dtype=torch.float32):
    """-> dict of numpy arrays: loss, terms, grad_q_r, grad_q_l of UPSTREAM * loss (and the mirror's `outputs`)."""
    mod = (mod.to(device) if dtype == torch.float32 else mod.to(device=device, dtype=dtype))
    ins = [torch.as_tensor(case[k]).to(device=device, dtype=dtype).requires_grad_(True) for k in ('q_r', 'q_l')]
    kinks = []
    hook = None
    if hasattr(mod, 'disc') and dtype == torch.float64:                # the fp64 mirror: the least |LeakyReLU input|
        hook = mod.disc.relu.register_forward_hook(lambda m, args, out: kinks.append(float(args[0].detach().abs().min())))
    loss, terms = mod(*ins)
    if hook is not None:
        hook.remove()
    assert loss.shape == () and terms.shape == (4,) and loss.dtype == dtype
    # the mirror with an empty side never uses that side's pose (with both empty the loss is a constant 0): zeros
    grads = torch.autograd.grad(loss * UPSTREAM, ins, allow_unused=True) if loss.requires_grad else (None, None)
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, ins)]
    out = {'loss': loss.detach().cpu().numpy(), 'terms': terms.detach().cpu().numpy(),
           'grad_q_r': grads[0].detach().cpu().numpy(), 'grad_q_l': grads[1].detach().cpu().numpy()}
    if getattr(mod, 'outputs', None) is not None:
        out['outputs'] = mod.outputs.cpu().numpy()
    if kinks:
        out['kink'] = np.float64(min(kinks))
    return out


def margin(outputs):
    return float(np.abs(np.asarray(outputs, np.float64)[..., 1] - 0.6).min())


_CASES = {}


def seeded_case(B, H, pred_scale):
    """The first seed (of the weights and of the poses) whose rows are all decided on the fp64 mirror and, at a
    pred_scale other than 1, fall on both sides of the mask -> {'q_r', 'q_l' fp32 [B,16,4], 'H', 'pred_scale', 'seed',
    'want': the fp64 mirror's result}.  Computed once and shared."""
    key = (B, H, pred_scale)
    if key not in _CASES:
        for seed in range(200):
            q = random_poses(np.random.RandomState(7000 + 131 * B + H + seed), B).astype(np.float32)
            case = {'q_r': q[0], 'q_l': q[1], 'H': H, 'pred_scale': pred_scale, 'seed': seed}
            want = evaluate(module(mirror_cls(), H, pred_scale, seed), case, 'cpu', torch.float64)
            masked = want['terms'][2] + want['terms'][3]
            if margin(want['outputs']) >= MARGIN and want['kink'] >= KINK and (pred_scale == 1.0 or 0 < masked < 2 * B):
                break
        else:
            raise AssertionError('no decided seed for %r' % (key,))
        assert margin(want['outputs']) >= MARGIN and want['kink'] >= KINK
        case['want'] = want
        _CASES[key] = case
    return _CASES[key]


def golden_case(name):
    """A case of tests/golden/nature_loss.npz with the REFERENCE's results as `want` (gradients scaled by UPSTREAM)."""
    z = golden()
    H, scale = int(z[name + '/hid_dim']), float(z[name + '/pred_scale'])
    want = {'loss': z[name + '/loss'], 'terms': z[name + '/terms'], 'outputs': z[name + '/outputs'],
            'grad_q_r': z[name + '/grad_q_r'] * np.float32(UPSTREAM), 'grad_q_l': z[name + '/grad_q_l'] * np.float32(UPSTREAM)}
    return {'q_r': z[name + '/q_r'], 'q_l': z[name + '/q_l'], 'H': H, 'pred_scale': scale, 'seed': int(z[name + '/seed']),
            'want': want}


def relative_deviation(got, want):
    """Largest relative deviation over the loss and the two means; the counts, and a term that is exactly 0, must be equal."""
    g = np.concatenate([np.asarray(got['terms'], np.float64), [float(got['loss'])]])
    w = np.concatenate([np.asarray(want['terms'], np.float64), [float(want['loss'])]])
    assert np.array_equal(g[2:4], w[2:4]), 'counts %s want %s' % (g[2:4], w[2:4])
    assert np.array_equal(g[w == 0], w[w == 0]), 'a term that must be exactly 0: %s want %s' % (g, w)
    nz = w != 0
    return float((np.abs(g[nz] - w[nz]) / np.abs(w[nz])).max()) if nz.any() else 0.0


def compare(got, want, what):
    dev = relative_deviation(got, want)
    print('%s: scalar relative deviation %.3g (bar %.3g)' % (what, dev, TERM_RTOL))
    for k in ('grad_q_r', 'grad_q_l'):
        testing.assert_close(torch.as_tensor(got[k]), torch.as_tensor(want[k]), 1e-4, 1e-5, '%s %s' % (what, k))
        assert not got[k][:, 0].any(), 'the root quaternion has a gradient'
    assert dev <= TERM_RTOL, '%s: loss %s terms %s want %s %s' % (what, got['loss'], got['terms'], want['loss'], want['terms'])
    t = np.asarray(got['terms'])
    assert got['loss'] == np.float32(t[0]) + np.float32(t[1])


def deviation_cases(cases):
    out = [('golden ' + n, golden_case(n)) for n in GOLDEN_CASES]
    return out + [('B%d H%d scale %g' % c, seeded_case(*c)) for c in cases]


def mirror_fp32_deviation(device, cases):
    """What TERM_RTOL is built from: fp32 mirror on `device` against the fp64 mirror on the CPU over every case."""
    worst = 0.0
    for name, case in deviation_cases(cases):
        mod64 = module(mirror_cls(), case['H'], case['pred_scale'], case.get('seed', 0))
        want = evaluate(mod64, case, 'cpu', torch.float64)
        got = evaluate(module(mirror_cls(), case['H'], case['pred_scale'], case.get('seed', 0)), case, device)
        dev = relative_deviation(got, want)
        print('fp32 mirror vs fp64 mirror on %s, %s: %.3g (counts %s, least margin %.3g, least |LeakyReLU input| %.3g)' %
              (device, name, dev, want['terms'][2:].tolist(), margin(want['outputs']), want['kink']))
        worst = max(worst, dev)
    print('largest: %.3g' % worst)
    return worst


def fused_vs(case, device, what, want=None):
    """The fused module against `want` (default: the case's own, the fp64 mirror's or the golden's); bit-identical repeat."""
    fused = module(fused_cls(), case['H'], case['pred_scale'], case.get('seed', 0))
    got = evaluate(fused, case, device)
    compare(got, case['want'] if want is None else want, what)
    again = evaluate(fused, case, device)
    for k in got:
        assert np.array_equal(got[k], again[k]), k                      # fixed summation order, plain stores
    return got
