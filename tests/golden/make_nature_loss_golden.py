#!/usr/bin/env python
"""Golden vectors of the pose optimiser's NatureLoss from the REFERENCE's own program:
pose_data_optimize/hocontact/postprocess/geo_optimizer_both_batch.py (`GeOptimizer.NatureLoss`, called unbound on a namespace
that holds `device` and `disc`) with the network of Ver2Code/Discriminator/discrim.py (`Pos2dDiscriminator`) and manopth's
`normalize_quaternion`, imported from a reference checkout at generation time and run unmodified on the CPU.

Imports: `reference_modules` of make_quat_mano_golden.py, then pose_data_optimize/ itself on the path, and stand-in modules for
sdf, open3d, termcolor and trimesh whose attribute lookups return dummy classes (the optimiser's module reads
`termcolor.colored` and `sdf.SDF` at import; none of the four is used by NatureLoss, none is installed here).  The weights are
NOT the reference's discrim.pth (not in the checkout): `renderih_amd.nature.synthetic_state_dict(seed, hid_dim, pred_scale)`
is loaded into the reference's network with `load_state_dict`, and only the recipe's arguments are stored.

Writes tests/golden/nature_loss.npz, three cases:
  a  hid_dim = 512, B = 4, pred_scale = 8: masked and unmasked rows on BOTH sides
  b  the same with every right-hand row replaced by an unmasked row of a: the right side is empty and adds exactly 0
  c  hid_dim = 64, B = 3
Per case: seed, hid_dim, pred_scale, the UN-normalised poses q_r, q_l [B,16,4] (rotations by up to ~80 degrees, norms in
[0.7, 1.4], as the prior golden draws them), the loss, terms = (right mean, left mean, right count, left count), the
discriminator's outputs [2,B,2], and the autograd gradient of the loss with respect to q_r and q_l through
`normalize_quaternion`.

Asserted here (another seed is tried until they hold; nothing is excused at test time): every row is decided --
|p1 - 0.6| >= 1e-3 with the network evaluated in fp64 (the mask p1 < 1.5 p0 is p1 < 0.6) -- so the undecided share is 0;
|m02| <= 0.95 for every joint (asin stays away from its clamp); the masks are as the case wants them; the two sides' means add
up to NatureLoss's value bit for bit; two runs write identical arrays.
       python tests/golden/make_nature_loss_golden.py <reference checkout>"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_quat_mano_golden import reference_modules  # noqa: E402

MARGIN, M02_MAX = 1e-3, 0.95


class _StandIn(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith('__'):
            raise AttributeError(name)
        return type(name, (), {})


def quaternions(rs, B):
    """[2,B,16,4]: rotations by up to ~80 degrees about random axes, norms in [0.7, 1.4]."""
    axis = rs.randn(2, B, 16, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * rs.uniform(0.0, 1.4, size=(2, B, 16, 1))
    q = np.concatenate([np.cos(half), np.sin(half) * axis], -1) * rs.uniform(0.7, 1.4, size=(2, B, 16, 1))
    return q.astype(np.float32)


def m02_of(q):
    q = q.astype(np.float64)[..., 1:, :]
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return 2.0 * (q[..., 1] * q[..., 3] + q[..., 2] * q[..., 0])


def load_reference(ref):
    reference_modules(ref)
    sys.path.insert(1, os.path.join(ref, 'pose_data_optimize'))
    for name in ('sdf', 'open3d', 'termcolor', 'trimesh'):
        sys.modules.setdefault(name, _StandIn(name))
    from hocontact.postprocess import geo_optimizer_both_batch as gob
    from manopth.quatutils import normalize_quaternion
    from Ver2Code.Discriminator import discrim
    for mod in (gob, discrim, sys.modules[normalize_quaternion.__module__]):
        assert os.path.abspath(mod.__file__).startswith(os.path.abspath(ref)), '%s is not the reference\'s' % mod.__name__
    assert gob.Pos2dDiscriminator is discrim.Pos2dDiscriminator
    return gob.GeOptimizer, discrim.Pos2dDiscriminator, normalize_quaternion


def evaluate(ref_mods, disc, q):
    """q [2,B,16,4] fp32 -> the case's arrays and the fp64 outputs."""
    GeOptimizer, _, normalize_quaternion = ref_mods
    T = torch.from_numpy
    B = q.shape[1]
    q_r, q_l = T(q[0].copy()).requires_grad_(True), T(q[1].copy()).requires_grad_(True)
    n_r, n_l = normalize_quaternion(q_r), normalize_quaternion(q_l)
    ns = types.SimpleNamespace(device='cpu', disc=disc)
    loss = GeOptimizer.NatureLoss(ns, n_r[:, 1:], n_l[:, 1:])
    grads = torch.autograd.grad(loss, (q_r, q_l), allow_unused=True)
    grads = [torch.zeros_like(q_r) if g is None else g for g in grads]
    real = torch.cat((torch.zeros((B, 1)), torch.ones((B, 1))), dim=1)
    outs, terms, counts = [], [], []
    with torch.no_grad():
        for n in (n_r, n_l):
            out = disc(n[:, 1:].reshape(B, -1))
            mask = out[:, 1] < 1.5 * out[:, 0]
            terms.append(torch.nn.functional.binary_cross_entropy(out[mask], real[mask]) if mask.sum() > 0 else torch.tensor(0.0))
            counts.append(mask.sum().float())
            outs.append(out)
        assert float(terms[0] + terms[1]) == float(loss), 'the two sides do not add up to NatureLoss'
        disc64 = copy.deepcopy(disc).double()
        out64 = torch.stack([disc64(normalize_quaternion(T(q[i].astype(np.float64)))[:, 1:].reshape(B, -1)) for i in (0, 1)])
    arrays = {'q_r': q[0], 'q_l': q[1], 'loss': loss.detach().numpy(), 'terms': torch.stack(terms + counts).numpy(),
              'outputs': torch.stack(outs).numpy(), 'grad_q_r': grads[0].numpy(), 'grad_q_l': grads[1].numpy()}
    assert all(np.isfinite(v).all() for v in arrays.values())
    return arrays, out64.numpy()


def decided(out64, q):
    return bool((np.abs(out64[..., 1] - 0.6) >= MARGIN).all() and (np.abs(m02_of(q)) <= M02_MAX).all())


def generate(ref_mods):
    from renderih_amd.nature import synthetic_state_dict
    _, Pos2dDiscriminator, _ = ref_mods
    out = {}

    def network(seed, H, scale):
        disc = Pos2dDiscriminator(num_joints=15, hid_dim=H, dropout=0.05).eval()
        print(disc.load_state_dict(synthetic_state_dict(seed, H, scale)))
        return disc

    def store(name, seed, H, scale, arrays):
        out[name + '/seed'], out[name + '/hid_dim'], out[name + '/pred_scale'] = np.int32(seed), np.int32(H), np.float32(scale)
        for k, v in arrays.items():
            out[name + '/' + k] = v

    # a: mixed masks on both sides; b: a's right hands replaced by one of its unmasked right rows
    for seed in range(200):
        disc = network(seed, 512, 8.0)
        q = quaternions(np.random.RandomState(6100 + seed), 4)
        a, a64 = evaluate(ref_mods, disc, q)
        masked = a64[..., 1] < 0.6
        if not (decided(a64, q) and all(0 < masked[i].sum() < 4 for i in (0, 1))):
            continue
        qb = q.copy()
        qb[0] = q[0][int(np.flatnonzero(~masked[0])[0])]
        b, b64 = evaluate(ref_mods, disc, qb)
        assert decided(b64, qb) and b['terms'][2] == 0 and b['terms'][0] == 0 and not b['grad_q_r'].any()
        assert b['terms'][3] == a['terms'][3] and b['terms'][1] == a['terms'][1]
        store('a', seed, 512, 8.0, a)
        store('b', seed, 512, 8.0, b)
        break
    else:
        raise AssertionError('no seed meets the conditions of case a')
    for seed in range(200):
        disc = network(seed, 64, 8.0)
        q = quaternions(np.random.RandomState(6400 + seed), 3)
        c, c64 = evaluate(ref_mods, disc, q)
        masked = c64[..., 1] < 0.6
        if decided(c64, q) and 0 < masked.sum() < 6:
            store('c', seed, 64, 8.0, c)
            break
    else:
        raise AssertionError('no seed meets the conditions of case c')
    return out


def main(ref):
    ref_mods = load_reference(ref)
    out = generate(ref_mods)
    again = generate(ref_mods)
    assert set(out) == set(again) and all(np.array_equal(out[k], again[k]) for k in out), 'two runs differ'
    path = os.path.join(HERE, 'nature_loss.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes; seeds', {n: int(out[n + '/seed']) for n in 'abc'},
          'terms', {n: out[n + '/terms'].tolist() for n in 'abc'})


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
