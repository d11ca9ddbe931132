#!/usr/bin/env python
"""Golden vectors of the joints -> MANO fit from the REFERENCE's own program: utils/mano_from_3djoint/AIK.py `adaptive_IK`,
utils.py `mat2aa` and lines 159-204 and 225-231 of convert2mano.py, read from a reference checkout at generation time and
executed unmodified on the CPU with the reference's `ManoLayer` (utils/mano_from_3djoint/manolayer.py) on
renderih_amd.assets.synthetic_mano_dict(side, seed=0), the left hand's shapedirs flipped as convert2mano.py:135 does.

convert2mano.py is a script that reads a csv on import, so its lines are compiled from the file and run in a namespace that
supplies what the script had built by then (`cur_mano_layer`, `ori_joints`) with recording wrappers around `adaptive_IK`,
`mat2aa` and the layers' `forward`.  `transforms3d` is not installed: `transforms3d.axangles.axangle2mat` is a stub here,
Rodrigues' formula on the normalised axis with math.cos / math.sin, as that package computes it.

Hands: synthetic MANO seed 0, both sides, seeds 1-3: the layer's joints at root axis-angle N(0, 0.8^2), PCA coefficients
N(0, 0.6^2), shape N(0, 0.5^2), times 110 plus an offset (centimetres, as the reference's mocap).  The generator asserts that
the IK is finite with det R0 = +1, that no NaN appears in the 200 iterations, and that this repository's fp32 mirror stays
within 1e-3 (relative to the largest parameter) of its fp64 mirror over the first PREFIX iterations, so that no chaotic hand
sits in the compared prefix.

Writes tests/golden/joint_fit.npz:
  joints [6,21,3] f32, side [6] (0 right, 1 left), template/<side> [21,3]
  aik [6,16,3,3] f64 (normalised as convert2mano.py:167-169), pre [6,21,3] f32 and aik_pre [6,16,3,3] f64 (the reference's IK
  on already normalised fp32 joints)
  m2a_R [N,3,3] f64, m2a_aa, m2a_w (upstream weights), m2a_grad (torch autograd through the reference's mat2aa)
  traj_P [6,PREFIX+1,16,3,3], traj_beta [6,PREFIX+1,10] f32: the parameters BEFORE iteration i; hist [6,200] the loss of
  every iteration; final_P, final_beta, ori_pose [6,48]
Seeded: two runs write identical arrays.       python tests/golden/make_joint_fit_golden.py <reference checkout>"""
import importlib.util
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
PREFIX = 8
SEEDS = (1, 2, 3)


def _axangle2mat(axis, angle, is_normalized=False):
    x, y, z = (float(a) for a in axis)
    if not is_normalized:
        n = math.sqrt(x * x + y * y + z * z)
        x, y, z = x / n, y / n, z / n
    angle = float(np.asarray(angle).reshape(-1)[0])
    c, s = math.cos(angle), math.sin(angle)
    C = 1 - c
    return np.array([[x * x * C + c, x * y * C - z * s, z * x * C + y * s],
                     [x * y * C + z * s, y * y * C + c, y * z * C - x * s],
                     [z * x * C - y * s, y * z * C + x * s, z * z * C + c]])


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def crafted_matrices(rs, extra):
    """Matrices well inside each of mat2quat's four branches (turns of about 2.8 rad about +-x, +-y, +-z: the negative axes
    give a negative quaternion w, quat2aa's cos < 0 branch; small and medium turns: branch 3), each also with a perturbation
    that makes it no rotation, plus the IK results `extra`."""
    mats = []
    for axis in np.eye(3):
        for sign in (1.0, -1.0):
            for jitter in (0.0, 0.05):
                a = axis * sign + rs.randn(3) * 0.1
                mats.append(_axangle2mat(a, 2.8 + 0.1 * rs.randn()) + jitter * rs.randn(3, 3))
    for scale in (0.05, 0.4, 1.2):
        for jitter in (0.0, 0.05):
            mats.append(_axangle2mat(rs.randn(3), scale * (1 + rs.rand())) + jitter * rs.randn(3, 3))
    return np.concatenate([np.stack(mats), extra.reshape(-1, 3, 3)])


def main(ref):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, ref)
    from renderih_amd import assets, joint_fit
    from renderih_amd.manolayer import rodrigues_batch
    t3d, ax = types.ModuleType('transforms3d'), types.ModuleType('transforms3d.axangles')
    ax.axangle2mat, t3d.axangles = _axangle2mat, ax
    sys.modules['transforms3d'], sys.modules['transforms3d.axangles'] = t3d, ax
    d = os.path.join(ref, 'utils', 'mano_from_3djoint')
    aik, utl, man = (_load('ref_jf_' + n, os.path.join(d, n + '.py')) for n in ('AIK', 'utils', 'manolayer'))
    src = open(os.path.join(d, 'convert2mano.py')).read().split('\n')
    assert src[12].startswith('class OptimizationSMPL') and src[159].startswith('for hand in') and 'ori_pose = ' in src[230]
    program = compile('\n'.join(src[158:204] + src[224:231] + ['    _finish(hand, parameters_smpl, ori_pose)']), 'convert2mano', 'exec')

    rec = {}
    layers, mirrors = {}, {}
    with tempfile.TemporaryDirectory() as tmp:
        for side in ('right', 'left'):
            pkl = assets.write_synthetic_mano_pkl(os.path.join(tmp, 'MANO_%s.pkl' % side.upper()), side, seed=0)
            layer = man.ManoLayer(manoPath=pkl)
            if side == 'left':
                layer.shapedirs[:, 0, :] *= -1

            def forward(*a, _f=layer.forward, _side=side):
                out = _f(*a)
                rec[_side]['layer'].append((a[0].detach().clone(), a[2].detach().clone(), out[1].detach().clone()))
                return out
            layer.forward = forward
            layers[side] = layer
            m = {}
            for dt in (torch.float32, torch.float64):
                mine = joint_fit.ManoLayer(assets.synthetic_mano_dict(side, seed=0))
                if side == 'left':
                    mine.shapedirs[:, 0, :] *= -1
                m[dt] = joint_fit.ManoJointFitter(mine, dtype=dt)
            mirrors[side] = m

    def family(side, seed):
        rs = np.random.RandomState(1000 * seed + (side == 'left'))
        f = mirrors[side][torch.float64]
        j = joint_fit._mano_mirror(f._constants(), rodrigues_batch(torch.tensor(rs.randn(1, 3) * 0.8)),
                                   torch.tensor(rs.randn(1, 45) * 0.6), torch.tensor(rs.randn(1, 10) * 0.5))[1][0]
        return (j.numpy() * 110 + rs.randn(1, 3) * 20).astype(np.float32)

    def rec_aik(T, P):
        out = aik.adaptive_IK(T, P)
        rec[rec['hand']]['aik'].append((T.copy(), P.copy(), out.copy()))
        return out

    def rec_mat2aa(R):
        rec[rec['hand']]['mat2aa'].append(R.detach().clone())
        return utl.mat2aa(R)

    def finish(hand, params, ori_pose):
        rec[hand]['final'] = (params.pose.detach().clone(), params.beta.detach().clone(), ori_pose.clone())

    cls_ns = {'torch': torch}
    exec(compile('\n'.join(src[12:20]), 'convert2mano', 'exec'), cls_ns)
    out = {k: [] for k in ('joints', 'side', 'aik', 'pre', 'aik_pre', 'traj_P', 'traj_beta', 'hist', 'final_P', 'final_beta', 'ori_pose')}
    for seed in SEEDS:
        for side in ('right', 'left'):
            rec[side] = {'layer': [], 'aik': [], 'mat2aa': []}
        ori_joints = {side: family(side, seed).astype(np.float64) for side in ('right', 'left')}

        class Layers(dict):
            def __getitem__(self, hand):
                rec['hand'] = hand
                return dict.__getitem__(self, hand)
        ns = {'torch': torch, 'np': np, 'adaptive_IK': rec_aik, 'mat2aa': rec_mat2aa, 'OptimizationSMPL': cls_ns['OptimizationSMPL'],
              'cur_mano_layer': Layers(layers), 'ori_joints': ori_joints, '_finish': finish}
        exec(program, ns)
        for side in ('right', 'left'):
            r = rec[side]
            assert len(r['layer']) == 201 and len(r['mat2aa']) == 202 and len(r['aik']) == 1
            T, pre, R = r['aik'][0]
            assert np.isfinite(R).all() and abs(np.linalg.det(R[0, 0]) - 1) < 1e-9
            joints = ori_joints[side].astype(np.float32)
            target = torch.from_numpy((ori_joints[side] - ori_joints[side][0:1]) / 100).float()
            hist = []
            for root, beta, j in r['layer'][1:]:
                hist.append(float(torch.abs((j - j[:, 0:1]) - target).mean()))
            assert np.isfinite(hist).all()
            P = [torch.cat([r['layer'][1 + i][0].view(1, 1, 3, 3), r['mat2aa'][1 + i].view(1, 15, 3, 3)], 1) for i in range(PREFIX + 1)]
            out['joints'].append(joints)
            out['side'].append(np.int32(side == 'left'))
            out['template/' + side] = T.astype(np.float32)
            out['aik'].append(R[0])
            out['pre'].append(pre.astype(np.float32))
            out['aik_pre'].append(aik.adaptive_IK(T, pre.astype(np.float32))[0])
            out['traj_P'].append(torch.cat(P).numpy())
            out['traj_beta'].append(torch.cat([r['layer'][1 + i][1] for i in range(PREFIX + 1)]).numpy())
            out['hist'].append(np.asarray(hist, np.float32))
            out['final_P'].append(r['final'][0][0].numpy())
            out['final_beta'].append(r['final'][1][0].numpy())
            out['ori_pose'].append(r['final'][2][0].numpy())
            # this repository's mirrors over the prefix: the fp32 one must stay near the fp64 one
            runs = {}
            for dt, f in mirrors[side].items():
                f.n_iter = 200
                f.start(torch.from_numpy(joints)[None])
                snaps = []
                for _ in range(PREFIX):
                    f.run(1)
                    snaps.append(torch.cat([f.P.detach().reshape(-1), f.beta.detach().reshape(-1)]).double())
                runs[dt] = torch.stack(snaps)
            dev = float((runs[torch.float32] - runs[torch.float64]).abs().max() / runs[torch.float64].abs().max())
            ref_dev = float((torch.cat([P[PREFIX].reshape(-1), r['layer'][1 + PREFIX][1].reshape(-1)]).double()
                             - runs[torch.float64][PREFIX - 1]).abs().max() / runs[torch.float64].abs().max())
            print('%s seed %d: loss %.3g -> %.3g (after %d) -> %.3g; fp32 mirror vs fp64 mirror over the prefix %.3g, reference '
                  'fp32 vs fp64 mirror at its end %.3g' % (side, seed, hist[0], hist[PREFIX], PREFIX, hist[-1], dev, ref_dev))
            assert dev < 1e-3, 'a chaotic hand in the prefix'
    res = {k: (np.stack(v) if isinstance(v, list) else v) for k, v in out.items()}
    rs = np.random.RandomState(7)
    Rm = torch.tensor(crafted_matrices(rs, res['aik']), requires_grad=True)
    w = torch.tensor(rs.randn(Rm.shape[0], 3))
    aa = utl.mat2aa(Rm)
    grad, = torch.autograd.grad((aa * w).sum(), Rm)
    assert torch.isfinite(aa).all() and torch.isfinite(grad).all(), 'a crafted matrix sits on one of the NaN rules'
    res.update(m2a_R=Rm.detach().numpy(), m2a_aa=aa.detach().numpy(), m2a_w=w.numpy(), m2a_grad=grad.numpy())
    path = os.path.join(HERE, 'joint_fit.npz')
    np.savez(path, **res)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
