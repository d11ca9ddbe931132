"""Generate tests/golden/mano_loss.npz by running the REAL reference loss of the MANO-head model (core/Loss_mano.py:
ManoLoss + mano_loss_GCN, the recipe core/lijun_trainer.py:215-283 trains `load_new_model` with) on CPU.

Run in the build container only:  python tests/golden/make_mano_loss_golden.py
Cases (B = 2): epoch 0 (edge term off) and 60 (on) without an up-sampling weight, and epoch 60 with one (the value-only
upsample_norm_loss).  Pose predictions and labels each hold one rotation of exactly zero.  Stored: the inputs, every term,
the total, and the gradients with respect to every prediction tensor.  Seeded: two runs write identical arrays.
"""
import os
import pickle
import sys
import tempfile
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
import ref_stubs  # noqa: E402

ref_stubs.install()                     # puts the reference checkout first on sys.path
warnings.filterwarnings('ignore')

import importlib.util  # noqa: E402


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


assets = _load('rih_assets', os.path.join(ROOT, 'renderih_amd', 'assets.py'))

PREDS = ['v3d_left', 'v3d_right', 'v2d_left', 'v2d_right', 'pose_left', 'pose_right', 'shape_left', 'shape_right',
         'rootrel_pred']
TERMS = ['vert2d_loss', 'vert3d_loss', 'joint_loss', 'norm_loss', 'edge_loss', 'pose_loss', 'shape_loss', 'rootrel_loss',
         'regularize_loss', 'upsample_norm_loss']
CASES = [('e0', 0, False), ('e60', 60, False), ('e60up', 60, True)]


def inputs(B=2, seed=321):
    g = torch.Generator().manual_seed(seed)
    t = {}
    for s in ('left', 'right'):
        t['v3d_gt_' + s] = 0.05 * torch.randn(B, 778, 3, generator=g)
        t['v2d_gt_' + s] = 256 * torch.rand(B, 778, 2, generator=g)
        t['v3d_' + s] = t['v3d_gt_' + s] + 0.02 * torch.randn(B, 778, 3, generator=g)
        t['v2d_' + s] = t['v2d_gt_' + s] + 8 * torch.randn(B, 778, 2, generator=g)
        t['pose_gt_' + s] = 0.6 * torch.randn(B, 48, generator=g)
        t['pose_' + s] = t['pose_gt_' + s] + 0.3 * torch.randn(B, 48, generator=g)
        t['shape_gt_' + s] = torch.randn(B, 10, generator=g)
        t['shape_' + s] = t['shape_gt_' + s] + 0.5 * torch.randn(B, 10, generator=g)
    t['v3d_left'][0, :5] += 3.0                      # both SmoothL1 branches
    t['pose_left'][0, 3:6] = 0.0                     # a predicted rotation of exactly zero (batch_rodrigues' 1e-8 shift)
    t['pose_gt_right'][1, 9:12] = 0.0                # and a label one
    t['pose_right'][1, :3] = 1e-6                    # a tiny one
    t['root_rel'] = 0.05 * torch.randn(B, 3, generator=g)
    t['rootrel_pred'] = t['root_rel'] + 0.02 * torch.randn(B, 3, generator=g)
    w0 = torch.from_numpy(assets.synthetic_upsample_weight())
    # a trained-looking w: w0 plus a structured offset (compresses, unlike noise; the .npz stays small)
    i = torch.arange(w0.numel(), dtype=torch.float32).reshape(w0.shape)
    t['upsample_weight'] = w0 * 1.25 + 0.002 * (torch.remainder(i, 7.0) - 3.0)
    return t


def main():
    import core.Loss_mano as RefLoss                    # reference (utils.manoutils -> cv2 / yacs stubs)
    from utils.config import load_cfg
    tmp = tempfile.mkdtemp()
    up = os.path.join(tmp, 'upsample.pkl')
    with open(up, 'wb') as f:
        pickle.dump(assets.synthetic_upsample_weight(), f)
    RefLoss.get_upsample_path = lambda: up              # misc/upsample.pkl is not in the checkout
    cfg = load_cfg(os.path.join(ref_stubs.REF, 'utils', 'defaults.yaml'))
    torch.set_num_threads(1)
    loss = {}
    for s in ('left', 'right'):
        md = assets.synthetic_mano_dict(s)
        J = torch.from_numpy(np.asarray(md['J_regressor'].todense(), np.float32))
        loss[s] = RefLoss.ManoLoss(J, np.asarray(md['f']), level=4, device='cpu')
    t0 = inputs()
    store = {'in/' + k: v.numpy().copy() for k, v in t0.items()}
    for key, epoch, with_up in CASES:
        t = {k: v.clone().requires_grad_(k in PREDS) for k, v in t0.items()}
        B = t['v3d_left'].shape[0]
        result = {'verts3d': {s: t['v3d_' + s] for s in ('left', 'right')},
                  'verts2d': {s: t['v2d_' + s] for s in ('left', 'right')}}
        other = {'root_rel': t['rootrel_pred'],
                 'verts3d_MANO_list': {s: {'mano_pose': t['pose_' + s], 'mano_shape': t['shape_' + s]}
                                       for s in ('left', 'right')}}
        z = torch.zeros(B, 21, 3)
        total, aux, terms, coarse = RefLoss.mano_loss_GCN(
            cfg, epoch, loss['left'], loss['right'], None, None, result, None, [], other, None, None, None,
            t['v2d_gt_left'], None, t['v2d_gt_right'], None, t['v3d_gt_left'], z, t['v3d_gt_right'], z, t['root_rel'], 256,
            t['pose_gt_left'], t['shape_gt_left'], t['pose_gt_right'], t['shape_gt_right'],
            upsample_weight=t['upsample_weight'].detach() if with_up else None)
        assert aux == {'total_loss': 0} and coarse == {} and sorted(terms) == sorted(TERMS)
        total.backward()
        store[key + '/total'] = np.float64(total.item())
        for k in TERMS:
            store[key + '/' + k] = np.float64(terms[k].item())
        for k in PREDS:
            store[key + '/grad_' + k] = t[k].grad.numpy().copy()
    path = os.path.join(HERE, 'mano_loss.npz')
    np.savez_compressed(path, **store)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(store), 'arrays')


if __name__ == '__main__':
    main()
