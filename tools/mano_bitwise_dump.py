#!/usr/bin/env python
"""Bitwise check that a change to csrc/rih_mano.hip leaves `renderih_amd.manolayer.ManoLayer` alone: dump v, j, the five
input gradients and the packed basis at B = 128 with a fixed seed (PCA input, rotation-matrix input with new_skel, PCA input
centred on a finger tip; translation and scale given) from two builds, then compare the dumps bit for bit.

    python tools/mano_bitwise_dump.py dump <root of a built tree> parent.npz      # e.g. a worktree of the parent commit
    python tools/mano_bitwise_dump.py dump . branch.npz
    python tools/mano_bitwise_dump.py compare parent.npz branch.npz               # exit status 1 if any array differs
"""
import os
import sys

import numpy as np


def dump(pkg_root, out):
    import torch
    pkg_root = os.path.abspath(pkg_root)
    sys.path.insert(0, pkg_root)
    import renderih_amd
    from renderih_amd import assets
    from renderih_amd.manolayer import ManoLayer
    assert os.path.abspath(renderih_amd.__file__).startswith(pkg_root), renderih_amd.__file__
    dev = torch.device('cuda:0')
    B = 128
    res = {}
    for tag, use_pca, new_skel, center in (('pca', True, False, 9), ('rotmat', False, True, 0), ('pca_tip', True, False, 8)):
        layer = ManoLayer(assets.synthetic_mano_dict('right', seed=0), center_idx=center, use_pca=use_pca, new_skel=new_skel).to(dev)
        g = torch.Generator().manual_seed(1234)
        root = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
        pose = torch.randn(B, 30, generator=g) * 0.5 if use_pca else torch.linalg.qr(torch.randn(B, 15, 3, 3, generator=g))[0]
        shape, trans = torch.randn(B, 10, generator=g), torch.randn(B, 3, generator=g) * 0.1
        scale = torch.rand(B, generator=g) + 0.5
        wv, wj = torch.rand(B, 778, 3, generator=g), torch.rand(B, 21, 3, generator=g)
        ins = [t.to(dev).requires_grad_(True) for t in (root, pose, shape, trans, scale)]
        v, j = layer(*ins)
        grads = torch.autograd.grad((wv.to(dev) * v).sum() + (wj.to(dev) * j).sum(), ins)
        res[tag + '/v'], res[tag + '/j'] = v.detach().cpu().numpy(), j.detach().cpu().numpy()
        for n, gr in zip(('root', 'pose', 'shape', 'trans', 'scale'), grads):
            res[tag + '/d_' + n] = gr.cpu().numpy()
        res[tag + '/packed'] = layer._pack_cache[1].cpu().numpy()
    np.savez(out, **res)
    print('dumped', out, len(res), 'arrays')


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert set(a.files) == set(b.files), (a.files, b.files)
    bad = 0
    print('ManoLayer at B = 128, fixed seed: %s against %s, bitwise' % (os.path.basename(pa), os.path.basename(pb)))
    for k in sorted(a.files):
        same = a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
        bad += not same
        print('%-18s %-16s %s' % (k, a[k].shape, 'bitwise equal' if same else 'DIFFERENT: max |diff| %g' % np.abs(a[k] - b[k]).max()))
    print('RESULT:', 'all %d arrays bitwise equal' % len(a.files) if not bad else '%d arrays differ' % bad)
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == 'dump':
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
