#!/usr/bin/env python
"""Bitwise check that a change to csrc/rih_mano.hip leaves `renderih_amd.manolayer.ManoLayer` alone: dump v, j, the five
input gradients and the packed basis at B = 128 with a fixed seed (PCA input, rotation-matrix input with new_skel, PCA input
centred on a finger tip; translation and scale given) from two builds, then compare the dumps bit for bit.

    python tools/mano_bitwise_dump.py dump <root of a built tree> parent.npz      # e.g. a worktree of the parent commit
    python tools/mano_bitwise_dump.py dump . branch.npz
    python tools/mano_bitwise_dump.py compare parent.npz branch.npz               # exit status 1 if any array differs

A second dump set, `dump <root> out.npz losses`, does the same for the two fused training losses (csrc/rih_loss.hip,
csrc/rih_mano_loss.hip, csrc/rih_mesh_terms.h): FusedMeshLoss and FusedManoLoss at B = 5, epoch 0 and 60 -- total, term
vector and every gradient.  The set defaults to `mano`.
"""
import os
import sys

import numpy as np


def dump(pkg_root, out, which='mano'):
    import torch
    pkg_root = os.path.abspath(pkg_root)
    sys.path.insert(0, pkg_root)
    import renderih_amd
    assert os.path.abspath(renderih_amd.__file__).startswith(pkg_root), renderih_amd.__file__
    res = {'mano': dump_mano, 'losses': dump_losses}[which](torch.device('cuda:0'))
    np.savez(out, **res)
    print('dumped', out, len(res), 'arrays')


def dump_mano(dev):
    import torch
    from renderih_amd import assets
    from renderih_amd.manolayer import ManoLayer
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
    return res


def dump_losses(dev):
    """Inputs that take both SmoothL1 branches of every term (vertex errors around 1, image 1 of the batch moved by 2 so that
    its joints are off by more than 1, edge lengths around 1), with a zero-length predicted edge in face 0 of image 0, an
    all-zero rotation, and root_rel on the right hand."""
    import torch
    from renderih_amd import assets
    from renderih_amd.decoder import GCN_vert_convert
    from renderih_amd.loss import FusedManoLoss, FusedMeshLoss, ManoLoss
    B, sides = 5, ('left', 'right')
    g = torch.Generator().manual_seed(4321)
    conv, gl, t = {}, {}, {}
    for s in sides:
        gd, md = assets.load_graph_dict(s), assets.synthetic_mano_dict(s)
        conv[s] = GCN_vert_convert(vertex_num=778, graph_perm_reverse=gd['graph_perm_reverse'], graph_perm=gd['graph_perm'])
        J = torch.from_numpy(np.asarray(md['J_regressor'].todense(), np.float32))
        gl[s] = ManoLoss(J, np.asarray(md['f']), level=4, device=dev,
                         upsample_weight=torch.from_numpy(assets.synthetic_upsample_weight()))
        t['gt3_' + s] = 0.05 * torch.randn(B, 778, 3, generator=g)
        t['gt2_' + s] = 256 * torch.rand(B, 778, 2, generator=g)
        t['v3d_' + s] = t['gt3_' + s] + 0.8 * torch.randn(B, 778, 3, generator=g)
        t['v3d_' + s][1] += 2.0
        f0 = np.asarray(md['f'])[0]
        t['v3d_' + s][0, int(f0[1])] = t['v3d_' + s][0, int(f0[0])]
        t['v2d_' + s] = t['gt2_' + s] + 20 * torch.randn(B, 778, 2, generator=g)
        t['c3d_' + s] = 0.8 * torch.randn(B, 252, 3, generator=g)
        t['c2d_' + s] = 256 * torch.rand(B, 252, 2, generator=g)
        t['gtpose_' + s] = torch.randn(B, 48, generator=g)
        t['pose_' + s] = t['gtpose_' + s] + 0.5 * torch.randn(B, 48, generator=g)
        t['gtshape_' + s] = torch.randn(B, 10, generator=g)
        t['shape_' + s] = 3 * torch.tanh(torch.randn(B, 10, generator=g))
    t['pose_left'][0, :3] = 0.0
    t['root_rel'] = 0.05 * torch.randn(B, 3, generator=g)
    t['rel'] = t['root_rel'] + 0.05 * torch.randn(B, 3, generator=g)
    t = {k: v.to(dev) for k, v in t.items()}
    both = lambda k: {s: t[k + s] for s in sides}                                       # noqa: E731
    gts = (t['gt2_left'], t['gt2_right'], t['gt3_left'], t['gt3_right'], t['root_rel'])
    mesh, mano = FusedMeshLoss(gl['left'], gl['right'], conv['left'], conv['right']), FusedManoLoss(gl['left'], gl['right'])
    res = {}
    for epoch in (0, 60):
        for tag, preds in (('mesh', ('v3d_', 'v2d_', 'c3d_', 'c2d_')), ('mano', ('v3d_', 'v2d_', 'pose_', 'shape_'))):
            names = [p + s for p in preds for s in sides] + (['rel'] if tag == 'mano' else [])
            for k in names:
                t[k] = t[k].detach().requires_grad_(True)
            result = {'verts3d': both('v3d_'), 'verts2d': both('v2d_')}
            if tag == 'mesh':
                total, terms = mesh(epoch, result, [{'verts3d': both('c3d_'), 'verts2d': both('c2d_')}], *gts)
            else:
                other = {'root_rel': t['rel'], 'verts3d_MANO_list': {s: {'mano_pose': t['pose_' + s],
                                                                         'mano_shape': t['shape_' + s]} for s in sides}}
                total, terms = mano(epoch, result, other, *gts, t['gtpose_left'], t['gtshape_left'], t['gtpose_right'],
                                    t['gtshape_right'])
                terms = torch.stack([terms[k] for k in sorted(terms)])
            key = '%s_e%d/' % (tag, epoch)
            res[key + 'total'], res[key + 'terms'] = total.detach().cpu().numpy(), terms.detach().cpu().numpy()
            for k, gr in zip(names, torch.autograd.grad(total, [t[k] for k in names])):
                res[key + 'd_' + k] = gr.cpu().numpy()
    return res


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert set(a.files) == set(b.files), (a.files, b.files)
    bad = 0
    print('fixed seed: %s against %s, bitwise' % (os.path.basename(pa), os.path.basename(pb)))
    for k in sorted(a.files):
        same = a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))
        bad += not same
        print('%-18s %-16s %s' % (k, a[k].shape, 'bitwise equal' if same else 'DIFFERENT: max |diff| %g' % np.abs(a[k] - b[k]).max()))
    print('RESULT:', 'all %d arrays bitwise equal' % len(a.files) if not bad else '%d arrays differ' % bad)
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) in (4, 5) and sys.argv[1] == 'dump' and sys.argv[4:] in ([], ['mano'], ['losses']):
        dump(*sys.argv[2:])
    elif len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
