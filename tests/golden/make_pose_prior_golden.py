#!/usr/bin/env python
"""Golden vectors of the pose optimiser's hand-prior and contact terms from the REFERENCE's own program:
pose_data_optimize/hocontact/postprocess/geo_loss.py (`HandLoss.batch_pose_quat_norm_loss`, `get_edge_idx`, `get_edge_len`,
`edge_len_loss`, `hand_pose_ergonomics_loss`, `FieldLoss.batch_contact_loss`) and scripts/HandPoseConverter.py
(`HandPoseConverter`, data_type='tensor', device='cpu'), imported from a reference checkout at generation time and run
unmodified on the CPU.

Imports: `reference_modules` of make_quat_mano_golden.py (synthetic MANO through the stubbed chumpy loader, the checkout's
manopth first on sys.path), then pose_data_optimize/ itself on the path, and EMPTY stand-in modules for open3d and trimesh (both
are imported at module top there, neither is used by these functions, neither is installed here).

Writes tests/golden/pose_prior.npz.  Per side: the two axis tables; for a B = 4 batch of un-normalised quaternions the
converter's matrices of the normalised batch, the ergonomics loss and its autograd gradient with respect to the UN-normalised
quaternions through manopth's normalize_quaternion, the quaternion-norm loss and gradient; the edge table (from the RIGHT
hand's faces for both sides, as the optimiser builds it), static lengths of the side's rest mesh (identity quaternions, zero
betas, center_idx=0), edge loss and vertex gradient at B = 2.  Contact: B = 2, A = 32, D = 4 with padded (masked-out)
entries, elastic 0 on some unmasked entries and nonzero on one masked-out entry, and a D = 1 case.  Total: the sum as loss_fn
builds it for mode='both' (lambda_contact_loss = 10) over the first two samples, and its seven terms.

Asserted here (another seed is tried until they hold; nothing is excused at test time): no splay or bend angle within 0.05
degrees of a range limit, no thumb twist cosine within 1e-3 of 0.5, no bend within 0.05 degrees of 0, |x_axis[..., :2]| > 1e-2;
every branch is taken in each side's batch (an angle above a range, one below, a negative bend that step 4 clamps, the pinky
term active, the thumb twist term active); two runs write identical arrays.
       python tests/golden/make_pose_prior_golden.py <reference checkout>"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_quat_mano_golden import reference_modules  # noqa: E402

B, A = 4, 32
SPLAY = {0: (-25, 15), 3: (-15, 15), 9: (-25, 15), 6: (-20, 30), 12: (-30, 30)}
BEND = {0: (-25, 70), 1: (-4, 110), 3: (-25, 80), 4: (-7, 100), 9: (-25, 70), 10: (-10, 100), 6: (-22, 70), 7: (-8, 90),
        12: (-20, 40), 13: (-35, 50), 14: (-10, 100), 2: (-8, 90), 5: (-8, 90), 11: (-8, 90), 8: (-8, 90)}


def quaternions(rs):
    """[B,16,4]: rotations by up to ~80 degrees about random axes, norms in [0.7, 1.4]."""
    axis = rs.randn(B, 16, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * rs.uniform(0.0, 1.4, size=(B, 16, 1))
    q = np.concatenate([np.cos(half), np.sin(half) * axis], -1) * rs.uniform(0.7, 1.4, size=(B, 16, 1))
    return q.astype(np.float32)


def conditions(rel):
    """rel [B,15,3,3] relative frames -> (well away from every kink, every branch taken)."""
    x = rel[..., 0]
    bend = np.degrees(np.arctan2(x[..., 1], x[..., 0]))
    splay = np.degrees(np.arctan2(-x[..., 2], x[..., 0]))
    twist = (rel[:, 12, 2, 1] - rel[:, 12, 1, 2]) / 2
    safe = (np.abs(x[..., :2]) > 1e-2).all() and (np.abs(bend) > 0.05).all() and (np.abs(twist - 0.5) > 1e-3).all()
    above = below = False
    for table, angle in ((SPLAY, splay), (BEND, bend)):
        for j, (lo, hi) in table.items():
            safe = safe and (np.abs(angle[:, j] - lo) > 0.05).all() and (np.abs(angle[:, j] - hi) > 0.05).all()
            above, below = above or (angle[:, j] > hi).any(), below or (angle[:, j] < lo).any()
    pos = np.maximum(bend, 0)
    pinky = pos[:, 10] - 0.75 * pos[:, 7]
    clamped = ((bend[:, 10] < 0) | (bend[:, 7] < 0)).any()
    return bool(safe), bool(above and below and clamped and (pinky < 0).any() and (twist > 0.5).any())


def contact_case(rs, D):
    ids = rs.randint(0, A, size=(2, A, D))
    mask = (rs.rand(2, A, D) < 0.6).astype(np.int64)
    elastic = (rs.rand(2, A, D) * mask).astype(np.float32)
    unmasked = np.argwhere(mask == 1)
    for k in unmasked[:: max(1, len(unmasked) // 5)]:
        elastic[tuple(k)] = 0.0                                   # elastic 0 on some unmasked entries
    off = np.argwhere(mask == 0)
    assert len(off) > 3
    elastic[tuple(off[1])] = 0.7                                  # nonzero on one masked-out entry: still counted
    ids[mask == 0] = 0                                            # padded entries point at anchor 0
    main = (rs.randn(2, A, 3) * 0.02).astype(np.float32)
    sub = (rs.randn(2, A, 3) * 0.02).astype(np.float32)
    return ids, mask, elastic, main, sub


def generate(ref):
    ManoLayer, _ = reference_modules(ref)
    sys.path.insert(1, os.path.join(ref, 'pose_data_optimize'))
    for name in ('open3d', 'trimesh'):
        sys.modules.setdefault(name, types.ModuleType(name))
    from hocontact.postprocess.geo_loss import FieldLoss, HandLoss
    from manopth.quatutils import normalize_quaternion
    from scripts.HandPoseConverter import HandPoseConverter
    T = torch.from_numpy
    out, keep = {}, {}
    ident = torch.zeros(1, 16, 4)
    ident[..., 0] = 1.0
    for si, side in enumerate(('right', 'left')):
        hpc = HandPoseConverter(side=side, root='mano/models', data_type='tensor', device='cpu')
        zero = hpc.mano_quat_2_mat_tensor(ident)
        k = side + '/'
        out[k + 'inv_m_u_0'], out[k + 'inv_u_m_1'] = hpc.invM_U_n_0.numpy(), hpc.invU_M_n_1.numpy()
        for seed in range(5100 + 1000 * si, 5100 + 1000 * si + 500):
            q = T(quaternions(np.random.RandomState(seed))).requires_grad_(True)
            ja = hpc.mano_quat_2_mat_tensor(normalize_quaternion(q))
            rel = (zero.repeat(B, 1, 1, 1)[:, 1:].transpose(3, 2) @ ja[:, 1:]).detach().numpy()
            safe, covered = conditions(rel)
            if safe and covered:
                break
        else:
            raise AssertionError('no seed meets the conditions for the %s hand' % side)
        ergo = HandLoss.hand_pose_ergonomics_loss(ja[:, 1:], zero.repeat(B, 1, 1, 1)[:, 1:], side[0])
        g_ergo, = torch.autograd.grad(ergo, q)
        assert torch.isfinite(g_ergo).all() and float(ergo) > 0
        qn = HandLoss.batch_pose_quat_norm_loss(q)
        g_qn, = torch.autograd.grad(qn, q)
        out[k + 'seed'], out[k + 'q'], out[k + 'mat'] = np.int32(seed), q.detach().numpy(), ja.detach().numpy()
        out[k + 'ergo'], out[k + 'grad_ergo'] = ergo.detach().numpy(), g_ergo.numpy()
        out[k + 'quat_norm'], out[k + 'grad_quat_norm'] = qn.detach().numpy(), g_qn.numpy()
        # edges: the optimiser builds BOTH hands' tables from the main (right) hand's faces; rest mesh of this side
        right = ManoLayer(joint_rot_mode='quat', root_rot_mode='quat', use_pca=False, mano_root='mano/models', center_idx=0,
                          flat_hand_mean=True, return_transf=True, return_full_pose=True, side='right')
        layer = ManoLayer(joint_rot_mode='quat', root_rot_mode='quat', use_pca=False, mano_root='mano/models', center_idx=0,
                          flat_hand_mean=True, return_transf=True, return_full_pose=True, side=side)
        edges = HandLoss.get_edge_idx(right.th_faces)
        rest = layer(ident.reshape(1, 64), torch.zeros(1, 10))[0]
        static = HandLoss.get_edge_len(rest, edges)
        rs = np.random.RandomState(seed + 7)
        small = q.detach()[:2].clone()
        small[:, :, 1:] *= 0.2                                     # gentle poses: the synthetic skinning weights are random
        posed = layer(small.reshape(2, 64), T((rs.randn(2, 10) * 0.5).astype(np.float32)))[0].detach()
        verts = (posed + T((rs.randn(2, 778, 3) * 3e-4).astype(np.float32))).requires_grad_(True)
        el = HandLoss.edge_len_loss(verts, edges, static)
        g_el, = torch.autograd.grad(el, verts)
        out[k + 'edges'], out[k + 'static_len'] = edges.numpy(), static[0].detach().numpy()
        out[k + 'verts'], out[k + 'edge'], out[k + 'grad_edge'] = verts.detach().numpy(), el.detach().numpy(), g_el.numpy()
        keep[side] = (hpc, zero, q.detach()[:2].clone(), verts.detach().clone(), edges, static)
    for name, D in (('contact', 4), ('contact_d1', 1)):
        ids, mask, elastic, main, sub = contact_case(np.random.RandomState(77 + D), D)
        am, asub = T(main).requires_grad_(True), T(sub).requires_grad_(True)
        indexed = am.unsqueeze(2).repeat(1, 1, D, 1).gather(1, T(ids).unsqueeze(-1).repeat(1, 1, 1, 3))      # loss_fn:603-606
        cl = FieldLoss.batch_contact_loss(indexed, asub.unsqueeze(2).repeat(1, 1, D, 1), T(mask), T(elastic))
        g_main, g_sub = torch.autograd.grad(cl, (am, asub))
        k = name + '/'
        out[k + 'anchor_id'], out[k + 'mask'], out[k + 'elastic'] = ids, mask, elastic
        out[k + 'anchors_main'], out[k + 'anchors_sub'] = main, sub
        out[k + 'loss'], out[k + 'grad_main'], out[k + 'grad_sub'] = cl.detach().numpy(), g_main.numpy(), g_sub.numpy()
        if D == 4:
            contact = (ids, mask, elastic, main, sub)
    # the sum as loss_fn builds it (:805-824, mode='both', lambda_contact_loss = 10), right = main hand, left = sub hand
    ids, mask, elastic, main, sub = contact
    leaves, terms = [], {}
    for side in ('right', 'left'):
        hpc, zero, q, verts, edges, static = keep[side]
        q, verts = q.requires_grad_(True), verts.requires_grad_(True)
        leaves += [q, verts]
        ja = hpc.mano_quat_2_mat_tensor(normalize_quaternion(q))
        terms[side] = (HandLoss.batch_pose_quat_norm_loss(q), HandLoss.edge_len_loss(verts, edges, static),
                       HandLoss.hand_pose_ergonomics_loss(ja[:, 1:], zero.repeat(2, 1, 1, 1)[:, 1:], side[0]))
    am, asub = T(main).requires_grad_(True), T(sub).requires_grad_(True)
    indexed = am.unsqueeze(2).repeat(1, 1, 4, 1).gather(1, T(ids).unsqueeze(-1).repeat(1, 1, 1, 3))
    cl = FieldLoss.batch_contact_loss(indexed, asub.unsqueeze(2).repeat(1, 1, 4, 1), T(mask), T(elastic))
    quat_norm = terms['right'][0] + terms['left'][0]
    edge = terms['right'][1] + terms['left'][1]
    ergo = terms['right'][2] + terms['left'][2]
    total = 1.0 * quat_norm + 1.0 * edge + 1 * 10.0 * cl + 1. * ergo
    grads = torch.autograd.grad(total, leaves + [am, asub])
    out['total/loss'] = total.detach().numpy()
    out['total/terms'] = np.array([float(t) for t in (terms['right'][0], terms['left'][0], terms['right'][1],
                                                      terms['left'][1], cl, terms['right'][2], terms['left'][2])], np.float32)
    for name, g in zip(('q_r', 'verts_r', 'q_l', 'verts_l', 'anchors_r', 'anchors_l'), grads):
        out['total/grad_' + name] = g.numpy()
    return out


def main(ref):
    out = generate(ref)
    again = generate(ref)
    assert set(out) == set(again) and all(np.array_equal(out[k], again[k]) for k in out), 'two runs differ'
    path = os.path.join(HERE, 'pose_prior.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes; seeds', int(out['right/seed']), int(out['left/seed']))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
