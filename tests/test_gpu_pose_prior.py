"""Fused hand-prior and contact loss (renderih_amd.pose_prior.FusedTwoHandPriorLoss, csrc/rih_pose_prior.hip) on the GPU: the
reference's golden total, the fused kernels against the fp64 mirror at B = 1, 3, 32 with D = 1 and 4 on the 778-vertex mesh and
on a 5-vertex mesh with an isolated vertex, bit-identical repeats, terms against the loss, and the optimiser's whole
differentiable chain (quaternions -> both meshes -> anchors -> penetration + contact + priors -> quaternion and translation
gradients) captured in one graph and replayed on other poses.  Helpers and tolerances: tests/test_pose_prior.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from quat_mano_cases import ANCHOR_DIR, mano_dict  # noqa: E402
from test_gpu_quat_mano import chain_poses  # noqa: E402
from test_gpu_two_hand_sdf import PART_VERT  # noqa: E402
from test_pose_prior import (CASES, INPUTS, TERM_RTOL, UPSTREAM, compare, fused_vs_fp64_mirror, golden, golden_total_case,  # noqa: E402
                             module, relative_deviation, seeded_case)
from test_two_hand_sdf import grad_tol  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def test_fused_matches_reference_golden():
    z = golden()
    got = fused_vs_fp64_mirror(golden_total_case(), dev(), 'fused vs fp64 mirror, golden case')
    want = {'loss': z['total/loss'], 'terms': z['total/terms']}
    want.update({'grad_' + k: z['total/grad_' + k] * np.float32(UPSTREAM) for k in INPUTS})
    compare(got, want, 'fused vs golden')


@pytest.mark.parametrize('B,D,mesh', CASES)
def test_fused_matches_fp64_mirror(B, D, mesh):
    """Also: two evaluations are bit-identical, terms (contact weighted) add up to the loss, and on the small mesh the
    isolated vertex gets an exact zero."""
    got = fused_vs_fp64_mirror(seeded_case(B, D, mesh), dev(), 'fused vs fp64 mirror B=%d D=%d %s' % (B, D, mesh))
    if mesh == 'small':
        for k in ('grad_verts_r', 'grad_verts_l'):
            assert not got[k][:, 4].any() and np.abs(got[k][:, :4]).min() > 0


def test_empty_mask_gives_zero_loss_and_zero_gradients():
    from renderih_amd.pose_prior import FusedTwoHandPriorLoss
    from test_pose_prior import evaluate
    case = seeded_case(3, 4, 'mano')
    case['mask'] = np.zeros_like(case['mask'])
    got = evaluate(module(FusedTwoHandPriorLoss), case, dev())
    assert got['terms'][4] == 0.0 and not got['grad_anchors_r'].any() and not got['grad_anchors_l'].any()
    assert got['terms'][0] > 0 and np.abs(got['grad_q_r']).max() > 0


def test_whole_objective_chain_inside_a_captured_graph():
    """right and left FusedQuatManoLayer -> FusedAnchorLayer x 2 -> FusedTwoHandSDFLoss (G = 8) + FusedTwoHandPriorLoss ->
    backward to quaternions and translations, captured once and replayed on OTHER poses: bit-identical to the eager evaluation
    of those.  Against the mirrors: the fused prior on the chain's own meshes and anchors against the mirror prior on the SAME
    tensors (TERM_RTOL: the inputs are identical, so the bar of the operator applies); the end-to-end gradients against the
    chain built from the mirrors at grad_tol(G) of the largest entry, the bar of the existing chain test (the penetration
    loss's, the loosest link)."""
    from renderih_amd.pose_prior import FusedTwoHandPriorLoss, TwoHandPriorLoss
    from renderih_amd.quat_mano import AnchorLayer, FusedAnchorLayer, FusedQuatManoLayer, QuatManoLayer
    from renderih_amd.sdf import FusedTwoHandSDFLoss, TwoHandSDFLoss
    B, G, D = 2, 8, 4
    d = dev()
    rs = np.random.RandomState(3)
    A = AnchorLayer(ANCHOR_DIR).face_vert_idx.shape[1]
    contacts = (rs.randint(0, A, size=(B, A, D)), (rs.rand(B, A, D) < 0.5).astype(np.int64), rs.rand(B, A, D).astype(np.float32))

    def build(mano_cls, anchor_cls, sdf_cls, prior_cls):
        hands = [mano_cls(mano_dict(s), side=s, center_idx=0, return_transf=True, return_full_pose=True).to(d) for s in ('right', 'left')]
        prior = module(prior_cls).to(d)
        prior.set_contacts(*contacts)
        return hands, anchor_cls(ANCHOR_DIR).to(d), sdf_cls(PART_VERT, grid_size=G).to(d), prior

    def chain(mods, q, t):
        hands, anchors, crit, prior = mods
        vr = hands[0](q[0])[0] + t[0].unsqueeze(1)
        vl = hands[1](q[1])[0] + t[1].unsqueeze(1)
        ar, al = anchors(vr), anchors(vl)
        pen = crit(torch.stack([vr, vl], 1))
        loss, terms = prior(q[0], q[1], vr, vl, ar, al)
        gq, gt = torch.autograd.grad(pen.sum() + loss, (q, t))
        return pen, loss, terms, gq, gt, vr, vl, ar, al
    fused = build(FusedQuatManoLayer, FusedAnchorLayer, FusedTwoHandSDFLoss, FusedTwoHandPriorLoss)
    q1, t1 = chain_poses(1, B)
    q2, t2 = chain_poses(2, B)
    q = torch.from_numpy(q1).to(d).requires_grad_(True)
    t = torch.from_numpy(t1).to(d).requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(fused, q, t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain(fused, q, t)
    with torch.no_grad():
        q.copy_(torch.from_numpy(q2))
        t.copy_(torch.from_numpy(t2))
    graph.replay()
    replayed = [o.detach().clone() for o in outs]
    eager = chain(fused, q, t)
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
    pen, loss, terms, gq, gt, vr, vl, ar, al = replayed
    mirror = module(TwoHandPriorLoss).double()
    mirror.set_contacts(*contacts)
    want_loss, want_terms = mirror(*[x.cpu().double() for x in (q[0].detach(), q[1].detach(), vr, vl, ar, al)])
    dev_prior = relative_deviation({'loss': loss.cpu().numpy(), 'terms': terms.cpu().numpy()},
                                   {'loss': want_loss.numpy(), 'terms': want_terms.numpy()})
    want = chain(build(QuatManoLayer, AnchorLayer, TwoHandSDFLoss, TwoHandPriorLoss), q, t)
    err_q = float((gq - want[3]).abs().max() / want[3].abs().max())
    err_t = float((gt - want[4]).abs().max() / want[4].abs().max())
    print('chain figures: prior', float(loss), 'terms', terms.cpu().numpy(), 'relative deviation', dev_prior, 'bar', TERM_RTOL,
          'penetration', pen.cpu().numpy(), 'gradient rel err q', err_q, 't', err_t, 'bar', grad_tol(G))
    assert (want[0] > 1e-3).all() and float(want[1]) > 0                   # the hands interpenetrate, the priors are active
    assert dev_prior <= TERM_RTOL
    assert err_q <= grad_tol(G) and err_t <= grad_tol(G)
