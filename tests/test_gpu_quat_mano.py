"""Fused quaternion MANO layer and anchor layer (renderih_amd.quat_mano.FusedQuatManoLayer / FusedAnchorLayer: the quaternion
mode of csrc/rih_mano.hip, csrc/rih_anchor.hip) on the GPU: every golden case of the reference's own manopth layer, the fused
kernels against the fp64 mirror across the 16-hand chunk (B = 1, 2, 17, 33) with every subset of upstream gradients, the
centring / translation / shared-betas configurations, bit-identical repeats, the anchors, and one captured graph of the
optimiser's chain pose -> both meshes -> anchors -> penetration loss -> quaternion gradients, replayed on other quaternions.
Helpers and the tolerance: tests/quat_mano_cases.py."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from quat_mano_cases import (ANCHOR_DIR, CASES, OUTS, SIDES, close, compare, evaluate, fused_vs_fp64_mirror,  # noqa: E402
                             golden_case, layer_for, mano_dict, seeded_case)
from test_gpu_two_hand_sdf import PART_VERT  # noqa: E402
from test_two_hand_sdf import VALUE_TOL, grad_tol  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('name', CASES)
def test_fused_matches_reference_golden(side, name):
    from renderih_amd.quat_mano import FusedAnchorLayer, FusedQuatManoLayer
    case = golden_case(side, name)
    got = evaluate(layer_for(FusedQuatManoLayer, side, case, dev()), case, dev(), flat=(name == 'c0'))
    compare(got, case, 'fused %s %s' % (side, name))
    assert got['full_pose_is_input']
    anchors = FusedAnchorLayer(ANCHOR_DIR).to(dev())(torch.from_numpy(case['verts']).to(dev()))
    close(anchors.cpu().numpy(), case['anchors'], 'fused anchors %s %s' % (side, name))


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('B', [1, 2, 17, 33])
def test_fused_matches_fp64_mirror_for_every_upstream_subset(side, B):
    """17 and 33 cross the fused kernel's 16-hand chunk with a partial chunk; B = 1 is the optimiser's smallest batch.  Two
    evaluations are bit-identical (no atomics, fixed summation order)."""
    for upstream in (OUTS, ('verts',), ('joints',), ('transf',)):
        fused, case, got = fused_vs_fp64_mirror(side, B, 0, True, False, dev(), upstream)
        if upstream == OUTS:
            again = evaluate(fused, case, dev())
            for k in got:
                assert np.array_equal(got[k], again[k]), k


@pytest.mark.parametrize('center_idx', [None, 0, 9, 4])
@pytest.mark.parametrize('trans', [False, True])
def test_fused_centring_translation_and_shared_betas(center_idx, trans):
    """center_idx 4 is a finger tip (every vertex tile then skins the tips itself); th_betas=None shares the buffer."""
    fused_vs_fp64_mirror('left', 5, center_idx, False, trans, dev())
    fused_vs_fp64_mirror('right', 3, center_idx, True, trans, dev(), seed=1)


def test_fused_without_transforms_and_without_gradients():
    from renderih_amd.quat_mano import FusedQuatManoLayer
    case = seeded_case(2, 3)
    full = FusedQuatManoLayer(mano_dict('right'), center_idx=0, return_transf=True).to(dev())
    bare = FusedQuatManoLayer(mano_dict('right'), center_idx=0).to(dev())
    q, b = torch.from_numpy(case['pose']).to(dev()), torch.from_numpy(case['betas']).to(dev())
    with torch.no_grad():
        v0, j0, T0 = full(q, b)
        out = bare(q, b)
    assert len(out) == 2 and torch.equal(out[0], v0) and torch.equal(out[1], j0)
    assert torch.equal(T0[:, :, :3, 3], j0[:, [0, 5, 6, 7, 9, 10, 11, 17, 18, 19, 13, 14, 15, 1, 2, 3]])     # joints = translations


@pytest.mark.parametrize('B', [1, 33])
def test_fused_anchors_match_mirror(B):
    from renderih_amd.quat_mano import AnchorLayer, FusedAnchorLayer
    rs = np.random.RandomState(B)
    v = rs.randn(B, 778, 3).astype(np.float32)
    fused = FusedAnchorLayer(ANCHOR_DIR).to(dev())
    A = fused.face_vert_idx.shape[1]
    w = rs.rand(B, A, 3).astype(np.float32)
    want_v = torch.from_numpy(v).double().requires_grad_(True)
    want = AnchorLayer(ANCHOR_DIR).double()(want_v)
    want_g, = torch.autograd.grad((torch.from_numpy(w).double() * want).sum(), want_v)
    got_v = torch.from_numpy(v).to(dev()).requires_grad_(True)
    got = fused(got_v)
    got_g, = torch.autograd.grad((torch.from_numpy(w).to(dev()) * got).sum(), got_v)
    close(got.detach().cpu().numpy(), want.detach().numpy(), 'anchors')
    close(got_g.cpu().numpy(), want_g.numpy(), 'anchor gradient')
    untouched = np.setdiff1d(np.arange(778), fused.face_vert_idx.cpu().numpy().reshape(-1))
    assert untouched.size > 0 and not got_g.cpu().numpy()[:, untouched].any()


def chain_poses(seed, B=2):
    """Quaternions and translations of two hands that interpenetrate: a free root rotation, fingers bent by a few degrees
    (the synthetic model's skinning weights are random, so large finger rotations would tear the mesh apart), the left hand
    pushed a fifth of its size into the right one -- the recipe of the penetration loss's golden cases, restated for POSES:
    the helpers of tests/test_gpu_two_hand_sdf.py produce vertices (spheres, or the golden's ready meshes), which cannot
    enter a chain that starts at quaternions, so only PART_VERT and the bars are imported from there."""
    rs = np.random.RandomState(seed)
    q = np.zeros((2, B, 16, 4))
    q[..., 0] = 1.0
    q[..., 1:] = 0.04 * rs.randn(2, B, 16, 3)
    q[:, :, 0, 1:] = 0.3 * rs.randn(2, B, 3)
    q *= rs.uniform(0.7, 1.5, size=(2, B, 16, 1))
    t = np.zeros((2, B, 3))
    t[1] = np.array([0.003, 0.004, 0.005]) + 0.001 * rs.randn(B, 3)       # the synthetic hand is 0.03 across
    return q.astype(np.float32), t.astype(np.float32)


def test_pose_to_penetration_loss_chain_inside_a_captured_graph():
    """right and left FusedQuatManoLayer -> FusedAnchorLayer -> FusedTwoHandSDFLoss (G = 8) -> backward to the quaternions,
    captured once and replayed on OTHER quaternions: bit-identical to the eager evaluation of those, and against the same
    chain built from the mirrors.  Bars against the mirrors: the penetration loss's own (tests/test_two_hand_sdf.py: VALUE_TOL
    per vertex; the loss within the per-vertex errors actually found plus the fp32 summation bound 2 (2V) eps sum |terms|;
    gradients grad_tol(G) of the largest entry) -- the meshes that enter it agree to 1e-5 + 1e-4 |v|, far inside a voxel
    (0.03 / 8), and the anchor term is linear."""
    from renderih_amd.quat_mano import AnchorLayer, FusedAnchorLayer, FusedQuatManoLayer, QuatManoLayer
    from renderih_amd.sdf import FusedTwoHandSDFLoss, TwoHandSDFLoss
    B, G = 2, 8
    d = dev()
    wa = torch.from_numpy(np.random.RandomState(2).rand(B, 108, 3).astype(np.float32)).to(d)

    def build(mano_cls, anchor_cls, sdf_cls):
        hands = [mano_cls(mano_dict(s), side=s, center_idx=0, return_transf=True, return_full_pose=True).to(d) for s in SIDES]
        return hands, anchor_cls(ANCHOR_DIR).to(d), sdf_cls(PART_VERT, grid_size=G).to(d)

    def chain(mods, q, t):
        hands, anchors, crit = mods
        vr = hands[0](q[0])[0] + t[0].unsqueeze(1)
        vl = hands[1](q[1])[0] + t[1].unsqueeze(1)
        pen, left, right = crit(torch.stack([vr, vl], 1), return_per_vert_loss=True)
        loss = pen.sum() + 1e-2 * ((wa * anchors(vr)).sum() + (wa * anchors(vl)).sum())
        g, = torch.autograd.grad(loss, q)
        return pen, loss, g, torch.cat([left, right], 1)
    fused = build(FusedQuatManoLayer, FusedAnchorLayer, FusedTwoHandSDFLoss)
    q1, t1 = chain_poses(1, B)
    q2, t2 = chain_poses(2, B)
    q = torch.from_numpy(q1).to(d).requires_grad_(True)
    t = torch.from_numpy(t1).to(d)
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
    replayed = [o.clone() for o in outs]
    eager = chain(fused, q, t)
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
    want = chain(build(QuatManoLayer, AnchorLayer, TwoHandSDFLoss), q, t)
    pen, pen_want = replayed[0].detach().cpu().numpy(), want[0].detach().cpu().numpy()
    g, g_want = replayed[2].cpu().numpy(), want[2].cpu().numpy()
    pv, pv_want = replayed[3].detach().cpu().numpy().astype(np.float64), want[3].detach().cpu().numpy().astype(np.float64)
    err_pv = np.abs(pv - pv_want)
    err_pen = np.abs(pen.astype(np.float64) - pen_want)
    bar_pen = err_pv.sum(1) + 2 * pv.shape[1] * np.finfo(np.float32).eps * np.abs(pv_want).sum(1)
    err_g = np.abs(g - g_want).max() / np.abs(g_want).max()
    print('chain figures: penetration', pen_want, 'err', err_pen, 'bar', bar_pen, 'per-vertex err', err_pv.max(), 'bar', VALUE_TOL,
          'gradient rel err', err_g, 'bar', grad_tol(G))
    assert (pen_want > 1e-3).all(), pen_want                      # the hands do interpenetrate
    assert err_pv.max() <= VALUE_TOL
    assert (err_pen <= bar_pen).all()
    assert err_g <= grad_tol(G)
