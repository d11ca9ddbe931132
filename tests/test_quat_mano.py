"""The pose optimiser's quaternion MANO layer and anchor layer (renderih_amd.quat_mano; reference pose_data_optimize/manopth)
on the CPU: the torch mirrors against values and gradients of the reference's own program (tests/golden/quat_mano.npz), the
real kernels (csrc/rih_mano.hip quaternion mode, csrc/rih_anchor.hip) through the host-compiled library against the golden
and against the mirror in fp64, the mirror's scale invariance, argument checks of the classes and of every new entry point,
the CSR of the anchor backward.  Helpers and the tolerance: tests/quat_mano_cases.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

from quat_mano_cases import (ANCHOR_DIR, CASES, OUTS, SIDES, close, compare, evaluate, fused_vs_fp64_mirror,  # noqa: E402
                             golden_case, layer_for, mano_dict, seeded_case)


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('name', CASES)
def test_mirror_matches_reference_golden(side, name):
    from renderih_amd.quat_mano import QuatManoLayer
    case = golden_case(side, name)
    got = evaluate(layer_for(QuatManoLayer, side, case, 'cpu'), case, 'cpu', flat=(name == 'c0'))
    compare(got, case, 'mirror %s %s' % (side, name))
    assert set(got) >= {'grad_' + k for k in ('pose', 'betas', 'trans') if k in case}
    assert (got['transf'][:, :, 3] == np.float32([0, 0, 0, 1])).all()


@pytest.mark.parametrize('side', SIDES)
def test_anchor_mirror_matches_reference_golden(side):
    from renderih_amd.quat_mano import AnchorLayer
    layer = AnchorLayer(ANCHOR_DIR)
    A = layer.face_vert_idx.shape[1]
    assert layer.face_vert_idx.shape == (1, A, 3) and layer.anchor_weight.shape == (1, A, 2)
    assert layer.face_vert_idx.dtype == torch.int64 and layer.anchor_weight.dtype == torch.float32
    for name in CASES:
        case = golden_case(side, name)
        close(layer(torch.from_numpy(case['verts'])).numpy(), case['anchors'], 'anchors %s %s' % (side, name))
    arrays = AnchorLayer((layer.face_vert_idx[0].numpy(), layer.anchor_weight[0].numpy()))
    assert torch.equal(arrays.face_vert_idx, layer.face_vert_idx) and torch.equal(arrays.anchor_weight, layer.anchor_weight)


@pytest.mark.parametrize('side', SIDES)
@pytest.mark.parametrize('name', CASES)
def test_fused_kernels_match_reference_golden_on_cpu(side, name):
    from host_kernels import host_kernels_abi
    from renderih_amd.quat_mano import FusedAnchorLayer, FusedQuatManoLayer
    case = golden_case(side, name)
    with host_kernels_abi():
        got = evaluate(layer_for(FusedQuatManoLayer, side, case, 'cpu'), case, 'cpu')
        anchors = FusedAnchorLayer(ANCHOR_DIR)(torch.from_numpy(case['verts'])).numpy()
    compare(got, case, 'fused %s %s' % (side, name))
    close(anchors, case['anchors'], 'fused anchors %s %s' % (side, name))


@pytest.mark.parametrize('side,B,center_idx,betas,trans', [('right', 1, 0, True, False), ('left', 17, 9, False, False),
                                                           ('left', 1, None, True, True), ('right', 17, None, True, True),
                                                           ('left', 2, 12, True, False)])          # centred on the tip 445
def test_fused_kernels_match_fp64_mirror_on_cpu(side, B, center_idx, betas, trans):
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        fused_vs_fp64_mirror(side, B, center_idx, betas, trans, 'cpu')


@pytest.mark.parametrize('upstream', [('verts',), ('joints',), ('transf',)])
def test_fused_kernels_take_any_subset_of_upstream_gradients_on_cpu(upstream):
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        fused_vs_fp64_mirror('left', 2, 0, True, False, 'cpu', upstream)


def test_fused_anchor_kernels_match_mirror_on_cpu():
    from host_kernels import host_kernels_abi
    from renderih_amd.quat_mano import AnchorLayer, FusedAnchorLayer
    rs = np.random.RandomState(3)
    v = rs.randn(3, 778, 3).astype(np.float32)
    w = torch.from_numpy(rs.rand(3, 108, 3).astype(np.float32))
    mirror, fused = AnchorLayer(ANCHOR_DIR), FusedAnchorLayer(ANCHOR_DIR)
    want_v = torch.from_numpy(v).double().requires_grad_(True)
    want = mirror.double()(want_v)
    want_g, = torch.autograd.grad((w.double() * want).sum(), want_v)
    with host_kernels_abi():
        got_v = torch.from_numpy(v).requires_grad_(True)
        got = fused(got_v)
        got_g, = torch.autograd.grad((w * got).sum(), got_v)
    close(got.detach().numpy(), want.detach().numpy(), 'anchors')
    close(got_g.numpy(), want_g.numpy(), 'anchor gradient')
    untouched = np.setdiff1d(np.arange(778), fused.face_vert_idx.numpy().reshape(-1))
    assert untouched.size > 0 and not got_g.numpy()[:, untouched].any()


@pytest.mark.parametrize('side', SIDES)
def test_mirror_is_invariant_to_the_scale_of_the_quaternions(side):
    """R = ceres form / |q|^2: scaling every quaternion by s > 0 leaves all outputs unchanged and scales the gradient by 1 / s."""
    from renderih_amd.quat_mano import QuatManoLayer
    case = seeded_case(3, 11)
    case['center_idx'] = 0
    layer = layer_for(QuatManoLayer, side, case, 'cpu', torch.float64)
    base = evaluate(layer, case, 'cpu', torch.float64)
    s = 1.7
    scaled = evaluate(layer, dict(case, pose=case['pose'].astype(np.float64) * s), 'cpu', torch.float64)
    for k in OUTS + ('grad_betas',):
        np.testing.assert_allclose(scaled[k], base[k], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(scaled['grad_pose'] * s, base['grad_pose'], rtol=1e-9, atol=1e-11)
    assert np.abs(base['grad_pose']).max() > 1e-2


def test_left_hand_full_pose_is_the_unmodified_input_and_tip_is_445():
    from renderih_amd.quat_mano import QuatManoLayer
    case = seeded_case(2, 5)
    left = QuatManoLayer(mano_dict('left'), side='left', return_transf=True, return_full_pose=True)
    pose = torch.from_numpy(case['pose'].reshape(2, 64))
    keep = pose.clone()
    v, j, T, full = left(pose, torch.from_numpy(case['betas']))
    assert full is pose and torch.equal(pose, keep) and full.shape == (2, 64)
    assert torch.equal(j[:, 12], v[:, 445]) and not torch.equal(j[:, 12], v[:, 444])        # joint 12 = tip 18 = the middle tip
    right = QuatManoLayer(mano_dict('right'), side='right')
    v, j = right(pose)
    assert torch.equal(j[:, 12], v[:, 444])
    # the left hand's first shape direction is flipped once, at construction; th_betas defaults to zeros
    sd = torch.from_numpy(np.asarray(mano_dict('left')['shapedirs'], np.float32))
    assert torch.equal(left.th_shapedirs[:, 0], -sd[:, 0]) and torch.equal(left.th_shapedirs[:, 1:], sd[:, 1:])
    assert left.th_betas.shape == (1, 10) and not left.th_betas.any()
    assert left.th_v_template.shape == (1, 778, 3) and left.th_J_regressor.shape == (16, 778) and left.th_faces.dtype == torch.int64


def test_refused_arguments_raise():
    from renderih_amd.quat_mano import AnchorLayer, FusedAnchorLayer, FusedQuatManoLayer, QuatManoLayer
    d = mano_dict('right')
    for kw in (dict(joint_rot_mode='axisang'), dict(root_rot_mode='rotmat'), dict(use_pca=True), dict(flat_hand_mean=False)):
        for cls in (QuatManoLayer, FusedQuatManoLayer):
            with pytest.raises(NotImplementedError):
                cls(d, **kw)
    QuatManoLayer(d, joint_rot_mode='quat', root_rot_mode='quat', use_pca=False, flat_hand_mean=True)
    with pytest.raises(ValueError):
        QuatManoLayer(d, side='both')
    with pytest.raises(ValueError):
        QuatManoLayer(d, center_idx=21)
    layer = QuatManoLayer(d)
    q = torch.from_numpy(seeded_case(2, 1)['pose'])
    with pytest.raises(NotImplementedError):
        layer(q, root_palm=True)
    with pytest.raises(NotImplementedError):
        layer(q, share_betas=torch.ones(1))
    layer(q, root_palm=torch.zeros(1), share_betas=False)
    with pytest.raises(ValueError):
        layer(q.reshape(2, 16, 2, 2))
    with pytest.raises(ValueError):
        layer(q, torch.zeros(3, 10))
    with pytest.raises(RuntimeError):                       # GPU fp32 only: no CPU fallback
        FusedQuatManoLayer(d)(q)
    with pytest.raises(RuntimeError):
        FusedAnchorLayer(ANCHOR_DIR)(torch.zeros(1, 778, 3))
    with pytest.raises(ValueError):
        AnchorLayer((np.zeros((3, 3), np.int64), np.zeros((2, 2))))
    with pytest.raises(ValueError):
        AnchorLayer((-np.ones((2, 3), np.int64), np.zeros((2, 2))))


def test_manopth_import_path(tmp_path):
    """The adapter takes manopth's constructor and maps mano_root / side to MANO_RIGHT.pkl / MANO_LEFT.pkl."""
    from renderih_amd import assets, quat_mano
    import manopth.anchorlayer
    import manopth.manolayer
    import manopth.quatutils
    assets.write_synthetic_mano_pkl(str(tmp_path / 'MANO_LEFT.pkl'), 'left')
    layer = manopth.manolayer.ManoLayer(joint_rot_mode='quat', root_rot_mode='quat', use_pca=False, mano_root=str(tmp_path),
                                        center_idx=0, flat_hand_mean=True, return_transf=True, return_full_pose=True, side='left')
    assert isinstance(layer, quat_mano.FusedQuatManoLayer) and layer.side == 'left' and layer.tips[2] == 445
    assert layer.mano_path.endswith('MANO_LEFT.pkl') and layer.center_idx == 0
    with pytest.raises(NotImplementedError):
        manopth.manolayer.ManoLayer(mano_root=str(tmp_path), side='left')        # manopth's defaults: axis-angle with PCA
    assert manopth.anchorlayer.AnchorLayer is quat_mano.FusedAnchorLayer
    assert manopth.quatutils.quaternion_to_rotation_matrix is quat_mano.quaternion_to_rotation_matrix
    q = torch.tensor([[0.0, 3.0, 0.0, 4.0]])
    assert torch.allclose(manopth.quatutils.normalize_quaternion(q), q / 5)
    R = manopth.quatutils.quaternion_to_rotation_matrix(q)
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3)[None], atol=1e-6)


def test_anchor_csr_lists_every_entry_once_and_checks_the_range():
    from renderih_amd.quat_mano import AnchorLayer, anchor_csr
    fvi = AnchorLayer(ANCHOR_DIR).face_vert_idx[0]
    vptr, vlist = anchor_csr(fvi, 778)
    assert vptr.dtype == torch.int32 and vlist.dtype == torch.int32 and vptr.shape == (779,) and vlist.shape == (fvi.numel(),)
    assert sorted(vlist.tolist()) == list(range(fvi.numel()))                     # each (anchor, corner) exactly once
    flat = fvi.reshape(-1)
    for v in range(778):
        seg = vlist[vptr[v]:vptr[v + 1]].tolist()
        assert seg == sorted(seg) and all(int(flat[e]) == v for e in seg)
    assert int(vptr[0]) == 0 and int(vptr[-1]) == fvi.numel()
    with pytest.raises(ValueError):
        anchor_csr(fvi, int(fvi.max()))                                           # the largest index is out of range
    with pytest.raises(ValueError):
        anchor_csr(torch.tensor([[0, 1, -1]]), 778)


def test_argument_checks_of_the_entry_points():
    from host_kernels import load
    from renderih_amd._lib import ManoModel
    lib = load()
    buf = np.zeros(1 << 20, np.float32)
    p = buf.ctypes.data
    p += (-p) % 16
    einval = lib.rih_sdf(None, p, p, 1, 1, 3, 8, None)
    assert einval != 0
    mm = ManoModel()
    mm.shapedirs = mm.posedirs = mm.v_template = mm.J_reg = mm.weights = p
    for i, par in enumerate([-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]):
        mm.parent[i] = par
    tips = (C.c_int32 * 5)(745, 317, 444, 556, 673)
    bad_tips = (C.c_int32 * 5)(745, 317, 778, 556, 673)
    m = C.byref(mm)
    fwd, bwd = lib.rih_mano_quat_fwd, lib.rih_mano_quat_bwd
    assert fwd(None, p, p, 0, p, 10, None, 0, tips, p, p, p, None, 1, None) == einval
    assert fwd(m, None, p, 0, p, 10, None, 0, tips, p, p, p, None, 1, None) == einval
    assert fwd(m, p, None, 0, p, 10, None, 0, tips, p, p, p, None, 1, None) == einval
    assert fwd(m, p, p, 0, None, 10, None, 0, tips, p, p, p, None, 1, None) == einval
    assert fwd(m, p, p, 0, p, 10, None, 0, None, p, p, p, None, 1, None) == einval
    assert fwd(m, p, p, 0, p, 10, None, 0, tips, None, p, p, None, 1, None) == einval
    assert fwd(m, p, p, 0, p, 10, None, 0, tips, p, None, p, None, 1, None) == einval
    assert fwd(m, p, p, 0, p, 10, None, 0, tips, p, p, p, None, 0, None) == einval               # B < 1
    assert fwd(m, p, p, 0, p, 10, None, 21, tips, p, p, p, None, 1, None) == einval              # center_idx not in -1..20
    assert fwd(m, p, p, 0, p, 10, None, -2, tips, p, p, p, None, 1, None) == einval
    assert fwd(m, p, p, 0, p, 7, None, 0, tips, p, p, p, None, 1, None) == einval                # stride neither 0 nor 10
    assert fwd(m, p, p, 0, p, 10, None, 0, bad_tips, p, p, p, None, 1, None) == einval
    assert bwd(None, p, p, 0, 0, tips, p, p, p, p, p, p, p, p, 1, None) == einval
    assert bwd(m, None, p, 0, 0, tips, p, p, p, p, p, p, p, p, 1, None) == einval
    assert bwd(m, p, None, 0, 0, tips, p, p, p, p, p, p, p, p, 1, None) == einval
    assert bwd(m, p, p, 0, 0, None, p, p, p, p, p, p, p, p, 1, None) == einval
    assert bwd(m, p, p, 0, 0, tips, p, p, p, None, p, p, p, p, 1, None) == einval                # the forward's workspace
    assert bwd(m, p, p, 0, 0, tips, p, p, p, p, None, p, p, p, 1, None) == einval                # d_quat
    assert bwd(m, p, p, 0, 0, tips, p, p, p, p, p, p, p, None, 1, None) == einval                # ws_bwd
    assert bwd(m, p, p, 0, 0, tips, p, p, p, p, p, p, p, p, 0, None) == einval
    assert bwd(m, p, p, 0, 21, tips, p, p, p, p, p, p, p, p, 1, None) == einval
    assert bwd(m, p, p, 0, -2, tips, p, p, p, p, p, p, p, p, 1, None) == einval
    assert lib.rih_anchor_fwd(None, p, p, p, 1, 4, 1, None) == einval
    assert lib.rih_anchor_fwd(p, None, p, p, 1, 4, 1, None) == einval
    assert lib.rih_anchor_fwd(p, p, None, p, 1, 4, 1, None) == einval
    assert lib.rih_anchor_fwd(p, p, p, None, 1, 4, 1, None) == einval
    assert lib.rih_anchor_fwd(p, p, p, p, 0, 4, 1, None) == einval
    assert lib.rih_anchor_fwd(p, p, p, p, 1, 4, 0, None) == einval                               # A < 1
    assert lib.rih_anchor_fwd(p, p, p, p, 1, 4, 1, None) == 0
    assert lib.rih_anchor_bwd(None, p, p, p, p, 1, 4, 1, None) == einval
    assert lib.rih_anchor_bwd(p, None, p, p, p, 1, 4, 1, None) == einval
    assert lib.rih_anchor_bwd(p, p, None, p, p, 1, 4, 1, None) == einval
    assert lib.rih_anchor_bwd(p, p, p, None, p, 1, 4, 1, None) == einval
    assert lib.rih_anchor_bwd(p, p, p, p, None, 1, 4, 1, None) == einval
    assert lib.rih_anchor_bwd(p, p, p, p, p, 0, 4, 1, None) == einval
    assert lib.rih_anchor_bwd(p, p, p, p, p, 1, 4, 0, None) == einval
    assert lib.rih_anchor_bwd(p, p, p, p, p, 1, 4, 1, None) == 0
