"""Loss of the MANO-head model (core/Loss_mano.py: ManoLoss + mano_loss_GCN), on the CPU: the torch mirror
(renderih_amd/loss.py) against values and gradients of the reference itself (tests/golden/make_mano_loss_golden.py), the
argument checks of rih_mano_loss / rih_mano_loss_final, and the real kernels (csrc/rih_mano_loss.hip) through the
host-compiled library against the mirror."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from renderih_amd import assets, testing  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'mano_loss.npz')
PREDS = ['v3d_left', 'v3d_right', 'v2d_left', 'v2d_right', 'pose_left', 'pose_right', 'shape_left', 'shape_right',
         'rootrel_pred']
TERMS = ['vert2d_loss', 'vert3d_loss', 'joint_loss', 'norm_loss', 'edge_loss', 'pose_loss', 'shape_loss', 'rootrel_loss',
         'regularize_loss', 'upsample_norm_loss']
CASES = [('e0', 0, False), ('e60', 60, False), ('e60up', 60, True)]


def hand_losses(device='cpu'):
    from renderih_amd.loss import ManoLoss
    out = {}
    for s in ('left', 'right'):
        md = assets.synthetic_mano_dict(s)
        J = torch.from_numpy(np.asarray(md['J_regressor'].todense(), np.float32))
        out[s] = ManoLoss(J, np.asarray(md['f']), level=4, device=device,
                          upsample_weight=torch.from_numpy(assets.synthetic_upsample_weight()))
    return out


def golden_inputs(device='cpu'):
    z = np.load(GOLDEN)
    return z, {k[3:]: torch.from_numpy(z[k]).to(device) for k in z.files if k.startswith('in/')}


def random_inputs(B, seed, device='cpu'):
    g = torch.Generator().manual_seed(seed)
    t = {}
    for s in ('left', 'right'):
        t['v3d_gt_' + s] = 0.05 * torch.randn(B, 778, 3, generator=g)
        t['v2d_gt_' + s] = 256 * torch.rand(B, 778, 2, generator=g)
        t['v3d_' + s] = t['v3d_gt_' + s] + 0.5 * torch.randn(B, 778, 3, generator=g)
        t['v2d_' + s] = t['v2d_gt_' + s] + 20 * torch.randn(B, 778, 2, generator=g)
        t['pose_gt_' + s] = torch.randn(B, 48, generator=g)
        t['pose_' + s] = t['pose_gt_' + s] + 0.5 * torch.randn(B, 48, generator=g)
        t['shape_gt_' + s] = torch.randn(B, 10, generator=g)
        t['shape_' + s] = 3 * torch.tanh(torch.randn(B, 10, generator=g))
    t['pose_left'][0, :3] = 0.0
    t['root_rel'] = 0.05 * torch.randn(B, 3, generator=g)
    t['rootrel_pred'] = t['root_rel'] + 0.05 * torch.randn(B, 3, generator=g)
    return {k: v.to(device) for k, v in t.items()}


def model_dicts(t):
    result = {'verts3d': {s: t['v3d_' + s] for s in ('left', 'right')}, 'verts2d': {s: t['v2d_' + s] for s in ('left', 'right')}}
    other = {'root_rel': t['rootrel_pred'],
             'verts3d_MANO_list': {s: {'mano_pose': t['pose_' + s], 'mano_shape': t['shape_' + s]} for s in ('left', 'right')}}
    return result, other


def evaluate(fn, first, epoch, losses, t, upsample_weight=None, scale=1.0):
    """fn = mano_loss_GCN or mano_loss_GCN_fused (first = cfg / the FusedManoLoss): (total, terms, {pred: grad})."""
    for k in PREDS:
        t[k] = t[k].detach().requires_grad_(True)
    result, other = model_dicts(t)
    B = t['v3d_left'].shape[0]
    z = torch.zeros(B, 21, 3, device=t['v3d_left'].device)
    total, aux, terms, coarse = fn(first, epoch, losses['left'], losses['right'], None, None, result, None, [], other, None,
                                   None, None, t['v2d_gt_left'], None, t['v2d_gt_right'], None, t['v3d_gt_left'], z,
                                   t['v3d_gt_right'], z, t['root_rel'], 256, t['pose_gt_left'], t['shape_gt_left'],
                                   t['pose_gt_right'], t['shape_gt_right'], upsample_weight=upsample_weight)
    assert aux == {'total_loss': 0} and coarse == {} and sorted(terms) == sorted(TERMS)
    (scale * total).backward()
    return total.detach().clone(), {k: v.detach().clone() for k, v in terms.items()}, {k: t[k].grad.clone() for k in PREDS}


def check_against(total, terms, grads, want_total, want_terms, want_grads, rel=1e-5):
    assert abs(float(total) - want_total) <= rel * abs(want_total), (float(total), want_total)
    for k in TERMS:
        assert abs(float(terms[k]) - want_terms[k]) <= rel * abs(want_terms[k]) + 1e-12, (k, float(terms[k]), want_terms[k])
    for k in PREDS:
        testing.assert_close(grads[k], want_grads[k], 1e-4, 1e-6, 'grad ' + k)


# ----------------------------------------------------------------------------------------------- mirror vs the reference
@pytest.mark.parametrize('key,epoch,with_up', CASES)
def test_mirror_matches_reference_golden(key, epoch, with_up):
    from renderih_amd.loss import mano_loss_GCN
    z, t = golden_inputs()
    total, terms, grads = evaluate(mano_loss_GCN, None, epoch, hand_losses(), t,
                                   upsample_weight=t['upsample_weight'] if with_up else None)
    check_against(total, terms, grads, float(z[key + '/total']), {k: float(z[key + '/' + k]) for k in TERMS},
                  {k: torch.from_numpy(z[key + '/grad_' + k]) for k in PREDS})
    # the zero rotation of the golden has a finite gradient (torch autograd's value through the 1e-8 shift)
    assert torch.isfinite(grads['pose_left'][0, 3:6]).all() and float(grads['pose_left'][0, 3:6].abs().max()) > 0


def test_mirror_weights_from_the_reference_config():
    """cfg.LOSS_WEIGHT (nested, utils/defaults.yaml layout) flattens to the defaults; a flat dict overrides; a changed
    nested weight reaches the total."""
    from renderih_amd.config import CfgNode
    from renderih_amd.loss import MANO_DEFAULT_WEIGHTS, mano_loss_GCN, mano_loss_weights
    defaults = CfgNode({'AUX': {'DENSEPOSE': 30, 'MASK': 500, 'HMS': 100},      # utils/defaults.yaml LOSS_WEIGHT
                        'DATA': {'LABEL_3D': 100, 'LABEL_2D': 50, 'MANO_POSE': 0.5, 'MANO_SHAPE': 0.01, 'BONE': 10,
                                 'MANO_REL': 1},
                        'GRAPH': {'NORM': {'EDGE': 2000, 'NORMAL': 10, 'NORM_EPOCH': 50}}, 'NORM': {'UPSAMPLE': 1.0}})
    assert mano_loss_weights(defaults) == MANO_DEFAULT_WEIGHTS
    assert mano_loss_weights({'EDGE': 7.0})['EDGE'] == 7.0
    with pytest.raises(KeyError):
        mano_loss_weights({'EDGES': 7.0})
    nested = {'DATA': {'MANO_POSE': 2.0}, 'GRAPH': {'NORM': {'NORM_EPOCH': 5}}}
    w = mano_loss_weights(nested)
    assert w['MANO_POSE'] == 2.0 and w['NORM_EPOCH'] == 5 and w['LABEL_3D'] == 100.0
    _, t = golden_inputs()
    base, terms, _ = evaluate(mano_loss_GCN, None, 0, hand_losses(), dict(t))
    moved, _, _ = evaluate(mano_loss_GCN, types.SimpleNamespace(LOSS_WEIGHT=nested), 10, hand_losses(), dict(t))
    want = base + 1.5 * terms['pose_loss'] + 2000 * terms['edge_loss']
    assert abs(float(moved) - float(want)) <= 1e-5 * float(want)


# ------------------------------------------------------------------------------------------------ C ABI argument checks
def test_entry_points_refuse_bad_arguments():
    from renderih_amd import _lib
    from renderih_amd._lib import MeshTopo
    lib = _lib.load()
    EINVAL = -1
    buf = (C.c_float * 64)()
    ibuf = (C.c_int32 * 64)()
    p, ip = C.addressof(buf), C.addressof(ibuf)

    def topo(V=778, F=1538, NJ=21, faces=ip):
        return MeshTopo(faces, ip, ip, p, None, V, F, NJ, 0, 0)

    def call(tp=None, pose_dim=48, shape_dim=10, img=256.0, B=2, null=None):
        ptrs = [p] * 14                     # 4 predictions, 4 labels, term weights, 4 gradients, partial
        if null is not None:
            ptrs[null] = None
        return lib.rih_mano_loss(C.byref(tp if tp is not None else topo()), *ptrs[:8], None, pose_dim, shape_dim, ptrs[8],
                                 img, *ptrs[9:], B, None)
    assert lib.rih_mano_loss(None, *([p] * 8), None, 48, 10, p, 256.0, *([p] * 5), 2, None) == EINVAL
    for i in range(14):
        assert call(null=i) == EINVAL, i
    assert call(B=0) == EINVAL
    assert call(pose_dim=45) == EINVAL and call(pose_dim=72) == EINVAL
    assert call(shape_dim=12) == EINVAL
    assert call(img=0.0) == EINVAL
    assert call(tp=topo(V=801)) == EINVAL and call(tp=topo(V=0)) == EINVAL
    assert call(tp=topo(F=1601)) == EINVAL and call(tp=topo(NJ=25)) == EINVAL
    assert call(tp=topo(faces=None)) == EINVAL
    fin = [p, p, p, p, 2, p, p, p, p, None]
    assert lib.rih_mano_loss_final(*fin[:4], 0, *fin[5:]) == EINVAL
    for i in (0, 1, 2, 3, 5, 6, 7, 8):
        a = list(fin)
        a[i] = None
        assert lib.rih_mano_loss_final(*a) == EINVAL, i
    # rih_mesh_loss validates the topology through the same function, and its perm, which it always reads
    good = dict(faces=ip, vptr=ip, vlist=ip, J=p, perm=ip, V=778, F=1538, NJ=21, Vc=252, pool=4)
    bad = [{k: None} for k in ('faces', 'vptr', 'vlist', 'J', 'perm')] + \
        [dict(V=0), dict(V=801), dict(F=1601), dict(NJ=25), dict(pool=3)]
    for change in bad:
        tp = MeshTopo(*{**good, **change}.values())
        assert lib.rih_mesh_loss(C.byref(tp), *([p] * 6), None, p, 256.0, *([p] * 5), 2, None) == EINVAL, change


# ----------------------------------------------------------------------------- real kernels through the host-built library
@pytest.fixture
def host():
    from hipcpu.host_kernels import host_kernels_abi
    with host_kernels_abi():
        yield


@pytest.mark.parametrize('epoch', [0, 60])
def test_kernel_on_cpu_matches_mirror(host, epoch):
    """rih_mano_loss + rih_mano_loss_final, compiled for the host, at B = 2 on random data against the mirror: every term,
    the total and every gradient; the gradients scale with the incoming gradient; the up-sampling term adds its value
    and no gradient."""
    from renderih_amd.loss import FusedManoLoss, mano_loss_GCN, mano_loss_GCN_fused
    losses = hand_losses()
    t = random_inputs(2, seed=5 + epoch)
    fused = FusedManoLoss(losses['left'], losses['right'])
    w = torch.from_numpy(assets.synthetic_upsample_weight()) * 1.1
    want = evaluate(mano_loss_GCN, None, epoch, losses, dict(t), upsample_weight=w, scale=3.0)
    got = evaluate(mano_loss_GCN_fused, fused, epoch, losses, dict(t), upsample_weight=w, scale=3.0)
    check_against(got[0], got[1], got[2], float(want[0]), {k: float(v) for k, v in want[1].items()}, want[2])
    assert float(got[1]['upsample_norm_loss']) > 0


def test_kernel_on_cpu_matches_reference_golden(host):
    """The same host-built kernels against the reference's own values at epoch 60, zero rotations included."""
    from renderih_amd.loss import FusedManoLoss, mano_loss_GCN_fused
    z, t = golden_inputs()
    losses = hand_losses()
    fused = FusedManoLoss(losses['left'], losses['right'])
    total, terms, grads = evaluate(mano_loss_GCN_fused, fused, 60, losses, t, upsample_weight=t['upsample_weight'])
    check_against(total, terms, grads, float(z['e60up/total']), {k: float(z['e60up/' + k]) for k in TERMS},
                  {k: torch.from_numpy(z['e60up/grad_' + k]) for k in PREDS})


def test_fused_set_epoch_moves_the_device_gate(host):
    """epoch=None keeps the gate; set_epoch(NORM_EPOCH, B, device) rewrites the device weights in place (same storage)."""
    from renderih_amd.loss import FusedManoLoss
    losses = hand_losses()
    fused = FusedManoLoss(losses['left'], losses['right'])
    wa, _ = fused.device_weights(2, torch.device('cpu'))
    assert float(wa[4]) == 0.0
    ptr = wa.data_ptr()
    fused.set_epoch(fused.w['NORM_EPOCH'], 2, 'cpu')
    wb, cb = fused.device_weights(2, torch.device('cpu'))
    assert wb.data_ptr() == ptr and float(wb[4]) > 0
    assert float(wb[4]) == pytest.approx(0.5 * 2000.0 / float(cb[4]), rel=1e-6)
