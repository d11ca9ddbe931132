"""Shared by tests/test_quat_mano.py (CPU) and tests/test_gpu_quat_mano.py: the golden cases of the reference's own manopth
layer (tests/golden/quat_mano.npz, written by tests/golden/make_quat_mano_golden.py), seeded inputs for the fused-against-fp64
comparisons, and one `evaluate` that runs a layer and returns outputs and gradients as numpy arrays.

Tolerance: torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-5), the project's bar for fp32 kernels against a
reference, for values and gradients alike.  The inputs keep it meaningful: |q| in [0.5, 2] bounds the 1/|q| factor of the
quaternion gradient by 2, the upstream weights are in [0, 1), the synthetic hand is 0.03 across."""
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'quat_mano.npz')
ANCHOR_DIR = os.path.join(HERE, 'golden', 'anchor')
SIDES = ('right', 'left')
CASES = ('c0', 'c9', 'trans')
RTOL, ATOL = 1e-4, 1e-5
OUTS = ('verts', 'joints', 'transf')


def close(got, want, what):
    torch.testing.assert_close(torch.as_tensor(np.asarray(got), dtype=torch.float64), torch.as_tensor(np.asarray(want), dtype=torch.float64),
                               rtol=RTOL, atol=ATOL, msg=lambda m: '%s: %s' % (what, m))


def mano_dict(side):
    from renderih_amd import assets
    return assets.synthetic_mano_dict(side, seed=0)


def golden_case(side, name):
    z = np.load(GOLDEN)
    k = '%s_%s/' % (side, name)
    case = {f[len(k):]: z[f] for f in z.files if f.startswith(k)}
    c = int(case.pop('center_idx'))
    case['center_idx'] = None if c < 0 else c
    return case


def seeded_case(B, seed, betas=True, trans=False):
    """Inputs in the golden's ranges: |q| in [0.5, 2], an exact identity and (from B = 2 on) a joint turned by nearly pi."""
    rs = np.random.RandomState(seed)
    q = rs.randn(B, 16, 4)
    q[..., 0] = np.abs(q[..., 0]) + 1.0
    q = q / np.linalg.norm(q, axis=-1, keepdims=True) * rs.uniform(0.5, 2.0, size=(B, 16, 1))
    q[0, 5] = (1.0, 0.0, 0.0, 0.0)
    if B > 1:
        half = 0.5 * (np.pi - 1e-3)
        q[B - 1, 2] = np.concatenate([[np.cos(half)], np.sin(half) * np.array([0.6, 0.0, 0.8])]) * 0.7
    case = {'pose': q.astype(np.float32)}
    if betas:
        case['betas'] = (rs.randn(B, 10) * 0.8).astype(np.float32)
    if trans:
        case['trans'] = (rs.randn(B, 3) * 0.1).astype(np.float32)
    case['wv'], case['wj'], case['wT'] = (rs.rand(*s).astype(np.float32) for s in ((B, 778, 3), (B, 21, 3), (B, 16, 4, 4)))
    return case


def evaluate(layer, case, device, dtype=torch.float32, upstream=OUTS, flat=False):
    """Run `layer` (return_transf=True) on the case's inputs; gradients of the weighted sum of the outputs named in
    `upstream` -> dict of numpy arrays (verts, joints, transf, grad_pose[, grad_betas, grad_trans])."""
    t = lambda a: torch.as_tensor(a).to(device=device, dtype=dtype)
    pose = t(case['pose'].reshape(-1, 64) if flat else case['pose']).requires_grad_(True)
    betas = t(case['betas']).requires_grad_(True) if 'betas' in case else None
    trans = t(case['trans']).requires_grad_(True) if 'trans' in case else None
    res = layer(pose, betas, trans)
    outs = dict(zip(OUTS, res[:3]))
    loss = sum((t(case[w]) * outs[o]).sum() for o, w in zip(OUTS, ('wv', 'wj', 'wT')) if o in upstream)
    leaves = {'grad_pose': pose, 'grad_betas': betas, 'grad_trans': trans}
    leaves = {k: v for k, v in leaves.items() if v is not None}
    grads = torch.autograd.grad(loss, list(leaves.values()))
    out = {k: v.detach().cpu().numpy() for k, v in outs.items()}
    out.update({k: g.detach().cpu().numpy().reshape(case['pose'].shape if k == 'grad_pose' else g.shape)
                for k, g in zip(leaves, grads)})
    if len(res) > 3:
        out['full_pose_is_input'] = res[3] is pose
    return out


def compare(got, want, what):
    for k in want:
        if k in got and k in OUTS + ('grad_pose', 'grad_betas', 'grad_trans'):
            close(got[k], want[k], '%s %s' % (what, k))


def layer_for(cls, side, case, device, dtype=torch.float32):
    layer = cls(mano_dict(side), side=side, center_idx=case.get('center_idx'), return_transf=True, return_full_pose=True)
    return layer.to(device=device, dtype=dtype) if dtype != torch.float32 else layer.to(device)


def fused_vs_fp64_mirror(side, B, center_idx, betas, trans, device, upstream=OUTS, seed=0):
    from renderih_amd.quat_mano import FusedQuatManoLayer, QuatManoLayer
    case = seeded_case(B, 7000 + 13 * B + seed, betas, trans)
    case['center_idx'] = center_idx
    want = evaluate(layer_for(QuatManoLayer, side, case, 'cpu', torch.float64), case, 'cpu', torch.float64, upstream)
    fused = layer_for(FusedQuatManoLayer, side, case, device)
    got = evaluate(fused, case, device, upstream=upstream)
    compare(got, want, 'fused vs fp64 mirror %s B=%d centre=%s' % (side, B, center_idx))
    assert (got['transf'][:, :, 3] == np.float32([0, 0, 0, 1])).all()
    return fused, case, got
