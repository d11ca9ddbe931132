"""The NatureLoss term inside the two-hand pose optimiser (renderih_amd.pose_opt with `nature=`; reference
geo_optimizer_both_batch.py:802, :824) on the CPU, the fused loop eager on the host-compiled kernels.
tests/test_gpu_pose_opt_nature.py shares the helpers and adds the captured graph.

The weights are `synthetic_state_dict(0, H, pred_scale=1)`: under that recipe every row's p1 lies in 0.45 .. 0.54
(tests/nature_cases.py measures the margin per case), far from the mask's threshold 0.6, so every hand stays judged over the
compared iterations and no rounding flips a row (asserted on the counts below).
Bar: that of tests/test_pose_opt.py -- over the compared iterations the fused loop's losses and parameters deviate from the fp64
mirror loop by at most 4 x what the fp32 mirror loop does -- with both mirrors carrying the term.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_pose_opt import K, KEYS, LOOP_SEED, deviation, make, opt_case, trajectory  # noqa: E402

_REF = {}


def weights(H):
    from renderih_amd.nature import synthetic_state_dict
    return synthetic_state_dict(0, H, 1.0)


def mirror_reference(device, B, n, H):
    """The fp64 and the fp32 mirror loops with the term, computed once."""
    from renderih_amd.pose_opt import TwoHandPoseOptimizer
    key = (str(device), B, n, H)
    if key not in _REF:
        case = opt_case(LOOP_SEED[B], B)
        _REF[key] = (trajectory(make(TwoHandPoseOptimizer, device, dtype=torch.float64, nature=weights(H)), case, n),
                     trajectory(make(TwoHandPoseOptimizer, device, nature=weights(H)), case, n))
    return _REF[key]


def nature_trajectory(opt, case, n):
    """`trajectory` plus the term's four numbers per iteration."""
    opt.set_opt_val(**case)
    opt.n_iter = 1
    out = []
    for _ in range(n):
        res = opt.optimize()
        out.append(dict(loss=float(opt.last_loss), pen=opt.last_terms['penetration'].double().cpu().numpy(),
                        nature=opt.last_terms['nature'].double().cpu().numpy(),
                        q=np.stack([res[KEYS[0]].double().numpy(), res[KEYS[2]].double().numpy()]),
                        t=np.stack([res[KEYS[1]].double().numpy(), res[KEYS[3]].double().numpy()])))
    return out


def check_loop_against_mirror(got, device, B, H, upto, log=print):
    want64, want32 = mirror_reference(device, B, upto, H)
    ref_loss, ref_par = deviation(want32, want64, upto)
    got_loss, got_par = deviation(got, want64, upto)
    log('loop with NatureLoss B=%d H=%d on %s, first %d iterations: fp32 mirror vs fp64 mirror: loss %.3g parameters %.3g; fused vs '
        'fp64 mirror: loss %.3g parameters %.3g' % (B, H, device, upto, ref_loss, ref_par, got_loss, got_par))
    log('losses fp64 %s' % [round(w['loss'], 6) for w in want64])
    assert (want64[0]['pen'] > 1e-3).all() and got[0]['pen'].min() > 1e-3              # the penetration term is active
    for g in got[:upto]:                                                                # and so is the new one, on every hand
        assert g['nature'].shape == (4,) and g['nature'][2] == B and g['nature'][3] == B and g['nature'][:2].min() > 0.5
    assert want64[upto - 1]['loss'] < want64[0]['loss'] and got[upto - 1]['loss'] < got[0]['loss']
    assert got_loss <= 4 * ref_loss and got_par <= 4 * ref_par


def check_none_changes_nothing(cls, device, n_iter, **kw):
    """nature=None: no 'nature' key, and one optimize() equals, bit for bit, that of an optimiser built without the argument."""
    case = opt_case(LOOP_SEED[1], 1)
    results = []
    for extra in ({}, {'nature': None}):
        opt = make(cls, device, n_iter=n_iter, **kw, **extra)
        opt.set_opt_val(**case)
        results.append((opt.optimize(), opt.last_loss.cpu(), opt.last_terms))
        assert opt.nature is None and sorted(opt.last_terms) == ['penetration', 'prior']
    for k in KEYS:
        assert torch.equal(results[0][0][k], results[1][0][k]), k
    assert torch.equal(results[0][1], results[1][1])
    for k in ('prior', 'penetration'):
        assert torch.equal(results[0][2][k].cpu(), results[1][2][k].cpu())


def test_without_weights_nothing_changes_on_cpu():
    from host_kernels import host_kernels_abi
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    with host_kernels_abi():
        check_none_changes_nothing(FusedTwoHandPoseOptimizer, 'cpu', 1, graph=False)


def test_fused_loop_with_nature_matches_mirror_loop_on_cpu():
    """Three eager iterations through the host-compiled kernels at H = 64; the GPU file runs K at the reference's H = 512."""
    from host_kernels import host_kernels_abi
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    with host_kernels_abi():
        case = opt_case(LOOP_SEED[1], 1)
        got = nature_trajectory(make(FusedTwoHandPoseOptimizer, graph=False, nature=weights(64)), case, 3)
        check_loop_against_mirror(got, 'cpu', 1, 64, upto=3)
    for k, name in ((0, 'hand_pose'), (1, 'obj_pose')):
        assert np.array_equal(got[2]['q'][k][:, 0], case[name + '_gt'][1][:, 0].double().numpy())      # the root never moves
    assert K >= 10
