"""The two-hand pose optimiser on the GPU (renderih_amd.pose_opt.FusedTwoHandPoseOptimizer, csrc/rih_pose_opt.hip): the step kernels
teacher-forced against torch's Adam and ReduceLROnPlateau, the replayed graph against the eager launches of the same kernels
(bit-identical, also after a second set_opt_val and across two optimize() calls), the fused loop against the mirror loops over
the first K iterations, and the surface.  Helpers and bars: tests/test_pose_opt.py.  Figures found on an MI355X:
profiles/pose_optimizer/deviation_gpu.log."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_pose_opt import (K, KEYS, LOOP_SEED, check_loop_against_mirror, check_surface, make, opt_case, run_step_kernels,  # noqa: E402
                           trajectory)

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.mark.parametrize('B', [1, 3])
def test_step_kernels_follow_torch_adam_and_plateau(B):
    run_step_kernels(B, dev())


def _state(opt):
    return [opt.stepper.state.clone()] + [e[k].clone() for e in opt.stepper.params for k in ('p', 'm', 'v')] + [opt.last_loss.clone()]


def test_replayed_graph_is_bit_identical_to_eager_launches():
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    graphed, eager = make(FusedTwoHandPoseOptimizer, dev(), n_iter=12), make(FusedTwoHandPoseOptimizer, dev(), n_iter=12, graph=False)
    results = []
    for seed in (1, 2):                                                   # the second set_opt_val reuses the graph
        case = opt_case(seed, 2)
        got = []
        for opt in (graphed, eager):
            opt.set_opt_val(**case)
            got.append((opt.optimize(), _state(opt)))
        for k in KEYS:
            assert torch.equal(got[0][0][k], got[1][0][k]), (seed, k)
        for a, b in zip(got[0][1], got[1][1]):
            assert torch.equal(a, b), seed
        if seed == 1:
            captured = graphed._graph
        results.append(got[0])
    assert graphed._graph is captured and eager._graph is None
    assert not torch.equal(results[0][0][KEYS[0]], results[1][0][KEYS[0]])
    assert graphed.stepper.read_state()['step'] == 12
    graphed.set_opt_val(**opt_case(2, 2))                                   # 6 + 6 iterations = 12, n_iter does not recapture
    graphed.n_iter = 6
    graphed.optimize()
    again = graphed.optimize()
    assert graphed._graph is captured
    for k in KEYS:
        assert torch.equal(again[k], results[1][0][k]), k
    for a, b in zip(_state(graphed), results[1][1]):
        assert torch.equal(a, b)


@pytest.mark.parametrize('B', sorted(LOOP_SEED))
def test_fused_loop_matches_mirror_loop(B):
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    got = trajectory(make(FusedTwoHandPoseOptimizer, dev()), opt_case(LOOP_SEED[B], B), K)
    check_loop_against_mirror(got, dev(), B)


def test_surface_and_recapture():
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    check_surface(FusedTwoHandPoseOptimizer, dev())
    opt = make(FusedTwoHandPoseOptimizer, dev(), n_iter=2)
    opt.set_opt_val(**opt_case(2, 3))
    opt.optimize()
    first = opt._graph
    opt.coef_val['lambda_repulsion_loss'] = 5.0
    opt.optimize()
    assert opt._graph is not first                                          # another coef_val: another graph
    second = opt._graph
    opt.set_opt_val(**opt_case(1, 2))                                       # another batch size: new buffers, another graph
    res = opt.optimize()
    assert opt._graph is not second and tuple(res[KEYS[0]].shape) == (2, 16, 4)
