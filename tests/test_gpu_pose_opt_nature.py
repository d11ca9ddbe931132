"""The NatureLoss term inside the two-hand pose optimiser on the GPU (renderih_amd.pose_opt.FusedTwoHandPoseOptimizer with
`nature=`) at the reference's hidden width 512: nothing changes without weights, the fused loop against the mirror loops over
the first K iterations, the replayed graph against the eager launches.  Helpers and bars: tests/test_pose_opt_nature.py."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_pose_opt import K, KEYS, LOOP_SEED, make, opt_case  # noqa: E402
from test_pose_opt_nature import check_loop_against_mirror, check_none_changes_nothing, nature_trajectory, weights  # noqa: E402

pytestmark = pytest.mark.gpu
H = 512


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def test_without_weights_nothing_changes():
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    check_none_changes_nothing(FusedTwoHandPoseOptimizer, dev(), 6)


@pytest.mark.parametrize('B', sorted(LOOP_SEED))
def test_fused_loop_with_nature_matches_mirror_loop(B):
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    got = nature_trajectory(make(FusedTwoHandPoseOptimizer, dev(), nature=weights(H)), opt_case(LOOP_SEED[B], B), K)
    check_loop_against_mirror(got, dev(), B, H, K)


def test_replayed_graph_with_nature_is_bit_identical_to_eager_launches():
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    graphed = make(FusedTwoHandPoseOptimizer, dev(), n_iter=12, nature=weights(H))
    eager = make(FusedTwoHandPoseOptimizer, dev(), n_iter=12, graph=False, nature=weights(H))
    for seed in (1, 2):                                                   # the second set_opt_val reuses the graph
        case = opt_case(seed, 2)
        got = []
        for opt in (graphed, eager):
            opt.set_opt_val(**case)
            got.append((opt.optimize(), opt.last_loss.clone(), opt.last_terms['nature'].clone(), opt.stepper.state.clone()))
        for k in KEYS:
            assert torch.equal(got[0][0][k], got[1][0][k]), (seed, k)
        for a, b in zip(got[0][1:], got[1][1:]):
            assert torch.equal(a, b), seed
        assert got[0][2][2] == 2 and got[0][2][3] == 2 and got[0][2][0] > 0.5
        if seed == 1:
            captured = graphed._graph
    assert graphed._graph is captured and eager._graph is None
