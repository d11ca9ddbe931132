"""The sequence driver on the GPU (renderih_amd.pose_driver.optimize_sequence over FusedTwoHandPoseOptimizer(graph=True) and
FusedTwoHandContactSearch): N = 3 frames in batches of 2 + 1 through the four attempts of the shortened schedule -- four
`coef_val` settings and the B = 2 -> 1 shape change, each a recapture -- bit-equal to the loop written out in
tests/test_pose_driver.py over the same objects, finite, both root quaternions bit-equal to the inputs."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_pose_driver import run_real  # noqa: E402

pytestmark = pytest.mark.gpu


def test_driver_equals_the_written_out_loop_on_the_fused_graph():
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    opt = run_real(FusedTwoHandPoseOptimizer, FusedTwoHandContactSearch, torch.device('cuda:0'), graph=True)
    assert opt._graph is not None and opt.batch_size == 1
