"""The joints -> MANO fit on the GPU (renderih_amd.joint_fit, csrc/rih_joint_fit.hip): the checks of tests/joint_fit_cases.py on
the device, the whole fit of 200 iterations, and the replayed graph against eager launches.  Figures found on an MI355X:
profiles/joint_fit/deviation_gpu.log."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import joint_fit_cases as JC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('side,B', [('right', 1), ('right', 3), ('left', 3), ('right', 9)])
def test_ik_matches_reference_and_oracle(side, B, normalize):
    JC.check_ik_parity(DEV, side, B, normalize)


def test_ik_rules():
    JC.check_ik_rules(DEV)


@pytest.mark.parametrize('N', [1, 15, 257])
def test_mat2aa_kernels_match_fp64_mirror(N):
    JC.check_mat2aa_parity(DEV, N)


def test_mat2aa_rules():
    JC.check_mat2aa_rules(DEV)


@pytest.mark.parametrize('B', [1, 3, 300])
def test_joint_l1_kernel(B):
    JC.check_joint_l1(DEV, B)


def test_lr_linear_step_equals_python():
    JC.check_lr_schedule(DEV)


def test_one_iteration_teacher_forced():
    JC.check_one_iteration(DEV)


@pytest.mark.parametrize('B', [1, 3])
def test_prefix_of_the_loop(B):
    JC.check_prefix(DEV, B)


@pytest.mark.parametrize('graph', [True, False])
def test_whole_fit(graph):
    JC.check_whole_fit(DEV, graph)


def test_graph_replay_is_bit_identical_to_eager_launches():
    JC.check_graph(DEV)


def test_surface():
    JC.check_surface(DEV)


def test_refusals():
    JC.check_refusals(DEV)
