"""The joints -> MANO fit (renderih_amd.joint_fit; reference utils/mano_from_3djoint/) on the CPU: the torch mirrors against the
reference's golden, and the kernels of csrc/rih_joint_fit.hip through the host-compiled library (tests/hipcpu) against the mirrors.
Cases, oracle, checks and bars: tests/joint_fit_cases.py; tests/test_gpu_joint_fit.py runs the same checks on the GPU.  The fused
whole fit (200 iterations) and the replayed graph run on the GPU only: an iteration of the host-compiled MANO kernels takes
about a second."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

import joint_fit_cases as JC  # noqa: E402


@pytest.fixture
def host():
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        yield 'cpu'


@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('side,B', [('right', 1), ('right', 3), ('left', 3), ('right', 9)])
def test_ik_matches_reference_and_oracle(host, side, B, normalize):
    JC.check_ik_parity(host, side, B, normalize)


def test_ik_rules(host):
    JC.check_ik_rules(host)


def test_mat2aa_mirror_matches_reference_and_its_autograd():
    JC.check_mat2aa_golden()


@pytest.mark.parametrize('N', [1, 15, 257])
def test_mat2aa_kernels_match_fp64_mirror(host, N):
    JC.check_mat2aa_parity(host, N)


def test_mat2aa_rules(host):
    JC.check_mat2aa_rules(host)


@pytest.mark.parametrize('B', [1, 3, 300])
def test_joint_l1_kernel(host, B):
    JC.check_joint_l1(host, B)


def test_lr_linear_step_equals_python(host):
    JC.check_lr_schedule(host)


def test_mirror_follows_the_reference_loop():
    JC.check_golden_prefix()


def test_one_iteration_teacher_forced(host):
    JC.check_one_iteration(host)


@pytest.mark.parametrize('B', [1, 3])
def test_prefix_of_the_loop(host, B):
    JC.check_prefix(host, B)


def test_mirror_whole_fit():
    JC.check_mirror_whole_fit()


def test_surface(host):
    JC.check_surface(host)


def test_refusals(host):
    JC.check_refusals(host)


def test_cpu_tensors_are_refused_without_the_host_library():
    import torch
    from renderih_amd import joint_fit as JF
    J = torch.tensor(JC.hands('right', 1))
    with pytest.raises(RuntimeError):
        JF.fused_adaptive_ik(torch.tensor(JC.golden()['template/right']), J)
    with pytest.raises(RuntimeError):
        JF.FusedMat2AA.apply(torch.eye(3)[None])
    with pytest.raises(ValueError):
        JF.FusedManoJointFitter(JC.layer('right', 'cpu'), device='cpu')               # graph=True needs a GPU
    with pytest.raises(RuntimeError):
        JF.FusedManoJointFitter(JC.layer('right', 'cpu'), device='cpu', graph=False).fit(J)
