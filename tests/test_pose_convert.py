"""The pose-data converter, augmenter and validity judge (renderih_amd.pose_convert; reference pose_data_optimize/scripts/
HandPoseConverter.py, scripts/HandPoseArguer.py, Ver2Code/NatureJudge/PoseArgue.py, Ver2Code/ValidJudge/ValidJudger.py) on the
CPU: the plain-torch mirror in fp64 and fp32 and the kernel (csrc/rih_pose_convert.hip) through the host-compiled library,
against tests/golden/pose_convert.npz; tests/pose_convert_cases.py describes the bars and the cases.
tests/test_gpu_pose_convert.py runs the same checks on the GPU.  Figures found: profiles/pose_convert/pytest_cpu.log."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

import pose_convert_cases as cc  # noqa: E402


@pytest.fixture
def host():
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        yield


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_against_the_fixture(dtype):
    cc.run_fixture(False, 'cpu', dtype)


def test_fp32_bars_are_four_times_the_mirrors_measured_error():
    """The bars of pose_convert_cases come from the fp32 mirror on the CPU, nothing else: measured again here (libm and the
    vector units differ a little from one CPU to another), the figures written there are within a factor 2 of what is found."""
    worst = cc.fixture_errors(False, 'cpu', torch.float32)
    for k, e in worst.items():
        print('fp32 mirror %s: %.3e (written down: %.3e)' % (k, e, cc.MIRROR_FP32[k]))
        assert 0.5 * cc.MIRROR_FP32[k] <= e <= 2 * cc.MIRROR_FP32[k], (k, e)
        assert cc.BARS[k] == 4 * cc.MIRROR_FP32[k]


def test_default_tables_are_the_fixtures():
    cc.run_tables()


@pytest.mark.parametrize('M', cc.TAILS)
def test_mirror_fp32_at_tail_shapes(M):
    cc.run_tail(False, 'cpu', M)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_round_trips_at_lock_identity_and_pi(dtype):
    cc.run_round_trips(False, 'cpu', dtype)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_keeps_adjusted_angles_in_range(dtype):
    cc.run_in_range(False, 'cpu', dtype)


def test_mirror_leaves_inputs_untouched_and_refuses_bad_input():
    cc.run_untouched(False, 'cpu')
    cc.run_bad_input(False, 'cpu')


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_loc_and_trans_against_the_layers_joint_0(dtype):
    cc.run_loc_trans('cpu', dtype)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_dict_glue_round_trip_on_the_mirror(dtype):
    cc.run_glue(False, 'cpu', dtype)


def test_hash_uniforms_restates_the_kernels_hash():
    from abi_emulator import hash_np
    idx = np.arange(3 * 32, 10 * 32, dtype=np.uint64)
    for seed in (0, 7, 0xFEDCBA9876543210):
        u = ((hash_np(seed, idx) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(7, 16, 2)
        assert np.array_equal(u, cc.pc.hash_uniforms(seed, 7, row_offset=3))
        assert u.min() >= 0 and u.max() < 1


# ------------------------------------------------------------------------------------------------ the kernel, on the host
def test_kernel_against_the_fixture_on_cpu(host):
    cc.run_fixture(True, 'cpu')


@pytest.mark.parametrize('M', cc.TAILS)
def test_kernel_at_tail_shapes_on_cpu(host, M):
    cc.run_tail(True, 'cpu', M)


def test_kernel_round_trips_at_lock_identity_and_pi_on_cpu(host):
    cc.run_round_trips(True, 'cpu')


def test_kernel_seeded_draws_on_cpu(host):
    from abi_emulator import hash_np
    cc.run_seeded('cpu', hash_np)


def test_kernel_keeps_adjusted_angles_in_range_on_cpu(host):
    cc.run_in_range(True, 'cpu')


def test_kernel_leaves_inputs_untouched_and_refuses_bad_input_on_cpu(host):
    cc.run_untouched(True, 'cpu')
    cc.run_bad_input(True, 'cpu')


def test_dict_glue_round_trip_on_the_host_kernels(host):
    cc.run_glue(True, 'cpu')


def test_kernel_refuses_bad_arguments():
    from host_kernels import load
    buf = np.zeros(64 * 44, np.float32)
    cc.run_einval(load(), buf.ctypes.data)


def test_fused_classes_have_no_cpu_fallback():
    q = torch.from_numpy(cc.FIX['right/quat'])
    with pytest.raises(RuntimeError):
        cc.make(cc.pc.FusedPoseConverter, 'right').quat_to_euler(q)                       # GPU only
    with pytest.raises(RuntimeError):
        cc.make(cc.pc.FusedPoseAugmenter, 'right', 'script')(torch.zeros(2, 16, 3), 2, seed=1)
    with pytest.raises(RuntimeError):
        cc.make(cc.pc.FusedPoseValidJudge)(q, q)
