"""The pose-data converter, augmenter and validity judge on the GPU (renderih_amd.pose_convert's fused classes,
csrc/rih_pose_convert.hip) against tests/golden/pose_convert.npz and the fp64 mirror; tests/pose_convert_cases.py describes the
bars and the cases: the fixture, the tail shapes (M = 1, 3, 4, 5, 35), round trips at gimbal lock, the identity and angle pi,
seeded draws, the in-range property, untouched inputs, refusals, the dict glue and a graph replay; the mirror on the device
beside it.  Figures found on an MI355X: profiles/pose_convert/pytest_gpu.log."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import pose_convert_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def test_kernel_against_the_fixture():
    cc.run_fixture(True, dev())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_on_the_device_against_the_fixture(dtype):
    cc.run_fixture(False, dev(), dtype)


@pytest.mark.parametrize('M', cc.TAILS)
def test_kernel_at_tail_shapes(M):
    cc.run_tail(True, dev(), M)


def test_kernel_round_trips_at_lock_identity_and_pi():
    cc.run_round_trips(True, dev())


def test_kernel_seeded_draws():
    from abi_emulator import hash_np
    cc.run_seeded(dev(), hash_np)


def test_kernel_keeps_adjusted_angles_in_range():
    cc.run_in_range(True, dev())


def test_kernel_leaves_inputs_untouched_and_refuses_bad_input():
    cc.run_untouched(True, dev())
    cc.run_bad_input(True, dev())


def test_kernel_refuses_bad_arguments():
    from renderih_amd import _lib
    buf = torch.zeros(64 * 44, device=dev())
    cc.run_einval(_lib.load(), buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def test_dict_glue_round_trip():
    cc.run_glue(True, dev())


def test_augmenter_replayed_from_a_graph_equals_eager_launches():
    """`FusedPoseAugmenter(out='quat')` captured once, replayed on other angles: bit-identical to eager calls."""
    a = cc.make(cc.pc.FusedPoseAugmenter, 'left', 'script')
    first, second = (cc.seeded_euler(5, s).to(device=dev(), dtype=torch.float32) for s in (21, 22))
    eager = [a(x, 7, seed=5, out='quat') for x in (first, second)]
    e, res = first.clone(), torch.empty(35, 16, 4, device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a(e, 7, seed=5, out='quat', result=res)                      # warm-up outside the capture (the table's upload)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a(e, 7, seed=5, out='quat', result=res)
    for x, want in ((second, eager[1]), (first, eager[0])):
        e.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(res, want)
    assert not torch.equal(eager[0], eager[1])
