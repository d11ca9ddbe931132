"""The two-hand collision count on the GPU (renderih_amd.collision.FusedTwoHandCollisionCount, csrc/rih_collision.hip) against
the numpy fp64 oracle of tests/collision_cases.py, where the bars and the cases are described: the fixture's 8 frames, the exact
crafted pairs, soups at the tile and chunk edges, under survivor-list pressure and on wide tables, the runtime properties (repeat
runs, offset, NaN, refusals, a bad table, graph replay) and filter_sequence; the mirror on the device beside it.
Figures found on an MI355X: profiles/collision/pytest_gpu_new.log."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import collision_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def fused():
    from renderih_amd.collision import FusedTwoHandCollisionCount
    return FusedTwoHandCollisionCount


def mirror():
    from renderih_amd.collision import TwoHandCollisionCount
    return TwoHandCollisionCount


def test_kernel_on_the_fixture_frames():
    cc.run_fixture(fused(), dev())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_on_the_device_on_the_fixture_frames(dtype):
    cc.run_fixture(mirror(), dev(), dtype)


def test_kernel_on_the_crafted_pairs():
    cc.run_crafted(fused(), dev())
    cc.run_crafted(mirror(), dev())


@pytest.mark.parametrize('name', cc.EDGE_SOUPS)
def test_kernel_at_tile_and_chunk_edges(name):
    cc.run_soup(fused(), dev(), name)


def test_kernel_under_survivor_list_pressure():
    cc.run_soup(fused(), dev(), 'survivor-list pressure')


@pytest.mark.parametrize('name', ['wide tables', 'sub table above 1538 faces'])
def test_kernel_on_wide_tables(name):
    cc.run_soup(fused(), dev(), name)


def test_kernel_repeated_runs_are_bit_identical():
    cc.run_repeat(fused(), dev())


def test_kernel_is_offset_invariant():
    cc.run_offset(fused(), dev())


def test_kernel_nan_vertex_zeroes_only_its_faces():
    cc.run_nan(fused(), dev())


def test_kernel_refuses_bad_arguments_and_bad_tables():
    from renderih_amd import _lib
    buf = torch.zeros(64, device=dev())
    cc.run_einval(_lib.load(), buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cc.run_bad_table(fused(), dev())


def test_kernel_replayed_from_a_graph_equals_eager_launches():
    """Captured on the fixture's first frames, replayed on its moved ones: nothing is read back by the host inside a call."""
    counter = fused()().to(dev())
    first = [torch.from_numpy(x).to(dev()) for x in cc.fixture()]
    second = [torch.from_numpy(x).to(dev()) for x in cc.fixture('2')]
    eager = [counter(*first), counter(*second)]
    vm, vs = first[0].clone(), first[1].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        counter(vm, vs)                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = counter(vm, vs)
    for frames, want in ((second, eager[1]), (first, eager[0])):
        vm.copy_(frames[0])
        vs.copy_(frames[1])
        graph.replay()
        torch.cuda.synchronize()
        for k in cc.KEYS:
            assert torch.equal(res[k], want[k]), k
    assert not torch.equal(eager[0]['count'], eager[1]['count'])


def test_filter_sequence_equals_the_written_out_composition():
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    cc.run_filter(FusedTwoHandPoseOptimizer, fused(), dev(), graph=True)
