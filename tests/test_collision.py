"""The two-hand collision count (renderih_amd.collision; reference pose_data_optimize/collision/CollisionFilter.py and
CollisionCheck.py) on the CPU: the plain-torch mirror in fp64 and fp32 and the kernel (csrc/rih_collision.hip) through the
host-compiled library, against the numpy fp64 oracle of tests/collision_cases.py, where the bars and the cases are described.
tests/test_gpu_collision.py runs the same checks on the GPU.  Figures found: profiles/collision/pytest_cpu_new.log."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import collision_cases as cc  # noqa: E402


def fused():
    from renderih_amd.collision import FusedTwoHandCollisionCount
    return FusedTwoHandCollisionCount


def mirror():
    from renderih_amd.collision import TwoHandCollisionCount
    return TwoHandCollisionCount


@pytest.fixture
def host():
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        yield


# ------------------------------------------------------------------------------------------------ the mirror
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_on_the_fixture_frames(dtype):
    cc.run_fixture(mirror(), 'cpu', dtype)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_on_the_crafted_pairs(dtype):
    cc.run_crafted(mirror(), 'cpu', dtype)


@pytest.mark.parametrize('name', list(cc.SOUPS))
def test_mirror_on_triangle_soups(name):
    cc.run_soup(mirror(), 'cpu', name)


def test_mirror_never_holds_all_pairs_at_once(monkeypatch):
    """With room for one frame's box tests of 7 main faces at a time the result is the same: the chunks are an implementation
    detail (and B x Fm x Fs intermediates never exist)."""
    from renderih_amd import collision
    whole = cc.run_soup(mirror(), 'cpu', 'past a tile B=3')[-1]
    monkeypatch.setattr(collision, 'MIRROR_PAIRS', 3 * 130 * 7)
    parts = cc.run_soup(mirror(), 'cpu', 'past a tile B=3')[-1]
    for k in cc.KEYS:
        assert torch.equal(whole[k], parts[k]), k


def test_mirror_properties():
    cc.run_offset(mirror(), 'cpu')
    cc.run_nan(mirror(), 'cpu')
    cc.run_bad_table(mirror(), 'cpu')


# ------------------------------------------------------------------------------------------------ the kernel, on the host
def test_kernel_on_the_fixture_frames_on_cpu(host):
    cc.run_fixture(fused(), 'cpu')


def test_kernel_on_the_crafted_pairs_on_cpu(host):
    cc.run_crafted(fused(), 'cpu')


@pytest.mark.parametrize('name', cc.EDGE_SOUPS)
def test_kernel_at_tile_and_chunk_edges_on_cpu(host, name):
    cc.run_soup(fused(), 'cpu', name)


def test_kernel_under_survivor_list_pressure_on_cpu(host):
    cc.run_soup(fused(), 'cpu', 'survivor-list pressure')


@pytest.mark.parametrize('name', ['wide tables', 'sub table above 1538 faces'])
def test_kernel_on_wide_tables_on_cpu(host, name):
    cc.run_soup(fused(), 'cpu', name)


def test_kernel_repeated_runs_are_bit_identical_on_cpu(host):
    cc.run_repeat(fused(), 'cpu')


def test_kernel_is_offset_invariant_on_cpu(host):
    cc.run_offset(fused(), 'cpu')


def test_kernel_nan_vertex_zeroes_only_its_faces_on_cpu(host):
    cc.run_nan(fused(), 'cpu')


def test_kernel_refuses_bad_arguments():
    from host_kernels import load
    buf = np.zeros(64, np.float64)
    cc.run_einval(load(), buf.ctypes.data)


def test_surface_refuses_what_it_cannot_run(host):
    cc.run_bad_table(fused(), 'cpu')
    vm, vs, fm, fs = cc.soup(1, 1, 4, 5, 0.05, 0.02)
    with pytest.raises(ValueError):
        fused()(fm, fs)(torch.from_numpy(vm).double(), torch.from_numpy(vs).double())      # fp32 only


def test_fused_count_has_no_cpu_fallback():
    vm, vs, fm, fs = cc.soup(1, 1, 4, 5, 0.05, 0.02)
    with pytest.raises(RuntimeError):
        fused()(fm, fs)(torch.from_numpy(vm), torch.from_numpy(vs))                        # GPU only


# ------------------------------------------------------------------------------------------------ filter_sequence
def test_filter_sequence_equals_the_written_out_composition_on_the_mirrors(host):
    from renderih_amd.pose_opt import TwoHandPoseOptimizer
    cc.run_filter(TwoHandPoseOptimizer, mirror(), 'cpu')


def test_filter_sequence_equals_the_written_out_composition_on_the_host_kernels(host):
    from renderih_amd.pose_opt import TwoHandPoseOptimizer           # the fused hand model on the host shim takes half a minute
    cc.run_filter(TwoHandPoseOptimizer, fused(), 'cpu')
