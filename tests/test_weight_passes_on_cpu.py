"""tests/test_gpu_weight_passes.py on the host-compiled kernels (tests/hipcpu, as tests/test_kernels_on_cpu.py): the wide and the
reference kernels of the split-K reduction, the weight repack and the H2 weight planes, executed on the CPU -- the same cases, the
same bitwise comparisons, the same poison around the outputs."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

import test_gpu_weight_passes as TW     # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture(autouse=True)
def _host_kernels(monkeypatch):
    from host_kernels import host_kernels_abi
    monkeypatch.setattr(TW, 'dev', lambda: CPU)
    with host_kernels_abi():
        yield


def test_reduce_multi_is_bitwise_the_contract_on_both_kernels():
    assert TW.check_reduce_multi() == 600


def test_reduce_list_lengths_around_the_pack_size():
    TW.check_reduce_list_lengths()


def test_reduce_unaligned_slabs_take_the_reference_kernel():
    TW.check_reduce_unaligned()


def test_reduce_plain_and_batched_entry_points():
    TW.check_reduce_plain_entry_points()


def test_pack_is_bitwise_the_numpy_maps_on_both_kernels():
    TW.check_pack()


def test_h2_planes_are_bitwise_the_reference_kernel():
    TW.check_h2()
