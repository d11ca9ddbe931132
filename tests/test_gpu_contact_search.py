"""The contact search on the GPU (renderih_amd.contact_search.FusedTwoHandContactSearch, csrc/rih_contact.hip): against the
reference's own outputs on the golden's decided rows (B = 4, A = 108, V = 778), the mirror on the device against the same, the
crafted 8-anchor table with its ascending-index tie rule (D = 4 and 1, B = 2 and 1, out-of-range previous ids), a refresh after
a fresh search on moved meshes, bit-identical repeated runs, and the refusals.  Helpers and bars: tests/test_contact_search.py.
Figures found on an MI355X: profiles/contact_search/pytest_gpu_new.log."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_contact_search import run_crafted, run_einval, run_golden, run_refresh, run_wide  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def test_kernel_matches_reference_on_decided_rows():
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    run_golden(FusedTwoHandContactSearch, dev())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_on_the_device_matches_reference_on_decided_rows(dtype):
    from renderih_amd.contact_search import TwoHandContactSearch
    run_golden(TwoHandContactSearch, dev(), dtype)


def test_kernel_orders_ties_by_ascending_index():
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    run_crafted(FusedTwoHandContactSearch, dev())


def test_kernel_above_128_anchors():
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    run_wide(FusedTwoHandContactSearch, dev())


def test_kernel_refresh_and_bit_identical_runs():
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    run_refresh(FusedTwoHandContactSearch, dev())


def test_kernel_refuses_bad_arguments():
    from renderih_amd import _lib
    buf = torch.zeros(64, device=dev())
    run_einval(_lib.load(), buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
