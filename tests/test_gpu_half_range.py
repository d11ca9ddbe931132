"""The fp16-storage backbone's kernels (csrc/rih_half.hip) on the hardware, away from unit scale and on the wide halo tiles.
tests/test_half.py::kernels_vs_torch draws N(0, 1) activations and BatchNorm statistics in [0.5, 1.5] and never launches
hconv3_halo_kernel<*, 128>; a trained checkpoint has BatchNorm weights over decades and dead channels, so its folded weights and
its activations reach into the fp16 subnormals and up to the saturation of the epilogue.  What the host build of the kernels
cannot say is how v_mfma_f32_32x32x16_f16 treats subnormal operands, how the _Float16 conversions round and saturate, and
whether the LDS-DMA zero page holds at the wide tile shapes; this file asks the GPU.

  * tests/half_cases.py, one test per (kernel, regime): fp64 reference of the same fp16 operands (test_half.check_range), fp16
    and fp32 output, and the plan code of rih_hconv_plan -- every instantiation of hconv_kernel and hconv3_halo_kernel is
    named by a passing test (test_half.py::test_half_case_plans_cover_every_instantiation keeps the table complete);
  * the list again in a child interpreter for each per-process switch of the library;
  * the other entry points called directly at their edges (test_half.ENTRY_POINTS);
  * the whole backbone on checkpoint-like statistics against the emulator, which rounds at the same points.
Every measured figure is printed before it is asserted."""
import os
import subprocess
import sys

import pytest
import torch

import half_cases
import test_half

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.mark.parametrize('kernel,regime', half_cases.CASES + half_cases.WIDE_CASES, ids=lambda v: v)
def test_conv_kernel_off_unit_scale(kernel, regime):
    half_cases.run_case(test_half.conv_case, dev(), kernel, regime)


@pytest.mark.parametrize('switch', ['RIH_HCONV_GLDS=0', 'RIH_HCONV_HALO=0', 'RIH_HCONV_BN=128'])
def test_conv_kernels_under_switch(switch):
    """The register-staged loaders, the implicit GEMM on the halo kernels' shapes and the 128-wide tile on one-k-tile
    reductions: each switch is read once per process by the library, hence its own interpreter, which runs the list once."""
    code = ('import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r); import half_cases, test_half; '
            'half_cases.run_all(test_half.conv_case, torch.device("cuda:0")); torch.cuda.synchronize(); print("SWITCH-OK")'
            % (ROOT, os.path.join(ROOT, 'tests')))
    name, value = switch.split('=')
    p = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **{name: value}))
    print(p.stdout[-20000:])
    assert p.returncode == 0 and 'SWITCH-OK' in p.stdout, (p.stdout + p.stderr)[-3000:]


@pytest.mark.parametrize('entry', sorted(test_half.ENTRY_POINTS))
def test_entry_point_at_its_edges(entry):
    test_half.ENTRY_POINTS[entry](dev())


def test_backbone_on_checkpoint_like_statistics():
    """HalfBackbone on the kernels against HalfBackbone on the emulator: 4 x what the host build of the kernels deviates from
    the emulator on the same model and image, since only the order of the fp32 sums differs."""
    test_half.backbone_kernels_vs_emulator(dev(), None, bar=4 * test_half.HOST_VS_EMULATOR)
