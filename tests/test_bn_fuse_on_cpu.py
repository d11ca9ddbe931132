"""tests/test_gpu_bn_fuse.py on the host-compiled kernels (tests/hipcpu, as tests/test_weight_passes_on_cpu.py): the fused
BatchNorm pair and the fused stem against the call sequences they replace, executed on the CPU -- the same bodies, the same
bitwise comparisons, the same poison around the outputs.

Host execution pays about 0.1 ms per wavefront collective, so a case costs 0.05 s at (7, 8), 1 s at (512, 64), 6 s at
(1030, 256) and 14 s at (65, 2048).  The small shapes run the full product of regimes and flags here; (512, 64) and the two
multi-chunk stem shapes run every regime and every flag set at least once; the two widest pair shapes run on the GPU only.

Also here: the model on the numpy restatement of the ABI (tests/abi_emulator.py), which has no fused entry points -- it must keep
issuing the unfused sequence."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))
sys.path.insert(0, HERE)

import test_gpu_bn_fuse as TB     # noqa: E402

CPU = torch.device('cpu')


@pytest.fixture
def host_kernels(monkeypatch):
    from host_kernels import host_kernels_abi
    monkeypatch.setattr(TB, 'dev', lambda: CPU)
    with host_kernels_abi():
        yield


@pytest.mark.parametrize('rows,Cc', TB.PAIR_SHAPES[:3])
def test_pair_is_bitwise_the_two_call_sequence(host_kernels, rows, Cc):
    assert TB.check_pair_shape(rows, Cc) == 48


@pytest.mark.parametrize('regime', TB.REGIMES)
def test_pair_multi_chunk_shape_every_regime_and_every_flag_set(host_kernels, regime):
    flags = TB.pair_flags()
    k = TB.REGIMES.index(regime)
    for relu, fa, fb in (flags[k], flags[(k + 4) % 8]):         # six regimes x two of the eight flag sets: each set at least once
        TB.check_pair(*TB.PAIR_SHAPES[3], relu, fa, fb, regime, seed=k)


def test_pair_refuses_what_it_cannot_do(host_kernels):
    TB.test_pair_refuses_what_it_cannot_do()


@pytest.mark.parametrize('rows,Cc', TB.MASK_Y_SHAPES[:3])
def test_bwd_gated_by_mask_is_bitwise_gated_by_y(host_kernels, rows, Cc):
    assert TB.check_bwd_mask_equals_y_shape(rows, Cc) == 24


@pytest.mark.parametrize('regime', TB.MASK_Y_REGIMES)
def test_bwd_gated_by_mask_is_bitwise_gated_by_y_multi_chunk_shape(host_kernels, regime):
    k = TB.MASK_Y_REGIMES.index(regime)
    frozen, with_dres = TB.mask_y_flags()[3 * k]        # (0, dres), (1, no dres), (3, dres)
    TB.check_bwd_mask_equals_y(*TB.MASK_Y_SHAPES[3], frozen, with_dres, regime, seed=k)


@pytest.mark.parametrize('N,H,W,Cc', TB.POOL_SHAPES[:5])
def test_stem_is_bitwise_the_four_call_sequence(host_kernels, N, H, W, Cc):
    assert TB.check_pool_shape(N, H, W, Cc) == 12


@pytest.mark.parametrize('N,H,W,Cc', TB.POOL_SHAPES[5:])
@pytest.mark.parametrize('part', range(3))
def test_stem_multi_chunk_shapes_every_regime_frozen_and_not(host_kernels, N, H, W, Cc, part):
    for k in (2 * part, 2 * part + 1):
        TB.check_pool(N, H, W, Cc, k % 2, TB.REGIMES[k], seed=k)
        TB.check_pool(N, H, W, Cc, 1 - k % 2, TB.REGIMES[k], seed=k + 6)


def test_stem_refuses_what_it_cannot_do(host_kernels):
    TB.test_stem_refuses_what_it_cannot_do()


def test_emulated_abi_has_no_fused_kernels_and_the_model_takes_the_unfused_sequence(monkeypatch):
    from abi_emulator import emulated_abi, EmulatedLib
    from renderih_amd import ops
    monkeypatch.setattr(TB, 'dev', lambda: CPU)
    calls = []
    for name in ('rih_bn_apply', 'rih_bn_bwd', 'rih_maxpool3x3s2_fwd', 'rih_maxpool3x3s2_bwd'):
        def spy(self, *a, _f=getattr(EmulatedLib, name), _n=name):
            calls.append((_n, bool(a[5]) if _n == 'rih_bn_apply' else bool(a[7]) if _n == 'rih_bn_bwd' else None))  # residual / dres?
            return _f(self, *a)
        monkeypatch.setattr(EmulatedLib, name, spy)
    state, x, w = TB.mini_inputs()
    with emulated_abi():
        assert ops.BN_PAIR_FUSE and ops.BN_POOL_FUSE and not ops.bn_pair_fused() and not ops.bn_pool_fused()
        out = TB.run_mini(state, x, w, True, True)
    assert all(torch.isfinite(v).all() for v in out.values())
    # the stem's BatchNorm, 2 x 3 in the blocks and the downsample branch's: one rih_bn_apply and one rih_bn_bwd each, both blocks
    # end with a residual; the pool runs as its own two calls
    names = [c[0] for c in calls]
    assert names.count('rih_bn_apply') == 8 and names.count('rih_bn_bwd') == 8
    assert calls.count(('rih_bn_apply', True)) == 2 and calls.count(('rih_bn_bwd', True)) == 2
    assert names.count('rih_maxpool3x3s2_fwd') == 1 and names.count('rih_maxpool3x3s2_bwd') == 1
