"""The pose optimiser's NatureLoss (renderih_amd.nature; reference geo_optimizer_both_batch.py:110-132 with the network of
Ver2Code/Discriminator/discrim.py) on the CPU: the torch mirror against values and gradients of the reference's own program
(tests/golden/nature_loss.npz, written by tests/golden/make_nature_loss_golden.py), the real kernels (csrc/rih_nature.hip)
through the host-compiled library against the golden and against the mirror evaluated in fp64, the empty masks, the clamped
asin, bit-identical repeats, the argument checks.  Helpers, cases and bars: tests/nature_cases.py (shared with
tests/test_gpu_nature_loss.py).

Measured for the loss / terms bar (profiles/nature_loss/deviation_cpu.log): the fp32 torch mirror deviates from the fp64 mirror
by at most 1.63e-7 over the CPU cases (golden case a); the fused kernels were then found at most 2.2e-7 from the golden and
1.1e-7 from the fp64 mirror.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import nature_cases as nc  # noqa: E402


def close_to_golden(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= 1e-6 * np.abs(want).max(), '%s: max err %g of max %g' % (what, err, np.abs(want).max())


# ------------------------------------------------------------------------------------------------ the mirror against the golden
@pytest.mark.parametrize('name', nc.GOLDEN_CASES)
def test_mirror_matches_reference_golden(name):
    case = nc.golden_case(name)
    want = case['want']
    got = nc.evaluate(nc.module(nc.mirror_cls(), case['H'], case['pred_scale'], case['seed']), case, 'cpu')
    close_to_golden(got['loss'], want['loss'], 'loss')
    close_to_golden(got['terms'], want['terms'], 'terms')
    close_to_golden(got['outputs'], want['outputs'], 'discriminator outputs')
    for k in ('grad_q_r', 'grad_q_l'):
        close_to_golden(got[k], want[k], k)
    assert nc.margin(want['outputs']) >= nc.MARGIN                       # the generator's condition, in the stored fp32 outputs
    if name == 'a':
        assert 0 < want['terms'][2] < 4 and 0 < want['terms'][3] < 4    # masked and unmasked rows on both sides
    if name == 'b':
        assert want['terms'][2] == 0 and want['terms'][0] == 0 and not want['grad_q_r'].any() and want['grad_q_l'].any()


def test_state_dict_keys_and_recipe():
    from renderih_amd.nature import KEYS, Pos2dDiscriminator, load_weights, synthetic_state_dict
    assert tuple(Pos2dDiscriminator(15, 64).state_dict()) == KEYS
    a, b = synthetic_state_dict(3, 64, 8.0), synthetic_state_dict(3, 64, 1.0)
    assert all(torch.equal(a[k], b[k]) for k in KEYS if k != 'layer_pred.weight')
    assert torch.equal(a['layer_pred.weight'], (b['layer_pred.weight'].double() * 8).float())
    assert float(a['pose_layer_1.weight'].abs().max()) <= 45 ** -0.5 and a['pose_layer_2.weight'].shape == (64, 64)
    assert load_weights(a)[1] == 64
    with pytest.raises(ValueError):
        load_weights({k: v for k, v in a.items() if k != 'layer_last.bias'})
    with pytest.raises(ValueError):
        load_weights(dict(a, **{'layer_pred.weight': torch.zeros(3, 64)}))


def test_weights_load_from_a_file(tmp_path):
    from renderih_amd.nature import synthetic_state_dict
    sd = synthetic_state_dict(5, 64, 8.0)
    path = str(tmp_path / 'discrim.pth')
    torch.save(sd, path)
    case = nc.seeded_case(3, 64, 8.0)
    a = nc.evaluate(nc.mirror_cls()(path), case, 'cpu')
    b = nc.evaluate(nc.mirror_cls()(sd), case, 'cpu')
    assert all(np.array_equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ the kernels on the host shim
def test_cases_cover_the_tile_edges():
    from host_kernels import load
    R = load().rih_nature_tile_rows()
    Bs = sorted({c[0] for c in nc.CPU_CASES})
    assert any(2 * B < R for B in Bs) or R == 1, (R, Bs)                 # fewer rows than a tile
    # a tile with hands of both sides (row B - 1 and row B in one tile) and a partial last tile
    assert any((B % R) and (2 * B) % R for B in Bs), (R, Bs)


@pytest.mark.parametrize('name', nc.GOLDEN_CASES)
def test_fused_kernels_match_reference_golden_on_cpu(name):
    from host_kernels import host_kernels_abi
    case = nc.golden_case(name)
    with host_kernels_abi():
        got = nc.fused_vs(case, 'cpu', 'fused vs golden ' + name)
        want64 = nc.evaluate(nc.module(nc.mirror_cls(), case['H'], case['pred_scale'], case['seed']), case, 'cpu', torch.float64)
    nc.compare(got, want64, 'fused vs fp64 mirror, golden ' + name)
    if name == 'b':                                                     # the empty side: exactly 0, value and gradient
        assert got['terms'][0] == 0 and got['terms'][2] == 0 and not got['grad_q_r'].any() and got['loss'] == got['terms'][1]


@pytest.mark.parametrize('B,H,scale', nc.CPU_CASES)
def test_fused_kernels_match_fp64_mirror_on_cpu(B, H, scale):
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        nc.fused_vs(nc.seeded_case(B, H, scale), 'cpu', 'fused vs fp64 mirror B=%d H=%d scale %g' % (B, H, scale))


def test_both_masks_empty_give_exact_zeros():
    from host_kernels import host_kernels_abi
    case = nc.seeded_case(3, 64, 8.0)
    mirror = nc.evaluate(nc.module(nc.mirror_cls(), 64, 8.0, case['seed'], bias1=20.0), case, 'cpu')
    with host_kernels_abi():
        fused = nc.evaluate(nc.module(nc.fused_cls(), 64, 8.0, case['seed'], bias1=20.0), case, 'cpu')
    for got in (mirror, fused):
        assert got['loss'] == 0 and not got['terms'].any() and not got['grad_q_r'].any() and not got['grad_q_l'].any()


def test_clamped_asin_gives_finite_loss_and_gradients():
    """A joint at (cos 45, 0, sin 45, 0): m02 = 1 up to rounding, where the reference's asin is one rounding from NaN and its
    derivative infinite, and m12 = m22 = m01 = m00 = 0 up to rounding (gimbal lock)."""
    from host_kernels import host_kernels_abi
    case = dict(nc.seeded_case(3, 64, 1.0))
    h = np.float32(np.sqrt(0.5))
    for k in ('q_r', 'q_l'):
        q = case[k].copy()
        q[:, 4] = (h, 0, h, 0)
        q[1, 7] = np.array([h, 0, h, 0], np.float32) * np.float32(1.3)
        q[2, 9] = (h, 0, -h, 0)
        case[k] = q
    with host_kernels_abi():
        got = nc.evaluate(nc.module(nc.fused_cls(), 64, 1.0, case['seed']), case, 'cpu')
    assert got['terms'][2] == 3 and got['terms'][3] == 3 and np.isfinite(got['loss']) and got['loss'] > 0
    for k in ('grad_q_r', 'grad_q_l'):
        assert np.isfinite(got[k]).all() and np.abs(got[k][:, 1:4]).max() > 0


def test_reversed_fiber_schedule_gives_equal_results(tmp_path):
    """A kernel whose result depends on the order in which the host shim visits the threads has a missing barrier."""
    code = ('import sys; sys.path.insert(0, %r); import numpy as np, nature_cases as nc\n'
            'from host_kernels import host_kernels_abi\n'
            'with host_kernels_abi():\n'
            '    got = nc.evaluate(nc.module(nc.fused_cls(), 64, 8.0, nc.seeded_case(5, 64, 8.0)["seed"]), '
            'nc.seeded_case(5, 64, 8.0), "cpu")\n'
            'np.savez(sys.argv[1], **got)\n' % HERE)
    from host_kernels import host_kernels_abi
    case = nc.seeded_case(5, 64, 8.0)
    with host_kernels_abi():                         # this process: the default order (HIPCPU_SCHED is read once per process)
        outs = [nc.evaluate(nc.module(nc.fused_cls(), 64, 8.0, case['seed']), case, 'cpu')]
    path = str(tmp_path / 'reverse.npz')
    subprocess.check_call([sys.executable, '-c', code, path], env=dict(os.environ, HIPCPU_SCHED='reverse'))
    outs.append(dict(np.load(path)))
    assert set(outs[0]) == set(outs[1]) and all(np.array_equal(outs[0][k], outs[1][k]) for k in outs[0])
    assert outs[0]['grad_q_r'].any() or outs[0]['grad_q_l'].any()


def test_refused_arguments_raise():
    from host_kernels import host_kernels_abi, load
    from renderih_amd.nature import synthetic_state_dict
    case = nc.seeded_case(3, 64, 8.0)
    ins = [torch.from_numpy(case[k]) for k in ('q_r', 'q_l')]
    for cls in (nc.mirror_cls(), nc.fused_cls()):
        mod = nc.module(cls, 64, 8.0)
        with pytest.raises(ValueError):
            mod(ins[0][:2], ins[1])
        with pytest.raises(ValueError):
            mod(ins[0][:, 1:], ins[1][:, 1:])
    with pytest.raises(RuntimeError):                                   # GPU fp32 only: no CPU fallback
        mod(*ins)
    with pytest.raises(ValueError):
        nc.fused_cls()(synthetic_state_dict(0, 96, 1.0))                # the mirror takes any width, the kernels do not
    nc.mirror_cls()(synthetic_state_dict(0, 96, 1.0))
    with host_kernels_abi():
        strided = [t.transpose(0, 1).contiguous().transpose(0, 1) for t in ins]
        assert not any(t.is_contiguous() for t in strided)
        loss, terms = mod(*strided)                                     # non-contiguous inputs are taken
        want, _ = mod(*ins)
        assert torch.equal(loss, want) and not terms.requires_grad
    lib = load()
    einval = lib.rih_anchor_fwd(None, 0, 0, 0, 1, 4, 1, None)
    assert lib.rih_nature_pack_floats(64) == 8 * 64 * 64 + 97 * 64 + 4 and lib.rih_nature_ws_floats(2, 64) >= 4 * (4 * 64 + 5)
    for H in (0, 32, 96, 576, -64):
        assert lib.rih_nature_pack_floats(H) == 0 and lib.rih_nature_ws_floats(1, H) == 0
    assert lib.rih_nature_ws_floats(0, 64) == 0
    buf = np.zeros(1 << 16, np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    ok = [p] * 13 + [64, None]
    for i in range(13):
        assert lib.rih_nature_pack(*(ok[:i] + [None] + ok[i + 1:])) == einval, i
    assert lib.rih_nature_pack(*(ok[:12] + [p + 4] + ok[13:])) == einval
    for H in (0, 32, 96, 576):
        assert lib.rih_nature_pack(*(ok[:13] + [H, None])) == einval
    for fn, ok, ptrs, ws_at, b_at in ((lib.rih_nature_fwd, [p, p, p, p, 1, 64, None], 4, (0, 3), 4),
                                      (lib.rih_nature_reduce, [p, p, p, 1, 64, None], 3, (0,), 3),
                                      (lib.rih_nature_bwd, [p, p, p, p, p, p, p, 1, 64, None], 7, (0, 3), 7)):
        for i in range(ptrs):
            assert fn(*(ok[:i] + [None] + ok[i + 1:])) == einval, (fn, i)
        for i in ws_at:                                                 # packed and the workspace: 16-byte aligned
            assert fn(*(ok[:i] + [p + 4] + ok[i + 1:])) == einval, (fn, i)
        for bad in (0, -1, (1 << 20) + 1):
            assert fn(*(ok[:b_at] + [bad] + ok[b_at + 1:])) == einval, (fn, bad)
        for H in (0, 32, 96, 576):
            assert fn(*(ok[:b_at + 1] + [H] + ok[b_at + 2:])) == einval, (fn, H)
