"""The auxiliary heads (renderih_amd.aux_heads; reference dataset/heatmap.py, core/Loss.py:180-198, dataset/inference.py:113-127,
core/loader_ori.py:117-145) on the CPU: the plain-torch mirror in fp64 and fp32 and the kernels (csrc/rih_aux.hip) through the
host-compiled library, against tests/golden/aux_heads.npz; tests/aux_heads_cases.py describes the bars and the cases.
tests/test_gpu_aux_heads.py runs the same checks on the GPU.  Figures found: profiles/aux_heads/pytest_cpu.log."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

import aux_heads_cases as cc  # noqa: E402

ah = cc.ah


@pytest.fixture
def host():
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        yield


# ------------------------------------------------------------------------------------------------ the mirror
def test_fp32_bars_are_four_times_the_mirrors_measured_error():
    """The bars of aux_heads_cases come from the fp32 mirror on the CPU, nothing else: measured again here (libm and the vector
    units differ a little from one CPU to another), the figures written there are within a factor 2 of what is found."""
    worst = cc.mirror_errors()
    for k, e in worst.items():
        print('fp32 mirror %s: %.3e (written down: %.3e)' % (k, e, cc.MIRROR_FP32[k]))
        assert 0.5 * cc.MIRROR_FP32[k] <= e <= 2 * cc.MIRROR_FP32[k], (k, e)
        assert cc.BARS[k] == 4 * cc.MIRROR_FP32[k]


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_heat_maps(dtype):
    cc.run_heatmaps(False, 'cpu', dtype)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_loss_against_the_fixture(dtype):
    cc.run_loss_fixture(False, 'cpu', dtype)


@pytest.mark.parametrize('absent', [None, 'mask', 'dense', 'hms'])
@pytest.mark.parametrize('shape', cc.LOSS_SHAPES[:3])
def test_mirror_fp32_loss(shape, absent):
    cc.run_loss(False, 'cpu', shape, absent=absent)


def test_mirror_loss_forms_properties_and_refusals():
    cc.run_loss_forms_agree(False, 'cpu', (1, 3, 5))
    cc.run_loss_properties(False, 'cpu')
    cc.run_loss_refusals(False, 'cpu')


def test_weights_come_from_the_reference_config_layout():
    class Node(dict):
        __getattr__ = dict.__getitem__
    cfg = Node(LOSS_WEIGHT=Node(AUX=Node(DENSEPOSE=3, MASK=5, HMS=7), DATA=Node(LABEL_3D=100)))
    for w in (cfg, cfg.LOSS_WEIGHT, cfg.LOSS_WEIGHT.AUX, {'DENSEPOSE': 3, 'MASK': 5, 'HMS': 7}):
        assert ah.aux_weights(w) == {'MASK': 5.0, 'DENSEPOSE': 3.0, 'HMS': 7.0}
    assert ah.aux_weights(None) == {'MASK': 500.0, 'DENSEPOSE': 30.0, 'HMS': 100.0}       # utils/defaults.yaml:51-54
    assert (ah.BLUR_KERNEL, ah.HEATMAP_SIZE, ah.HEATMAP_SIGMA) == (5, 64, 2)              # dataset/dataset_utils.py:4-8
    with pytest.raises(KeyError):
        ah.aux_weights({'BONE': 1})
    hand_loss = type('L', (), {'smoothL1Loss': torch.nn.SmoothL1Loss(beta=0.5)})()
    d = cc.shape_inputs(1, 3, 5)
    pred = {'mask': cc.t(d['p_mask'])}
    out = ah.calc_aux_loss(cfg, hand_loss, pred, cc.t(d['t_mask']), None, None)            # beta read from hand_loss
    want = torch.nn.functional.smooth_l1_loss(pred['mask'], cc.t(d['t_mask']), beta=0.5)
    assert float(out['mask_loss']) == float(want) and float(out['total_loss']) == 5 * float(want)
    assert float(out['dense_loss']) == 0 and float(out['hms_loss']) == 0


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_decoder_against_the_fixture(dtype):
    cc.run_decode_fixture(False, 'cpu', dtype)


@pytest.mark.parametrize('kernel', cc.DECODE_KERNELS)
@pytest.mark.parametrize('size', cc.DECODE_SIZES)
def test_mirror_fp32_decoder(size, kernel):
    for NJ in (1, 126):
        cc.run_decode(False, 'cpu', size, NJ, kernel)
    cc.run_decode_refusals(False, 'cpu')


# ------------------------------------------------------------------------------------------------ the kernels, on the host
def test_kernel_heat_maps_on_cpu(host):
    cc.run_heatmaps(True, 'cpu')


def test_kernel_loss_against_the_fixture_on_cpu(host):
    cc.run_loss_fixture(True, 'cpu')


@pytest.mark.parametrize('absent', [None, 'mask', 'dense', 'hms'])
@pytest.mark.parametrize('shape', cc.LOSS_SHAPES[:3])
def test_kernel_loss_on_cpu(host, shape, absent):
    cc.run_loss(True, 'cpu', shape, absent=absent)


@pytest.mark.parametrize('form', ['tensor', 'joints'])
def test_kernel_loss_at_several_items_a_plane_on_cpu(host, form):
    cc.run_loss(True, 'cpu', cc.LOSS_SHAPES[3], form=form)


@pytest.mark.parametrize('shape', cc.LOSS_SHAPES[:3])
def test_kernel_loss_label_forms_agree_on_cpu(host, shape):
    cc.run_loss_forms_agree(True, 'cpu', shape)


def test_kernel_loss_properties_and_refusals_on_cpu(host):
    cc.run_loss_properties(True, 'cpu')
    cc.run_loss_refusals(True, 'cpu')


def test_kernel_loss_on_unaligned_views_takes_the_dword_path_on_cpu(host):
    """A plane size that is a multiple of 4 behind a pointer that is not 16-byte aligned: same result as the aligned call."""
    B, Jh, S = 1, 1, 4
    d = cc.shape_inputs(B, Jh, S)
    loss = ah.FusedAuxLoss()

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32)
        v = buf[1:].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    pred = {k: shifted(d['p_' + k]).requires_grad_(True) for k in ('mask', 'dense', 'hms')}
    total, _ = loss(pred, shifted(d['t_mask']), shifted(d['t_dense']), hms=shifted(d['t_hms']))
    total.backward()
    want = cc.loss_reference(B, Jh, S)
    assert cc.rel(total, want[0][0]) <= cc.BARS['loss']
    assert max(cc.rel(pred[k].grad, want[1][k]) for k in pred) <= cc.BARS['grad']


def test_kernel_decoder_against_the_fixture_on_cpu(host):
    cc.run_decode_fixture(True, 'cpu')


@pytest.mark.parametrize('kernel', cc.DECODE_KERNELS)
@pytest.mark.parametrize('size', cc.DECODE_SIZES)
def test_kernel_decoder_on_cpu(host, size, kernel):
    cc.run_decode(True, 'cpu', size, 1, kernel)
    if size != (64, 64) or kernel == 5:                  # (126 maps of 64 x 64 through the fibers: the training kernel only)
        cc.run_decode(True, 'cpu', size, 126, kernel)


def test_kernel_decoder_refusals_on_cpu(host):
    cc.run_decode_refusals(True, 'cpu')


def test_kernels_refuse_bad_arguments():
    from host_kernels import load
    buf = np.zeros(64 * 44, np.float32)
    cc.run_einval(load(), buf.ctypes.data)


def test_labels_on_cpu(host):
    cc.run_labels('cpu', 16)


def test_fused_classes_have_no_cpu_fallback():
    d = cc.shape_inputs(1, 1, 4)
    with pytest.raises(RuntimeError):
        ah.FusedHeatmapGenerator(4, 1)(torch.zeros(1, 1, 3))                             # GPU only
    with pytest.raises(RuntimeError):
        ah.FusedAuxLoss()({'mask': cc.t(d['p_mask'], dtype=torch.float32)}, cc.t(d['t_mask'], dtype=torch.float32))
    with pytest.raises(RuntimeError):
        ah.FusedHeatmapDecoder()(torch.zeros(1, 1, 8, 8))


def test_calc_loss_gcn_takes_the_aux_term():
    """`loss.calc_loss_GCN(..., aux=AuxLoss(), ...)`: the total gains the aux total, as the un-commented core/Loss.py:211 would,
    and aux_lost_dict carries the terms; with aux=None the result and its arity are what they were."""
    from renderih_amd import assets, loss as L
    from renderih_amd.manolayer import ManoLayer
    from renderih_amd.decoder import GCN_vert_convert
    g = torch.Generator().manual_seed(5)
    B = 2
    gl, conv, tt = {}, {}, {}
    for s in ('left', 'right'):
        m = ManoLayer(assets.synthetic_mano_dict(s))
        gl[s] = L.GraphLoss(m.J_regressor, m.get_faces(), level=4, device='cpu')
        gd = assets.load_graph_dict(s)
        conv[s] = GCN_vert_convert(vertex_num=778, graph_perm_reverse=gd['graph_perm_reverse'], graph_perm=gd['graph_perm'])
        tt['v3d_' + s], tt['v2d_' + s] = 0.05 * torch.randn(B, 778, 3, generator=g), 256 * torch.rand(B, 778, 2, generator=g)
    result = {'verts3d': {s: tt['v3d_' + s] + 0.01 for s in gl}, 'verts2d': {s: tt['v2d_' + s] + 2 for s in gl}}
    hd = [{'verts3d': {s: 0.05 * torch.randn(B, 252, 3, generator=g) for s in gl},
           'verts2d': {s: 256 * torch.rand(B, 252, 2, generator=g) for s in gl}}]
    d = cc.shape_inputs(2, 42, 8)
    other = {k: cc.t(d['p_' + k], dtype=torch.float32) for k in ('mask', 'dense', 'hms')}
    args = (None, 0, gl['left'], gl['right'], conv['left'], conv['right'], result, None, hd, other, tt['v2d_left'], tt['v2d_right'],
            tt['v3d_left'], tt['v3d_right'], torch.zeros(B, 3))
    plain = L.calc_loss_GCN(*args)
    assert len(plain) == 2
    lab = [cc.t(d[k], dtype=torch.float32) for k in ('t_mask', 't_dense', 't_hms')]
    total, mano, aux = L.calc_loss_GCN(*args, aux=ah.AuxLoss(), mask=lab[0], dense=lab[1], hms=lab[2])
    want = ah.AuxLoss()(other, lab[0], lab[1], hms=lab[2])
    assert set(aux) == set(cc.TERM_KEYS) and float(aux['total_loss']) == float(want[0])
    assert float(total) == float(plain[0] + want[0]) and set(mano) == set(plain[1])
