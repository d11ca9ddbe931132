"""The auxiliary heads on the GPU (renderih_amd.aux_heads' fused classes, csrc/rih_aux.hip) against tests/golden/aux_heads.npz
and the fp64 mirror; tests/aux_heads_cases.py describes the bars and the cases: heat maps at R = 4, 5, 64, the loss at its four
shapes with each term absent in turn and both heat-map label forms, a graph replay that follows a change of weights, the decoder
at 8 x 8, 8 x 12 and 64 x 64 with kernels 1, 3, 5, 7, the labels at S = 16 and 64, and the composition with the network and
TrainStep; the mirror on the device beside it.  Figures found on an MI355X: profiles/aux_heads/pytest_gpu.log."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import aux_heads_cases as cc  # noqa: E402

ah = cc.ah
pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


# ------------------------------------------------------------------------------------------------ heat maps
def test_kernel_heat_maps():
    cc.run_heatmaps(True, dev())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_heat_maps_on_the_device(dtype):
    cc.run_heatmaps(False, dev(), dtype)


# ------------------------------------------------------------------------------------------------ loss
def test_kernel_loss_against_the_fixture():
    cc.run_loss_fixture(True, dev())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_loss_on_the_device_against_the_fixture(dtype):
    cc.run_loss_fixture(False, dev(), dtype)


@pytest.mark.parametrize('absent', [None, 'mask', 'dense', 'hms'])
@pytest.mark.parametrize('shape', cc.LOSS_SHAPES)
def test_kernel_loss(shape, absent):
    cc.run_loss(True, dev(), shape, absent=absent)


@pytest.mark.parametrize('shape', cc.LOSS_SHAPES)
def test_kernel_loss_joints_label(shape):
    cc.run_loss(True, dev(), shape, form='joints')
    cc.run_loss_forms_agree(True, dev(), shape)


def test_kernel_loss_properties_and_refusals():
    cc.run_loss_properties(True, dev())
    cc.run_loss_refusals(True, dev())
    d = cc.shape_inputs(1, 3, 5)
    with pytest.raises(RuntimeError, match='GPU tensors'):                 # CPU tensors are refused, not copied
        ah.FusedAuxLoss()({'mask': cc.t(d['p_mask'], 'cpu', torch.float32)}, cc.t(d['t_mask'], 'cpu', torch.float32))


def test_kernel_loss_on_unaligned_views_takes_the_dword_path():
    B, Jh, S = 1, 1, 4
    d = cc.shape_inputs(B, Jh, S)

    def shifted(a):
        buf = torch.zeros(a.size + 1, dtype=torch.float32, device=dev())
        v = buf[1:].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 != 0 and v.is_contiguous()
        return v
    pred = {k: shifted(d['p_' + k]).requires_grad_(True) for k in ('mask', 'dense', 'hms')}
    total, _ = ah.FusedAuxLoss()(pred, shifted(d['t_mask']), shifted(d['t_dense']), hms=shifted(d['t_hms']))
    total.backward()
    want = cc.loss_reference(B, Jh, S)
    assert cc.rel(total, want[0][0]) <= cc.BARS['loss']
    assert max(cc.rel(pred[k].grad, want[1][k]) for k in pred) <= cc.BARS['grad']


def test_captured_loss_follows_a_change_of_weights():
    """Forward + backward of FusedAuxLoss (joints label) captured once; `set_weights` between two replays rewrites the device
    array in place: the replayed total and gradients are those of the new weights, bit-identical to an eager call."""
    B, Jh, S = 2, 42, 8
    d = cc.shape_inputs(B, Jh, S)
    loss = ah.FusedAuxLoss()
    pred = {k: cc.t(d['p_' + k], dev(), torch.float32).requires_grad_(True) for k in ('mask', 'dense', 'hms')}
    lab = [cc.t(d[k], dev(), torch.float32) for k in ('t_mask', 't_dense', 'joints')]

    def run():
        total, terms = loss(pred, lab[0], lab[1], joints2d=lab[2], sigma=cc.loss_sigma(S))
        return [total.detach()] + list(torch.autograd.grad(total, list(pred.values())))
    eager = {}
    for w in (500.0, 20.0):
        loss.set_weights(MASK=w)
        eager[w] = [x.clone() for x in run()]
    loss.set_weights(MASK=500.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = run()
    for w in (20.0, 500.0):
        loss.set_weights(MASK=w)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager[w]):
            assert torch.equal(a, b), 'replay with MASK = %g' % w
    assert not torch.equal(eager[500.0][0], eager[20.0][0]) and not torch.equal(eager[500.0][1], eager[20.0][1])
    assert torch.equal(eager[500.0][3], eager[20.0][3])                    # (the heat-map gradient does not depend on MASK)


# ------------------------------------------------------------------------------------------------ decoder
def test_kernel_decoder_against_the_fixture():
    cc.run_decode_fixture(True, dev())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_decoder_on_the_device_against_the_fixture(dtype):
    cc.run_decode_fixture(False, dev(), dtype)


@pytest.mark.parametrize('kernel', cc.DECODE_KERNELS)
@pytest.mark.parametrize('size', cc.DECODE_SIZES)
def test_kernel_decoder(size, kernel):
    for NJ in (1, 126):
        cc.run_decode(True, dev(), size, NJ, kernel)


def test_kernel_decoder_refusals_and_the_largest_map():
    cc.run_decode_refusals(True, dev())
    with pytest.raises(RuntimeError, match='GPU tensors'):
        ah.FusedHeatmapDecoder()(torch.zeros(1, 1, 8, 8))


def test_decoder_replayed_from_a_graph_equals_eager_launches():
    maps = [cc.t(cc.decoder_case(64, 64, 126)[0], dev(), torch.float32), None]
    maps[1] = maps[0].flip(-1).contiguous()
    dec = ah.FusedHeatmapDecoder()
    eager = [tuple(x.clone() for x in dec(m)) for m in maps]
    hm, p, v = maps[0].clone(), torch.empty(3, 42, 2, device=dev()), torch.empty(3, 42, device=dev())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dec(hm, preds=p, maxvals=v)
    for m, want in ((maps[1], eager[1]), (maps[0], eager[0])):
        hm.copy_(m)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(p, want[0]) and torch.equal(v, want[1])
    assert not torch.equal(eager[0][0], eager[1][0])


def test_kernels_refuse_bad_arguments():
    from renderih_amd import _lib
    buf = torch.zeros(64 * 44, device=dev())
    cc.run_einval(_lib.load(), buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ labels
@pytest.mark.parametrize('S', [16, 64])
def test_labels(S):
    cc.run_labels(dev(), S)


# ------------------------------------------------------------------------------------------------ composition
def _training_setup(B):
    from renderih_amd import assets, testing
    from renderih_amd.loss import GraphLoss, FusedMeshLoss
    from renderih_amd.manolayer import ManoLayer
    from renderih_amd.model import build_model

    def model():
        torch.manual_seed(0)
        m = build_model(dropout=0.0)
        m.load_state_dict(testing.deterministic_state(m.state_dict(), seed=4))
        m = m.cuda().train()
        m.decoder.unsample_layer.weight.requires_grad_(False)
        return m
    g = torch.Generator().manual_seed(11)
    lab = {'v3d_l': 0.05 * torch.randn(B, 778, 3, generator=g), 'v3d_r': 0.05 * torch.randn(B, 778, 3, generator=g),
           'v2d_l': 256 * torch.rand(B, 778, 2, generator=g), 'v2d_r': 256 * torch.rand(B, 778, 2, generator=g),
           'root_rel': 0.05 * torch.randn(B, 3, generator=g),
           'mask': (torch.rand(B, 2, 64, 64, generator=g) < 0.3).float(), 'dense': torch.rand(B, 3, 64, 64, generator=g),
           'joints2d': torch.cat([64 * torch.rand(B, 42, 2, generator=g), torch.ones(B, 42, 1)], -1)}
    lab = {k: v.cuda() for k, v in lab.items()}
    mano = {s: ManoLayer(assets.synthetic_mano_dict(s)) for s in ('left', 'right')}
    gl = {s: GraphLoss(mano[s].J_regressor, mano[s].get_faces(), level=4, device=dev()) for s in ('left', 'right')}

    def mesh_loss(m):
        conv = m.decoder.converter
        return FusedMeshLoss(gl['left'], gl['right'], conv['left'], conv['right'])
    return model, mesh_loss, testing.seeded_image(B, 7).cuda(), lab


HEADS = ('encoder.hms_decoder.final_layer.weight', 'encoder.dp_decoder.final_layer.weight')


def test_aux_term_reaches_the_last_convolution_of_each_head_and_trainstep_replays_it():
    """B = 2.  One eager forward, calc_loss_GCN_fused(..., aux=FusedAuxLoss()) and backward: finite non-zero gradients on the
    last convolution of the heat-map head and of the mask / dense head, which stay None with aux=None; the aux total equals the
    fp64 mirror's within the bars and is inside the total.  Then one TrainStep with that loss_fn (SGD, lr 0), replayed from its
    graph: the same loss as the eager step -- to 1e-5, the replayed forward being the eager one's kernels on weights the step
    packs ahead of time (the suite holds replayed gradients to 1e-4 of eager ones, test_gpu_model.py)."""
    from renderih_amd import ops
    from renderih_amd.loss import calc_loss_GCN_fused
    from renderih_amd.train import TrainStep
    B = 2
    model, mesh_loss, img, lab = _training_setup(B)
    m1 = model()
    fused, aux = mesh_loss(m1), ah.FusedAuxLoss()
    mesh_args = lambda l: (l['v2d_l'], l['v2d_r'], l['v3d_l'], l['v3d_r'], l['root_rel'])          # noqa: E731
    aux_args = lambda l: dict(mask=l['mask'], dense=l['dense'], joints2d=l['joints2d'], sigma=ah.HEATMAP_SIGMA)  # noqa: E731
    named = dict(m1.named_parameters())

    out = m1(img)
    plain, _ = calc_loss_GCN_fused(fused, None, *out, *mesh_args(lab))
    plain.backward()
    assert all(named[k].grad is None for k in HEADS), 'without the aux term the heads get no gradient'
    assert out[3]['mask'].is_contiguous() and out[3]['dense'].is_contiguous() and out[3]['hms'].is_contiguous()

    m1.zero_grad(set_to_none=True)
    out = m1(img)
    total, mano, aux_lost = calc_loss_GCN_fused(fused, None, *out, *mesh_args(lab), aux=aux, **aux_args(lab))
    total.backward()
    for k in HEADS:
        g = named[k].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    heads64 = {k: out[3][k].detach().double() for k in ('mask', 'dense', 'hms')}
    want, want_terms = ah.AuxLoss()(heads64, lab['mask'].double(), lab['dense'].double(), joints2d=lab['joints2d'].double(),
                                    sigma=ah.HEATMAP_SIGMA)
    assert set(aux_lost) == set(cc.TERM_KEYS)
    for k in cc.TERM_KEYS:
        e = cc.rel(aux_lost[k], want_terms[k])
        print('composition %s: %.3e' % (k, e))
        assert e <= cc.BARS['loss'], (k, e)
    plain2 = calc_loss_GCN_fused(fused, None, *out, *mesh_args(lab))[0]
    e = abs(float(total.detach()) - (float(plain2.detach()) + float(want))) / float(total.detach())
    print('composition total: %.3e' % e)
    assert e <= cc.BARS['loss'], e
    eager = total.detach().clone()

    m2 = model()
    fused2 = mesh_loss(m2)
    opt = torch.optim.SGD([p for p in m2.parameters() if p.requires_grad], lr=0.0)

    def loss_fn(o, l):
        return calc_loss_GCN_fused(fused2, None, *o, *mesh_args(l), aux=aux, **aux_args(l))[0]
    try:
        step = TrainStep(m2, opt, loss_fn, (img.clone(), {k: v.clone() for k, v in lab.items()}), process_group=False,
                         stages='auto')
        assert step.use_graph
        for rep in range(3):
            loss = step(img, lab)
            e = cc.rel(loss, eager)
            print('TrainStep call %d against the eager step: %.3e' % (rep, e))
            assert e <= 1e-5, (rep, e)
        named2 = dict(m2.named_parameters())
        for k in HEADS:
            assert named2[k].grad is not None and float(named2[k].grad.abs().max()) > 0
            assert cc.rel(named2[k].grad, named[k].grad) <= 1e-4, k
    finally:
        ops.DROPOUT_SEED_TENSOR = None


def test_hrnet_one_channel_mask_is_refused():
    heads = {'mask': torch.zeros(2, 64, 64, device=dev()), 'dense': torch.zeros(2, 6, 64, 64, device=dev())}
    for loss in (ah.FusedAuxLoss(), ah.AuxLoss()):
        with pytest.raises(ValueError, match='HRNet'):
            loss(heads, torch.zeros(2, 2, 64, 64, device=dev()), torch.zeros(2, 3, 64, 64, device=dev()))
