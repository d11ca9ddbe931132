"""The demo's image-to-overlay path on the MI355X (csrc/rih_demo.hip, renderih_amd/demo.py): the checks of tests/test_demo.py
on the device -- bit-equal against the numpy oracle and the reference's fixtures -- and what only the device shows: a
480 x 640 frame, render size 512, a non-default stream, a captured graph replayed on new pixels, the real network in fp32 and
through the fp16 backbone."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import demo_cases as dc                  # noqa: E402
import test_demo as cpu                  # noqa: E402
from renderih_amd import demo, testing   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('H,W', dc.SHAPES16)
def test_prepare_each_shape(H, W):
    cpu.check_prepare_shape(H, W, 16, DEV)


def test_prepare_300x200_to_256():
    cpu.check_prepare_shape(*dc.BIG[0], dc.BIG[1], DEV)


def test_prepare_480x640_frame():
    cpu.check_prepare_shape(480, 640, 256, DEV)


def test_prepare_ragged_batch_in_two_orders():
    cpu.check_ragged(DEV)


def test_white_stays_white():
    cpu.check_white(DEV)


def test_resize_bgr():
    cpu.check_resize_public(DEV)


def test_process_img_against_the_reference_fixtures():
    cpu.check_process_img_fixtures(DEV)


@pytest.mark.parametrize('name', sorted(cpu.COMPOSE))
def test_compose(name):
    cpu.check_compose_case(name, DEV)


def test_compose_saturates():
    cpu.check_compose_saturates(DEV)


def test_compose_at_512_with_a_frame_behind():
    rgb, mask = dc.render_like(1, 512, 3)
    dc.check_compose(rgb, mask, [dc.image(480, 640)], DEV, strided=True)


def test_render_against_the_reference_fixtures():
    cpu.check_render_fixtures(DEV)


@pytest.mark.parametrize('B,V,theta', [(1, 778, 60), (3, 778, 0), (3, 5, 60), (1, 5, 0)])
def test_other_view(B, V, theta):
    dc.check_other_view(B, V, theta, DEV)


def test_other_view_against_the_reference_fixtures():
    cpu.check_other_view_fixtures(DEV)


def test_smoother():
    dc.check_smoother(DEV)
    dc.check_smoother(DEV, strided=True)
    dc.check_smoother(DEV, demo.ParamSmootherMirror)


def test_refusals():
    cpu.check_refusals(DEV)
    with pytest.raises(RuntimeError, match='GPU tensors'):
        demo.compose(torch.zeros((1, 4, 4, 3)), torch.zeros((1, 4, 4)))


def test_end_to_end_with_a_stand_in_network_at_512():
    ir = demo.InterRender(input_size=16, render_size=512, model=cpu.TinyNet(), renderer=cpu.two_hand_renderer(512, DEV),
                          device=DEV)
    singles = cpu.check_end_to_end(ir, [dc.image(40, 28), dc.image(21, 33, 1)], DEV)
    assert all((s[1] != 255).any() for s in singles)


def test_non_default_stream():
    imgs = [dc.image(23, 10), dc.image(33, 33)]
    rgb, mask = dc.render_like(2, 16, 8)
    want = demo.prepare(imgs, 16, DEV, h8=True, u8=True) + (demo.compose(dc.t(rgb, DEV), dc.t(mask, DEV), imgs),)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = demo.prepare(imgs, 16, DEV, h8=True, u8=True) + (demo.compose(dc.t(rgb, DEV), dc.t(mask, DEV), imgs),)
    stream.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_captured_graph_replays_on_new_pixels():
    """process_imgs -> render_batch in one graph.  The renderer returns device-resident arrays (the mesh renderer uploads its
    vertex colours from the host on every call, which a capture cannot hold); everything of this path is captured."""
    R, S = 32, 16
    rgb, mask = dc.render_like(2, R, 21)
    ir = demo.InterRender(input_size=S, render_size=R, model=torch.nn.Identity(), renderer=cpu.Recorded(rgb, mask, DEV), device=DEV)
    first = [dc.image(23, 10), dc.image(40, 28)]
    static = [dc.t(im, DEV) for im in first]
    ir.process_imgs(static), ir.render_batch({k: None for k in cpu.KEYS}, bg_imgs=static)     # warm-up: the plans are cached
    plans = len(demo._PLANS)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        x = ir.process_imgs(static)
        over = ir.render_batch({k: None for k in cpu.KEYS}, bg_imgs=static)
    assert len(demo._PLANS) == plans                                     # nothing was built or uploaded inside the capture
    for imgs in ([dc.image(23, 10, 3), dc.image(40, 28, 4)], first):
        for s, im in zip(static, imgs):
            s.copy_(dc.t(im, DEV))
        graph.replay()
        torch.cuda.synchronize()
        for b, im in enumerate(imgs):
            dc.eq(x[b], dc.prepare_oracle(im, S)[0], 'replayed prepare %d' % b)
            dc.eq(over[b], dc.compose_oracle(rgb[b], mask[b], im), 'replayed overlay %d' % b)


def _network():
    from renderih_amd.model import build_model
    m = build_model(dropout=0.0)
    m.load_state_dict(testing.deterministic_state(m.state_dict(), seed=1))
    return m


def test_end_to_end_with_the_network():
    """input 256 (the network's size), render size 32, a 40 x 28 image and a second one for the batched forms."""
    ir = demo.InterRender(input_size=256, render_size=32, model=_network(), renderer=cpu.two_hand_renderer(32, DEV), device=DEV)
    cpu.check_end_to_end(ir, [dc.image(40, 28), dc.image(21, 33, 1)], DEV, exact_batch=False)


def test_fp16_backbone_once():
    """fp16=True: HalfBackbone fed by the NHWC8 output, against the fp32 path at the bar tests/test_half.py::backbone_vs_fp32
    sets for that backbone through the decoder (relative error 1e-2 on the vertices)."""
    net, img = _network(), dc.image(40, 28)
    renderer = cpu.two_hand_renderer(32, DEV)
    ref = demo.InterRender(input_size=256, render_size=32, model=net, renderer=renderer, device=DEV).run_model(img)
    with pytest.raises(ValueError, match='use_fp16_backbone'):          # an injected network is not switched behind its owner
        demo.InterRender(input_size=256, render_size=32, model=net, renderer=renderer, device=DEV, fp16=True)
    assert net._half is None
    net.use_fp16_backbone()                                             # from here on every holder of `net` runs fp16
    half = demo.InterRender(input_size=256, render_size=32, model=net, renderer=renderer, device=DEV, fp16=True)
    x = half.process_imgs([img])
    assert x.dtype == torch.float16 and tuple(x.shape) == (1, 256, 256, 8)
    dc.eq(x[0], dc.prepare_oracle(img, 256)[1], 'fp16 nhwc8 input')
    got = half.run_model(img)
    for k in ('v3d_left', 'v3d_right'):
        assert testing.rel_err(got[k], ref[k]) < 1e-2, (k, testing.rel_err(got[k], ref[k]))
    assert half.render(got, bg_img=img).shape == (32, 32, 3)
