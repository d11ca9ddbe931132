"""The demo's image-to-overlay path (renderih_amd/demo.py, csrc/rih_demo.hip) on the CPU: the REAL kernels, compiled for the
host (tests/hipcpu), against the numpy oracle of tests/demo_cases.py and the fixtures made by the reference's own
process_img / render / render_other_view (tests/golden/make_demo_golden.py).  tests/test_gpu_demo.py re-runs every check_* on
the device.  The full network (input 256) is too slow on the host build of the kernels: that end-to-end test is in the GPU
file; here the end-to-end checks run a small stand-in network through the same class, with the real renderer."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

import demo_cases as dc                  # noqa: E402
from renderih_amd import assets, demo, testing    # noqa: E402

DEV = 'cpu'


@pytest.fixture(autouse=True)
def _host_kernels():
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        yield


# ---------------------------------------------------------------------------------------------------------------- tables

TABLE_L = list(range(1, 70)) + [255, 257, 300, 480, 511, 513, 640, 1000]
TABLE_S = [1, 2, 3, 7, 16, 31, 32, 256]


def test_tables_match_the_contract_and_keep_white_white():
    rs = np.random.RandomState(0)
    worst = 0.0
    for L in TABLE_L:
        for S in TABLE_S:
            tab = dc.axis_taps(L, S)
            assert np.array_equal(demo.axis_table(L, S), tab.astype(np.int32)), (L, S)
            assert (tab[:, 2] + tab[:, 3] == 2048).all() and (tab[:, :2] >= 0).all() and (tab[:, :2] < L).all()
            if (L, S) in ((L, L), (2 * S, S)):
                continue                      # copy / box take no table
            white = dc.resize_u8(np.full((L, 3, 3), 255, np.uint8), S, 2)
            assert (white == 255).all(), (L, S)
            col = rs.randint(0, 256, (L, 1, 3)).astype(np.uint8)
            got = dc.resize_u8(np.repeat(col, 3, 1), S, 2)[:, 0].astype(np.float64)
            f = np.clip((np.arange(S) + 0.5) * (L / S) - 0.5, 0, L - 1)
            lo = np.floor(f).astype(int)
            hi = np.minimum(lo + 1, L - 1)
            want = col[lo, 0] * (1 - (f - lo))[:, None] + col[hi, 0] * (f - lo)[:, None]
            worst = max(worst, np.abs(got - want).max())
    assert worst <= 0.80, worst               # the integer pipeline against fp64 bilinear, in grey levels


# --------------------------------------------------------------------------------------------------- resize and prepare

def check_prepare_shape(H, W, S, dev):
    dc.check_prepare([dc.image(H, W)], S, dev)


def check_ragged(dev):
    imgs = [dc.image(H, W) for (H, W) in dc.SHAPES16]
    a = dc.check_prepare(imgs, 16, dev)
    order = [4, 0, 8, 2, 7, 1, 6, 3, 5]
    b = dc.check_prepare([imgs[i] for i in order], 16, dev)
    for x, y in zip(a, b):
        assert torch.equal(x[order], y)


def check_white(dev):
    imgs = [np.full((H, W, 3), 255, np.uint8) for (H, W) in dc.SHAPES16 + [(40, 27)]]
    for size in (16, (12, 20)):
        assert (dc.check_resize(imgs, size, dev) == 255).all()
    u8 = demo.prepare([imgs[2], imgs[3]], 16, dev, norm=False, u8=True)[2]           # square sources have no border
    assert (u8 == 255).all()


def check_resize_public(dev):
    imgs = [dc.image(H, W, 5) for (H, W) in dc.SHAPES16]
    dc.check_resize(imgs, 16, dev)
    dc.check_resize(imgs, (20, 9), dev)                    # (width, height): anisotropic
    dc.check_resize([dc.image(32, 24)], (12, 16), dev)     # the box on both axes of a non-square image
    one = demo.resize_bgr(dc.image(9, 20), 16, dev)
    assert one.shape == (16, 16, 3) and one.dtype == torch.uint8
    stacked = np.stack([dc.image(11, 13, s) for s in range(3)])
    got = demo.resize_bgr(dc.t(stacked, dev), 7)           # one [B, H, W, 3] tensor, the device taken from it
    dc.eq(got[2], dc.resize_u8(stacked[2], 7, 7), 'stacked')


def check_process_img_fixtures(dev):
    g = dc.load_golden('process_img')
    cases = ['%dx%d' % s for s in dc.SHAPES16]
    assert sorted(g) == sorted(cases)
    ir = demo.InterRender(input_size=16, render_size=16, model=torch.nn.Identity(), renderer=object(), device=dev)
    for c in cases:
        assert '%dx%d' % g[c]['img'].shape[:2] == c
        dc.eq(ir.process_img(g[c]['img']), g[c]['out'], 'process_img fixture ' + c)
    batch = ir.process_imgs([g[c]['img'] for c in cases])
    dc.eq(batch, np.concatenate([g[c]['out'] for c in cases]), 'process_imgs fixtures')


@pytest.mark.parametrize('H,W', dc.SHAPES16)
def test_prepare_each_shape(H, W):
    check_prepare_shape(H, W, 16, DEV)


def test_prepare_300x200_to_256():
    check_prepare_shape(*dc.BIG[0], dc.BIG[1], DEV)


def test_prepare_ragged_batch_in_two_orders():
    check_ragged(DEV)


def test_white_stays_white():
    check_white(DEV)


def test_resize_bgr():
    check_resize_public(DEV)


def test_process_img_against_the_reference_fixtures():
    check_process_img_fixtures(DEV)


# -------------------------------------------------------------------------------------------------------------- compose

COMPOSE = {
    'exact_masks': dict(B=1, R=16, masks=(0.0, 1.0), bgs=[(20, 12)]),
    'fractional': dict(B=1, R=16, masks=(0.25, 1.0 / 3.0, 0.7), bgs=[(16, 16)]),
    'white': dict(B=2, R=16, masks=(0.0, 1.0, 0.25, 1.0 / 3.0, 0.7), bgs=None),
    'anisotropic': dict(B=1, R=16, masks=(0.0, 1.0, 0.25, 1.0 / 3.0, 0.7), bgs=[(20, 12)]),
    'box': dict(B=1, R=16, masks=(0.0, 1.0, 0.25, 1.0 / 3.0, 0.7), bgs=[(32, 32)]),
    'three': dict(B=3, R=24, masks=(0.0, 1.0, 0.25, 1.0 / 3.0, 0.7), bgs=[(20, 12), (48, 48), (24, 24)]),
}


def check_compose_case(name, dev):
    c = COMPOSE[name]
    rgb, mask = dc.render_like(c['B'], c['R'], len(name), c['masks'])
    bgs = None if c['bgs'] is None else [dc.image(H, W, 9) for (H, W) in c['bgs']]
    a = dc.check_compose(rgb, mask, bgs, dev)
    b = dc.check_compose(rgb, mask, bgs, dev, strided=True)
    assert torch.equal(a, b)


def check_compose_saturates(dev):
    rgb, mask = dc.render_like(1, 16, 5)
    rgb[0, 0, :4] = [[2.0, -1.0, 1.5], [1.0, 1.0, 1.0], [-0.5, 0.0, 300.0], [np.nan, 1.0, 0.0]]
    mask[0, 0, :4] = 1.0
    mask[0, 1, :2] = [1.5, -0.5]
    got = dc.check_compose(rgb, mask, None, dev).cpu().numpy()
    assert got[0, 0, 0].tolist() == [255, 0, 255] and got[0, 0, 2].tolist() == [0, 0, 255] and got[0, 0, 3].tolist() == [0, 255, 0]


def check_render_fixtures(dev):
    g = dc.load_golden('render')
    assert sorted(g) == ['aniso', 'box', 'up', 'white']
    for name, c in g.items():
        bg = c.get('bg')
        got = demo.compose(dc.t(c['rgb'], dev), dc.t(c['mask'], dev), None if bg is None else [bg])
        dc.eq(got[0], c['out'], 'render fixture ' + name)


@pytest.mark.parametrize('name', sorted(COMPOSE))
def test_compose(name):
    check_compose_case(name, DEV)


def test_compose_saturates():
    check_compose_saturates(DEV)


def test_render_against_the_reference_fixtures():
    check_render_fixtures(DEV)


# ------------------------------------------------------------------------------------------------ other view, smoother

class Recorded:
    """A renderer that returns recorded arrays and records what it is handed."""

    def __init__(self, rgb, mask, dev):
        self.rgb, self.mask, self.calls = dc.t(rgb, dev), dc.t(mask, dev), []

    def render_rgb_orth(self, **kw):
        self.calls.append(kw)
        return self.rgb, self.mask


def check_other_view_fixtures(dev):
    g = dc.load_golden('other_view')
    assert len(g) == 3
    for name, c in g.items():
        rec = Recorded(c['rgb'], c['mask'], dev)
        ir = demo.InterRender(input_size=16, render_size=16, model=torch.nn.Identity(), renderer=rec, device=dev)
        vl, vr = c['vl'], c['vr']
        got = ir.render_other_view({'v3d_left': dc.t(vl, dev), 'v3d_right': dc.t(vr, dev)}, theta=int(c['theta']))
        assert isinstance(got, np.ndarray)
        dc.eq(got, c['out'], 'other view fixture ' + name)
        call = rec.calls[0]
        for k in ('scale_left', 'scale_right', 'trans2d_left', 'trans2d_right'):
            dc.eq(call[k], c[k], k)
        verts = torch.cat([call['v3d_left'], call['v3d_right']], 1).cpu().numpy()
        atol = 1e-5 * max(np.abs(vl).max(), np.abs(vr).max())
        assert np.abs(verts.astype(np.float64) - c['verts']).max() <= atol


@pytest.mark.parametrize('B,V,theta', [(1, 778, 60), (3, 778, 0), (3, 5, 60), (1, 5, 0)])
def test_other_view(B, V, theta):
    dc.check_other_view(B, V, theta, DEV)


def test_other_view_against_the_reference_fixtures():
    check_other_view_fixtures(DEV)


def test_smoother():
    dc.check_smoother(DEV)
    dc.check_smoother(DEV, strided=True)
    dc.check_smoother(DEV, demo.ParamSmootherMirror)


def test_smoother_refuses_changed_shapes():
    sm = demo.ParamSmoother()
    sm({'a': torch.zeros(3)})
    with pytest.raises(ValueError, match='reset'):
        sm({'a': torch.zeros(4)})


# ----------------------------------------------------------------------------------------------------------- end to end

class TinyNet(torch.nn.Module):
    """A stand-in network with the model's return contract: two template hands moved by the image's channel means."""

    def __init__(self):
        super().__init__()
        self.register_buffer('left', torch.from_numpy(assets.obj_template('left')))
        self.register_buffer('right', torch.from_numpy(assets.obj_template('right')))

    def forward(self, img):
        m = img.mean((2, 3))                                            # [B, 3]
        B = img.shape[0]
        left = self.left[None] + 0.01 * m[:, None, :] + torch.tensor([-0.05, 0., 0.], device=img.device)
        right = self.right[None] - 0.01 * m[:, None, :] + torch.tensor([0.05, 0., 0.], device=img.device)
        scale = {'left': 3 + 0.1 * m[:, 0], 'right': 3 - 0.1 * m[:, 1]}
        trans = {'left': 0.05 * m[:, :2], 'right': -0.05 * m[:, 1:]}
        return {'verts3d': {'left': left, 'right': right}}, {'scale': scale, 'trans2d': trans}, [], {'B': B}


def two_hand_renderer(R, dev):
    from renderih_amd.render import mano_two_hands_renderer
    return mano_two_hands_renderer(mano_path={'left': None, 'right': None}, img_size=R, device=dev)   # the packaged faces


KEYS = ('v3d_left', 'v3d_right', 'scale_left', 'scale_right', 'trans2d_left', 'trans2d_right')


def check_end_to_end(ir, imgs, dev, exact_batch=True):
    """run_model on the oracle-prepared tensor, render against the oracle blend of the renderer's own output, the batched
    forms against the single ones (bit for bit; the network's own outputs at the fp32 parity bar when `exact_batch` is off)."""
    S, singles = ir.input_size, []
    for im in imgs:
        params = ir.run_model(im)
        x = dc.t(dc.prepare_oracle(im, S)[0][None], dev)
        with torch.no_grad():
            result, pd, _, other = ir.model(x)
        assert torch.equal(params['v3d_left'], result['verts3d']['left'])
        assert torch.equal(params['v3d_right'], result['verts3d']['right'])
        assert torch.equal(params['scale_left'], pd['scale']['left']) and torch.equal(params['trans2d_right'], pd['trans2d']['right'])
        assert isinstance(params['otherInfo'], dict)
        kw = {k: v for k, v in params.items() if k != 'otherInfo'}
        rgb, mask = ir.renderer.render_rgb_orth(**kw)
        for bg in (im, None):
            got = ir.render(params, bg_img=bg)
            assert isinstance(got, np.ndarray)
            dc.eq(got, dc.compose_oracle(rgb[0].cpu().numpy(), mask[0].cpu().numpy(), bg), 'render')
        side = ir.render_other_view(params, theta=60)
        assert side.shape == (ir.render_size, ir.render_size, 3) and side.dtype == np.uint8
        singles.append((params, ir.render(params, bg_img=im), side))
    batch = ir.run_model_batch(imgs)
    for b, (params, _, _) in enumerate(singles):
        for k in KEYS:
            if exact_batch:
                assert torch.equal(batch[k][b:b + 1], params[k]), k
            else:
                testing.assert_close(batch[k][b:b + 1], params[k], what=k)
    if not exact_batch:      # a network whose kernels are chosen by the batch size: the glue is compared on the same parameters
        batch = {k: torch.cat([s[0][k] for s in singles]) for k in KEYS}
    over = ir.render_batch(batch, bg_imgs=imgs)
    side = ir.render_other_view_batch(batch, theta=60)
    assert over.dtype == torch.uint8 and over.device.type == torch.device(dev).type
    for b, (params, one, one_side) in enumerate(singles):
        dc.eq(over[b], one, 'batched render %d' % b)
        dc.eq(side[b], one_side, 'batched other view %d' % b)
    # the smoother on the network's own outputs (the decoder's scale_* / trans2d_* are strided views): a still sequence stays put
    params = ir.run_model_batch(imgs)
    sm, mirror = demo.ParamSmoother(), demo.ParamSmootherMirror()
    for _ in range(5):
        got, want = sm(params), mirror(params)
        assert got['otherInfo'] is params['otherInfo']
        for k in KEYS:
            atol = 1e-6 * float(params[k].abs().max())
            assert got[k].shape == params[k].shape
            assert float((got[k] - params[k]).abs().max()) <= atol and float((got[k] - want[k]).abs().max()) <= atol, k
    return singles


def check_refusals(dev):
    ir = demo.InterRender(input_size=16, render_size=16, model=TinyNet(), renderer=object(), device=dev)
    with pytest.raises(ValueError, match='uint8'):
        ir.process_img(np.zeros((4, 4, 3), np.float32))
    with pytest.raises(ValueError, match='uint8'):
        ir.process_imgs([torch.zeros((4, 4, 3), dtype=torch.int32)])
    with pytest.raises(ValueError, match='H x W x 3'):
        ir.process_imgs([np.zeros((4, 4, 4), np.uint8)])
    with pytest.raises(ValueError, match='H x W x 3'):
        ir.process_img(np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match='empty'):
        ir.process_imgs([np.zeros((0, 4, 3), np.uint8)])
    with pytest.raises(ValueError, match='empty'):
        ir.process_imgs([])
    with pytest.raises(ValueError, match='32767'):
        ir.process_imgs([np.zeros((1, 32768, 3), np.uint8)])
    with pytest.raises(ValueError, match='backgrounds'):
        demo.compose(torch.zeros((2, 4, 4, 3), device=dev), torch.zeros((2, 4, 4), device=dev), [np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(ValueError, match='use_fp16_backbone'):
        demo.InterRender(input_size=16, render_size=16, model=TinyNet(), renderer=object(), device=dev, fp16=True)
    with pytest.raises(ValueError, match='destination size'):
        demo.resize_bgr(np.zeros((4, 4, 3), np.uint8), 0, dev)


def test_end_to_end_with_a_stand_in_network():
    ir = demo.InterRender(input_size=16, render_size=32, model=TinyNet(), renderer=two_hand_renderer(32, DEV), device=DEV)
    singles = check_end_to_end(ir, [dc.image(40, 28), dc.image(21, 33, 1)], DEV)
    assert any((s[1] != 255).any() for s in singles)                  # something was drawn


def test_refusals():
    check_refusals(DEV)


def test_save_obj(tmp_path):
    p = str(tmp_path / 'm.obj')
    demo.InterRender.save_obj(p, np.array([[0., 1., 2.], [3., 4., 5.], [6., 7., 8.]]), np.array([[0, 1, 2]]), color=(1, 0, 0))
    assert open(p).read() == 'v 0.0 1.0 2.0 1 0 0\nv 3.0 4.0 5.0 1 0 0\nv 6.0 7.0 8.0 1 0 0\nf 1 2 3\n'
