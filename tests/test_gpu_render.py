"""Two-hand renderer on the MI355X (csrc/rih_render.hip): the camera convention against the network's own projection, the
kernels against the numpy oracle (tests/render_oracle.py) at 256^2 and 512^2, large batches, run-to-run bit identity, exact
mask colours and the drop-in import on the GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import render_cases as rc        # noqa: E402
import render_oracle as ro       # noqa: E402
from renderih_amd import render  # noqa: E402
from test_render import check_orth_projection, check_persp_projection   # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize('S', [256, 512])
def test_camera_convention(S):
    r = render.mano_two_hands_renderer(img_size=S, device=DEV)
    check_orth_projection(r, S, 4, DEV)
    check_orth_projection(r, S, 4, DEV, overlap=True, seed=1)
    check_persp_projection(r, S, 4, DEV)


@pytest.mark.parametrize('S', [256, 512])
@pytest.mark.parametrize('kind', ['orth', 'orth_overlap', 'persp'])
@pytest.mark.parametrize('light', ['phong', 'ambient', 'mask', 'densepose'])
def test_kernels_against_oracle(S, kind, light):
    r = render.mano_two_hands_renderer(img_size=S, device=DEV)
    if kind.startswith('orth'):
        vl, vr, sl, tl, sr, tr = rc.ortho_scene(4, seed=S, overlap=kind == 'orth_overlap')
        cam = (sl, tl, sr, tr)
    else:
        vl, vr, cam = rc.persp_scene(4, S, seed=S)
    res = rc.check_against_oracle(r, 'persp' if kind == 'persp' else 'orth', light, S, vl, vr, cam, DEV)
    assert res['covered'] > 0.05


def test_densepose_on_synthetic_dense_coor():
    from renderih_amd import assets
    r = render.mano_two_hands_renderer(img_size=256, device=DEV)
    assert np.allclose(r.dense_coor.numpy(), assets.synthetic_dense_coor() * 255)
    vl, vr, sl, tl, sr, tr = rc.ortho_scene(4, seed=7, overlap=True)
    res = rc.check_against_oracle(r, 'orth', 'densepose', 256, vl, vr, (sl, tl, sr, tr), DEV)
    img = res['img'][res['p2f'] >= 0]
    assert img.std(0).min() > 0.05            # the dense colours vary over the hands


@pytest.mark.parametrize('B', [64, 257])
def test_large_batch_against_oracle(B):
    r = render.mano_two_hands_renderer(img_size=256, device=DEV)
    vl, vr, sl, tl, sr, tr = rc.ortho_scene(B, seed=B, overlap=True)
    for light in ('phong', 'mask'):
        rc.check_against_oracle(r, 'orth', light, 256, vl, vr, (sl, tl, sr, tr), DEV, images=[0, B // 2 + 1, B - 1])
    vl, vr, K = rc.persp_scene(B, 256, seed=B)
    rc.check_against_oracle(r, 'persp', 'phong', 256, vl, vr, K, DEV, images=[1, B - 2])


def test_bit_identical_across_launches():
    r = render.mano_two_hands_renderer(img_size=256, device=DEV)
    vl, vr, sl, tl, sr, tr = (t(a) for a in rc.ortho_scene(64, seed=3, overlap=True))
    verts = torch.cat([vl, vr], 1)
    cam = render.orthographic_camera(sl, tl)
    outs = []
    for _ in range(2):
        frags = render.rasterize(verts, r._faces, cam, 256)
        rgba = render.shade(frags, verts, r._faces, r._default_colors(), 'point', cam)
        img, alpha = r.render_rgb_orth(sl, tl, sr, tr, vl, vr)
        outs.append([frags.pix_to_face, frags.zbuf, frags.bary, rgba, img, alpha])
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert (outs[0][0] >= 0).float().mean() > 0.05


def test_mask_colours_exact():
    S = 256
    r = render.mano_two_hands_renderer(img_size=S, device=DEV)
    vl, vr, sl, tl, sr, tr = rc.ortho_scene(4, seed=5, overlap=True)
    vr_cam = rc.right_in_left_camera(vr, sl, tl, sr, tr)
    rgb = r.render_mask(scale=t(sl), trans2d=t(tl), v3d_left=t(vl), v3d_right=t(vr_cam)).cpu().numpy()
    p2f = render.rasterize(t(np.concatenate([vl, vr_cam], 1)), r._faces, render.orthographic_camera(t(sl), t(tl)),
                           S).pix_to_face.cpu().numpy()
    f = np.where(p2f >= 0, p2f % 3076, -1)
    bg = np.float32(1) / np.float32(255)
    assert (rgb[f < 0] == bg).all()
    assert (rgb[(f >= 0) & (f < 1538)] == [0, 0, 1]).all()           # left hand: (0, 0, 255) / 255
    assert (rgb[f >= 1538] == [0, 1, 0]).all()                       # right hand: (0, 255, 0) / 255
    assert (f < 0).any() and ((f >= 0) & (f < 1538)).any() and (f >= 1538).any()
    single = r.render_single_mask(scale=t(sl), trans2d=t(tl), v3d=t(vl)).cpu().numpy()
    p2s = render.rasterize(t(vl), r._faces_single, render.orthographic_camera(t(sl), t(tl)), S).pix_to_face.cpu().numpy()
    assert (single[p2s >= 0] == 1).all() and (single[p2s < 0] == bg).all() and (p2s >= 0).any()


def test_drop_in_on_gpu():
    import utils.vis_utils as v
    r = v.mano_two_hands_renderer(img_size=256, device=DEV)
    vl, vr, sl, tl, sr, tr = (t(a) for a in rc.ortho_scene(3, seed=9))
    img, mask = r.render_rgb_orth(sl, tl, sr, tr, vl, vr)
    assert img.shape == (3, 256, 256, 3) and mask.shape == (3, 256, 256)
    assert img.dtype == torch.float32 and mask.dtype == torch.float32 and img.is_cuda and mask.is_cuda
    assert img.grad_fn is None and 0.05 < mask.mean().item() < 0.9
