"""Two-hand renderer (csrc/rih_render.hip, renderih_amd/render.py; reference utils/vis_utils.py on pytorch3d 0.7.2), on the
CPU: the numpy oracle (tests/render_oracle.py) against closed forms, the camera convention against the network's own
projection, the real kernels through the host-compiled library against the oracle, the drop-in import paths, refusals."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import render_cases as rc        # noqa: E402
import render_oracle as ro       # noqa: E402
from renderih_amd import render  # noqa: E402

REFERENCE = '/root/reference'


def identity_ortho():
    p = np.zeros((1, 16), np.float32)
    p[0, 0] = p[0, 4] = p[0, 8] = p[0, 12] = p[0, 13] = 1
    return p


# ------------------------------------------------------------------------------------------------- 1. oracle vs closed forms

def test_oracle_square_covers_predicted_pixels():
    S = 16
    x0, x1, y0, y1 = -0.5, 0.5, -0.25, 0.75       # pixel edges: no centre lies on the boundary
    v = np.array([[[x0, y0, 1], [x1, y0, 1], [x1, y1, 1], [x0, y1, 1]]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3]])
    o = ro.rasterize(v, f, identity_ortho(), False, S)
    ax = ro.pixel_centres(S)
    want = ((ax >= y0) & (ax <= y1))[:, None] & ((ax >= x0) & (ax <= x1))[None, :]
    assert want.sum() == 64
    assert ((o['pix_to_face'][0] >= 0) == want).all()
    # +X left, +Y up: the square's left edge in NDC (x = 0.5) is the image's column 4, its top (y = 0.75) row 2
    assert np.argwhere(want)[0].tolist() == [2, 4]


def test_oracle_depth_order_and_ties():
    S = 8
    tri = np.array([[-0.9, -0.9], [0.9, -0.9], [0.0, 0.9]], np.float32)
    for z_a, z_b, winner in ((2.0, 1.0, 1), (1.0, 2.0, 0), (1.5, 1.5, 0)):
        v = np.concatenate([np.c_[tri, np.full(3, z_a)], np.c_[tri, np.full(3, z_b)]])[None].astype(np.float32)
        o = ro.rasterize(v, np.array([[0, 1, 2], [3, 4, 5]]), identity_ortho(), False, S)
        hit = o['pix_to_face'][0] >= 0
        assert hit.sum() > 10
        assert (o['pix_to_face'][0][hit] == winner).all()
        assert np.allclose(o['zbuf'][0][hit], min(z_a, z_b))


def test_oracle_phong_flat_quad_closed_form():
    S = 16
    params = ro.orthographic_params([0.6], [[0.0, 0.0]])        # camera at (0, 0, -10), looking along +z
    # a quad in the plane z = 0 whose normal points at the light (0, 0, -1)
    v = np.array([[[-0.9, -0.9, 0], [0.9, -0.9, 0], [0.9, 0.9, 0], [-0.9, 0.9, 0]]], np.float32)
    f = np.array([[0, 2, 1], [0, 3, 2]])
    assert np.allclose(ro.vertex_normals(v, f)[0], [0, 0, -1])
    tex = np.array([0.2, 0.4, 0.6], np.float32)
    o = ro.rasterize(v, f, params, False, S)
    rgba = ro.shade(o, v, f, tex, params, ambient=False)
    hit = o['pix_to_face'][0] >= 0
    assert hit.all()
    P = np.einsum('hwk,hwkc->hwc', o['bary'][0].astype(np.float64), v[0][f[o['pix_to_face'][0]]].astype(np.float64))
    n = np.array([0, 0, -1.0])
    L = np.array([0, 0, -1.0]) - P
    L /= np.linalg.norm(L, axis=-1, keepdims=True)
    Vd = np.array([0, 0, -10.0]) - P
    Vd /= np.linalg.norm(Vd, axis=-1, keepdims=True)
    cosl = L @ n
    r = -L + 2 * cosl[..., None] * n
    spec = 0.2 * np.maximum((Vd * r).sum(-1), 0) ** 64
    want = (0.5 + 0.3 * np.maximum(cosl, 0))[..., None] * tex + spec[..., None]
    assert np.abs(rgba[0, ..., :3] - want).max() < 1e-6
    assert (rgba[0, ..., 3] == 1).all()


def test_oracle_ambient_is_vertex_colour():
    v = np.array([[[-0.9, -0.9, 1], [0.9, -0.9, 1], [0.0, 0.9, 1]]], np.float32)
    o = ro.rasterize(v, np.array([[0, 1, 2]]), identity_ortho(), False, 8)
    rgba = ro.shade(o, v, np.array([[0, 1, 2]]), np.array([10.0, 20.0, 30.0], np.float32), identity_ortho(), ambient=True)
    hit = o['pix_to_face'][0] >= 0
    assert np.allclose(rgba[0][hit, :3], [10, 20, 30], rtol=1e-6)
    assert (rgba[0][~hit] == [1, 1, 1, 0]).all()


# ------------------------------------------------------------------------------- real kernels through the host-built library

@pytest.fixture
def host():
    from hipcpu.host_kernels import host_kernels_abi
    with host_kernels_abi():
        yield


def capture_fragments(monkeypatch):
    seen = []
    real = render._raster

    def spy(*a, **k):
        seen.append(real(*a, **k))
        return seen[-1]
    monkeypatch.setattr(render, '_raster', spy)
    return seen


def check_orth_projection(renderer, S, B, dev, overlap=False, seed=0):
    """render_rgb_orth: every covered pixel's barycentric combination of the reference's own 2-D projection of the vertices
    (ops.projection_batch, each hand with its own scale / trans2d) is the pixel centre (c + 0.5, r + 0.5)."""
    from renderih_amd import ops
    vl, vr, sl, tl, sr, tr = rc.ortho_scene(B, seed, overlap)
    t = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    with pytest.MonkeyPatch.context() as mp:
        seen = capture_fragments(mp)
        img, mask = renderer.render_rgb_orth(t(sl), t(tl), t(sr), t(tr), t(vl), t(vr))
    assert img.shape == (B, S, S, 3) and mask.shape == (B, S, S) and img.dtype == torch.float32
    assert img.grad_fn is None
    frags = seen[-1]
    v2d = torch.cat([ops.projection_batch(t(sl), t(tl), t(vl), S), ops.projection_batch(t(sr), t(tr), t(vr), S)], 1)
    return check_projection(frags, v2d.cpu().numpy().astype(np.float64), S, mask)


def check_projection(frags, v2d, S, mask):
    faces = rc.two_hand_faces()
    p2f, w = frags.pix_to_face.cpu().numpy(), frags.bary.cpu().numpy().astype(np.float64)
    B = p2f.shape[0]
    hit = p2f >= 0
    assert hit.mean() > 0.05
    assert ((mask.cpu().numpy() == 1) == hit).all()
    b, r, c = np.nonzero(hit)
    f = p2f[hit] - b * len(faces)
    uv = (w[hit][..., None] * v2d[b[:, None], faces[f]]).sum(1) / w[hit].sum(1, keepdims=True)
    err = np.abs(uv - np.stack([c + 0.5, r + 0.5], -1)).max()
    assert err < 1e-3, 'covered pixel off its projected position by %g px' % err
    return B


def check_persp_projection(renderer, S, B, dev, seed=0):
    """render_rgb(cameras=K): the perspective-correct interpolated 3-D point, projected with K, is the pixel centre."""
    vl, vr, K = rc.persp_scene(B, S, seed)
    t = lambda a: torch.from_numpy(a).to(dev)     # noqa: E731
    with pytest.MonkeyPatch.context() as mp:
        seen = capture_fragments(mp)
        img, mask = renderer.render_rgb(cameras=t(K), v3d_left=t(vl), v3d_right=t(vr))
    frags = seen[-1]
    faces = rc.two_hand_faces()
    V = np.concatenate([vl, vr], 1).astype(np.float64)
    p2f, w = frags.pix_to_face.cpu().numpy(), frags.bary.cpu().numpy().astype(np.float64)
    hit = p2f >= 0
    assert hit.mean() > 0.05
    assert ((mask.cpu().numpy() == 1) == hit).all()
    b, r, c = np.nonzero(hit)
    f = p2f[hit] - b * len(faces)
    P = (w[hit][..., None] * V[b[:, None], faces[f]]).sum(1)
    Kb = K[b].astype(np.float64)
    u = Kb[:, 0, 0] * P[:, 0] / P[:, 2] + Kb[:, 0, 2]
    v = Kb[:, 1, 1] * P[:, 1] / P[:, 2] + Kb[:, 1, 2]
    err = max(np.abs(u - (c + 0.5)).max(), np.abs(v - (r + 0.5)).max())
    assert err < 1e-3, 'perspective: covered pixel off its projected position by %g px' % err


@pytest.mark.parametrize('S', [32, 48])
def test_camera_convention_on_cpu(host, S):
    r = render.mano_two_hands_renderer(img_size=S, device='cpu')
    check_orth_projection(r, S, 2, 'cpu')
    check_persp_projection(r, S, 2, 'cpu')


@pytest.mark.parametrize('S', [32, 48])
@pytest.mark.parametrize('kind', ['orth', 'persp'])
@pytest.mark.parametrize('light', ['phong', 'ambient', 'mask', 'densepose'])
def test_kernels_against_oracle_on_cpu(host, S, kind, light):
    r = render.mano_two_hands_renderer(img_size=S, device='cpu')
    if kind == 'orth':
        vl, vr, sl, tl, sr, tr = rc.ortho_scene(2, seed=S)
        cam = (sl, tl, sr, tr)
    else:
        vl, vr, cam = rc.persp_scene(2, S, seed=S)
    res = rc.check_against_oracle(r, kind, light, S, vl, vr, cam, 'cpu')
    assert res['covered'] > 0.05


def test_single_mask_on_cpu(host):
    S = 32
    r = render.mano_two_hands_renderer(img_size=S, device='cpu')
    vl, vr, sl, tl, sr, tr = rc.ortho_scene(2)
    rgb = r.render_single_mask(scale=torch.from_numpy(sl), trans2d=torch.from_numpy(tl), v3d=torch.from_numpy(vl)).numpy()
    o = ro.rasterize(vl, rc.two_hand_faces()[:1538], ro.orthographic_params(sl, tl), False, S)
    ok, _ = rc.trusted(o)
    hit = o['pix_to_face'] >= 0
    assert (rgb[hit & ok] == 1).all() and (rgb[~hit & ok] == np.float32(1) / np.float32(255)).all()


# ------------------------------------------------------------------------------------------------------------ 4. drop-in

def test_drop_in_import_paths():
    code = r'''
import sys
sys.path[:0] = [%r] + (%r if len(sys.argv) > 1 else [])
import utils.vis_utils as v, common.vis_utils as cv
import renderih_amd.render as R
assert v.mano_two_hands_renderer is R.mano_two_hands_renderer and cv.mano_two_hands_renderer is R.mano_two_hands_renderer
assert v.Renderer is R.Renderer and v.mano_renderer is R.mano_renderer
r = v.mano_two_hands_renderer(img_size=64)
assert tuple(r.faces.shape) == (1, 3076, 3) and tuple(r.dense_coor.shape) == (778, 3)
assert 'cv2' not in sys.modules and 'yacs' not in sys.modules, 'construction imported cv2 / yacs'
if len(sys.argv) > 1:
    import utils
    assert any(p.startswith(%r) for p in utils.__path__), utils.__path__
    import importlib.util
    spec = importlib.util.find_spec('utils.manoutils')
    assert spec is not None and spec.origin.startswith(%r), spec
print('ok')
''' % (ROOT, [REFERENCE], REFERENCE, REFERENCE)
    env = dict(os.environ)
    env.pop('PYTHONPATH', None)
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, env=env, cwd='/')
    assert out.returncode == 0 and 'ok' in out.stdout, out.stderr
    if os.path.isdir(os.path.join(REFERENCE, 'utils')):     # the reference checkout behind the repository, where present
        out = subprocess.run([sys.executable, '-c', code, 'ref'], capture_output=True, text=True, env=env, cwd='/')
        assert out.returncode == 0 and 'ok' in out.stdout, out.stderr


# ----------------------------------------------------------------------------------------------------------- 5. refusals

def test_refusals():
    with pytest.raises(ValueError, match='square'):
        render.mano_two_hands_renderer(img_size=(256, 192))
    r = render.mano_two_hands_renderer(img_size=32)
    vl, vr, sl, tl, sr, tr = (torch.from_numpy(a) for a in rc.ortho_scene(1))
    with pytest.raises(NotImplementedError, match='UV'):
        r.render_rgb(scale=sl, trans2d=tl, v3d_left=vl, v3d_right=vr, uv_verts=torch.zeros(1, 10, 2),
                     uv_faces=torch.zeros(1, 3076, 3, dtype=torch.long), texture=torch.zeros(1, 8, 8, 3))
    with pytest.raises(NotImplementedError, match='lights'):
        r.render_rgb(scale=sl, trans2d=tl, v3d_left=vl, v3d_right=vr, lights=object())
    with pytest.raises(RuntimeError, match='GPU tensors'):          # CPU tensors outside the host-kernel harness
        r.render_rgb(scale=sl, trans2d=tl, v3d_left=vl, v3d_right=vr)
    with pytest.raises(RuntimeError, match='GPU tensors'):
        render.rasterize(torch.cat([vl, vr], 1), r._faces, render.orthographic_camera(sl, tl), 32)
