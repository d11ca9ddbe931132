"""TEST INFRASTRUCTURE: two-hand scenes for the renderer tests (tests/test_render.py on the CPU through the host-compiled
kernels, tests/test_gpu_render.py on the GPU) and the comparison of the kernels against tests/render_oracle.py."""
import numpy as np
import torch

import render_oracle as ro
from renderih_amd import assets, render

MARGIN = 1e-4      # pixels within this barycentric distance of an edge may flip on the last bit of an edge function
ZGAP = 1e-5        # ... and pixels whose two nearest faces are this close in depth


def hands(B, seed=0, jitter=0.3):
    """MANO templates (the real topology) centred and rotated rigidly per image: v3d_left, v3d_right [B, 778, 3] fp32."""
    rs = np.random.RandomState(seed)
    out = []
    for side in ('left', 'right'):
        vt = assets.obj_template(side)
        vt = vt - vt.mean(0)
        vs = []
        for _ in range(B):
            R = _rodrigues(rs.randn(3) * jitter)
            vs.append(vt @ R.T)
        out.append(np.stack(vs).astype(np.float32))
    return out


def _rodrigues(a):
    t = np.linalg.norm(a) + 1e-12
    k = a / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return (np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K).astype(np.float32)


def ortho_scene(B, seed=0, overlap=False):
    """Hands and per-hand orthographic cameras (scale [B], trans2d [B, 2]) that keep both on screen."""
    rs = np.random.RandomState(100 + seed)
    vl, vr = hands(B, seed)
    sl = (1.8 + 0.4 * rs.rand(B)).astype(np.float32)
    sr = (1.8 + 0.4 * rs.rand(B)).astype(np.float32)
    off = 0.05 if overlap else 0.42
    tl = np.stack([-off + 0.05 * rs.randn(B), 0.1 * rs.randn(B)], -1).astype(np.float32)
    tr = np.stack([off + 0.05 * rs.randn(B), 0.1 * rs.randn(B)], -1).astype(np.float32)
    return vl, vr, sl, tl, sr, tr


def right_in_left_camera(vr, sl, tl, sr, tr):
    """render_rgb_orth's mapping of the right hand into the left hand's camera (vis_utils.py:206-228), in numpy."""
    s = (sr / sl)[:, None, None]
    d = (-(tl - tr) / 2 / sl[:, None])[:, None, :]
    v = s * vr
    v[..., :2] = v[..., :2] + d
    return v.astype(np.float32)


def persp_scene(B, S, seed=0):
    """Hands in front of a pinhole camera (z ~ 0.5 m) and intrinsics K [B, 3, 3] in pixels."""
    rs = np.random.RandomState(200 + seed)
    vl, vr = hands(B, seed)
    vl = vl + np.array([-0.07, 0.0, 0.5], np.float32) + (0.01 * rs.randn(B, 1, 3)).astype(np.float32)
    vr = vr + np.array([0.07, 0.0, 0.55], np.float32) + (0.01 * rs.randn(B, 1, 3)).astype(np.float32)
    K = np.zeros((B, 3, 3), np.float32)
    K[:, 0, 0] = K[:, 1, 1] = S * (1.1 + 0.2 * rs.rand(B))
    K[:, 0, 2] = S / 2 + rs.randn(B) * 2
    K[:, 1, 2] = S / 2 + rs.randn(B) * 2
    K[:, 2, 2] = 1
    return vl.astype(np.float32), vr.astype(np.float32), K


def two_hand_faces():
    right = assets.hand_faces('right')
    return np.concatenate([right[:, [1, 0, 2]], right + 778], 0)


def trusted(o):
    """Pixels on which the kernel must agree with the oracle exactly (and the fraction left out)."""
    ok = (o['margin'] >= MARGIN) & (o['zgap'] >= ZGAP)
    return ok, 1.0 - ok.mean()


def check_against_oracle(renderer, kind, light, S, vl, vr, cam, dev, colors=None, images=None):
    """Render with `renderer` (a mano_two_hands_renderer) on `dev` and compare pix_to_face, alpha and RGB with the oracle.
    kind: 'orth' (cam = (sl, tl, sr, tr), through render_rgb_orth / render_mask / render_densepose on the left camera) or
    'persp' (cam = K).  light: 'phong', 'ambient', 'mask' or 'densepose'.  images: the image indices compared."""
    faces = two_hand_faces()
    B = vl.shape[0]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    if kind == 'orth':
        sl, tl, sr, tr = cam
        vr_cam = right_in_left_camera(vr, sl, tl, sr, tr)
        params = ro.orthographic_params(sl, tl)
        camkw = dict(scale=t(sl), trans2d=t(tl))
        camera = render.orthographic_camera(t(sl), t(tl))
    else:
        vr_cam = vr
        params = ro.perspective_params(cam, S)
        camkw = dict(cameras=t(cam))
        camera = render.perspective_camera(t(cam), S)
    if light == 'phong':
        if kind == 'orth':
            img, alpha = renderer.render_rgb_orth(t(sl), t(tl), t(sr), t(tr), t(vl), t(vr))
        else:
            img, alpha = renderer.render_rgb(v3d_left=t(vl), v3d_right=t(vr), **camkw)
        col = renderer._default_colors().numpy()
    elif light == 'ambient':
        img, alpha = renderer.render_rgb(v3d_left=t(vl), v3d_right=t(vr_cam), amblights=True, **camkw)
        col = renderer._default_colors().numpy()
    elif light == 'mask':
        img = renderer.render_mask(v3d_left=t(vl), v3d_right=t(vr_cam), **camkw)
        alpha = None
        col = np.zeros((1556, 3), np.float32)
        col[:778, 2] = 255
        col[778:, 1] = 255
    else:
        img, alpha = renderer.render_densepose(v3d_left=t(vl), v3d_right=t(vr_cam), **camkw)
        col = np.concatenate([renderer.dense_coor.numpy()] * 2, 0)
    verts = np.concatenate([vl, vr_cam], 1)
    frags = render.rasterize(t(verts), renderer._faces, camera, S)
    p2f = frags.pix_to_face.cpu().numpy()
    img = img.cpu().numpy()
    alpha = None if alpha is None else alpha.cpu().numpy()
    idx = list(range(B)) if images is None else list(images)
    o = ro.rasterize(verts[idx], faces, params[idx], kind == 'persp', S)
    o['pix_to_face'] = np.where(o['pix_to_face'] >= 0, o['pix_to_face'] - np.arange(len(idx))[:, None, None] * len(faces)
                                + np.asarray(idx)[:, None, None] * len(faces), -1)
    ok, excluded = trusted(o)
    assert excluded < 0.005, 'too many ambiguous pixels (%.3f %%)' % (100 * excluded)
    bad = (p2f[idx] != o['pix_to_face']) & ok
    assert not bad.any(), 'pix_to_face differs on %d trusted pixels (first %s)' % (bad.sum(), np.argwhere(bad)[:3].tolist())
    ob = dict(o)
    ob['pix_to_face'] = np.where(o['pix_to_face'] >= 0, o['pix_to_face'] % len(faces)
                                 + np.arange(len(idx))[:, None, None] * len(faces), -1)
    rgba = ro.shade(ob, verts[idx], faces, np.broadcast_to(col, (len(idx), 1556, 3)), params[idx],
                    ambient=light != 'phong')
    want_img = rgba[..., :3] / np.float32(255)
    if alpha is not None:
        assert (alpha[idx] == rgba[..., 3])[ok].all(), 'alpha differs from the oracle'
    err = np.abs(img[idx] - want_img)[ok]
    assert err.size == 0 or err.max() < 1e-5, 'RGB differs from the oracle by %g' % err.max()
    return dict(p2f=p2f, img=img, alpha=alpha, excluded=excluded, covered=(o['pix_to_face'] >= 0).mean())
