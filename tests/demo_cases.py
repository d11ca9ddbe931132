"""Shared cases and the numpy oracle of the demo path (renderih_amd/demo.py, csrc/rih_demo.hip): the contract restated in
int64 / float64 / float32 exactly as it reads, independent of the package's own table builder; the checks that
tests/test_demo.py runs on the host build of the kernels and tests/test_gpu_demo.py on the device."""
import math
import os

import numpy as np
import torch

from renderih_amd import demo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'demo')

# (H, W) of `prepare` / `resize` sources at S = 16: portrait with an odd difference (pads 6 and 7), landscape, copy, box,
# box reading border pixels, just off the box, upscale (both edge clamps), degenerate sides
SHAPES16 = [(23, 10), (9, 20), (16, 16), (32, 32), (32, 31), (33, 33), (7, 5), (1, 1), (1, 40)]
BIG = ((300, 200), 256)


def image(H, W, seed=0):
    return np.random.RandomState(1000 + 7 * H + 13 * W + seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle

def axis_taps(L, S):
    """(s, s', a0, a1) per destination index, one index at a time."""
    out = []
    for d in range(S):
        f = np.float32((np.float64(d) + 0.5) * (np.float64(L) / np.float64(S)) - 0.5)
        s = int(math.floor(float(f)))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= L - 1:
            s, f = L - 1, np.float32(0)
        a1 = int(np.rint(np.float32(f * np.float32(2048))))
        a0 = int(np.rint(np.float32(np.float32(np.float32(1) - f) * np.float32(2048))))
        out.append((s, min(s + 1, L - 1), a0, a1))
    return np.array(out, np.int64)


def resize_u8(P, Sy, Sx):
    """The contract's 8-bit resize of a (padded) uint8 image [PH, PW, 3] to [Sy, Sx, 3]."""
    PH, PW = P.shape[:2]
    P = P.astype(np.int64)
    if (PH, PW) == (Sy, Sx):
        return P.astype(np.uint8)
    if (PH, PW) == (2 * Sy, 2 * Sx):
        return ((P[0::2, 0::2] + P[0::2, 1::2] + P[1::2, 0::2] + P[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    ty, tx = axis_taps(PH, Sy), axis_taps(PW, Sx)
    T = P[:, tx[:, 0]] * tx[:, 2][None, :, None] + P[:, tx[:, 1]] * tx[:, 3][None, :, None]
    v = (((ty[:, 2][:, None, None] * (T[ty[:, 0]] >> 4)) >> 16) + ((ty[:, 3][:, None, None] * (T[ty[:, 1]] >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def pad_square(img):
    H, W = img.shape[:2]
    side, lead = max(H, W), int(abs(H - W) / 2)
    P = np.zeros((side, side, 3), np.uint8)
    if H > W:
        P[:, lead:lead + W] = img
    else:
        P[lead:lead + H] = img
    return P


def prepare_oracle(img, S):
    """(fp32 [3, S, S], fp16 [S, S, 8], uint8 [S, S, 3]) of process_img."""
    u8 = resize_u8(pad_square(img), S, S)
    rgb = u8[..., ::-1].astype(np.float32) / np.float32(255)
    n = (rgb - np.array(demo.MEAN, np.float32)) / np.array(demo.STD, np.float32)
    assert n.dtype == np.float32
    h8 = np.zeros((S, S, 8), np.float16)
    h8[..., :3] = n.astype(np.float16)
    return np.ascontiguousarray(n.transpose(2, 0, 1)), h8, u8


def compose_oracle(rgb, mask, bg=None):
    """InterRender.render lines 89-98 in numpy, saturating where numpy would wrap."""
    R = rgb.shape[0]
    img = rgb.astype(np.float32) * 255
    m = mask.astype(np.float32)[..., np.newaxis]
    back = np.ones_like(img) * 255 if bg is None else resize_u8(bg, R, R)
    v = img * m + back * (1 - m)
    assert v.dtype == np.float32
    with np.errstate(invalid='ignore'):
        v = np.where(v >= 255, np.float32(255), np.where(v > 0, v, np.float32(0)))
    return v.astype(np.uint8)


def other_view_oracle(vl, vr, theta):
    vl, vr = vl.astype(np.float64), vr.astype(np.float64)
    c = (vl.mean(1) + vr.mean(1))[:, None] / 2
    t = 3.14159 / 180 * theta
    R = np.array([[math.cos(t), 0, math.sin(t)], [0, 1, 0], [-math.sin(t), 0, math.cos(t)]], np.float32).astype(np.float64)
    return np.concatenate([(vl - c) @ R, (vr - c) @ R], 1)


def smooth_oracle(frames):
    """apps/demo.py:103-128 with `smooth` on, in float64, `None` for what does not exist yet."""
    last = last_v = v = a = None
    out = []
    for p in frames:
        p = {k: x.astype(np.float64) for k, x in p.items()}
        if last is not None and v is not None and a is not None:
            p = {k: 0.7 * p[k] + 0.3 * (last[k] + v[k] + 0.5 * a[k]) for k in p}
        if last is not None:
            v = {k: p[k] - last[k] for k in p}
        if last_v is not None and v is not None:
            a = {k: v[k] - last_v[k] for k in p}
        last, last_v = p, v
        out.append(p)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# checks (dev: 'cpu' inside host_kernels_abi, or 'cuda')

def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def eq(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype.kind == 'f':
        same = got.view('u%d' % got.dtype.itemsize) == want.view('u%d' % want.dtype.itemsize)
    else:
        same = got == want
    assert same.all(), (what, int((~same).sum()), np.argwhere(~same)[:4].tolist())


def check_prepare(imgs, S, dev, mirror=True):
    """Every output of one launch over `imgs` against the oracle, image by image, bit for bit."""
    n, h, u = demo.prepare(imgs, S, dev, norm=True, h8=True, u8=True)
    for i, im in enumerate(imgs):
        wn, wh, wu = prepare_oracle(im, S)
        tag = 'image %d %s' % (i, im.shape[:2])
        eq(u[i], wu, tag + ' u8')
        eq(n[i], wn, tag + ' fp32')
        eq(h[i], wh, tag + ' fp16 nhwc8')
    if mirror:
        for g, w, what in zip((n, h, u), demo.prepare_mirror(imgs, S, dev), ('fp32', 'fp16 nhwc8', 'u8')):
            eq(g, w.cpu().numpy(), 'mirror ' + what)
    return n, h, u


def check_resize(imgs, size, dev):
    Sy, Sx = demo._size2(size)
    got = demo.resize_bgr(imgs, size, dev)
    for i, im in enumerate(imgs):
        eq(got[i], resize_u8(im, Sy, Sx), 'resize %d %s -> %s' % (i, im.shape[:2], (Sy, Sx)))
    assert torch.equal(got, demo.resize_bgr_mirror(imgs, size, dev))
    return got


def render_like(B, R, seed, masks=(0.0, 1.0, 0.25, 1.0 / 3.0, 0.7)):
    """rgb [B, R, R, 3] in the renderer's units (colour / 255) and a mask cycling through exact and fractional values."""
    rs = np.random.RandomState(seed)
    rgb = (rs.rand(B, R, R, 3) * 255).astype(np.float32) / np.float32(255)
    mask = np.array(masks, np.float32)[rs.randint(0, len(masks), (B, R, R))]
    return rgb, mask


def check_compose(rgb, mask, bgs, dev, strided=False):
    B, R = rgb.shape[:2]
    if strided:              # the renderer's own layout: the mask is channel 3 of an RGBA tensor
        rgba = t(np.concatenate([rgb, mask[..., None]], -1), dev)
        got = demo.compose(rgba[..., :3], rgba[..., 3], bgs)
    else:
        got = demo.compose(t(rgb, dev), t(mask, dev), bgs)
    for b in range(B):
        eq(got[b], compose_oracle(rgb[b], mask[b], None if bgs is None else bgs[b]), 'compose %d' % b)
    assert torch.equal(got, demo.compose_mirror(t(rgb, dev), t(mask, dev), bgs))
    return got


def hands(B, V, seed, offset=0.2):
    rs = np.random.RandomState(seed)
    vl = (rs.randn(B, V, 3) * 0.04 + np.array([-offset, 0.01, 0.6])).astype(np.float32)
    vr = (rs.randn(B, V, 3) * 0.04 + np.array([offset, -0.02, 0.6])).astype(np.float32)
    return vl, vr


def check_other_view(B, V, theta, dev):
    vl, vr = hands(B, V, 3 * B + V)
    got = demo.other_view(t(vl, dev), t(vr, dev), theta)
    want = other_view_oracle(vl, vr, theta)
    atol = 1e-5 * max(np.abs(vl).max(), np.abs(vr).max())
    assert got.shape == (B, 2 * V, 3) and got.dtype == torch.float32
    assert np.abs(got.cpu().numpy().astype(np.float64) - want).max() <= atol
    assert torch.equal(got, demo.other_view(t(vl, dev), t(vr, dev), theta))            # two calls, identical bits
    mir = demo.other_view_mirror(t(vl, dev), t(vr, dev), theta)
    assert np.abs(mir.cpu().numpy().astype(np.float64) - want).max() <= atol
    if theta == 0:           # centred only: the two means cancel
        g = got.cpu().numpy().astype(np.float64)
        assert np.abs(g[:, :V].mean(1) + g[:, V:].mean(1)).max() <= 2 * atol


def smoother_frames(n=5, seed=0):
    rs = np.random.RandomState(seed)
    shapes = {'scale_left': (2,), 'trans2d_left': (2, 2), 'v3d_left': (2, 7, 3), 'v3d_right': (2, 7, 3)}
    base = {k: rs.randn(*s) for k, s in shapes.items()}
    return [{k: (base[k] + 0.1 * i + 0.05 * rs.randn(*s)).astype(np.float32) for k, s in shapes.items()} for i in range(n)]


def check_smoother(dev, cls=None, strided=False):
    """strided: scale_left and trans2d_left are the views temp[:, 0] and temp[:, 1:] of one [B, 3] tensor, as the decoder
    returns them -- not contiguous, so the smoother works on copies that must outlive its launch."""
    frames = smoother_frames()
    want = smooth_oracle(frames)
    sm = (cls or demo.ParamSmoother)()
    marker = {'hms': object()}
    for rnd in range(2):                                # the second round follows reset()
        for i, f in enumerate(frames):
            params = {k: t(x, dev) for k, x in f.items()}
            if strided:
                temp = torch.cat([params['scale_left'][:, None], params['trans2d_left']], 1)
                params['scale_left'], params['trans2d_left'] = temp[:, 0], temp[:, 1:]
                assert not params['scale_left'].is_contiguous() and not params['trans2d_left'].is_contiguous()
                del temp
            params['otherInfo'] = marker
            got = sm(params)
            assert got['otherInfo'] is marker
            for k in f:
                g = got[k].cpu().numpy()
                atol = 1e-6 * max(np.abs(x[k]).max() for x in frames)
                assert g.dtype == np.float32 and np.abs(g.astype(np.float64) - want[i][k]).max() <= atol, (rnd, i, k)
                if i < 3:                                # frames 1-3: nothing to predict from yet, the input passes through
                    assert np.array_equal(g, f[k]), (rnd, i, k)
            if i == 3:
                assert any(not np.array_equal(got[k].cpu().numpy(), f[k]) for k in f)
        sm.reset()


def load_golden(prefix):
    """{case: {key: array}} of the fixture files tests/golden/demo/<prefix>_<case>.npz (one small file per case)."""
    out = {}
    for f in sorted(os.listdir(GOLDEN)):
        if f.startswith(prefix + '_') and f.endswith('.npz'):
            with np.load(os.path.join(GOLDEN, f)) as z:
                out[f[len(prefix) + 1:-4]] = {k: z[k] for k in z.files}
    return out
