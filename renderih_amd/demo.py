"""The demo's image-to-overlay path -- drop-in for the reference's core/test_utils.py:19-128 (`InterRender`, driven by
apps/demo.py), which needs cv2, torchvision.transforms and pytorch3d.  In a RenderIH checkout, core/test_utils.py becomes

    from renderih_amd.demo import InterRender

The reference's glue is a per-image host loop (pad and resize on the CPU, copy, normalise, copy the fp32 render and mask
back, blend in numpy).  Here it is five batched kernels (csrc/rih_demo.hip); images go in as uint8 BGR and overlays come out as
uint8 BGR, and no fp32 image crosses the bus:

    ir = InterRender(cfg_path, model_path, render_size=512)        # or model=..., renderer=... (already built)
    params = ir.run_model(img)                                     # img: H x W x 3 uint8 BGR (numpy or tensor)
    overlay = ir.render(params, bg_img=img)                        # numpy uint8 [R, R, 3]
    side = ir.render_other_view(params, theta=60)
    params = ir.run_model_batch([img0, img1, ...])                 # images of differing sizes, or one [B, H, W, 3]
    overlays = ir.render_batch(params, bg_imgs=[img0, img1, ...])  # uint8 device tensor [B, R, R, 3]

Semantics
  * process_img: pad2squre (utils/manoutils.py:120-135: side max(H, W), leading pad int(diff / 2), black border, which takes
    part in the interpolation), 8-bit bilinear resize, BGR -> RGB, / 255, (x - mean) / std in float32.
  * resize (`resize_bgr`, `axis_table`): copy at equal size; the 2 x 2 box (sum + 2) >> 2 at an exact factor of two on both
    axes; otherwise per axis f = float32((d + 0.5) (L / S) - 0.5) (evaluated in double), s = floor(f), f -= s, clamped to
    [0, L - 1] with f = 0 at either clamp, second tap min(s + 1, L - 1), a1 = rint(2048 f), a0 = rint(2048 (1 - f)) in float32;
    T = P[r, s] a0 + P[r, s'] a1; out = clamp((((b0 (T0 >> 4)) >> 16) + ((b1 (T1 >> 4)) >> 16) + 2) >> 2, 0, 255).
    The tables are built here in numpy and cached per (L, S); the device does integer work only.
  * render: uint8(fl(fl(img 255) mask) + fl(bg fl(1 - mask))), float32 roundings as numpy's, truncation; the background is
    resized to R x R WITHOUT padding (anisotropic, as the reference's cv.resize), white when absent; the renderer's channels are
    blended into the BGR background as they come.  The single difference from numpy: values outside 0 .. 255 (which renderer
    output cannot produce) saturate instead of wrapping.
  * render_other_view: both hands minus the mean of their two vertex means, times the reference's float32 matrix of
    theta 3.14159 / 180, scale 3, no translation, white background.
  * ParamSmoother: apps/demo.py:103-128 -- from the fourth frame on p <- 0.7 p + 0.3 (last + v + 0.5 a); v and a are the first
    and second differences of the filtered parameters; non-tensor entries (`otherInfo`) pass through.

Every kernel has a torch mirror (`*_mirror`, `ParamSmootherMirror`): the same arithmetic in torch ops on whatever device the
tensors are on -- the baseline of tools/demo_bench.py and a second check beside the numpy oracle of tests/demo_cases.py.

Out of scope: cv.VideoCapture, cv.imshow, cv.line, cv.imwrite, JPEG decoding and demo_myintag.py -- decode and display stay with
the caller.

Plans (descriptor rows and tap tables on the device) are cached per set of image shapes, at most 1024 of them; a call with a
cached plan uploads nothing but the pixels, so the kernels of this module can be captured in a graph after one warm-up call on device-resident images (not `render_batch`
over the real mesh renderer, which uploads its vertex colours from the host on every call).  A list of device tensors is packed
with one `torch.cat` per call (a launch and a copy of the pixels); one contiguous [B, H, W, 3] tensor is used in place.

STATUS: the resize restates cv::resize (CV_8U, INTER_LINEAR) from memory of the OpenCV 4 sources; conformity with a real OpenCV
build is NOT verified (no OpenCV to compare with).  Sequence, dtypes and blend order are pinned by fixtures made by the
reference's own process_img / render / render_other_view (tests/golden/make_demo_golden.py).
"""
import ctypes as C
import functools
import math
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .ops import check

MAX_SIDE = 32767
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
DESC = 10               # = RIH_DEMO_DESC
SMOOTH_MAX = 16         # = RIH_DEMO_SMOOTH_MAX
_PLANS = OrderedDict()
_MAX_PLANS = 1024


# ---------------------------------------------------------------------------------------------------------------------------
# host side of the resize

@functools.lru_cache(maxsize=None)
def axis_table(L, S):
    """int32 [S, 4] = (s, s', a0, a1) per destination index of an axis resized from L to S."""
    d = np.arange(S, dtype=np.float64)
    f = ((d + 0.5) * (float(L) / float(S)) - 0.5).astype(np.float32)
    s = np.floor(f)
    f = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    low, high = s < 0, s >= L - 1
    s = np.where(low, 0, np.where(high, L - 1, s))
    f = np.where(low | high, np.float32(0), f).astype(np.float32)
    a1 = np.rint(f * np.float32(2048)).astype(np.int32)
    a0 = np.rint((np.float32(1) - f) * np.float32(2048)).astype(np.int32)
    t = np.stack([s, np.minimum(s + 1, L - 1), a0, a1], 1).astype(np.int32)
    t.setflags(write=False)
    return t


def pad_to_square(H, W):
    """pad2squre: (pad_top, pad_left, side)."""
    if H > W:
        return 0, int((H - W) / 2), H
    return int((W - H) / 2), 0, W


def _check_image(shape, dtype):
    if not (dtype == torch.uint8 if isinstance(dtype, torch.dtype) else np.dtype(dtype) == np.uint8):
        raise ValueError('renderih_amd.demo: images must be uint8 BGR (got %s)' % (dtype,))
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError('renderih_amd.demo: an image must be H x W x 3 (got shape %s)' % (tuple(shape),))
    if shape[0] < 1 or shape[1] < 1:
        raise ValueError('renderih_amd.demo: empty image (shape %s)' % (tuple(shape),))
    if shape[0] > MAX_SIDE or shape[1] > MAX_SIDE:
        raise ValueError('renderih_amd.demo: image sides must not exceed %d (got shape %s)' % (MAX_SIDE, tuple(shape)))


def pack_images(images, device):
    """A list of H x W x 3 uint8 images of differing sizes, or one [B, H, W, 3] array or tensor (host or device) ->
    (flat uint8 tensor on `device`, [(H, W)] * B).  A contiguous device tensor is used in place."""
    if isinstance(images, (np.ndarray, torch.Tensor)):
        if images.ndim == 3:
            images = images[None]
        if images.ndim != 4:
            raise ValueError('renderih_amd.demo: an image must be H x W x 3 (got shape %s)' % (tuple(images.shape),))
        if images.shape[0] < 1:
            raise ValueError('renderih_amd.demo: empty batch')
        _check_image(tuple(images.shape[1:]), images.dtype)
        t = torch.from_numpy(np.ascontiguousarray(images)) if isinstance(images, np.ndarray) else images.contiguous()
        return t.reshape(-1).to(device), [(int(images.shape[1]), int(images.shape[2]))] * int(images.shape[0])
    images = list(images)
    if not images:
        raise ValueError('renderih_amd.demo: empty batch')
    flat, shapes = [], []
    for im in images:
        if not isinstance(im, (np.ndarray, torch.Tensor)):
            raise ValueError('renderih_amd.demo: images must be numpy arrays or tensors (got %s)' % type(im).__name__)
        _check_image(tuple(im.shape), im.dtype)
        shapes.append((int(im.shape[0]), int(im.shape[1])))
        t = torch.from_numpy(np.ascontiguousarray(im)) if isinstance(im, np.ndarray) else im.contiguous()
        flat.append(t.reshape(-1))
    if all(t.device.type == 'cpu' for t in flat):
        return torch.cat(flat).to(device), shapes
    return torch.cat([t.to(device) for t in flat]), shapes


class Plan:
    """Descriptor rows and tap tables of one set of image shapes, on the device."""

    def __init__(self, rows, tabs, device):
        self.rows = rows
        self.desc = torch.from_numpy(np.asarray(rows, np.int64).reshape(-1, DESC)).to(device)
        self.tabs = None if tabs is None else torch.from_numpy(tabs).to(device)
        self.entries = 0 if tabs is None else int(tabs.shape[0])


def plan_for(shapes, Sy, Sx, device, square):
    """The cached Plan of images of `shapes` resized to Sy x Sx, after pad2squre when `square`."""
    key = (str(device), tuple(shapes), Sy, Sx, square)
    plan = _PLANS.get(key)
    if plan is not None:
        _PLANS.move_to_end(key)
        return plan
    rows, parts, where, n, off = [], [], {}, 0, 0

    def table(L, S):
        nonlocal n
        if (L, S) not in where:
            where[(L, S)] = n
            parts.append(axis_table(L, S))
            n += S
        return where[(L, S)]
    for (H, W) in shapes:
        pt, pl, side = pad_to_square(H, W) if square else (0, 0, 0)
        PH, PW = (side, side) if square else (H, W)
        same, box = (PH == Sy and PW == Sx), (PH == 2 * Sy and PW == 2 * Sx)
        rows.append([off, H, W, pt, pl, PH, PW, 0] + ([0, 0] if same or box else [table(PH, Sy), table(PW, Sx)]))
        off += H * W * 3
    plan = Plan(rows, np.concatenate(parts) if parts else None, device)
    _PLANS[key] = plan
    while len(_PLANS) > _MAX_PLANS:
        _PLANS.popitem(last=False)
    return plan


def _size2(size):
    """cv.resize's dsize: an int, or (width, height) -> (Sy, Sx)."""
    Sx, Sy = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    if not (1 <= Sx <= MAX_SIDE and 1 <= Sy <= MAX_SIDE):
        raise ValueError('renderih_amd.demo: destination size must be in [1, %d] (got %r)' % (MAX_SIDE, size))
    return Sy, Sx


def resize_bgr(images, size, device=None):
    """cv.resize(img, size) (8-bit INTER_LINEAR, no padding) for a ragged batch in one launch: uint8 tensor
    [B, Sy, Sx, 3] on the device ([Sy, Sx, 3] for a single H x W x 3 image).  size: an int or (width, height)."""
    single = isinstance(images, (np.ndarray, torch.Tensor)) and images.ndim == 3
    if device is None:           # where the first tensor lies; host arrays go to the GPU
        some = [images] if isinstance(images, (np.ndarray, torch.Tensor)) else list(images)
        device = next((im.device for im in some if isinstance(im, torch.Tensor)), torch.device('cuda'))
    Sy, Sx = _size2(size)
    flat, shapes = pack_images(images, device)
    ops._chk(flat, dtype=torch.uint8)
    plan = plan_for(shapes, Sy, Sx, flat.device, False)
    out = torch.empty((len(shapes), Sy, Sx, 3), device=flat.device, dtype=torch.uint8)
    check(ops._L().rih_demo_resize(flat.data_ptr(), flat.numel(), plan.desc.data_ptr(), ops._p(plan.tabs), plan.entries,
                                   len(shapes), Sy, Sx, out.data_ptr(), ops._stream()), 'rih_demo_resize')
    return out[0] if single else out


def prepare(images, S, device, norm=True, h8=False, u8=False):
    """`process_img` for a batch in one launch: (fp32 [B, 3, S, S] | None, fp16 [B, S, S, 8] | None, uint8 [B, S, S, 3] | None)."""
    if not (norm or h8 or u8):
        raise ValueError('renderih_amd.demo: ask for at least one output')
    flat, shapes = pack_images(images, device)
    ops._chk(flat, dtype=torch.uint8)
    B, dev = len(shapes), flat.device
    plan = plan_for(shapes, S, S, dev, True)
    o_n = torch.empty((B, 3, S, S), device=dev, dtype=torch.float32) if norm else None
    o_h = torch.empty((B, S, S, 8), device=dev, dtype=torch.float16) if h8 else None
    o_u = torch.empty((B, S, S, 3), device=dev, dtype=torch.uint8) if u8 else None
    check(ops._L().rih_demo_prepare(flat.data_ptr(), flat.numel(), plan.desc.data_ptr(), ops._p(plan.tabs), plan.entries, B, S,
                                    ops._p(o_n), ops._p(o_h), ops._p(o_u), ops._stream()), 'rih_demo_prepare')
    return o_n, o_h, o_u


def _pixel_ld(t, tail):
    """(tensor, elements between pixels) of a [B, R, R(, 3)] fp32 tensor whose pixels are evenly spaced, else of its copy."""
    lead = t.shape[:3]
    ld = t.stride(2)
    want = (lead[1] * lead[2] * ld, lead[2] * ld, ld) + ((1,) if tail else ())
    if ld >= max(tail, 1) and all(n == 1 or s == w for n, s, w in zip(t.shape, t.stride(), want)):
        return t, ld
    return t.contiguous(), max(tail, 1)


def compose(rgb, mask, bg_imgs=None):
    """`InterRender.render` lines 89-98 for a batch in one launch: rgb [B, R, R, 3] fp32 in the renderer's 0 .. 1 units, mask
    [B, R, R] fp32, backgrounds a ragged uint8 batch or None (white) -> uint8 [B, R, R, 3]."""
    ops._chk(rgb, mask)
    B, R = rgb.shape[0], rgb.shape[1]
    if rgb.dim() != 4 or tuple(rgb.shape) != (B, R, R, 3) or tuple(mask.shape) != (B, R, R):
        raise ValueError('renderih_amd.demo: compose takes rgb [B, R, R, 3] and mask [B, R, R] (got %s, %s)'
                         % (tuple(rgb.shape), tuple(mask.shape)))
    rgb, rgb_ld = _pixel_ld(rgb.detach(), 3)
    mask, mask_ld = _pixel_ld(mask.detach(), 0)
    flat = plan = None
    if bg_imgs is not None:
        flat, shapes = pack_images(bg_imgs, rgb.device)
        ops._chk(flat, dtype=torch.uint8)
        if len(shapes) != B:
            raise ValueError('renderih_amd.demo: %d backgrounds for %d images' % (len(shapes), B))
        plan = plan_for(shapes, R, R, rgb.device, False)
    out = torch.empty((B, R, R, 3), device=rgb.device, dtype=torch.uint8)
    check(ops._L().rih_demo_compose(rgb.data_ptr(), rgb_ld, mask.data_ptr(), mask_ld, ops._p(flat),
                                    0 if flat is None else flat.numel(), 0 if plan is None else plan.desc.data_ptr(),
                                    0 if plan is None else ops._p(plan.tabs), 0 if plan is None else plan.entries, B, R,
                                    out.data_ptr(), ops._stream()), 'rih_demo_compose')
    return out


def view_matrix(theta):
    """The reference's float32 matrix (core/test_utils.py:107-111), pi = 3.14159 included."""
    t = 3.14159 / 180 * theta
    return np.array([[math.cos(t), 0, math.sin(t)], [0, 1, 0], [-math.sin(t), 0, math.cos(t)]], dtype=np.float32)


def other_view(v3d_left, v3d_right, theta=60):
    """render_other_view lines 103-114 in one launch: [B, 2 V, 3] = cat(left - c, right - c) R."""
    ops._chk(v3d_left, v3d_right)
    if v3d_left.dim() != 3 or v3d_left.shape[2] != 3 or v3d_left.shape != v3d_right.shape or v3d_left.shape[1] < 1:
        raise ValueError('renderih_amd.demo: other_view takes two [B, V, 3] tensors (got %s, %s)'
                         % (tuple(v3d_left.shape), tuple(v3d_right.shape)))
    vl, vr = v3d_left.detach().contiguous(), v3d_right.detach().contiguous()
    B, V = vl.shape[0], vl.shape[1]
    out = torch.empty((B, 2 * V, 3), device=vl.device, dtype=torch.float32)
    rot = (C.c_float * 9)(*view_matrix(theta).reshape(-1).tolist())
    check(ops._L().rih_demo_other_view(vl.data_ptr(), vr.data_ptr(), rot, B, V, out.data_ptr(), ops._stream()),
          'rih_demo_other_view')
    return out


class ParamSmoother:
    """The constant-acceleration filter of apps/demo.py:103-128 over every tensor entry of `params`, one launch per frame."""

    def __init__(self):
        self.reset()

    def reset(self):
        self._state, self._frames = {}, 0

    def __call__(self, params):
        keys = [k for k, v in params.items() if isinstance(v, torch.Tensor)]
        if not keys:
            return dict(params)
        if len(keys) > SMOOTH_MAX:
            raise ValueError('renderih_amd.demo: at most %d tensors per frame' % SMOOTH_MAX)
        ops._chk(*[params[k] for k in keys])
        if self._frames and (set(keys) != set(self._state) or
                             any(params[k].shape != self._state[k][0].shape for k in keys)):
            raise ValueError('renderih_amd.demo: the parameters changed their keys or shapes; call reset()')
        out, rows, keep = dict(params), [], []
        for k in keys:
            p = params[k].detach().contiguous()         # a COPY when the entry is a strided view (the network's scale_*, trans2d_*)
            keep.append(p)                              # its pointer is in `rows`: alive until the launch is queued
            if self._frames == 0:
                self._state[k] = tuple(torch.empty_like(p) for _ in range(3))        # last, last_v, acc
            out[k] = torch.empty_like(p)
            rows += [p.data_ptr(), out[k].data_ptr()] + [s.data_ptr() for s in self._state[k]] + [p.numel()]
        check(ops._L().rih_demo_smooth((C.c_int64 * len(rows))(*rows), len(keys), min(self._frames, 3), ops._stream()),
              'rih_demo_smooth')
        del keep
        self._frames += 1
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# torch mirrors: the same arithmetic in torch ops, on whatever device the tensors are on

def _resize_one_mirror(img, pt, pl, PH, PW, Sy, Sx):
    H, W = img.shape[0], img.shape[1]
    P = torch.zeros((PH, PW, 3), dtype=torch.int32, device=img.device)
    P[pt:pt + H, pl:pl + W] = img.to(torch.int32)
    if PH == Sy and PW == Sx:
        return P.to(torch.uint8)
    if PH == 2 * Sy and PW == 2 * Sx:
        return ((P[0::2, 0::2] + P[0::2, 1::2] + P[1::2, 0::2] + P[1::2, 1::2] + 2) >> 2).to(torch.uint8)
    ty = torch.from_numpy(axis_table(PH, Sy).copy()).to(img.device).long()
    tx = torch.from_numpy(axis_table(PW, Sx).copy()).to(img.device).long()
    a0, a1 = tx[:, 2].to(torch.int32)[None, :, None], tx[:, 3].to(torch.int32)[None, :, None]
    T = P[:, tx[:, 0]] * a0 + P[:, tx[:, 1]] * a1
    b0, b1 = ty[:, 2].to(torch.int32)[:, None, None], ty[:, 3].to(torch.int32)[:, None, None]
    v = (((b0 * (T[ty[:, 0]] >> 4)) >> 16) + ((b1 * (T[ty[:, 1]] >> 4)) >> 16) + 2) >> 2
    return v.clamp(0, 255).to(torch.uint8)


def _unpack(images, device):
    flat, shapes = pack_images(images, device)
    out, off = [], 0
    for (H, W) in shapes:
        out.append(flat[off:off + H * W * 3].reshape(H, W, 3))
        off += H * W * 3
    return out


def resize_bgr_mirror(images, size, device='cpu'):
    Sy, Sx = _size2(size)
    return torch.stack([_resize_one_mirror(im, 0, 0, im.shape[0], im.shape[1], Sy, Sx) for im in _unpack(images, device)])


def prepare_mirror(images, S, device='cpu'):
    """(fp32 [B, 3, S, S], fp16 [B, S, S, 8], uint8 [B, S, S, 3])."""
    u8 = []
    for im in _unpack(images, device):
        pt, pl, side = pad_to_square(im.shape[0], im.shape[1])
        u8.append(_resize_one_mirror(im, pt, pl, side, side, S, S))
    u8 = torch.stack(u8)
    # a division by a TENSOR: torch turns a division by a Python scalar into a multiplication by its reciprocal on the GPU,
    # which is not the reference's (and the kernel's) correctly rounded x / 255
    rgb = u8.flip(-1).to(torch.float32) / torch.tensor(255., device=u8.device)
    mean = torch.tensor(MEAN, dtype=torch.float32, device=u8.device)
    std = torch.tensor(STD, dtype=torch.float32, device=u8.device)
    nhwc = (rgb - mean) / std
    h8 = torch.zeros(nhwc.shape[:3] + (8,), dtype=torch.float16, device=u8.device)
    h8[..., :3] = nhwc.to(torch.float16)
    return nhwc.permute(0, 3, 1, 2).contiguous(), h8, u8


def compose_mirror(rgb, mask, bg_imgs=None):
    R = rgb.shape[1]
    if bg_imgs is None:
        bg = torch.full_like(rgb, 255.)
    else:
        bg = resize_bgr_mirror(bg_imgs, R, rgb.device).to(torch.float32)
    m = mask[..., None]
    v = (rgb * 255) * m + bg * (1 - m)
    return torch.nan_to_num(v, nan=0.0).clamp(0, 255).to(torch.uint8)


def other_view_mirror(v3d_left, v3d_right, theta=60):
    c = (torch.mean(v3d_left, 1) + torch.mean(v3d_right, 1)).unsqueeze(1) / 2
    R = torch.from_numpy(view_matrix(theta)).to(v3d_left.device)
    return torch.cat((torch.matmul(v3d_left - c, R), torch.matmul(v3d_right - c, R)), 1)


class ParamSmootherMirror:
    """apps/demo.py:103-128 with `smooth` on, line for line."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.last = self.last_v = self.v = self.a = None

    def __call__(self, params):
        params = dict(params)
        tensors = [k for k, v in params.items() if isinstance(v, torch.Tensor)]
        if self.last is not None and self.v is not None and self.a is not None:
            for k in tensors:
                pred = self.last[k] + self.v[k] + 0.5 * self.a[k]
                params[k] = 0.7 * params[k] + 0.3 * pred
        if self.last is not None:
            self.v = {k: params[k] - self.last[k] for k in tensors}
        if self.last_v is not None and self.v is not None:
            self.a = {k: self.v[k] - self.last_v[k] for k in tensors}
        self.last, self.last_v = params, self.v
        return params


# ---------------------------------------------------------------------------------------------------------------------------

class InterRender:
    """core/test_utils.py:19-128.  The four positional arguments keep their meaning; `model=` / `renderer=` inject a built
    network / two-hand renderer (then cfg_path / model_path are not read); fp16=True runs the backbone as half.HalfBackbone,
    fed by the fp16 NHWC8 output of the preparation kernel.  A network built here is switched to that backbone here; an
    injected one is shared with its owner (an InterRender of the same network without fp16 would run fp16 too once it is
    switched), so fp16=True takes an injected network only after its owner called `model.use_fp16_backbone()`, and an injected
    network is put in eval mode and moved to `device`, nothing else."""

    def __init__(self, cfg_path=None, model_path=None, input_size=256, render_size=512, *, model=None, renderer=None,
                 device='cuda', fp16=False):
        self.input_size, self.render_size = int(input_size), int(render_size)
        self.device, self.fp16 = torch.device(device), bool(fp16)
        if renderer is None:
            from .render import mano_two_hands_renderer
            renderer = mano_two_hands_renderer(img_size=self.render_size, device=self.device)
        self.renderer = renderer
        faces = getattr(renderer, 'faces', None)
        if faces is not None:
            from .render import NF_HAND, NV_HAND
            f = faces[0].detach().cpu().numpy()
            self.left_faces, self.right_faces = f[:NF_HAND], f[NF_HAND:] - NV_HAND
        injected = model is not None
        if not injected:
            from .model import load_model
            model = load_model(cfg_path)
            if model_path is not None:
                from .checkpoint import load_checkpoint
                load_checkpoint(model, model_path)            # bare or {'epoch', 'network'}, `module.` prefix fallback
        self.model = model.eval().to(self.device)
        if self.fp16:
            # the switch changes the network for everyone who holds it, so only a network built here is switched here
            if injected and getattr(self.model, '_half', None) is None:
                raise ValueError('renderih_amd.demo: fp16=True with an injected model needs model.use_fp16_backbone() called '
                                 'by its owner (on the eval-mode model, on its device); it is not switched behind their back')
            if not injected:
                self.model.use_fp16_backbone()

    # -- preparation
    def process_imgs(self, images):
        """fp32 [B, 3, S, S] (the reference's tensor); with fp16=True the fp16 [B, S, S, 8] tensor the backbone takes."""
        n, h, _ = prepare(images, self.input_size, self.device, norm=not self.fp16, h8=self.fp16)
        return h if self.fp16 else n

    def process_img(self, img):
        _single(img)
        return prepare(img, self.input_size, self.device)[0]

    @staticmethod
    def save_obj(path, verts, faces, color=None):
        """Wavefront OBJ: `v x y z [r g b]` per vertex, `f a b c` (1-based) per face."""
        tail = '' if color is None else ' {} {} {}'.format(color[0], color[1], color[2])
        with open(path, 'w') as fh:
            for v in verts:
                fh.write('v {} {} {}{}\n'.format(v[0], v[1], v[2], tail))
            for f in faces:
                fh.write('f {} {} {}\n'.format(f[0] + 1, f[1] + 1, f[2] + 1))

    # -- network
    @torch.no_grad()
    def run_model_batch(self, images):
        result, paramsDict, handDictList, otherInfo = self.model(self.process_imgs(images))
        return {'scale_left': paramsDict['scale']['left'], 'trans2d_left': paramsDict['trans2d']['left'],
                'scale_right': paramsDict['scale']['right'], 'trans2d_right': paramsDict['trans2d']['right'],
                'v3d_left': result['verts3d']['left'], 'v3d_right': result['verts3d']['right'], 'otherInfo': otherInfo}

    def run_model(self, img):
        _single(img)
        return self.run_model_batch(img)

    # -- overlays
    @torch.no_grad()
    def render_batch(self, params, bg_imgs=None):
        img_out, mask_out = self.renderer.render_rgb_orth(scale_left=params['scale_left'], trans2d_left=params['trans2d_left'],
                                                          scale_right=params['scale_right'],
                                                          trans2d_right=params['trans2d_right'],
                                                          v3d_left=params['v3d_left'], v3d_right=params['v3d_right'])
        return compose(img_out, mask_out, bg_imgs)

    def render(self, params, bg_img=None):
        if bg_img is not None:
            _single(bg_img)
        return self.render_batch(params, bg_img)[0].cpu().numpy()

    @torch.no_grad()
    def render_other_view_batch(self, params, theta=60):
        v = other_view(params['v3d_left'], params['v3d_right'], theta)
        B, V, dev = v.shape[0], v.shape[1] // 2, v.device
        three, zero = torch.full((B,), 3., device=dev), torch.zeros((B, 2), device=dev)
        img_out, mask_out = self.renderer.render_rgb_orth(scale_left=three, scale_right=three, trans2d_left=zero,
                                                          trans2d_right=zero, v3d_left=v[:, :V], v3d_right=v[:, V:])
        return compose(img_out, mask_out, None)

    def render_other_view(self, params, theta=60):
        return self.render_other_view_batch(params, theta)[0].cpu().numpy()


def _single(img):
    if not isinstance(img, (np.ndarray, torch.Tensor)) or img.ndim != 3:
        raise ValueError('renderih_amd.demo: one H x W x 3 image expected (the batched forms take lists)')
