"""The auxiliary heads of the encoders -- 42 joint heat maps, the 2-channel hand mask, the 6-channel dense-correspondence map
(`otherInfo['hms' | 'mask' | 'dense']`) -- from the label to the loss and back to 2-D joints: the label generator
(dataset/heatmap.py:11-39 `HeatmapGenerator`), the label images of the loader (core/loader_ori.py:117-145), the loss
(core/Loss.py:180-198 `calc_aux_loss`, the line the reference ships commented out at core/Loss.py:211) and the decoder the
trainer logs with (dataset/inference.py:113-127 `get_final_preds2`, core/gcn_trainer.py:282,287).  Each as a plain-torch mirror
(fp64 or fp32, any device) and as a fused class on csrc/rih_aux.hip (GPU, fp32, no fallback).

Conventions
  * Everything is NCHW.  Heat maps: channels 0..20 the LEFT hand's joints, 21..41 the RIGHT hand's (loader_ori.py:100,
    `hms_left + hms_right`).  A joint is (x, y) or (x, y, v) in heat-map pixels, x along the columns; v <= 0 switches it off.
  * Mask and dense labels, channel order.  `render_mask` paints the left hand's vertices into colour channel 2 and the right
    hand's into channel 1 (utils/vis_utils.py:232-234).  cv.imwrite / cv.imread treat an array as BGR both ways, so the array
    the loader reads has the channels where the renderer put them, and `mask[..., 1:]` (loader_ori.py:132) keeps (channel 1,
    channel 2): mask label channel 0 is the RIGHT hand, channel 1 the LEFT hand.  The dense label is the three channels of
    `render_densepose` as they come.  calc_aux_loss pairs prediction channels 0:3 of 'dense' with mask channel 0 (right hand)
    and 3:6 with mask channel 1 (left hand).
  * Flip (loader_ori.py:117-143): columns mirrored, the two mask channels swapped, the two blocks of 21 heat maps swapped; the
    dense channels stay.
  * SmoothL1: calc_aux_loss uses `hand_loss.smoothL1Loss`, which core/Loss.py:26 builds with beta = 0.05 (NOT the beta = 1 of
    `L1Loss` there); `SMOOTH_L1_BETA` holds it, and both loss classes take `beta=`.  MSE for the heat maps.  Weights
    utils/defaults.yaml:51-54: DENSEPOSE 30, MASK 500, HMS 100.
  * The decoder's blur taps are OpenCV's fixed table for sigma = 0 (3: (1, 2, 1)/4, 5: (1, 4, 6, 4, 1)/16, 7: (1, 3.5, 7, 9, 7,
    3.5, 1)/32), zero padding.  The fixture tests/golden/aux_heads.npz was made with a numpy stand-in for cv2.GaussianBlur that
    uses these taps (cv2 is not a dependency): the taps are pinned by that stand-in, not by OpenCV.

DELIBERATE DEVIATIONS
  * `total_loss` is always in the returned dict.  The reference adds the key only `if total_loss > 0`, a host sync.
  * Labels are drawn at the heat-map size S directly (`aux_labels`).  The reference renders at 256, stores JPEG files, warps
    them with the augmentation and resizes with OpenCV; there is no 8-bit quantisation and no JPEG round trip here.
  * In the joints form of the flip the JOINT is mirrored (x -> S - 1 - x) and the map drawn from it; the loader mirrors the drawn
    image.  A joint that the generator does not draw (x < 0 or x >= S) is carried through the flip as off (x = -1), so its
    map stays zero as the loader's mirrored image is -- without that, -1 < x < 0 would mirror into range and be drawn.  One
    case remains different: a joint in the last pixel (S - 1 < x < S) is drawn by the generator, and its mirror image
    (-1 < x < 0) cannot be expressed as a joint the generator draws: its map is zero here and a mirrored Gaussian there.
  * The HRNet encoder's mask has ONE channel (encoder.py:395); calc_aux_loss does not fit it in the reference either (its
    `mask[:, 1:]` is empty there).  It is refused with a ValueError.
  * `get_final_preds2` blurs its argument in place; nothing here writes its input.  A map whose maximum is not positive gives
    (0, 0) and never a NaN (the reference divides by zero in the rescale of such a map but does not read the result).  A map
    with a positive maximum whose blurred maximum is <= 0 (an isolated positive pixel among large negatives, kernel > 1) is
    rescaled by raw / blurred maximum as the reference does: its coordinates can be inf or NaN, as the reference's.  NaNs in a
    map are not defined behaviour (the kernel's arg-max skips them).
"""
import numpy as np
import torch
import torch.nn.functional as F

BLUR_KERNEL = 5          # dataset/dataset_utils.py:4-8
HEATMAP_SIZE = 64
HEATMAP_SIGMA = 2
IMG_SIZE = 256
SMOOTH_L1_BETA = 0.05    # core/Loss.py:26
AUX_DEFAULT_WEIGHTS = {'MASK': 500.0, 'DENSEPOSE': 30.0, 'HMS': 100.0}
AUX_TERMS = ['mask_loss', 'dense_loss', 'hms_loss']
BLUR_TAPS = {3: (0.25, 0.5, 0.25), 5: (0.0625, 0.25, 0.375, 0.25, 0.0625),
             7: (0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125)}


def aux_weights(weights=None):
    """{'MASK', 'DENSEPOSE', 'HMS'} from None (utils/defaults.yaml), a flat dict, the reference's cfg (cfg.LOSS_WEIGHT.AUX is
    read), its LOSS_WEIGHT node or its AUX node."""
    w = dict(AUX_DEFAULT_WEIGHTS)
    if weights is None:
        return w
    node = weights
    for key in ('LOSS_WEIGHT', 'AUX'):
        sub = node.get(key) if isinstance(node, dict) else getattr(node, key, None)
        if sub is not None:
            node = sub
    get = node.get if isinstance(node, dict) else (lambda k, d=None: getattr(node, k, d))
    if isinstance(node, dict):
        unknown = set(node) - set(w)
        if unknown:
            raise KeyError('unknown aux loss weights %s' % sorted(unknown))
    for k in w:
        if get(k) is not None:
            w[k] = float(get(k))
    return w


# ------------------------------------------------------------------------------------------------ heat-map labels
def _joints_3d(joints):
    """[J, C] or [N, J, C] (heatmap.py:19-20) -> [N, J, C], C in (2, 3)."""
    if joints.dim() == 2:
        joints = joints.unsqueeze(0)
    if joints.dim() != 3 or joints.shape[-1] not in (2, 3):
        raise ValueError('heat-map joints must be [J, 2|3] or [N, J, 2|3]; got %s' % (tuple(joints.shape),))
    return joints


def heatmaps(joints, res, sigma):
    """build_hm over a batch in torch: joints [N, J, 2|3] -> [N, J, res, res] in the dtype of `joints`."""
    joints = _joints_3d(joints)
    x, y = joints[..., 0, None, None], joints[..., 1, None, None]
    ar = torch.arange(res, device=joints.device, dtype=joints.dtype)
    xl, yl = ar[None, None, None, :], ar[None, None, :, None]
    hm = torch.exp(-((xl - x) ** 2 + (yl - y) ** 2) / (2 * sigma ** 2))
    on = ~((x < 0) | (y < 0) | (x >= res) | (y >= res))
    if joints.shape[-1] == 3:
        on = on & (joints[..., 2, None, None] > 0)
    return torch.where(on, hm, torch.zeros_like(hm))


class HeatmapGenerator:
    """dataset/heatmap.py:11-39 in torch.  numpy in: numpy float32 out, computed in fp64, as the reference;
    torch in: a tensor of the same dtype and device."""

    def __init__(self, output_res=128, sigma=-1):
        self.output_res = output_res
        self.sigma = output_res / 32 if sigma < 0 else sigma

    def __call__(self, joints, scale=1):
        if isinstance(joints, np.ndarray):
            t = torch.from_numpy(np.ascontiguousarray(joints)).double()
            return heatmaps(t, self.output_res, self.sigma * scale).float().numpy()
        return heatmaps(joints, self.output_res, self.sigma * scale)


def _fused_input(what, *tensors):
    """HIP kernels only: fp32, contiguous, on the GPU (no silent copy, no CPU fallback)."""
    from . import ops
    ops._chk(*tensors)
    for t in tensors:
        if t is None:
            continue
        if t.dtype != torch.float32:
            raise RuntimeError('%s expects float32; got %s' % (what, t.dtype))
        if not t.is_contiguous():
            raise ValueError('%s expects contiguous tensors; got strides %s for shape %s' % (what, t.stride(), tuple(t.shape)))


def _p(t):
    return 0 if t is None else t.data_ptr()


class FusedHeatmapGenerator:
    """`HeatmapGenerator` on rih_heatmaps: GPU fp32 tensors only, one launch, capturable.  `out`: a result buffer to fill."""

    def __init__(self, output_res=128, sigma=-1):
        self.output_res = output_res
        self.sigma = output_res / 32 if sigma < 0 else sigma

    def __call__(self, joints, scale=1, out=None):
        from . import _lib
        from .ops import _stream, check
        if not isinstance(joints, torch.Tensor):
            raise RuntimeError('FusedHeatmapGenerator takes GPU float32 tensors (HeatmapGenerator takes numpy)')
        joints = _joints_3d(joints)
        _fused_input('FusedHeatmapGenerator', joints, out)
        N, J, C = joints.shape
        R = self.output_res
        if out is None:
            out = torch.empty((N, J, R, R), device=joints.device, dtype=torch.float32)
        elif tuple(out.shape) != (N, J, R, R) or out.device != joints.device:
            raise ValueError('FusedHeatmapGenerator: out must be %s on %s' % ((N, J, R, R), joints.device))
        check(_lib.load().rih_heatmaps(joints.data_ptr(), out.data_ptr(), N * J, C, R, float(self.sigma * scale), _stream()),
              'rih_heatmaps')
        return out


# ------------------------------------------------------------------------------------------------ the loss
def _check_heads(dataDict, mask, dense, hms, joints2d):
    """The shapes calc_aux_loss needs; returns (B, S).  Refuses the HRNet encoder's one-channel mask."""
    ref = None
    for k in ('mask', 'dense', 'hms'):
        if k in dataDict:
            ref = dataDict[k]
            break
    if ref is None:
        raise ValueError('aux loss: the prediction dict has none of mask, dense, hms')
    if 'mask' in dataDict and (dataDict['mask'].dim() != 4 or dataDict['mask'].shape[1] != 2):
        raise ValueError('aux loss: the mask prediction has shape %s; calc_aux_loss needs the two-channel mask of the ResNet '
                         'encoder.  The HRNet encoder emits ONE channel, which does not fit calc_aux_loss in the reference either'
                         % (tuple(dataDict['mask'].shape),))
    if ref.dim() != 4 or ref.shape[-1] != ref.shape[-2]:
        raise ValueError('aux loss: predictions must be [B, C, S, S]; got %s' % (tuple(ref.shape),))
    B, S = ref.shape[0], ref.shape[-1]
    want = {'mask': (B, 2, S, S), 'dense': (B, 6, S, S)}
    for k in ('mask', 'dense'):
        if k in dataDict and tuple(dataDict[k].shape) != want[k]:
            raise ValueError('aux loss: %s prediction has shape %s, expected %s' % (k, tuple(dataDict[k].shape), want[k]))
    if 'mask' in dataDict or 'dense' in dataDict:
        if mask is None or tuple(mask.shape) != (B, 2, S, S):
            raise ValueError('aux loss: the mask label must be %s' % ((B, 2, S, S),))
    if 'dense' in dataDict and (dense is None or tuple(dense.shape) != (B, 3, S, S)):
        raise ValueError('aux loss: the dense label must be %s' % ((B, 3, S, S),))
    if 'hms' in dataDict:
        p = dataDict['hms']
        if p.dim() != 4 or p.shape[0] != B or tuple(p.shape[2:]) != (S, S):
            raise ValueError('aux loss: hms prediction has shape %s, expected [%d, Jh, %d, %d]' % (tuple(p.shape), B, S, S))
        if (hms is None) == (joints2d is None):
            raise ValueError('aux loss: give the heat-map label as hms= (a tensor) or as joints2d= (with sigma=), one of the two')
        if hms is not None and tuple(hms.shape) != tuple(p.shape):
            raise ValueError('aux loss: the hms label must be %s' % (tuple(p.shape),))
        if joints2d is not None and (joints2d.dim() != 3 or tuple(joints2d.shape[:2]) != (B, p.shape[1]) or
                                     joints2d.shape[2] not in (2, 3)):
            raise ValueError('aux loss: joints2d must be [%d, %d, 2|3]' % (B, p.shape[1]))
    return B, S


class AuxLoss:
    """calc_aux_loss restated in torch, differentiable by autograd.  `weights`: see aux_weights."""

    def __init__(self, weights=None, beta=SMOOTH_L1_BETA):
        self.w = aux_weights(weights)
        self.beta = beta

    def set_weights(self, **kw):
        aux_weights(kw)                                  # (refuses unknown keys)
        self.w.update({k: float(v) for k, v in kw.items()})

    def __call__(self, dataDict, mask=None, dense=None, hms=None, joints2d=None, sigma=None):
        """dataDict: the predictions ('mask' [B,2,S,S], 'dense' [B,6,S,S], 'hms' [B,Jh,S,S]; a missing key = an absent term);
        mask, dense: the labels; the heat-map label as hms= or as joints2d= [B,Jh,2|3] in heat-map pixels with sigma=
        (default HEATMAP_SIGMA).  Returns (total, {'mask_loss', 'dense_loss', 'hms_loss', 'total_loss'})."""
        _, S = _check_heads(dataDict, mask, dense, hms, joints2d)
        ref = next(dataDict[k] for k in ('mask', 'dense', 'hms') if k in dataDict)
        zero = ref.new_zeros(())
        d = {k: zero for k in AUX_TERMS}
        if 'mask' in dataDict:
            d['mask_loss'] = F.smooth_l1_loss(dataDict['mask'], mask, beta=self.beta)
        if 'dense' in dataDict:
            p = dataDict['dense']
            d['dense_loss'] = (F.smooth_l1_loss(p[:, :3] * mask[:, :1], dense * mask[:, :1], beta=self.beta) +
                               F.smooth_l1_loss(p[:, 3:] * mask[:, 1:], dense * mask[:, 1:], beta=self.beta)) / 2
        if 'hms' in dataDict:
            if hms is None:
                hms = heatmaps(joints2d.to(dataDict['hms'].dtype), S, HEATMAP_SIGMA if sigma is None else sigma)
            d['hms_loss'] = F.mse_loss(dataDict['hms'], hms)
        d['total_loss'] = self.w['MASK'] * d['mask_loss'] + self.w['DENSEPOSE'] * d['dense_loss'] + self.w['HMS'] * d['hms_loss']
        return d['total_loss'], d


class _AuxLossFn(torch.autograd.Function):
    """calc_aux_loss and the gradients of its total in two launches (rih_aux_loss + rih_aux_loss_final); backward only scales
    the saved gradients by the incoming one."""

    @staticmethod
    def forward(ctx, fused, sigma, t_hms, t_joints, t_mask, t_dense, p_hms, p_mask, p_dense):
        from . import _lib
        from .ops import _stream, check
        lib = _lib.load()
        preds = (p_hms, p_mask, p_dense)
        ref = next(t for t in preds if t is not None)
        _fused_input('FusedAuxLoss', *preds, t_hms, t_joints, t_mask, t_dense)
        for t in (t_hms, t_joints, t_mask, t_dense) + preds:
            if t is not None and t.device != ref.device:
                raise ValueError('FusedAuxLoss: every tensor must be on %s' % ref.device)
        B, S = ref.shape[0], ref.shape[-1]
        Jh = 0 if p_hms is None else p_hms.shape[1]
        C = 0 if t_joints is None else t_joints.shape[-1]
        has_md = int(p_mask is not None or p_dense is not None)
        nblk = lib.rih_aux_loss_blocks(B, Jh, S, int(p_hms is not None), has_md)
        if nblk < 1:
            raise ValueError('FusedAuxLoss: sizes B = %d, Jh = %d, S = %d are outside what rih_aux_loss takes' % (B, Jh, S))
        grads = [None if t is None else torch.empty_like(t) for t in preds]
        parts = torch.empty((nblk, 4), device=ref.device, dtype=torch.float32)
        out = torch.empty((4,), device=ref.device, dtype=torch.float32)
        wdev = fused.device_weights(ref.device)
        check(lib.rih_aux_loss(_p(p_hms), _p(p_mask), _p(p_dense), _p(t_hms), _p(t_joints), _p(t_mask), _p(t_dense),
                               wdev.data_ptr(), B, Jh, S, C, float(sigma), float(fused.beta), _p(grads[0]), _p(grads[1]),
                               _p(grads[2]), parts.data_ptr(), _stream()), 'rih_aux_loss')
        check(lib.rih_aux_loss_final(parts.data_ptr(), wdev.data_ptr(), B, Jh, S, int(p_hms is not None), has_md,
                                     out.data_ptr(), _stream()), 'rih_aux_loss_final')
        ctx.present = [g is not None for g in grads]
        ctx.save_for_backward(*[g for g in grads if g is not None])
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        # out of place: the saved gradients may be read again (retain_graph); ONE multi-tensor launch
        scaled = iter(torch._foreach_mul(list(ctx.saved_tensors), g_total))
        return (None,) * 6 + tuple(next(scaled) if here else None for here in ctx.present)


class FusedAuxLoss:
    """`AuxLoss` (same call, same total, terms and gradients) on csrc/rih_aux.hip: GPU fp32 contiguous tensors only.  The three
    weights live in a device tensor that the kernels read at run time: `set_weights()` rewrites it in place, so a captured
    graph follows the change."""

    def __init__(self, weights=None, beta=SMOOTH_L1_BETA):
        self.w = aux_weights(weights)
        self.beta = beta
        self._dev = {}

    def _values(self):
        return (self.w['MASK'], self.w['DENSEPOSE'], self.w['HMS'])

    def device_weights(self, device):
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = [torch.zeros(4, device=device, dtype=torch.float32), None]
        slot = self._dev[device]
        if slot[1] != self._values():
            if device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('FusedAuxLoss: the weights changed during stream capture; call set_weights() or run one '
                                   'eager step before capturing')
            slot[0].copy_(torch.tensor(self._values() + (0.0,), dtype=torch.float32))
            slot[1] = self._values()
        return slot[0]

    def set_weights(self, **kw):
        """set_weights(MASK=..., DENSEPOSE=..., HMS=...): also refreshes, in place, every device copy that exists."""
        aux_weights(kw)                                  # (refuses unknown keys)
        self.w.update({k: float(v) for k, v in kw.items()})
        for device in list(self._dev):
            self.device_weights(device)

    def __call__(self, dataDict, mask=None, dense=None, hms=None, joints2d=None, sigma=None):
        _check_heads(dataDict, mask, dense, hms, joints2d)
        has_md = 'mask' in dataDict or 'dense' in dataDict
        total, out = _AuxLossFn.apply(self, HEATMAP_SIGMA if sigma is None else sigma,
                                      hms if 'hms' in dataDict else None, joints2d if 'hms' in dataDict else None,
                                      mask if has_md else None, dense if 'dense' in dataDict else None,
                                      dataDict.get('hms'), dataDict.get('mask'), dataDict.get('dense'))
        return total, {'mask_loss': out[1], 'dense_loss': out[2], 'hms_loss': out[3], 'total_loss': total}


def calc_aux_loss(cfg_or_weights, hand_loss, dataDict, mask, dense, hms, joints2d=None, sigma=None):
    """core/Loss.py:180-198 with its argument order; returns the loss dict (`total_loss` always present).  `cfg_or_weights`: an
    `AuxLoss` / `FusedAuxLoss` to run, or what `aux_weights` takes (then the mirror runs).  `hand_loss` is where the reference
    finds its two loss modules; only its `smoothL1Loss.beta` is read here (None: SMOOTH_L1_BETA)."""
    if isinstance(cfg_or_weights, (AuxLoss, FusedAuxLoss)):
        fn = cfg_or_weights
    else:
        beta = getattr(getattr(hand_loss, 'smoothL1Loss', None), 'beta', SMOOTH_L1_BETA)
        fn = AuxLoss(cfg_or_weights, beta=beta)
    return fn(dataDict, mask, dense, hms=hms, joints2d=joints2d, sigma=sigma)[1]


# ------------------------------------------------------------------------------------------------ the decoder
def _blur(maps, kernel):
    """maps [M, H, W] -> the zero-padded separable blur: rows first (left to right), then columns (top to bottom)."""
    taps, r = BLUR_TAPS[kernel], kernel // 2
    H, W = maps.shape[-2:]
    p = F.pad(maps, (r, r, r, r))
    rows = sum(taps[j] * p[:, :, j:j + W] for j in range(kernel))
    return sum(taps[i] * rows[:, i:i + H] for i in range(kernel))


def decode_heatmaps(hm, kernel=BLUR_KERNEL):
    """get_final_preds2 in vectorised torch (any device, fp64 or fp32): hm [N, J, H, W] -> (preds [N, J, 2] = (x, y),
    maxvals [N, J]).  `hm` is not written."""
    if hm.dim() != 4:
        raise ValueError('decode_heatmaps: hm must be [N, J, H, W]; got %s' % (tuple(hm.shape),))
    if kernel > 1 and kernel not in BLUR_TAPS:
        raise ValueError('heat-map decoder: blur kernel %r; the fixed taps exist for 3, 5 and 7 (and <= 1 = no blur)' % (kernel,))
    N, J, H, W = hm.shape
    maps = hm.reshape(N * J, H, W)
    flat = maps.reshape(N * J, H * W)
    maxvals = flat.max(dim=1).values
    ar = torch.arange(H * W, device=hm.device)
    idx = torch.where(flat == maxvals[:, None], ar[None], torch.full_like(ar, H * W)[None]).min(dim=1).values     # first index
    idx = idx.clamp(max=H * W - 1)
    pos = maxvals > 0
    px, py = (idx % W) * pos, torch.div(idx, W, rounding_mode='floor') * pos
    preds = torch.stack([px, py], dim=1).to(hm.dtype)
    if H >= 5 and W >= 5:
        if kernel > 1:
            b = _blur(maps, kernel)
            maps = b * (maxvals / b.reshape(N * J, -1).max(dim=1).values)[:, None, None]
        L = torch.log(torch.clamp_min(maps, 1e-10))
        inside = (px > 1) & (px < W - 2) & (py > 1) & (py < H - 2)
        cx, cy, m = px.clamp(2, W - 3), py.clamp(2, H - 3), torch.arange(N * J, device=hm.device)
        at = lambda dy, dx: L[m, cy + dy, cx + dx]                           # noqa: E731
        dx, dy = 0.5 * (at(0, 1) - at(0, -1)), 0.5 * (at(1, 0) - at(-1, 0))
        dxx = 0.25 * (at(0, 2) - 2 * at(0, 0) + at(0, -2))
        dxy = 0.25 * (at(1, 1) - at(-1, 1) - at(1, -1) + at(-1, -1))
        dyy = 0.25 * (at(2, 0) - 2 * at(0, 0) + at(-2, 0))
        det = dxx * dyy - dxy ** 2
        ok = inside & (det != 0) & pos
        safe = torch.where(ok, det, torch.ones_like(det))
        off = torch.stack([-(dyy * dx - dxy * dy) / safe, -(dxx * dy - dxy * dx) / safe], dim=1)
        preds = preds + torch.where(ok[:, None], off, torch.zeros_like(off))
    return preds.reshape(N, J, 2), maxvals.reshape(N, J)


def get_final_preds2(hm, kernel):
    """dataset/inference.py:113-127: numpy in, numpy out -- preds [N, J, 2] float32 and maxvals [N, J, 1] in hm's dtype --
    computed in hm's dtype.  `hm` is not written (the reference blurs it in place)."""
    assert isinstance(hm, np.ndarray), 'batch_heatmaps should be numpy.ndarray'
    assert hm.ndim == 4, 'batch_images should be 4-ndim'
    preds, maxvals = decode_heatmaps(torch.from_numpy(np.ascontiguousarray(hm)), kernel)
    return preds.numpy().astype(np.float32), maxvals.numpy()[..., None]


class FusedHeatmapDecoder:
    """`decode_heatmaps` on rih_hms_decode: one workgroup per map, the map in LDS, one launch, capturable, nothing read back by
    the host.  GPU fp32 contiguous tensors only; H * W <= 16384; kernel 1, 3, 5 or 7."""

    def __init__(self, kernel=BLUR_KERNEL):
        if kernel != 1 and kernel not in BLUR_TAPS:
            raise ValueError('FusedHeatmapDecoder: blur kernel %r; the fixed taps exist for 3, 5 and 7 (and 1 = no blur)' % (kernel,))
        self.kernel = kernel

    def __call__(self, hm, preds=None, maxvals=None):
        from . import _lib
        from .ops import _stream, check
        if not isinstance(hm, torch.Tensor) or hm.dim() != 4:
            raise ValueError('FusedHeatmapDecoder: hm must be a [N, J, H, W] tensor')
        _fused_input('FusedHeatmapDecoder', hm, preds, maxvals)
        N, J, H, W = hm.shape
        if H * W * 4 > 65536:
            raise ValueError('FusedHeatmapDecoder: a %d x %d map does not fit 64 KB of LDS' % (H, W))
        if preds is None:
            preds = torch.empty((N, J, 2), device=hm.device, dtype=torch.float32)
        if maxvals is None:
            maxvals = torch.empty((N, J), device=hm.device, dtype=torch.float32)
        if tuple(preds.shape) != (N, J, 2) or tuple(maxvals.shape) != (N, J):
            raise ValueError('FusedHeatmapDecoder: preds must be %s and maxvals %s' % ((N, J, 2), (N, J)))
        check(_lib.load().rih_hms_decode(hm.data_ptr(), preds.data_ptr(), maxvals.data_ptr(), N * J, H, W, self.kernel,
                                         _stream()), 'rih_hms_decode')
        return preds, maxvals


# ------------------------------------------------------------------------------------------------ the label images
def aux_labels(renderer, v3d_left, v3d_right, cameras=None, scale=None, trans2d=None, joints2d=None, flip=None,
               img_size=None, heatmaps_as='joints', sigma=HEATMAP_SIGMA):
    """The three labels of calc_aux_loss for a batch, drawn at the heat-map size: `renderer` is a mano_two_hands_renderer built
    at img_size = S; the camera arguments are those of its render_mask / render_densepose (at that size).
      mask  [B, 2, S, S] in {0, 1}: channel 0 the RIGHT hand, channel 1 the LEFT hand (module docstring); the loader's
            threshold 127 of 255 (loader_ori.py:130).
      dense [B, 3, S, S] in [0, 1]: render_densepose's three channels.
      hms   from joints2d [B, 42, 2|3] (left 21, right 21) given in pixels of an image of side `img_size` (None: S, no scaling;
            the reference draws `joints * HEATMAP_SIZE / IMG_SIZE`): heatmaps_as = 'joints' returns the scaled joints, the
            label of the loss's in-kernel form; 'tensor' the maps [B, 42, S, S] (rih_heatmaps on GPU fp32 joints, the mirror
            otherwise).  None when joints2d is None.
    flip: None, a bool, or a bool tensor [B] (per sample, no host read): columns mirrored, mask channels and the two blocks of
    21 heat maps swapped."""
    S = renderer.img_size[0] if isinstance(renderer.img_size, (tuple, list)) else renderer.img_size
    if heatmaps_as not in ('joints', 'tensor'):
        raise ValueError("aux_labels: heatmaps_as is 'joints' or 'tensor'")
    cam = dict(cameras=cameras, scale=scale, trans2d=trans2d)
    rgb = renderer.render_mask(v3d_left=v3d_left, v3d_right=v3d_right, **cam)                 # [B, S, S, 3]
    mask = (rgb[..., 1:] * 255 > 127).to(rgb.dtype).permute(0, 3, 1, 2)
    dense = renderer.render_densepose(v3d_left=v3d_left, v3d_right=v3d_right, **cam)[0].permute(0, 3, 1, 2)
    B = mask.shape[0]
    hms = None
    if joints2d is not None:
        j = torch.as_tensor(joints2d).to(mask.device)
        if j.dim() != 3 or j.shape[0] != B or j.shape[1] % 2 != 0 or j.shape[2] not in (2, 3):
            raise ValueError('aux_labels: joints2d must be [%d, 2 * J, 2|3]; got %s' % (B, tuple(j.shape)))
        if img_size is not None and img_size != S:
            j = torch.cat([j[..., :2] * (S / img_size), j[..., 2:]], dim=-1)
        hms = j.contiguous()
        if heatmaps_as == 'tensor':
            gen = FusedHeatmapGenerator if hms.is_cuda and hms.dtype == torch.float32 else HeatmapGenerator
            hms = gen(S, sigma)(hms)
    if flip is not None:
        f = torch.full((B,), flip, device=mask.device) if isinstance(flip, bool) else \
            torch.as_tensor(flip, device=mask.device).expand(B)
        f4 = f[:, None, None, None]
        mask = torch.where(f4, mask.flip(-1)[:, [1, 0]], mask)
        dense = torch.where(f4, dense.flip(-1), dense)
        if hms is not None:
            half = hms.shape[1] // 2
            if heatmaps_as == 'tensor':                   # the drawn image is mirrored, as the loader does
                other = hms.flip(-1)
            else:                                         # the joint is mirrored (module docstring)
                x = hms[..., :1]
                x = torch.where((x < 0) | (x >= S), torch.full_like(x, -1.0), (S - 1) - x)     # off stays off
                other, f4 = torch.cat([x, hms[..., 1:]], dim=-1), f[:, None, None]
            hms = torch.where(f4, torch.cat([other[:, half:], other[:, :half]], dim=1), hms)
    return mask.contiguous(), dense.contiguous(), None if hms is None else hms.contiguous()
