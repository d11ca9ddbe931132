"""Two-hand silhouette IoU -- the interaction level behind the reference's IoU-binned evaluation (apps/eval_interhand.py:230-234,
471-536), whose side file `iou_0_27w.npy` the reference does not ship.  utils/compute_maskiou.py:219-275 (`render_data`) builds
that file one sample at a time: two MANO forwards, two pytorch3d silhouette renders (`render_single_mask`), a threshold at 0.2,
a copy to the host and `bm0` (:59-64):

    area_left  = count(left_mask == 1)          area_right = count(right_mask == 1)
    inter      = count(left_mask != 0 and right_mask != 0)
    iou        = inter / (area_left + area_right - inter)

A covered pixel of `render_single_mask` is exactly 1 (the colour 255 under ambient light, divided by 255) and the background
1/255 falls under the threshold, so the three counts are counts of COVERED pixels: covered by a hand exactly when
`render.rasterize` of that hand's faces alone reports pix_to_face >= 0.

`TwoHandMaskIoU` is the mirror: those lines restated on this project's renderer, in torch on the device (two renders of three
launches each per call).  `FusedTwoHandMaskIoU` is the same surface on rih_mask_iou (csrc/rih_render.hip): one
rih_render_setup launch over cat(left, right) and one coverage-only pass that keeps two flags per pixel and leaves three
integers per image -- no fragments, no RGBA, nothing on the host; a call can be captured in a `torch.cuda.graph`.  Both return
(iou fp32 [B], counts int32 [B, 3] = area_left, area_right, intersection).

The one departure from the reference: the IoU of an image whose union is empty is 0 (`bm0` raises ZeroDivisionError there).
The face table: both hands go through ONE table, as in the reference, where both go through `_faces_single`; `faces=None` is
`assets.hand_faces('right')` here (the reference's table is the same with the first two corners swapped; coverage does not
depend on the winding beyond the last bit of an edge function).  Square images only, as the renderer.

`iou_bins` gives the three masks of eval_interhand.py:232-234, `scan_annotations` builds the side file from the annotation
dicts `render_data` reads, and `evaluate.summarize_by_iou` prints the breakdown.  Out of scope: the convex-hull IoU of
utils/get_maskiou.py, depth-aware visible areas, non-square images (the 480 x 640 Tzionas call).
"""
import numpy as np
import torch

from . import assets, ops, render
from .ops import check


def _table(faces):
    f = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces)
    if f.ndim == 3:
        f = f[0]
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
        raise ValueError('renderih_amd.render: faces must be [F, 3] with F >= 1 (got %s)' % (tuple(f.shape),))
    return torch.from_numpy(np.ascontiguousarray(f.astype(np.int64)))


def _two_tables(faces):
    """faces: None (the right hand's table for both), one table (for both) or a pair (left, right)."""
    if faces is None:
        faces = assets.hand_faces('right')
    if isinstance(faces, (tuple, list)) and len(faces) == 2 and np.ndim(faces[0]) >= 2:
        return _table(faces[0]), _table(faces[1])
    t = _table(faces)
    return t, t


def _check_hands(v3d_left, v3d_right):
    for v in (v3d_left, v3d_right):
        if not torch.is_tensor(v) or v.dim() != 3 or v.shape[2] != 3:
            raise ValueError('renderih_amd.render: verts must be [B, V, 3]')
    if v3d_left.shape[0] != v3d_right.shape[0]:
        raise ValueError('renderih_amd.render: verts must be [B, V, 3] with one B for both hands (got %d and %d)'
                         % (v3d_left.shape[0], v3d_right.shape[0]))


def _ratio(counts):
    inter = counts[:, 2]
    union = counts[:, 0] + counts[:, 1] - inter
    # bm0's fp64 quotient, rounded once more to fp32: for integers below 2^24 that is the correctly rounded fp32 quotient
    iou = (inter.double() / union.clamp(min=1).double()).float()
    return torch.where(union > 0, iou, torch.zeros_like(iou))


class TwoHandMaskIoU:
    """compute_maskiou.py:263-270 on `render.mano_two_hands_renderer`: `render_single_mask` per hand (both through
    `_faces_single`), `mask[mask < 0.2] = 0`, channel 0, the three counts and the ratio in torch on the device.  MANO meshes
    only ([B, 778, 3]), one face table; see the module docstring."""

    def __init__(self, img_size, device, faces=None):
        self.img_size = render._square(img_size)
        self.device = device
        left, right = _two_tables(faces)
        if left is not right:
            raise ValueError('the mirror renders both hands with one face table, as the reference does')
        self.renderer = render.mano_two_hands_renderer(img_size=self.img_size, device=device)
        self.renderer._faces_single = left.to(device)

    def masks(self, v3d_left, v3d_right, cameras=None, scale=None, trans2d=None):
        """(left_mask, right_mask) [B, S, S]: channel 0 after the threshold."""
        _check_hands(v3d_left, v3d_right)
        out = []
        for v in (v3d_left, v3d_right):
            mask = self.renderer.render_single_mask(cameras=cameras, scale=scale, trans2d=trans2d, v3d=v.to(self.device))
            mask[mask < 0.2] = 0
            out.append(mask[:, :, :, 0])
        return out

    def __call__(self, v3d_left, v3d_right, cameras=None, scale=None, trans2d=None):
        left, right = self.masks(v3d_left, v3d_right, cameras, scale, trans2d)
        counts = torch.stack(((left == 1).sum((1, 2)), (right == 1).sum((1, 2)),
                              ((left != 0) & (right != 0)).sum((1, 2))), 1).to(torch.int32)
        return _ratio(counts), counts


class FusedTwoHandMaskIoU:
    """`TwoHandMaskIoU` on rih_mask_iou: one setup launch over cat(left, right) and one coverage-only pass; see the module
    docstring.  `faces`: None, one table for both hands, or a pair (left, right) of tables of any lengths; the hands may have
    any numbers of vertices.  fp32 GPU tensors only."""

    def __init__(self, img_size, device, faces=None):
        self.img_size = render._square(img_size)
        self.device = device
        self.faces_left, self.faces_right = _two_tables(faces)
        self._joined = {}                                        # V_left -> cat(left, right + V_left), topology cached on it
        self.build_camera = render.Renderer(self.img_size, device).build_camera

    def _faces(self, V_left):
        if V_left not in self._joined:
            if int(self.faces_left.max()) >= V_left:            # the joined table would reach into the right hand
                raise ValueError('renderih_amd.render: face index %d out of range for %d vertices'
                                 % (int(self.faces_left.max()), V_left))
            self._joined[V_left] = torch.cat((self.faces_left, self.faces_right + V_left), 0)
        return self._joined[V_left]

    def __call__(self, v3d_left, v3d_right, cameras=None, scale=None, trans2d=None, return_masks=False, out=None):
        """-> (iou [B], counts [B, 3]) and, with return_masks, the uint8 [B, S, S] mask (bit 0 left, bit 1 right).
        `out` = (iou, counts) or (iou, counts, mask): buffers to write into instead of fresh ones.  For a captured graph give
        `out` and, as `cameras`, a `render.Camera` built beforehand (`build_camera` copies constants from the host); its
        `params` are then a static buffer like the vertices."""
        _check_hands(v3d_left, v3d_right)
        S = self.img_size
        camera = cameras if isinstance(cameras, render.Camera) else self.build_camera(cameras, scale, trans2d)
        with torch.no_grad():
            verts = torch.cat((v3d_left.to(self.device), v3d_right.to(self.device)), 1)
            if verts.dtype != torch.float32:
                raise ValueError('the fused IoU is fp32 only; got %s' % verts.dtype)
            verts, topo, B, V = render._prepare(verts, self._faces(v3d_left.shape[1]), camera)
            F = topo[0].shape[0]
            rec, _ = render._setup(verts, topo, camera, B, V)
            if out is None:
                iou = torch.empty((B,), device=verts.device, dtype=torch.float32)
                counts = torch.empty((B, 3), device=verts.device, dtype=torch.int32)
                mask = torch.empty((B, S, S), device=verts.device, dtype=torch.uint8) if return_masks else None
            else:
                iou, counts = out[0], out[1]
                mask = out[2] if return_masks else None
                ops._chk(iou)
                ops._chk(counts, dtype=torch.int32)
                ops._chk(mask, dtype=torch.uint8)
                if tuple(iou.shape) != (B,) or tuple(counts.shape) != (B, 3) or not (iou.is_contiguous() and
                                                                                      counts.is_contiguous()) or \
                        (mask is not None and (tuple(mask.shape) != (B, S, S) or not mask.is_contiguous())):
                    raise ValueError('renderih_amd.mask_iou: out must be contiguous iou [%d], counts [%d, 3] and mask '
                                     '[%d, %d, %d]' % (B, B, B, S, S))
            check(ops._L().rih_mask_iou(rec.data_ptr(), B, F, self.faces_left.shape[0], S, S, camera.kind, counts.data_ptr(),
                                        iou.data_ptr(), ops._p(mask), ops._stream()), 'rih_mask_iou')
        return (iou, counts, mask) if return_masks else (iou, counts)


def iou_bins(iou, edges=(0.33, 0.67)):
    """The three masks of eval_interhand.py:232-234: iou < lo, lo <= iou < hi, iou >= hi (numpy bool [N] each)."""
    iou = np.asarray(iou.detach().cpu() if torch.is_tensor(iou) else iou)
    lo, hi = edges
    if iou.ndim != 1 or not lo <= hi:
        raise ValueError('iou must be [N] and the edges ascending; got %s and %r' % (iou.shape, (lo, hi)))
    return iou < lo, np.logical_and(iou < hi, iou >= lo), iou >= hi


def _field(annos, pick, shape):
    return torch.from_numpy(np.stack([np.asarray(pick(a), np.float32).reshape(shape) for a in annos]))


def scan_annotations(annos, mano_left, mano_right, img_size=256, batch_size=256, device='cuda', faces=None):
    """The scan of `render_data` (compute_maskiou.py:233-275) in batches: `annos` is an iterable of its annotation dicts
    (`mano_params[side] = {R [1,3,3], pose [1,ncomps], shape [1,10], trans [1,3]}`, `camera = {R [3,3], t [3], camera [3,3]}`),
    `mano_left` / `mano_right` the two `ManoLayer`s (center_idx=None in the reference; its `fix_shape` is the caller's to
    apply).  Per batch: the two MANO forwards, v @ R.T + t, the perspective camera from K, the fused IoU, ONE copy to the
    host.  -> float64 numpy [N] in the order of `annos`, what the reference `np.save`s."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError('batch_size must be at least 1; got %r' % (batch_size,))
    fused = FusedTwoHandMaskIoU(img_size, device, faces)
    layers = {'left': mano_left, 'right': mano_right}
    out, batch = [], []

    def flush():
        R = _field(batch, lambda a: a['camera']['R'], (3, 3)).to(device)
        t = _field(batch, lambda a: a['camera']['t'], (1, 3)).to(device)
        K = _field(batch, lambda a: a['camera']['camera'], (3, 3)).to(device)
        verts = []
        for side in ('left', 'right'):
            p = [a['mano_params'][side] for a in batch]
            v, _ = layers[side](_field(p, lambda q: q['R'], (3, 3)).to(device), _field(p, lambda q: q['pose'], (-1,)).to(device),
                                _field(p, lambda q: q['shape'], (-1,)).to(device),
                                trans=_field(p, lambda q: q['trans'], (3,)).to(device))
            verts.append(v.detach() @ R.transpose(1, 2) + t)
        iou, _ = fused(verts[0], verts[1], cameras=K)
        out.append(iou.cpu().numpy().astype(np.float64))
        del batch[:]

    with torch.no_grad():
        for a in annos:
            batch.append(a)
            if len(batch) == batch_size:
                flush()
        if batch:
            flush()
    return np.concatenate(out) if out else np.zeros((0,), np.float64)
