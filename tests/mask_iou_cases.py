"""TEST INFRASTRUCTURE: scenes and checks of the two-hand silhouette IoU (renderih_amd/mask_iou.py, rih_mask_iou of
csrc/rih_render.hip), shared by tests/test_mask_iou.py (the CPU, through the host-compiled kernels) and
tests/test_gpu_mask_iou.py (the GPU).  The scenes are those of tests/render_cases.py; the two references are the project's
own rasteriser run per hand on the same device (exact: no pixel left out, no tolerance) and tests/render_oracle.py."""
import functools

import numpy as np
import torch

import render_cases as rc
import render_oracle as ro
from renderih_amd import assets, mask_iou, render

FACES = assets.hand_faces('right')            # one table for both hands, the default of both classes
SCENES = ('orth', 'orth_overlap', 'persp', 'persp_overlap')
UNDECIDED_CAP = 0.005                         # the bar of the renderer tests


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def scene(name, S, B=3):
    """-> (v3d_left, v3d_right [B, 778, 3] numpy in the ONE camera both are rendered with, camera dict of numpy arrays:
    {'scale', 'trans2d'} or {'cameras'})."""
    if name.startswith('orth'):
        vl, vr, sl, tl, sr, tr = rc.ortho_scene(B, seed=S, overlap=name == 'orth_overlap')
        return vl, rc.right_in_left_camera(vr, sl, tl, sr, tr), {'scale': sl, 'trans2d': tl}
    vl, vr, K = rc.persp_scene(B, S, seed=S)
    if name == 'persp_overlap':
        vr = vr + np.array([-0.10, 0.0, -0.03], np.float32)
    elif name == 'persp_high':
        vr = vl + np.array([0.002, 0.0, 0.0], np.float32)
    elif name == 'persp_mid':
        vr = vl + np.array([0.02, 0.0, 0.0], np.float32)
    else:
        assert name == 'persp', name
    return vl, vr.astype(np.float32), {'cameras': K}


def cam_kw(cam, dev):
    return {k: t(v, dev) for k, v in cam.items()}


def run_fused(S, dev, vl, vr, cam, faces=None, **kw):
    fused = mask_iou.FusedTwoHandMaskIoU(S, dev, faces)
    return fused(t(vl, dev), t(vr, dev), return_masks=True, **cam_kw(cam, dev), **kw)


def by_rasterize(S, dev, vl, vr, cam, faces_left=FACES, faces_right=FACES):
    """(counts [B, 3], mask [B, S, S] uint8) from `render.rasterize` of each hand's faces alone: pix_to_face >= 0."""
    camera = render.Renderer(S, dev).build_camera(**cam_kw(cam, dev))
    hit = [(render.rasterize(t(v, dev), torch.from_numpy(np.asarray(f)), camera, S).pix_to_face >= 0).cpu().numpy()
           for v, f in ((vl, faces_left), (vr, faces_right))]
    return counts_of(hit[0], hit[1]), hit[0].astype(np.uint8) | (hit[1].astype(np.uint8) << 1)


def counts_of(left, right):
    return np.stack([left.sum((1, 2)), right.sum((1, 2)), (left & right).sum((1, 2))], 1).astype(np.int32)


def check_exact(S, dev, vl, vr, cam, faces=None, faces_left=FACES, faces_right=FACES):
    """Bar 1: counts and mask equal the rasteriser's, every pixel, and the IoU is the fp32 quotient of the counts."""
    iou, counts, mask = run_fused(S, dev, vl, vr, cam, faces)
    want_counts, want_mask = by_rasterize(S, dev, vl, vr, cam, faces_left, faces_right)
    counts, mask, iou = counts.cpu().numpy(), mask.cpu().numpy(), iou.cpu().numpy()
    assert counts.dtype == np.int32 and mask.dtype == np.uint8 and iou.dtype == np.float32
    assert (mask == want_mask).all(), 'mask differs from the rasteriser on %d pixels' % (mask != want_mask).sum()
    assert (counts == want_counts).all(), (counts.tolist(), want_counts.tolist())
    assert (counts == counts_of(mask & 1 > 0, mask & 2 > 0)).all()
    check_ratio(iou, counts)
    return iou, counts, mask


def check_ratio(iou, counts):
    inter, union = counts[:, 2], counts[:, 0] + counts[:, 1] - counts[:, 2]
    with np.errstate(invalid='ignore', divide='ignore'):
        want = np.where(union > 0, inter.astype(np.float32) / union.astype(np.float32), np.float32(0))
    assert (iou == want).all(), (iou.tolist(), want.tolist())
    some = union > 0
    bm0 = inter[some].astype(np.float64) / union[some].astype(np.float64)        # the reference's quotient, in fp64
    assert np.allclose(iou[some], bm0, rtol=1.2e-7, atol=0)                      # one fp32 rounding


@functools.lru_cache(maxsize=None)
def oracle(name, S, B=3):
    """The numpy oracle per hand on `scene(name, S, B)`: (mask [B, S, S] uint8, undecided [B, S, S] bool = within
    render_cases.MARGIN of an edge of a face of either hand)."""
    vl, vr, cam = scene(name, S, B)
    persp = 'cameras' in cam
    params = ro.perspective_params(cam['cameras'], S) if persp else ro.orthographic_params(cam['scale'], cam['trans2d'])
    o = [ro.rasterize(v, FACES, params, persp, S) for v in (vl, vr)]
    mask = (o[0]['pix_to_face'] >= 0).astype(np.uint8) | ((o[1]['pix_to_face'] >= 0).astype(np.uint8) << 1)
    return mask, (o[0]['margin'] < rc.MARGIN) | (o[1]['margin'] < rc.MARGIN)


def check_oracle(name, S, counts, mask, B=3):
    """Bar 2: the mask equals the oracle's on every decided pixel, each count is within the image's undecided pixels."""
    want, undecided = oracle(name, S, B)
    n_und = undecided.sum((1, 2))
    assert (n_und < UNDECIDED_CAP * S * S).all(), 'undecided pixels per image: %s of %d' % (n_und.tolist(), S * S)
    bad = (mask != want) & ~undecided
    assert not bad.any(), 'mask differs from the oracle on %d decided pixels (first %s)' % (bad.sum(), np.argwhere(bad)[:3])
    diff = np.abs(counts.astype(np.int64) - counts_of(want & 1 > 0, want & 2 > 0))
    assert (diff <= n_und[:, None]).all(), (diff.tolist(), n_und.tolist())
    return want


# --------------------------------------------------------------------------------------------------------- crafted meshes

ORTHO_UNIT = {'scale': np.array([0.5], np.float32), 'trans2d': np.zeros((1, 2), np.float32)}     # x_ndc = -x, y_ndc = -y


def rectangles(flip):
    """Two axis-aligned rectangles of two triangles each whose edges lie on pixel boundaries of a 16 x 16 image (as
    test_render.test_oracle_square_covers_predicted_pixels): NDC x in [-0.5, 0.5], y in [-0.25, 0.75] and x in [0, 0.75],
    y in [-0.5, 0.25].  -> (vl, vr [1, 4, 3], faces [2, 3], the two expected boolean masks [16, 16])."""
    ax = ro.pixel_centres(16)
    out, want = [], []
    for x0, x1, y0, y1 in ((-0.5, 0.5, -0.25, 0.75), (0.0, 0.75, -0.5, 0.25)):
        out.append(-np.array([[[x0, y0, -1], [x1, y0, -1], [x1, y1, -1], [x0, y1, -1]]], np.float32))
        want.append(((ax >= y0) & (ax <= y1))[:, None] & ((ax >= x0) & (ax <= x1))[None, :])
    faces = np.array([[0, 2, 1], [0, 3, 2]] if flip else [[0, 1, 2], [0, 2, 3]])
    return out[0], out[1], faces, want


def pixel_triangles(S, pixels):
    """One triangle per listed pixel (flat index into the S x S image) that holds that pixel's centre well inside and no other
    centre: (verts [1, 3 n, 3] with its own three vertices per face, faces [n, 3])."""
    ax = ro.pixel_centres(S).astype(np.float64)
    h = 1.0 / S
    pixels = np.asarray(pixels)
    cx, cy = ax[pixels % S], ax[pixels // S]
    tri = np.stack([np.stack([cx - 0.9 * h, cy - 0.6 * h], -1), np.stack([cx + 0.9 * h, cy - 0.6 * h], -1),
                    np.stack([cx, cy + 0.9 * h], -1)], 1)                                        # [n, 3, 2] in NDC
    v = np.concatenate([-tri, np.ones((len(pixels), 3, 1))], -1).reshape(1, -1, 3).astype(np.float32)
    return v, np.arange(3 * len(pixels)).reshape(-1, 3)


def split_case(S, F_left, F_right):
    """Left: F_left one-pixel triangles, right: F_right, on pixels scattered over every tile; the right hand starts half-way
    into the left hand's pixels.  -> (vl, vr, (faces_left, faces_right), expected counts [1, 3], expected mask [S, S])."""
    where = lambda i: (np.asarray(i) * 7) % (S * S)           # noqa: E731   7 and S*S coprime: distinct pixels
    assert np.gcd(7, S * S) == 1 and F_left // 2 + F_right <= S * S
    pl, pr = where(np.arange(F_left)), where(F_left // 2 + np.arange(F_right))
    vl, fl = pixel_triangles(S, pl)
    vr, fr = pixel_triangles(S, pr)
    mask = np.zeros(S * S, np.uint8)
    mask[pl] |= 1
    mask[pr] |= 2
    inter = min(F_left, F_left // 2 + F_right) - F_left // 2
    assert inter == (mask == 3).sum()
    return vl, vr, (fl, fr), np.array([[F_left, F_right, inter]], np.int32), mask.reshape(S, S)


# ------------------------------------------------------------------------------------------------------------ annotations

def synthetic_annotations(N, S=64, seed=0):
    """N dicts with the fields `render_data` (compute_maskiou.py:233-266) reads, shaped as `load_mano` (:141-154) writes
    them: both hands about half a metre in front of a camera that sees them."""
    rs = np.random.RandomState(seed)
    annos = []
    for _ in range(N):
        params = {}
        for side, x in (('left', -0.005), ('right', 0.005)):
            params[side] = {'R': rc._rodrigues(rs.randn(3) * 0.3)[None].astype(np.float32),
                            'pose': (rs.randn(1, 45) * 0.3).astype(np.float32),
                            'shape': (rs.randn(1, 10) * 0.5).astype(np.float32),
                            'trans': np.array([[x, 0.0, 0.0]], np.float32) + (rs.randn(1, 3) * 0.005).astype(np.float32)}
        K = np.array([[S * 1.2, 0, S / 2], [0, S * 1.2, S / 2], [0, 0, 1]], np.float64)
        annos.append({'mano_params': params,
                      'camera': {'R': rc._rodrigues(rs.randn(3) * 0.1).astype(np.float64),
                                 't': np.array([0.0, 0.0, 0.5]) + rs.randn(3) * 0.01, 'camera': K}})
    return annos


def scan_by_hand(annos, layers, S, dev):
    """The per-sample loop of `render_data` on the same layers and the fused class: one sample per call."""
    fused = mask_iou.FusedTwoHandMaskIoU(S, dev)
    out = []
    for a in annos:
        verts = []
        for side in ('left', 'right'):
            p = a['mano_params'][side]
            v, _ = layers[side](t(p['R'], dev).float(), t(p['pose'], dev).float(), t(p['shape'], dev).float(),
                                trans=t(p['trans'], dev).float())
            R, T = t(a['camera']['R'], dev).float(), t(a['camera']['t'], dev).float()
            verts.append(v @ R.T + T)
        iou, _ = fused(verts[0], verts[1], cameras=t(a['camera']['camera'], dev).float()[None])
        out.append(float(iou[0]))
    return np.array(out)
