#!/usr/bin/env python
"""Golden vectors of the auxiliary heads from the REFERENCE's own program: core/Loss.py `calc_aux_loss` on a `GraphLoss` (with
autograd gradients), dataset/heatmap.py `HeatmapGenerator` and dataset/inference.py `get_final_preds2`, imported from a
reference checkout at generation time and run unmodified on the CPU.

Imports: the stubs of make_golden.py (ref_stubs: yacs, torchvision, the checkout first on sys.path; misc/upsample.pkl, which
`GraphLoss.__init__` loads and the checkout does not hold, is replaced by the synthetic matrix as there).  dataset/inference.py
imports cv2, which is not installed: a stand-in module supplies `cv2.GaussianBlur(src, (k, k), 0)` as a numpy separable filter
(rows, then columns, BORDER_REFLECT_101 as OpenCV's default) with OpenCV's fixed taps for sigma = 0 -- 3: (1, 2, 1)/4,
5: (1, 4, 6, 4, 1)/16, 7: (1, 3.5, 7, 9, 7, 3.5, 1)/32.  THE BLUR TAPS OF THE FIXTURE ARE THEREFORE PINNED BY THIS STAND-IN, NOT
BY OPENCV.  (The reference pads the map by the kernel's radius with zeros and crops afterwards, so the border mode never
reaches the result.)

What is arranged around the reference's code, none of it an edit of it:
  * every input is fp32-representable and handed to the reference in fp64, so that the fixture is the fp64 result on exactly
    the numbers an fp32 kernel reads.  `HeatmapGenerator` returns float32 and `get_final_preds2` float32 coordinates
    (inference.py:39) whatever it is given; they are stored as they come.
  * `get_final_preds2` blurs its argument in place: it gets a copy.
  * the inputs come from tests/aux_heads_cases.py (`heatmap_joints`, `loss_inputs`, `decoder_maps`) and are stored beside the
    results.

Writes tests/golden/aux_heads.npz: hm<i>/joints, hm<i>/out for the heat-map cases FIXTURE_HEATMAP_CASES; loss/in/*, the four
terms loss/{total,mask,dense,hms}_loss, loss/grad_{mask,dense,hms} (d total / d prediction), loss/weights (MASK, DENSEPOSE, HMS
of utils/defaults.yaml), loss/beta (`hand_loss.smoothL1Loss.beta`) at (B, Jh, S) = (2, 42, 8); dec<H>x<W>/maps and, per kernel
1, 3, 5, 7, dec<H>x<W>/k<kernel>/preds, /maxvals for 14 maps of 8 x 8 and 8 x 12 and 6 of 64 x 64.
       python tests/golden/make_aux_heads_golden.py"""
import os
import pickle
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..'))

TAPS = {3: np.array([1, 2, 1]) / 4.0, 5: np.array([1, 4, 6, 4, 1]) / 16.0, 7: np.array([1, 3.5, 7, 9, 7, 3.5, 1]) / 32.0}


def gaussian_blur(src, ksize, sigma):
    assert sigma == 0 and ksize[0] == ksize[1] and ksize[0] in TAPS and src.ndim == 2
    k, r = TAPS[ksize[0]], ksize[0] // 2
    p = np.pad(np.asarray(src, np.float64), r, mode='reflect')
    H, W = src.shape
    rows = sum(k[j] * p[:, j:j + W] for j in range(len(k)))
    return sum(k[i] * rows[i:i + H] for i in range(len(k)))


def main():
    cv2 = types.ModuleType('cv2')
    cv2.GaussianBlur = gaussian_blur
    sys.modules['cv2'] = cv2
    import ref_stubs
    ref_stubs.install()
    sys.path.append(ROOT)
    from renderih_amd import assets
    import aux_heads_cases as cc
    import core.Loss as RefLoss
    import dataset.heatmap as ref_heatmap
    import dataset.inference as ref_inference
    from utils.config import load_cfg
    for m in (RefLoss, ref_heatmap, ref_inference):
        assert os.path.abspath(m.__file__).startswith(os.path.abspath(ref_stubs.REF) + os.sep), m.__file__
    store = {}

    # ---- heat maps
    for ci in cc.FIXTURE_HEATMAP_CASES:
        R, J, C, sigma, scale = cc.HEATMAP_CASES[ci]
        j = cc.heatmap_joints(R, J, C, 10 + ci)
        out = ref_heatmap.HeatmapGenerator(R, sigma)(j.copy(), scale)
        assert out.dtype == np.float32 and out.shape == (j.shape[0], J, R, R)
        assert (out.reshape(-1, R * R).max(1) == 0).any() and (out.reshape(-1, R * R).max(1) > 0).any()
        store['hm%d/joints' % ci], store['hm%d/out' % ci] = j, out

    # ---- loss
    tmp = tempfile.mkdtemp()
    up = os.path.join(tmp, 'upsample.pkl')
    with open(up, 'wb') as f:
        pickle.dump(assets.synthetic_upsample_weight(), f)
    RefLoss.get_upsample_path = lambda: up
    cfg = load_cfg(os.path.join(ref_stubs.REF, 'utils', 'defaults.yaml'))
    md = assets.synthetic_mano_dict('left')
    gl = RefLoss.GraphLoss(torch.from_numpy(np.asarray(md['J_regressor'].todense(), np.float32)), np.asarray(md['f']), level=4,
                           device='cpu')
    B, Jh, S = cc.FIXTURE_LOSS_SHAPE
    d = cc.loss_inputs(B, Jh, S)
    pred = {k: torch.from_numpy(d['p_' + k]).double().requires_grad_(True) for k in ('mask', 'dense', 'hms')}
    out = RefLoss.calc_aux_loss(cfg, gl, pred, torch.from_numpy(d['t_mask']), torch.from_numpy(d['t_dense']),
                                torch.from_numpy(d['t_hms']))
    assert set(out) == {'mask_loss', 'dense_loss', 'hms_loss', 'total_loss'}
    out['total_loss'].backward()
    for k, v in d.items():
        store['loss/in/' + k] = v
    for k, v in out.items():
        assert v.dtype == torch.float64
        store['loss/' + k] = np.float64(v.item())
    for k, v in pred.items():
        store['loss/grad_' + k] = v.grad.numpy().copy()
    aux = cfg.LOSS_WEIGHT.AUX
    store['loss/weights'] = np.array([aux.MASK, aux.DENSEPOSE, aux.HMS], np.float64)
    store['loss/beta'] = np.float64(gl.smoothL1Loss.beta)

    # ---- decoder
    for H, W in cc.DECODE_SIZES:
        n = 6 if H * W > 1024 else 14
        maps, kinds = cc.decoder_maps(H, W, n, 900 + H + W)
        maps = maps[None]
        store['dec%dx%d/maps' % (H, W)] = maps
        for kernel in cc.DECODE_KERNELS:
            with np.errstate(all='ignore'):                       # (the reference's rescale divides 0 by 0 on the all-zero map)
                preds, maxvals = ref_inference.get_final_preds2(maps.astype(np.float64).copy(), kernel)
            assert preds.dtype == np.float32 and np.isfinite(preds).all()
            store['dec%dx%d/k%d/preds' % (H, W, kernel)] = preds
            store['dec%dx%d/k%d/maxvals' % (H, W, kernel)] = maxvals
    path = os.path.join(HERE, 'aux_heads.npz')
    np.savez_compressed(path, **store)
    print('wrote', path, os.path.getsize(path), 'bytes,', len(store), 'arrays')


if __name__ == '__main__':
    main()
