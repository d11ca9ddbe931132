"""Generates tests/golden/demo/*.npz by executing the REFERENCE's own `InterRender.process_img`, `.render` and
`.render_other_view` (core/test_utils.py, /root/reference) as unbound functions on a stand-in `self` that carries only what
they read: input_size, render_size, img_processor, renderer.  Run in the build container only.

Import stubs (the packages are absent here): cv2 (copyMakeBorder with a constant border and cvtColor = exact index operations;
resize = the numpy restatement of the resize contract in tests/demo_cases.py -- so the resize arithmetic itself is not pinned by
these fixtures, everything around it is: pad, resize, swap, divide, normalise order, the blend's order, dtypes and truncation),
torchvision.transforms (Normalize = sub mean, div std, as torchvision does), utils.vis_utils (pytorch3d; the stand-in renderer
returns recorded arrays and records the vertices it is handed), Tensor.cuda (identity).
    python tests/golden/make_demo_golden.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, '..', '..'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, HERE)
import demo_cases as dc                    # noqa: E402
import ref_stubs                           # noqa: E402

REF = '/root/reference'
OUT = os.path.join(HERE, 'demo')


def install():
    ref_stubs.install()
    cv = sys.modules['cv2']
    cv.COLOR_BGR2RGB = 4
    cv.BORDER_CONSTANT = 0

    def copy_make_border(img, top, bottom, left, right, border_type, value=0):
        assert border_type == cv.BORDER_CONSTANT and not np.any(value)
        out = np.zeros((img.shape[0] + top + bottom, img.shape[1] + left + right) + img.shape[2:], img.dtype)
        out[top:top + img.shape[0], left:left + img.shape[1]] = img
        return out
    cv.copyMakeBorder = copy_make_border
    cv.resize = lambda img, dsize: dc.resize_u8(img, dsize[1], dsize[0])
    cv.cvtColor = lambda img, code: np.ascontiguousarray(img[..., ::-1])
    tr = types.ModuleType('torchvision.transforms')

    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = torch.tensor(mean).view(-1, 1, 1), torch.tensor(std).view(-1, 1, 1)

        def __call__(self, x):
            return (x - self.mean) / self.std
    tr.Normalize = Normalize
    sys.modules['torchvision'].transforms = tr
    sys.modules['torchvision.transforms'] = tr
    vis = types.ModuleType('utils.vis_utils')
    vis.mano_two_hands_renderer = object
    sys.modules['utils.vis_utils'] = vis
    torch.Tensor.cuda = lambda self, *a, **k: self
    sys.path.insert(0, REF)


class RecordedRenderer:
    def __init__(self, rgb, mask):
        self.rgb, self.mask, self.calls = torch.from_numpy(rgb), torch.from_numpy(mask), []

    def render_rgb_orth(self, **kw):
        self.calls.append({k: v.detach().numpy().copy() for k, v in kw.items()})
        return self.rgb, self.mask


def main():
    install()
    from core.test_utils import InterRender
    from torchvision.transforms import Normalize
    os.makedirs(OUT, exist_ok=True)
    S = 16
    me = types.SimpleNamespace(input_size=S, render_size=None, renderer=None,
                               img_processor=Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]))

    for (H, W) in dc.SHAPES16:                          # one small file per case
        img = dc.image(H, W)
        res = InterRender.process_img(me, img.copy())
        assert tuple(res.shape) == (1, 3, S, S) and res.dtype == torch.float32
        np.savez_compressed(os.path.join(OUT, 'process_img_%dx%d.npz' % (H, W)), img=img, out=res.numpy())

    params = {k: torch.zeros(1) for k in ('scale_left', 'trans2d_left', 'scale_right', 'trans2d_right', 'v3d_left', 'v3d_right')}
    for name, R, bg in (('white', 16, None), ('aniso', 16, dc.image(20, 12, 1)), ('box', 16, dc.image(32, 32, 2)),
                        ('up', 24, dc.image(9, 31, 4))):
        rgb, mask = dc.render_like(1, R, 40 + R + len(name))
        me.render_size, me.renderer = R, RecordedRenderer(rgb, mask)
        res = InterRender.render(me, params, None if bg is None else bg.copy())
        assert res.shape == (R, R, 3) and res.dtype == np.uint8
        out = {'rgb': rgb, 'mask': mask, 'out': res}
        if bg is not None:
            out['bg'] = bg
        np.savez_compressed(os.path.join(OUT, 'render_%s.npz' % name), **out)

    for name, V, theta in (('v5_t0', 5, 0), ('v5_t60', 5, 60), ('v40_t60', 40, 60)):
        vl, vr = dc.hands(1, V, 11 + V + theta)
        rgb, mask = dc.render_like(1, 16, 90 + V + theta)
        me.render_size, me.renderer = 16, RecordedRenderer(rgb, mask)
        res = InterRender.render_other_view(me, {'v3d_left': torch.from_numpy(vl), 'v3d_right': torch.from_numpy(vr)}, theta)
        call = me.renderer.calls[0]
        assert res.shape == (16, 16, 3) and res.dtype == np.uint8
        out = {k: call[k] for k in ('scale_left', 'scale_right', 'trans2d_left', 'trans2d_right')}
        out.update(vl=vl, vr=vr, theta=np.array(theta), verts=np.concatenate([call['v3d_left'], call['v3d_right']], 1),
                   rgb=rgb, mask=mask, out=res)
        np.savez_compressed(os.path.join(OUT, 'other_view_%s.npz' % name), **out)
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)), 'bytes')


if __name__ == '__main__':
    main()
