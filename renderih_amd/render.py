"""Two-hand mesh renderer -- drop-in for the reference's utils/vis_utils.py:39-289 (copies in common/vis_utils.py and
common/myhand/utils/vis_utils.py), which builds it on pytorch3d 0.7.2.  pytorch3d has no ROCm build; here the rasteriser and
the shader are the HIP kernels of csrc/rih_render.hip (setup, raster, shade), forward only.

Semantics (pytorch3d 0.7.2 MeshRasterizer with blur_radius 0 and faces_per_pixel 1, HardPhongShader, TexturesVertex,
hard_rgb_blend), as implemented here and restated in numpy by tests/render_oracle.py:

Screen space
  * world -> view is X R + T (row vectors).  Orthographic: x_ndc = f_x x_v + p_x, y_ndc = f_y y_v + p_y.  Perspective:
    x_ndc = f_x x_v / z_v + p_x, y_ndc = f_y y_v / z_v + p_y.  Depth is always the view z_v.
  * pixel (row r, column c) of an S x S image has its centre at x_ndc = 1 - (2c+1)/S, y_ndc = 1 - (2r+1)/S (+X left, +Y up,
    row 0 at the top).
Coverage
  * area = (x2 - x0)(y1 - y0) - (y2 - y0)(x1 - x0) in NDC; faces with |area| < 1e-8 are skipped.  Screen barycentrics are the
    2-D edge functions times 1/(area + 1e-8): w0 = e(p; v1, v2), w1 = e(p; v2, v0), w2 = e(p; v0, v1) with
    e(p; a, b) = (p.x - a.x)(b.y - a.y) - (p.y - a.y)(b.x - a.x).
  * a pixel is covered when w0, w1, w2 >= 0 (signed distance <= blur radius 0, no back-face culling).
  * perspective: faces with a vertex at z_v <= 0 are skipped; w'_i = (w_i z_j z_k) / max(sum, 1e-8), i.e. w_i / z_i
    normalised.  zbuf = sum w'_i z_i (w_i under the orthographic camera); a pixel whose zbuf is < 0 is behind the image
    plane and not covered.
  * the nearest face wins; ties of z go to the lower face index (the minimum of (z, face) compared lexicographically).
  * fragments: pix_to_face int32 [B, S, S] = b F + f or -1, zbuf [B, S, S] or -1, bary [B, S, S, 3] or -1.
Shading
  * colours, normals and world points are interpolated with the (corrected) barycentrics; colours as
    c0 + w1 (c1 - c0) + w2 (c2 - c0), so that a face of one colour shades to exactly that colour (pytorch3d's sum w_i c_i
    differs by (1 - sum w_i) c0, a few 1e-6 of the colour, from the 1e-8 in the barycentrics' denominator).  Vertex normals are
    Meshes.verts_normals: the sum over incident faces of the corner cross product (p1 - p0) x (p2 - p0) (p0 the vertex, p1 p2
    the next two corners of the face in order), normalised with eps 1e-6.
  * PointLights at (0, 0, -1): ambient 0.5, diffuse 0.3, specular 0.2; Materials 1, shininess 64.  The camera centre is
    -T R^T.  n, l (towards the light) and v (towards the camera) are normalised with eps 1e-6.  Diffuse 0.3 relu(n.l);
    specular 0.2 (relu(v.r) [n.l > 0])^64 with r = -l + 2 (n.l) n.  Colour = (0.5 + diffuse) texel + specular.
  * AmbientLights: colour = texel.
  * hard_rgb_blend: background (1, 1, 1) with alpha 0, covered pixels alpha 1.  RGBA fp32 [B, S, S, 4].

The reference's Renderer / mano_renderer / mano_two_hands_renderer come with the same constructors, methods and return shapes;
their quirks are kept (left faces = right faces [..., [1, 0, 2]], two-hand faces = cat(left, right + 778), render_single_* on
the first 1538 faces, default colours (204, 153, 0) / (102, 102, 255), render_rgb_orth maps the right hand into the left hand's
camera, RGB divided by 255 after blending so the background is 1/255).  Refused with a clear error: UV textures, `lights`
objects, non-square images (pytorch3d's non-square NDC convention is not pinned).
"""
import os
import pickle
import sys
from collections import namedtuple

import numpy as np
import torch

from . import assets, ops
from .ops import check

ORTHOGRAPHIC, PERSPECTIVE = 0, 1           # RIH_CAM_*
_LIGHT_KIND = {'point': 0, 'ambient': 1}   # RIH_LIGHT_*
REC_FLOATS = 16                            # floats per face record of rih_render_setup
NV_HAND = 778
NF_HAND = 1538

Fragments = namedtuple('Fragments', ['pix_to_face', 'zbuf', 'bary'])


class Camera:
    """params [B, 16] fp32 on the device = R (3x3 row-major), T (3), focal (2), principal point (2); kind ORTHOGRAPHIC or
    PERSPECTIVE.  Batch-varying parameters stay on the device: building one never syncs."""

    def __init__(self, params, kind):
        if kind not in (ORTHOGRAPHIC, PERSPECTIVE):
            raise ValueError('camera kind must be ORTHOGRAPHIC or PERSPECTIVE')
        self.params, self.kind = params.detach().float().contiguous(), kind


def orthographic_camera(scale, trans2d):
    """Renderer.build_camera(scale=, trans2d=) (vis_utils.py:60-72): focal 2 scale, principal point -trans2d,
    R = diag(-1, -1, 1), T = (0, 0, 10)."""
    scale, trans2d = torch.as_tensor(scale).detach().float(), torch.as_tensor(trans2d).detach().float()
    B = scale.shape[0]
    f = (2 * scale).reshape(B, -1).expand(B, 2)
    fixed = torch.tensor([-1., 0., 0., 0., -1., 0., 0., 0., 1., 0., 0., 10.], device=scale.device).expand(B, 12)
    return Camera(torch.cat([fixed, f, -trans2d.reshape(B, 2).to(scale.device)], 1), ORTHOGRAPHIC)


def perspective_camera(K, image_size):
    """Renderer.build_camera(cameras=K) (vis_utils.py:73-80) from a [B, 3, 3] intrinsics batch in pixels:
    f = -(fx, fy) 2/S, principal point = -(cx, cy) 2/S + 1, R = I, T = 0."""
    S = _square(image_size)
    K = torch.as_tensor(K).detach().float()
    B = K.shape[0]
    f = -torch.stack((K[:, 0, 0], K[:, 1, 1]), -1) * 2 / S
    pp = -K[:, :2, 2] * 2 / S + 1
    fixed = torch.tensor([1., 0., 0., 0., 1., 0., 0., 0., 1., 0., 0., 0.], device=K.device).expand(B, 12)
    return Camera(torch.cat([fixed, f, pp], 1), PERSPECTIVE)


def _square(image_size):
    if isinstance(image_size, torch.Tensor):
        image_size = tuple(int(s) for s in image_size.reshape(-1).tolist())
    if isinstance(image_size, (tuple, list)):
        if len(image_size) != 2 or int(image_size[0]) != int(image_size[1]):
            raise ValueError('renderih_amd.render: only square images are supported (got %r)' % (image_size,))
        image_size = image_size[0]
    S = int(image_size)
    if not 1 <= S <= 4096:
        raise ValueError('renderih_amd.render: image size must be in [1, 4096] (got %d)' % S)
    return S


def _topology(faces, device):
    """(faces int32 [F, 3], vertex -> (face, corner) CSR ptr / list int32, number of vertices the faces need) on `device`.
    Built once per face tensor -- where the indices are checked -- and cached on the tensor itself."""
    faces = torch.as_tensor(faces)
    if faces.dim() == 3:
        faces = faces[0]
    key = (faces._version, str(device), tuple(faces.shape))
    cached = getattr(faces, '_rih_topology', None)
    if cached is not None and cached[0] == key:
        return cached[1]
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError('renderih_amd.render: faces must be [F, 3] with F >= 1 (got %s)' % (tuple(faces.shape),))
    f = faces.detach().to('cpu', torch.int64).numpy().reshape(-1)
    if f.min() < 0 or f.max() >= 2 ** 31 - 1:
        raise ValueError('renderih_amd.render: face index out of range')
    nv = int(f.max()) + 1
    order = np.argsort(f, kind='stable')          # per vertex: ascending (face, corner) = entry 3 f + corner
    ptr = np.concatenate([[0], np.cumsum(np.bincount(f, minlength=nv))])

    def i32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(device)
    topo = (i32(f.reshape(-1, 3)), i32(ptr), i32(order), nv)
    try:
        faces._rih_topology = (key, topo)
    except (AttributeError, RuntimeError):
        pass
    return topo


def _prepare(verts, faces, camera):
    if not isinstance(camera, Camera):
        raise TypeError('renderih_amd.render: camera must be a render.Camera (orthographic_camera / perspective_camera)')
    ops._chk(verts, camera.params)
    verts = verts.detach().contiguous()
    topo = _topology(faces, verts.device)
    B, V = verts.shape[0], verts.shape[1]
    if verts.dim() != 3 or verts.shape[2] != 3:
        raise ValueError('renderih_amd.render: verts must be [B, V, 3]')
    if topo[3] > V:
        raise ValueError('renderih_amd.render: face index %d out of range for %d vertices' % (topo[3] - 1, V))
    if camera.params.shape != (B, 16):
        raise ValueError('renderih_amd.render: camera batch %s does not match %d meshes' % (tuple(camera.params.shape), B))
    return verts, topo, B, V


def _setup(verts, topo, camera, B, V, records=True, normals=False):
    F = topo[0].shape[0]
    rec = torch.empty((B, F, REC_FLOATS), device=verts.device, dtype=torch.float32) if records else None
    vn = torch.empty((B, V, 3), device=verts.device, dtype=torch.float32) if normals else None
    check(ops._L().rih_render_setup(verts.data_ptr(), topo[0].data_ptr(), topo[1].data_ptr(), topo[2].data_ptr(),
                                    camera.params.data_ptr(), camera.kind, B, V, topo[3], F, ops._p(rec), ops._p(vn),
                                    ops._stream()), 'rih_render_setup')
    return rec, vn


def _raster(rec, B, F, S, kind, device):
    p2f = torch.empty((B, S, S), device=device, dtype=torch.int32)
    zbuf = torch.empty((B, S, S), device=device, dtype=torch.float32)
    bary = torch.empty((B, S, S, 3), device=device, dtype=torch.float32)
    check(ops._L().rih_render_raster(rec.data_ptr(), B, F, S, S, kind, p2f.data_ptr(), zbuf.data_ptr(), bary.data_ptr(),
                                     ops._stream()), 'rih_render_raster')
    return Fragments(p2f, zbuf, bary)


def _shade(frags, verts, topo, vn, colors, light, camera, B, V):
    S = frags.pix_to_face.shape[1]
    colors = torch.as_tensor(colors).detach().to(device=verts.device, dtype=torch.float32).expand(B, V, 3).contiguous()
    rgba = torch.empty((B, S, S, 4), device=verts.device, dtype=torch.float32)
    check(ops._L().rih_render_shade(frags.pix_to_face.data_ptr(), frags.bary.data_ptr(), verts.data_ptr(),
                                    topo[0].data_ptr(), ops._p(vn), colors.data_ptr(), camera.params.data_ptr(),
                                    _LIGHT_KIND[light], B, V, topo[0].shape[0], S, S, rgba.data_ptr(), ops._stream()),
          'rih_render_shade')
    return rgba


def _light(lights):
    if lights not in _LIGHT_KIND:
        raise ValueError("renderih_amd.render: lights must be 'point' or 'ambient' (got %r)" % (lights,))
    return lights


def rasterize(verts, faces, camera, image_size):
    """verts [B, V, 3] world space, faces [F, 3] (shared by the batch), camera a Camera -> Fragments(pix_to_face int32
    [B, S, S], zbuf [B, S, S], bary [B, S, S, 3])."""
    S = _square(image_size)
    with torch.no_grad():
        verts, topo, B, V = _prepare(verts, faces, camera)
        rec, _ = _setup(verts, topo, camera, B, V)
        return _raster(rec, B, topo[0].shape[0], S, camera.kind, verts.device)


def shade(fragments, verts, faces, vertex_colors, lights='point', camera=None):
    """RGBA [B, S, S, 4] of hard_rgb_blend over the fragments of `rasterize`: lights 'point' (HardPhongShader with the
    default PointLights, needs the camera) or 'ambient' (AmbientLights); vertex_colors broadcastable to [B, V, 3]."""
    _light(lights)
    if camera is None:
        if lights == 'point':
            raise ValueError('renderih_amd.render.shade: point lighting needs the camera')
        camera = Camera(torch.zeros((verts.shape[0], 16), device=verts.device), ORTHOGRAPHIC)
    with torch.no_grad():
        verts, topo, B, V = _prepare(verts, faces, camera)
        ops._chk(fragments.bary)
        ops._chk(fragments.pix_to_face, dtype=torch.int32)
        S = fragments.pix_to_face.shape[1]
        if tuple(fragments.pix_to_face.shape) != (B, S, S) or tuple(fragments.bary.shape) != (B, S, S, 3) or \
                not (fragments.pix_to_face.is_contiguous() and fragments.bary.is_contiguous()):
            raise ValueError('renderih_amd.render.shade: fragments do not match %d meshes (use rasterize)' % B)
        vn = _setup(verts, topo, camera, B, V, records=False, normals=True)[1] if lights == 'point' else None
        return _shade(fragments, verts, topo, vn, vertex_colors, lights, camera, B, V)


def render_mesh(verts, faces, camera, image_size, vertex_colors, lights='point'):
    """rasterize + shade with one setup launch: RGBA [B, S, S, 4]."""
    S = _square(image_size)
    _light(lights)
    with torch.no_grad():
        verts, topo, B, V = _prepare(verts, faces, camera)
        rec, vn = _setup(verts, topo, camera, B, V, normals=lights == 'point')
        frags = _raster(rec, B, topo[0].shape[0], S, camera.kind, verts.device)
        return _shade(frags, verts, topo, vn, vertex_colors, lights, camera, B, V)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's classes (utils/vis_utils.py:39-289)

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_root():
    """The reference checkout behind this repository on sys.path (where its utils/manoutils.py lies), found without importing
    it (utils.manoutils needs cv2 and yacs)."""
    for p in sys.path:
        d = os.path.abspath(p or '.')
        if d != _REPO and os.path.isfile(os.path.join(d, 'utils', 'manoutils.py')):
            return d
    return None


def _default_mano_path():
    """get_mano_path() (utils/manoutils.py:68-74, MISC.MANO_PATH = misc/mano) when those files exist, else None."""
    root = _reference_root()
    if root is None:
        return None
    p = {s: os.path.join(root, 'misc', 'mano', 'MANO_%s.pkl' % s.upper()) for s in ('left', 'right')}
    return p if all(os.path.isfile(v) for v in p.values()) else None


def _default_dense_path():
    """get_dense_color_path() (utils/manoutils.py:85-89, MISC.DENSE_COLOR = misc/v_color.pkl) when it exists, else None."""
    root = _reference_root()
    p = None if root is None else os.path.join(root, 'misc', 'v_color.pkl')
    return p if p is not None and os.path.isfile(p) else None


def _mano_faces(path, side):
    if isinstance(path, dict):
        path = path[side]
    if path is not None and os.path.isfile(path):
        with open(path, 'rb') as fh:
            return np.asarray(pickle.load(fh, encoding='latin1')['f']).astype(np.int64)
    return assets.hand_faces(side)


def _dense_coor(dense_path):
    if dense_path is not None and os.path.isfile(dense_path):
        with open(dense_path, 'rb') as fh:
            return torch.from_numpy(np.asarray(pickle.load(fh), dtype=np.float32)) * 255
    return torch.from_numpy(assets.synthetic_dense_coor()) * 255


class Renderer():
    def __init__(self, img_size, device='cpu'):
        self.img_size = _square(img_size)
        self.device = device

    def build_camera(self, cameras=None, scale=None, trans2d=None):
        if scale is not None and trans2d is not None:
            return orthographic_camera(torch.as_tensor(scale).to(self.device), torch.as_tensor(trans2d).to(self.device))
        if cameras is not None:
            return perspective_camera(torch.as_tensor(cameras).to(self.device), self.img_size)
        raise ValueError('renderih_amd.render: give scale and trans2d (orthographic) or cameras [B, 3, 3] (perspective)')

    def build_texture(self, uv_verts=None, uv_faces=None, texture=None, v_color=None):
        if uv_verts is not None or uv_faces is not None or texture is not None:
            raise NotImplementedError('renderih_amd.render: UV textures (TexturesUV) are not supported; give vertex colours')
        if v_color is not None:
            return torch.as_tensor(v_color).to(self.device)

    def render(self, verts, faces, cameras, textures, amblights=False, lights=None):
        """verts [B, V, 3], faces [F, 3] or [B, F, 3] (the same for every image), cameras from build_camera, textures the
        vertex colours [B, V, 3] -> (img [B, S, S, 3] = RGB / 255, alpha [B, S, S])."""
        if lights is not None:
            raise NotImplementedError('renderih_amd.render: only the default PointLights (lights=None) or amblights=True')
        rgba = render_mesh(verts.to(self.device), faces, cameras, self.img_size, textures,
                           'ambient' if amblights else 'point')
        return rgba[..., :3] / 255, rgba[..., 3]


class mano_renderer(Renderer):
    def __init__(self, mano_path=None, dense_path=None, img_size=224, device='cpu'):
        super(mano_renderer, self).__init__(img_size, device)
        if mano_path is None:
            mano_path = _default_mano_path()
            mano_path = None if mano_path is None else mano_path['right']
        if dense_path is None:
            dense_path = _default_dense_path()
        self.mano_path = mano_path
        self._mano = None
        self.faces_np = _mano_faces(mano_path, 'right')
        self.faces = torch.from_numpy(self.faces_np).to(self.device).unsqueeze(0)
        self._faces = self.faces[0].contiguous()
        self.dense_coor = _dense_coor(dense_path)

    @property
    def mano(self):
        if self._mano is None:
            if self.mano_path is None or not os.path.isfile(self.mano_path):
                raise RuntimeError('renderih_amd.render: no MANO model file; pass v3d')
            from .manolayer import ManoLayer
            self._mano = ManoLayer(self.mano_path, center_idx=9, use_pca=True).to(self.device)
        return self._mano

    def render_rgb(self, cameras=None, scale=None, trans2d=None, R=None, pose=None, shape=None, trans=None, v3d=None,
                   uv_verts=None, uv_faces=None, texture=None, v_color=(255, 255, 255), amblights=False):
        if v3d is None:
            v3d, _ = self.mano(R, pose, shape, trans=trans)
        bs, vNum = v3d.shape[0], v3d.shape[1]
        if not isinstance(v_color, torch.Tensor):
            v_color = torch.tensor(v_color)
        v_color = v_color.expand(bs, vNum, 3).to(v3d)
        return self.render(v3d, self._faces, self.build_camera(cameras, scale, trans2d),
                           self.build_texture(uv_verts, uv_faces, texture, v_color), amblights)

    def render_densepose(self, cameras=None, scale=None, trans2d=None, R=None, pose=None, shape=None, trans=None, v3d=None):
        if v3d is None:
            v3d, _ = self.mano(R, pose, shape, trans=trans)
        bs, vNum = v3d.shape[0], v3d.shape[1]
        return self.render(v3d, self._faces, self.build_camera(cameras, scale, trans2d),
                           self.build_texture(v_color=self.dense_coor.expand(bs, vNum, 3).to(v3d)), True)


class mano_two_hands_renderer(Renderer):
    def __init__(self, mano_path=None, dense_path=None, img_size=224, device='cpu'):
        super(mano_two_hands_renderer, self).__init__(img_size, device)
        if mano_path is None:
            mano_path = _default_mano_path()
        if dense_path is None:
            dense_path = _default_dense_path()
        right_faces = torch.from_numpy(_mano_faces(mano_path, 'right')).to(self.device).unsqueeze(0)
        left_faces = right_faces[..., [1, 0, 2]]
        self.faces = torch.cat((left_faces, right_faces + NV_HAND), dim=1)
        self._faces = self.faces[0].contiguous()                 # the topology (CSR) is cached on these two
        self._faces_single = self._faces[:NF_HAND].contiguous()
        self.dense_coor = _dense_coor(dense_path)

    @staticmethod
    def _default_colors():
        v_color = torch.zeros((NV_HAND * 2, 3))
        v_color[:NV_HAND] = torch.tensor([204., 153., 0.])
        v_color[NV_HAND:] = torch.tensor([102., 102., 255.])
        return v_color

    def render_rgb(self, cameras=None, scale=None, trans2d=None, v3d_left=None, v3d_right=None, uv_verts=None, uv_faces=None,
                   texture=None, v_color=None, amblights=False, lights=None):
        bs, vNum = v3d_left.shape[0], v3d_left.shape[1]
        if v_color is None:
            v_color = self._default_colors()
        if not isinstance(v_color, torch.Tensor):
            v_color = torch.tensor(v_color)
        v_color = v_color.expand(bs, 2 * vNum, 3).float().to(self.device)
        v3d = torch.cat((v3d_left, v3d_right), dim=1)
        return self.render(v3d, self._faces, self.build_camera(cameras, scale, trans2d),
                           self.build_texture(uv_verts, uv_faces, texture, v_color), amblights, lights)

    def render_rgb_orth(self, scale_left=None, trans2d_left=None, scale_right=None, trans2d_right=None, v3d_left=None,
                        v3d_right=None, uv_verts=None, uv_faces=None, texture=None, v_color=None, amblights=False):
        # the right hand in the left hand's camera (vis_utils.py:206-228)
        s = (scale_right / scale_left).unsqueeze(-1).unsqueeze(-1)
        d = (-(trans2d_left - trans2d_right) / 2 / scale_left.unsqueeze(-1)).unsqueeze(1)
        v3d_right = s * v3d_right
        v3d_right[..., :2] = v3d_right[..., :2] + d
        return self.render_rgb(None, scale=scale_left, trans2d=trans2d_left, v3d_left=v3d_left, v3d_right=v3d_right,
                               uv_verts=uv_verts, uv_faces=uv_faces, texture=texture, v_color=v_color, amblights=amblights)

    def render_mask(self, cameras=None, scale=None, trans2d=None, v3d_left=None, v3d_right=None):
        v_color = torch.zeros((NV_HAND * 2, 3))
        v_color[:NV_HAND, 2] = 255
        v_color[NV_HAND:, 1] = 255
        rgb, mask = self.render_rgb(cameras, scale, trans2d, v3d_left, v3d_right, v_color=v_color, amblights=True)
        return rgb

    def render_single_rgb(self, cameras=None, scale=None, trans2d=None, v3d_left=None, v3d_right=None, uv_verts=None,
                          uv_faces=None, texture=None, v_color=None, amblights=False, lights=None):
        bs, vNum = v3d_left.shape[0], v3d_left.shape[1]
        if v_color is None:
            v_color = torch.ones((NV_HAND, 3))
        if not isinstance(v_color, torch.Tensor):
            v_color = torch.tensor(v_color)
        v_color = v_color.expand(bs, vNum, 3).float().to(self.device)
        return self.render(v3d_left, self._faces_single, self.build_camera(cameras, scale, trans2d),
                           self.build_texture(uv_verts, uv_faces, texture, v_color), amblights, lights)

    def render_single_mask(self, cameras=None, scale=None, trans2d=None, v3d=None):
        v_color = torch.ones((NV_HAND, 3)) * 255
        rgb, mask = self.render_single_rgb(cameras, scale, trans2d, v3d, v_color=v_color, amblights=True)
        return rgb

    def render_densepose(self, cameras=None, scale=None, trans2d=None, v3d_left=None, v3d_right=None):
        bs, vNum = v3d_left.shape[0], v3d_left.shape[1]
        v3d = torch.cat((v3d_left, v3d_right), dim=1)
        v_color = torch.cat((self.dense_coor, self.dense_coor), dim=0)
        return self.render(v3d, self._faces, self.build_camera(cameras, scale, trans2d),
                           self.build_texture(v_color=v_color.expand(bs, 2 * vNum, 3).to(v3d_left)), True)
