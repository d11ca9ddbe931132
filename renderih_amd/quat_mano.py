"""The pose optimiser's hand model: manopth's ManoLayer in quaternion mode and its AnchorLayer -- drop-ins for the reference's
pose_data_optimize/manopth/manopth/manolayer.py (as hocontact/postprocess/geo_optimizer_both_batch.py:54-79,539-575 builds and
calls it: joint_rot_mode = root_rot_mode = 'quat', use_pca=False, flat_hand_mean=True) and manopth/anchorlayer.py.

`QuatManoLayer` / `AnchorLayer` are plain-torch mirrors (CPU-capable, pinned to the reference by tests/golden/quat_mano.npz);
`FusedQuatManoLayer` / `FusedAnchorLayer` run the same computation on csrc/rih_mano.hip (rih_mano_quat_fwd: ONE launch,
rih_mano_quat_bwd: three) and csrc/rih_anchor.hip (one launch each way).  GPU fp32 only, no host read of device memory:
usable under graph capture.  Quirks of the reference that both keep:
  * quaternions are (w, x, y, z) and are NOT normalised: R is the ceres form divided by |q|^2 (quatutils.py:168-221), no
    epsilon -- |q| = 0 is non-finite there and here.  The gradient carries the 1/|q|^2 term.
  * left hand: y and z are negated on a COPY before the conversion (manolayer.py:242-245); `full_pose` is the untouched input
    (:239, the "dummy assignment"), returned as it came in (flat [B,64] stays flat).
  * left hand: th_shapedirs[:, 0, :] is negated once at construction (:169-170).
  * finger tips are vertices 745, 317, 444, 556, 673 for the right hand and 745, 317, 445, 556, 673 for the left (:335-338).
  * pose feature = R_local - I over the 15 finger joints (tensutils.subtract_flat_id), root excluded.
  * the kinematic tree is hard-wired as three levels of five joints (:281-283), whatever the pickle's kintree_table says;
    a transform's translation is the posed joint itself, so joints[:16] are the transforms' translations.
  * joints = 16 transform translations + 5 tips, reordered by [0,13,14,15,16,1,2,3,17,4,5,6,18,10,11,12,19,7,8,9,20] (:345).
  * th_betas=None uses the `th_betas` buffer (:259-263; zeros when the model has none), shared by the batch.
  * without th_trans: joint `center_idx` (in the reordered list) is subtracted from vertices, joints and the transforms'
    translations; center_idx=None subtracts nothing (:347-354,363).
  * with th_trans: nothing is centred; th_trans is added to all three (:355-359,363).
  * transforms come back as [B,16,4,4] with bottom rows [0,0,0,1] (:361-366); the return tuple is (verts, joints) +
    (transf,) if return_transf + (full_pose,) if return_full_pose (:371-380).
  * AnchorLayer: anchor = w1 (v1 - v0) + w2 (v2 - v0) + v0 over the three vertices of a face (anchorutils.py:51-65).
DELIBERATE DEVIATION: the reference picks the centring / translation branch by reading `torch.norm(th_trans) == 0` on the host
(:347).  Here th_trans=None selects centring and ANY tensor selects translation, so `forward` never reads device memory.
(An all-zero th_trans with a center_idx therefore translates by zero instead of centring.)
Not reproduced: axis-angle / rotation-matrix / PCA modes, `root_palm`, `share_betas` (refused), the region-name pickle and the
vertex assignment that `anchor_load` also opens (nothing in the forward reads them).
"""
import ctypes as C
import os
import pickle

import numpy as np
import torch
from torch.nn import Module

from . import _lib, ops
from ._lib import ManoModel, check

NEW_ORDER = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]
TIPS = {'right': (745, 317, 444, 556, 673), 'left': (745, 317, 445, 556, 673)}
PARENT = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]       # the three hard-wired levels of manolayer.py:281-283


def normalize_quaternion(quaternion, eps=1e-12):
    """q / max(|q|, eps) over the last axis, which must hold (w, x, y, z)."""
    if not torch.is_tensor(quaternion) or quaternion.shape[-1] != 4:
        raise ValueError('normalize_quaternion expects a tensor [..., 4]')
    return quaternion / quaternion.norm(dim=-1, keepdim=True).clamp_min(eps)


# R(q) = N(q) / |q|^2 with N quadratic in q = (w, x, y, z): N[r][c] = sum_ab _QUAT_FORM[r][c][a][b] q_a q_b -- the same
# numerators as quat_fwd of csrc/rih_mano.hip, written as one constant tensor
_QUAT_FORM = torch.zeros(3, 3, 4, 4)
for _r, _c, _terms in ((0, 0, ((0, 0, 1), (1, 1, 1), (2, 2, -1), (3, 3, -1))), (0, 1, ((1, 2, 2), (0, 3, -2))),
                       (0, 2, ((0, 2, 2), (1, 3, 2))), (1, 0, ((0, 3, 2), (1, 2, 2))),
                       (1, 1, ((0, 0, 1), (1, 1, -1), (2, 2, 1), (3, 3, -1))), (1, 2, ((2, 3, 2), (0, 1, -2))),
                       (2, 0, ((1, 3, 2), (0, 2, -2))), (2, 1, ((0, 1, 2), (2, 3, 2))),
                       (2, 2, ((0, 0, 1), (1, 1, -1), (2, 2, -1), (3, 3, 1)))):
    for _a, _b, _k in _terms:
        _QUAT_FORM[_r, _c, _a, _b] = _k


def quaternion_to_rotation_matrix(quaternion):
    """[..., 4] in (w, x, y, z) -> [..., 3, 3]; the quaternion is not normalised first, the quadratic form is divided by |q|^2
    (no epsilon: |q| = 0 is non-finite, as in the reference)."""
    form = _QUAT_FORM.to(device=quaternion.device, dtype=quaternion.dtype)
    outer = quaternion.unsqueeze(-1) * quaternion.unsqueeze(-2)                          # [..., 4, 4]
    N = (outer.unsqueeze(-3).unsqueeze(-4) * form).sum((-1, -2))                          # [..., 3, 3]
    return N / (quaternion * quaternion).sum(-1)[..., None, None]


def _with_zeros(M):
    """[n,3,4] -> [n,4,4] with the row [0,0,0,1] (tensutils.th_with_zeros)."""
    bottom = M.new_zeros((M.shape[0], 1, 4))
    bottom[:, 0, 3] = 1.0
    return torch.cat([M, bottom], 1)


class QuatManoLayer(Module):
    """manopth's ManoLayer, quaternion mode, in plain torch (see the module docstring for the quirks kept)."""

    def __init__(self, mano, side='right', center_idx=None, return_transf=False, return_full_pose=False,
                 joint_rot_mode='quat', root_rot_mode='quat', use_pca=False, flat_hand_mean=True):
        super().__init__()
        if joint_rot_mode != 'quat' or root_rot_mode != 'quat' or use_pca or not flat_hand_mean:
            raise NotImplementedError("only joint_rot_mode='quat', root_rot_mode='quat', use_pca=False, flat_hand_mean=True "
                                      '(the pose optimiser\'s configuration) are built here')
        if side not in TIPS:
            raise ValueError("side must be 'right' or 'left'; got %r" % (side,))
        if center_idx is not None and not 0 <= int(center_idx) <= 20:
            raise ValueError('center_idx must be None or 0..20; got %r' % (center_idx,))
        self.side, self.center_idx = side, None if center_idx is None else int(center_idx)
        self.return_transf, self.return_full_pose = return_transf, return_full_pose
        self.joint_rot_mode = self.root_rot_mode = 'quat'
        self.use_pca, self.flat_hand_mean, self.rot, self.ncomps = False, True, 4, 45
        if isinstance(mano, dict):
            data = mano
        else:
            with open(mano, 'rb') as f:
                data = pickle.load(f, encoding='latin1')

        def arr(a):
            a = a.r if hasattr(a, 'r') else a                     # chumpy objects of the original MANO pickle
            a = a.toarray() if hasattr(a, 'toarray') else a
            return np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        betas = arr(data['betas']).reshape(1, 10) if 'betas' in data else np.zeros((1, 10), np.float32)
        self.register_buffer('th_betas', torch.from_numpy(betas))
        self.register_buffer('th_shapedirs', torch.from_numpy(arr(data['shapedirs'])).clone())
        self.register_buffer('th_posedirs', torch.from_numpy(arr(data['posedirs'])))
        self.register_buffer('th_v_template', torch.from_numpy(arr(data['v_template'])).unsqueeze(0))
        self.register_buffer('th_J_regressor', torch.from_numpy(arr(data['J_regressor'])))
        self.register_buffer('th_weights', torch.from_numpy(arr(data['weights'])))
        self.register_buffer('th_faces', torch.from_numpy(np.asarray(data['f']).astype(np.int32)).long())
        self.kintree_table = data.get('kintree_table')
        self.kintree_parents = PARENT
        self.tips = TIPS[side]
        if side == 'left':
            self.th_shapedirs[:, 0, :] *= -1

    def _args(self, th_pose_coeffs, th_betas, th_trans, root_palm, share_betas):
        if root_palm is not None and bool(root_palm):
            raise NotImplementedError('root_palm is not built here')
        if share_betas is not None and bool(share_betas):
            raise NotImplementedError('share_betas is not built here')
        B = th_pose_coeffs.shape[0]
        if tuple(th_pose_coeffs.shape) not in ((B, 64), (B, 16, 4)):
            raise ValueError('th_pose_coeffs must be [B,64] or [B,16,4]; got %s' % (tuple(th_pose_coeffs.shape),))
        if th_betas is not None and tuple(th_betas.shape) != (B, 10):
            raise ValueError('th_betas must be [B,10] or None; got %s' % (tuple(th_betas.shape),))
        if th_trans is not None and tuple(th_trans.shape) != (B, 3):
            raise ValueError('th_trans must be [B,3] or None; got %s' % (tuple(th_trans.shape),))
        return B

    def _returns(self, verts, joints, transf, full_pose):
        out = (verts, joints)
        if self.return_transf:
            out = out + (transf,)
        if self.return_full_pose:
            out = out + (full_pose,)
        return out

    def forward(self, th_pose_coeffs, th_betas=None, th_trans=None, root_palm=None, share_betas=None):
        B = self._args(th_pose_coeffs, th_betas, th_trans, root_palm, share_betas)
        q = th_pose_coeffs.view(B, 16, 4).clone()
        if self.side == 'left':
            q[:, :, 2] = -q[:, :, 2]
            q[:, :, 3] = -q[:, :, 3]
        rots = quaternion_to_rotation_matrix(q)                                          # [B,16,3,3]
        pose_map = (rots[:, 1:] - torch.eye(3, dtype=rots.dtype, device=rots.device)).reshape(B, 135)
        betas = self.th_betas if th_betas is None else th_betas
        v_shaped = torch.matmul(self.th_shapedirs, betas.transpose(1, 0)).permute(2, 0, 1) + self.th_v_template
        th_j = torch.matmul(self.th_J_regressor, v_shaped)
        if th_betas is None:
            th_j = th_j.repeat(B, 1, 1)
        v_posed = v_shaped + torch.matmul(self.th_posedirs, pose_map.transpose(0, 1)).permute(2, 0, 1)
        # chain: a transform's translation is the joint's position relative to its parent's joint
        G = [None] * 16
        G[0] = _with_zeros(torch.cat([rots[:, 0], th_j[:, 0].unsqueeze(2)], 2))
        for i in range(1, 16):
            p = PARENT[i]
            rel = _with_zeros(torch.cat([rots[:, i], (th_j[:, i] - th_j[:, p]).unsqueeze(2)], 2))
            G[i] = torch.matmul(G[p], rel)
        results = torch.stack(G, 1)                                                       # [B,16,4,4]
        joint_h = torch.cat([th_j, th_j.new_zeros(B, 16, 1)], 2)
        tmp = torch.matmul(results, joint_h.unsqueeze(3))
        results2 = (results - torch.cat([tmp.new_zeros(B, 16, 4, 3), tmp], 3)).permute(0, 2, 3, 1)
        T = torch.matmul(results2, self.th_weights.transpose(0, 1))                       # [B,4,4,778]
        rest_h = torch.cat([v_posed.transpose(2, 1), v_posed.new_ones((B, 1, v_posed.shape[1]))], 1)
        verts = (T * rest_h.unsqueeze(1)).sum(2).transpose(2, 1)[:, :, :3]
        jtr = torch.cat([results[:, :, :3, 3], verts[:, list(self.tips)]], 1)[:, NEW_ORDER]
        if th_trans is None:
            centre = jtr[:, self.center_idx].unsqueeze(1) if self.center_idx is not None else torch.zeros_like(jtr[:, :1])
            jtr, verts, shift = jtr - centre, verts - centre, -centre
        else:
            jtr, verts, shift = jtr + th_trans.unsqueeze(1), verts + th_trans.unsqueeze(1), th_trans.unsqueeze(1)
        transf = torch.cat([results[:, :, :3, :3], results[:, :, :3, 3:] + shift.unsqueeze(-1)], 3)
        transf = _with_zeros(transf.reshape(-1, 3, 4)).view(B, 16, 4, 4)
        return self._returns(verts, jtr, transf, th_pose_coeffs)


class _QuatManoFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, layer, quat, betas, trans, want_transf):
        ops._chk(quat, betas, trans)                     # fp32 GPU tensors only: there is no CPU fallback
        lib = _lib.load()
        B, dev = quat.shape[0], quat.device
        q = quat.contiguous()
        betas_c = None if betas is None else betas.contiguous()
        trans_c = None if trans is None else trans.contiguous()
        f32 = dict(device=dev, dtype=torch.float32)
        v, j = torch.empty((B, 778, 3), **f32), torch.empty((B, 21, 3), **f32)
        transf = torch.empty((B, 16, 4, 4), **f32) if want_transf else None
        need_ws = any(ctx.needs_input_grad)
        ws = torch.empty((int(lib.rih_mano_ws_floats(B)),), **f32) if need_ws else None
        mm = layer._model_struct()
        packed = layer._packed_basis(mm)
        cidx = -1 if (trans is not None or layer.center_idx is None) else layer.center_idx
        left = 1 if layer.side == 'left' else 0
        tips = (C.c_int32 * 5)(*layer.tips)
        check(lib.rih_mano_quat_fwd(C.byref(mm), packed.data_ptr(), q.data_ptr(), left,
                                    layer.th_betas.data_ptr() if betas_c is None else betas_c.data_ptr(),
                                    0 if betas_c is None else 10, ops._p(trans_c), cidx, tips, v.data_ptr(), j.data_ptr(),
                                    ops._p(transf), ops._p(ws), B, ops._stream()), 'rih_mano_quat_fwd')
        ctx.layer, ctx.cfg = layer, (cidx, left, tuple(quat.shape), betas is not None, trans is not None)
        ctx.save_for_backward(q, ws)
        ctx.set_materialize_grads(False)
        if transf is None:
            transf = v.new_empty(0)
            ctx.mark_non_differentiable(transf)
        return v, j, transf

    @staticmethod
    def backward(ctx, dv, dj, dT):
        q, ws = ctx.saved_tensors
        cidx, left, qshape, has_betas, has_trans = ctx.cfg
        layer, lib = ctx.layer, _lib.load()
        B, dev = q.shape[0], q.device
        gs = [None if g is None else g.contiguous() for g in (dv, dj, dT)]
        ops._chk(*gs)
        f32 = dict(device=dev, dtype=torch.float32)
        d_quat = torch.empty((B, 16, 4), **f32)
        d_shape = torch.empty((B, 10), **f32) if has_betas and ctx.needs_input_grad[2] else None
        d_trans = torch.empty((B, 3), **f32) if has_trans and ctx.needs_input_grad[3] else None
        wsb = torch.empty((int(lib.rih_mano_bwd_ws_floats(B)),), **f32)
        mm = layer._model_struct()
        packed = layer._packed_basis(mm)
        tips = (C.c_int32 * 5)(*layer.tips)
        check(lib.rih_mano_quat_bwd(C.byref(mm), packed.data_ptr(), q.data_ptr(), left, cidx, tips, ops._p(gs[0]), ops._p(gs[1]),
                                    ops._p(gs[2]), ws.data_ptr(), d_quat.data_ptr(), ops._p(d_shape), ops._p(d_trans),
                                    wsb.data_ptr(), B, ops._stream()), 'rih_mano_quat_bwd')
        return None, d_quat.view(qshape), d_shape, d_trans, None


class FusedQuatManoLayer(QuatManoLayer):
    """`QuatManoLayer` on the fused MANO kernels: the quaternion -> rotation front end (with the left hand's signs), the tips of
    this hand and the 16 global transforms are part of the ONE forward launch (rih_mano_quat_fwd); the backward
    (rih_mano_quat_bwd, three launches, no atomics) takes any subset of d verts / d joints / d transf and returns the
    gradients of the quaternions, th_betas and th_trans.  The packed blend basis is cached on the buffers' version counters
    as in `renderih_amd.manolayer.ManoLayer`."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        # flat_hand_mean=True: the mean pose is zero.  Not read in quaternion mode; the model struct wants it non-null
        self.register_buffer('_hands_mean', torch.zeros(45), persistent=False)

    def _model_struct(self):
        mm = ManoModel()
        mm.comps = None
        mm.hands_mean = self._hands_mean.data_ptr()
        mm.shapedirs, mm.posedirs = self.th_shapedirs.data_ptr(), self.th_posedirs.data_ptr()
        mm.v_template, mm.J_reg = self.th_v_template.data_ptr(), self.th_J_regressor.data_ptr()
        mm.weights = self.th_weights.data_ptr()
        for i in range(16):
            mm.parent[i] = PARENT[i]
        for t in (self.th_shapedirs, self.th_posedirs, self.th_v_template, self.th_J_regressor, self.th_weights, self.th_betas):
            ops._chk(t)
            if not t.is_contiguous():
                raise RuntimeError('FusedQuatManoLayer buffers must be contiguous GPU tensors (call .cuda() on the layer)')
        return mm

    def _packed_basis(self, mm):
        srcs = (self.th_shapedirs, self.th_posedirs, self.th_v_template, self.th_J_regressor)
        key = tuple((t.data_ptr(), t._version) for t in srcs)
        cache = getattr(self, '_pack_cache', None)
        if cache is None or cache[0] != key:
            lib = _lib.load()
            buf = torch.empty((int(lib.rih_mano_pack_floats()),), device=self.th_posedirs.device, dtype=torch.float32)
            check(lib.rih_mano_pack(C.byref(mm), buf.data_ptr(), ops._stream()), 'rih_mano_pack')
            cache = (key, buf)
            object.__setattr__(self, '_pack_cache', cache)
        return cache[1]

    def forward(self, th_pose_coeffs, th_betas=None, th_trans=None, root_palm=None, share_betas=None):
        B = self._args(th_pose_coeffs, th_betas, th_trans, root_palm, share_betas)
        v, j, transf = _QuatManoFn.apply(self, th_pose_coeffs.view(B, 16, 4), th_betas, th_trans, bool(self.return_transf))
        return self._returns(v, j, transf, th_pose_coeffs)


# ------------------------------------------------------------------------------------------------ anchors
def _anchor_arrays(anchor):
    if isinstance(anchor, (str, os.PathLike)):
        fvi = np.loadtxt(os.path.join(anchor, 'face_vertex_idx.txt'), dtype=np.int64)
        w = np.loadtxt(os.path.join(anchor, 'anchor_weight.txt'))
    else:
        fvi, w = anchor
        fvi = fvi.detach().cpu().numpy() if torch.is_tensor(fvi) else np.asarray(fvi)
        w = w.detach().cpu().numpy() if torch.is_tensor(w) else np.asarray(w)
    fvi, w = np.asarray(fvi).astype(np.int64).reshape(-1, 3), np.asarray(w, np.float32).reshape(-1, 2)
    if fvi.shape[0] < 1 or fvi.shape[0] != w.shape[0]:
        raise ValueError('anchors: %d index rows, %d weight rows' % (fvi.shape[0], w.shape[0]))
    if fvi.min() < 0:
        raise ValueError('anchors: negative vertex index')
    return fvi, w


def anchor_csr(face_vert_idx, V):
    """For every vertex the (anchor * 3 + corner) entries that read it, ascending -> int32 vptr [V+1], vlist [3A].  Indices are
    range-checked here, on the host, once per index tensor (the backward kernel trusts the lists)."""
    fvi = np.asarray(face_vert_idx.detach().cpu() if torch.is_tensor(face_vert_idx) else face_vert_idx).astype(np.int64).reshape(-1)
    if fvi.size == 0 or fvi.min() < 0 or fvi.max() >= V:
        raise ValueError('anchors name vertex %d of %d' % (int(fvi.max()) if fvi.size else -1, V))
    order = np.argsort(fvi, kind='stable')
    vptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(fvi, minlength=V), out=vptr[1:])
    return torch.from_numpy(vptr.astype(np.int32)), torch.from_numpy(order.astype(np.int32))


class AnchorLayer(Module):
    """manopth/anchorlayer.py in plain torch.  `anchor`: the directory that holds face_vertex_idx.txt and anchor_weight.txt,
    or the pair (indices [A,3], weights [A,2])."""

    def __init__(self, anchor):
        super().__init__()
        fvi, w = _anchor_arrays(anchor)
        self.register_buffer('face_vert_idx', torch.from_numpy(fvi).long().unsqueeze(0))
        self.register_buffer('anchor_weight', torch.from_numpy(w).float().unsqueeze(0))

    def forward(self, vertices):
        iv = vertices[:, self.face_vert_idx[0]]                                          # [B,A,3,3]
        b1, b2 = iv[:, :, 1] - iv[:, :, 0], iv[:, :, 2] - iv[:, :, 0]
        return self.anchor_weight[:, :, 0:1] * b1 + self.anchor_weight[:, :, 1:2] * b2 + iv[:, :, 0]


class _AnchorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, fvi32, weight, vptr, vlist):
        ops._chk(vertices, weight)
        ops._chk(fvi32, vptr, vlist, dtype=torch.int32)
        v = vertices.contiguous()
        B, V, _ = v.shape
        A = fvi32.shape[0]
        out = torch.empty((B, A, 3), device=v.device, dtype=torch.float32)
        check(ops._L().rih_anchor_fwd(v.data_ptr(), fvi32.data_ptr(), weight.data_ptr(), out.data_ptr(), B, V, A,
                                      ops._stream()), 'rih_anchor_fwd')
        ctx.save_for_backward(fvi32, weight, vptr, vlist)
        ctx.V = V
        return out

    @staticmethod
    def backward(ctx, g):
        fvi32, weight, vptr, vlist = ctx.saved_tensors
        g = g.contiguous()
        ops._chk(g)
        B, A, _ = g.shape
        dv = torch.empty((B, ctx.V, 3), device=g.device, dtype=torch.float32)
        check(ops._L().rih_anchor_bwd(g.data_ptr(), vptr.data_ptr(), vlist.data_ptr(), weight.data_ptr(), dv.data_ptr(), B,
                                      ctx.V, A, ops._stream()), 'rih_anchor_bwd')
        return dv, None, None, None, None


class FusedAnchorLayer(AnchorLayer):
    """`AnchorLayer` on csrc/rih_anchor.hip: rih_anchor_fwd (thread = sample x anchor x coordinate) and rih_anchor_bwd (thread =
    sample x vertex x coordinate gathering through the vertex -> (anchor, corner) lists of `anchor_csr`: no atomics, exact
    zeros for vertices no anchor reads).  The lists are built on the host once per vertex count."""

    def __init__(self, anchor):
        super().__init__(anchor)
        self.register_buffer('_fvi32', self.face_vert_idx[0].to(torch.int32).contiguous(), persistent=False)
        self._csr = {}

    def _lists(self, V, device):
        key = (V, str(device))
        if key not in self._csr:
            vptr, vlist = anchor_csr(self.face_vert_idx[0], V)
            self._csr[key] = (vptr.to(device), vlist.to(device))
        return self._csr[key]

    def forward(self, vertices):
        if vertices.dim() != 3 or vertices.shape[2] != 3:
            raise ValueError('vertices must be [B,V,3]; got %s' % (tuple(vertices.shape),))
        vptr, vlist = self._lists(vertices.shape[1], vertices.device)
        return _AnchorFn.apply(vertices, self._fvi32, self.anchor_weight[0].contiguous(), vptr, vlist)
