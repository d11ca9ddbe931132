"""The contact search of the pose optimiser's driver -- `search_anchors` of pose_data_optimize/batch_optimize_mocap_origin.py
:62-130 on the anchors and face normals that `update_scene` :260-270 computes -- for a batch of frames: from the two hands'
translated vertices to the `vertex_contact`, `anchor_id`, `anchor_elasti` and `anchor_padding_mask` that `set_opt_val` takes.

`TwoHandContactSearch` is the plain-torch mirror (any floating dtype); `FusedTwoHandContactSearch` is the same surface on
csrc/rih_contact.hip (rih_contact_search: one launch, one workgroup per frame, outputs stay on the device; fp32 only).

Per frame: anchors as `AnchorLayer`, unit normals cross(v1 - v0, v2 - v0) of the same faces, the sub (left) hand's negated.  For
sub anchor i and main anchor j, dis = |sub_i - main_j|.
  fresh search (prev_anchor_id=None, radius `fresh_radius` = 0.015): dis counts as 1000 where n_sub_i . n_main_j > against_cos
      (-0.6); anchor_id[i] = the `dim` smallest; vertex_contact[i] = any(dis < radius).
  refresh (prev_anchor_id given, radius `refresh_radius` = 0.02): anchor_id = prev_anchor_id, the true distance to each of them,
      no against rule (:75-91); vertex_contact[i] = any of the row's ids within the radius.
  both: elastic = (dis < radius) (0.5 cos(pi dis / radius) + 0.5), mask = elastic > 0, and elastic *= damp (0.3) where neither
      class_type[i] nor class_type[id] is tip_class (4) (:129).
`optimize_it` [B] = vertex_contact.any(1), the flag the driver builds at :533-538.

DELIBERATE DEVIATIONS.  Equal distances -- in practice the 1000s of a row with fewer than `dim` facing anchors -- are ordered by
ascending j: numpy's unstable argsort leaves that order unspecified, and the refreshes of attempts 1 and 2 read those ids
again.  A previous id outside [0, A) gives elastic 0 and mask 0 and is copied through (the reference's -1 padding, which its own
search never produces, would index from the end).  The elastic weight is computed as cos^2(pi dis / (2 radius)), the same
function, which stays positive up to the radius in fp32 where 0.5 cos + 0.5 rounds to 0.  Degenerate faces (a zero normal) are
outside the contract.  Not reproduced: `judge_hand_contact=True` (no caller passes it), the -1 padding, visualisation.
"""
import math
import os

import numpy as np
import torch

from . import ops
from .ops import check
from .quat_mano import _anchor_arrays

AGAINST_DISTANCE = 1000.0                     # search_anchors :100, :118
MAX_ANCHORS, MAX_DIM = 1024, 8                # rih_contact_search's limits


def _class_types(anchor, class_type, A):
    if class_type is None:
        if not isinstance(anchor, (str, os.PathLike)):
            raise ValueError('class_type=None needs an anchor directory (it reads merged_vertex_assignment.txt there)')
        class_type = np.loadtxt(os.path.join(anchor, 'merged_vertex_assignment.txt'), dtype=np.int64)
    ct = np.asarray(class_type.detach().cpu() if torch.is_tensor(class_type) else class_type).astype(np.int64).reshape(-1)
    if ct.shape[0] != A:
        raise ValueError('class_type has %d entries for %d anchors' % (ct.shape[0], A))
    return ct


class TwoHandContactSearch(torch.nn.Module):
    """The search in plain torch; see the module docstring.  `anchor`: the anchor directory or (indices [A,3], weights [A,2]) as
    `AnchorLayer` takes it; `class_type` [A] (None: merged_vertex_assignment.txt of the directory)."""

    def __init__(self, anchor, class_type=None, fresh_radius=0.015, refresh_radius=0.02, against_cos=-0.6, damp=0.3, tip_class=4,
                 dim=4):
        super().__init__()
        fvi, w = _anchor_arrays(anchor)
        A = fvi.shape[0]
        if not 1 <= int(dim) <= A:
            raise ValueError('dim must be in 1..%d; got %r' % (A, dim))
        if not (fresh_radius > 0 and refresh_radius > 0):
            raise ValueError('the radii must be positive')
        self.register_buffer('face_vert_idx', torch.from_numpy(fvi).long())
        self.register_buffer('anchor_weight', torch.from_numpy(w).float())
        self.register_buffer('class_type', torch.from_numpy(_class_types(anchor, class_type, A)))
        self._checked_V = set()                                # vertex counts the index table was range-checked against
        self.fresh_radius, self.refresh_radius = float(fresh_radius), float(refresh_radius)
        self.against_cos, self.damp, self.tip_class, self.dim = float(against_cos), float(damp), int(tip_class), int(dim)

    # ------------------------------------------------------------------ checks
    def _check(self, verts_main, verts_sub, prev_anchor_id):
        A = self.face_vert_idx.shape[0]
        if verts_main.dim() != 3 or verts_main.shape[2] != 3 or verts_sub.shape != verts_main.shape:
            raise ValueError('verts_main and verts_sub must both be [B,V,3]; got %s and %s'
                             % (tuple(verts_main.shape), tuple(verts_sub.shape)))
        if verts_main.shape[0] < 1 or verts_sub.dtype != verts_main.dtype or not verts_main.is_floating_point():
            raise ValueError('the vertices must be floating point, of one dtype, with B >= 1')
        if prev_anchor_id is not None and (tuple(prev_anchor_id.shape) != (verts_main.shape[0], A, self.dim)
                                           or prev_anchor_id.dtype != torch.int64):
            raise ValueError('prev_anchor_id must be int64 [B,%d,%d]; got %s %s'
                             % (A, self.dim, prev_anchor_id.dtype, tuple(prev_anchor_id.shape)))
        return verts_main.shape[0], verts_main.shape[1], A

    def _check_range(self, V):
        """Once per vertex count, on the host, as `anchor_csr` does for the anchor layer's backward."""
        if V not in self._checked_V:
            low, top = int(self.face_vert_idx.min()), int(self.face_vert_idx.max())
            if low < 0 or top >= V:
                raise ValueError('anchors name vertex %d of %d' % (low if low < 0 else top, V))
            self._checked_V.add(V)

    @staticmethod
    def _result(vertex_contact, anchor_id, elastic, mask):
        return {'vertex_contact': vertex_contact, 'anchor_id': anchor_id, 'anchor_elasti': elastic, 'anchor_padding_mask': mask,
                'optimize_it': vertex_contact.any(1)}

    # ------------------------------------------------------------------ the search
    def _geometry(self, verts):
        iv = verts[:, self.face_vert_idx]                                               # [B,A,3,3]
        b1, b2 = iv[:, :, 1] - iv[:, :, 0], iv[:, :, 2] - iv[:, :, 0]
        w = self.anchor_weight.to(verts.dtype)
        n = torch.cross(b1, b2, dim=-1)
        return w[None, :, 0:1] * b1 + w[None, :, 1:2] * b2 + iv[:, :, 0], n / n.norm(dim=-1, keepdim=True)

    def forward(self, verts_main, verts_sub, prev_anchor_id=None):
        B, V, A = self._check(verts_main, verts_sub, prev_anchor_id)
        self._check_range(V)
        with torch.no_grad():
            main, n_main = self._geometry(verts_main)
            sub, n_sub = self._geometry(verts_sub)
            dis = (sub[:, :, None] - main[:, None]).norm(dim=-1)                        # [B,A(sub),A(main)]
            if prev_anchor_id is None:
                radius = self.fresh_radius
                against = torch.einsum('bic,bjc->bij', -n_sub, n_main) > self.against_cos
                dis = torch.where(against, torch.full_like(dis, AGAINST_DISTANCE), dis)
                picked, anchor_id = torch.sort(dis, dim=-1, stable=True)
                picked, anchor_id = picked[..., :self.dim], anchor_id[..., :self.dim].contiguous()
                vertex_contact = (dis < radius).any(-1)
                valid = torch.ones_like(anchor_id, dtype=torch.bool)
            else:
                radius = self.refresh_radius
                anchor_id = prev_anchor_id.to(dis.device)
                valid = (anchor_id >= 0) & (anchor_id < A)
                picked = dis.gather(2, anchor_id.clamp(0, A - 1))
                vertex_contact = (valid & (picked < radius)).any(-1)
            elastic = torch.cos((0.5 * math.pi / radius) * picked) ** 2 * (valid & (picked < radius))
            mask = elastic > 0
            tip = self.class_type == self.tip_class
            undamped = tip[None, :, None] | tip[anchor_id.clamp(0, A - 1)]
            elastic = torch.where(undamped, elastic, elastic * self.damp)
        return self._result(vertex_contact.long(), anchor_id, elastic.float(), mask.long())


class FusedTwoHandContactSearch(TwoHandContactSearch):
    """`TwoHandContactSearch` on csrc/rih_contact.hip: both hands' anchors and normals, the A x A scan, the D-entry insertion
    list and the elastic weights in ONE launch per call (one workgroup per frame), however many frames.  GPU fp32 only; the
    anchor tables are range-checked against V on the host once per V; the five outputs are device tensors."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        A = self.face_vert_idx.shape[0]
        if A > MAX_ANCHORS or self.dim > MAX_DIM:
            raise ValueError('the fused search takes at most %d anchors and dim %d; got %d and %d' % (MAX_ANCHORS, MAX_DIM, A, self.dim))
        self.register_buffer('_fvi32', self.face_vert_idx.to(torch.int32).contiguous(), persistent=False)
        self.register_buffer('_cls32', self.class_type.to(torch.int32).contiguous(), persistent=False)

    def forward(self, verts_main, verts_sub, prev_anchor_id=None):
        B, V, A = self._check(verts_main, verts_sub, prev_anchor_id)
        if verts_main.dtype != torch.float32:
            raise ValueError('the fused search is fp32 only; got %s' % verts_main.dtype)
        self._check_range(V)
        vm, vs = verts_main.detach().contiguous(), verts_sub.detach().contiguous()
        weight = self.anchor_weight.contiguous()
        ops._chk(vm, vs, weight)
        ops._chk(self._fvi32, self._cls32, dtype=torch.int32)
        prev = None
        if prev_anchor_id is not None:
            prev = prev_anchor_id.contiguous()
            ops._chk(prev, dtype=torch.int64)
        dev, D = vm.device, self.dim
        anchor_id = torch.empty((B, A, D), device=dev, dtype=torch.int64)
        elastic = torch.empty((B, A, D), device=dev, dtype=torch.float32)
        mask = torch.empty((B, A, D), device=dev, dtype=torch.int64)
        vertex_contact = torch.empty((B, A), device=dev, dtype=torch.int64)
        check(ops._L().rih_contact_search(
            vm.data_ptr(), vs.data_ptr(), self._fvi32.data_ptr(), weight.data_ptr(), self._cls32.data_ptr(),
            None if prev is None else prev.data_ptr(), self.fresh_radius if prev is None else self.refresh_radius, self.against_cos,
            self.damp, self.tip_class, anchor_id.data_ptr(), elastic.data_ptr(), mask.data_ptr(), vertex_contact.data_ptr(), B, V, A,
            D, ops._stream()), 'rih_contact_search')
        return self._result(vertex_contact, anchor_id, elastic, mask)
