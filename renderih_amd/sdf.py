"""Interior distance field of closed meshes on a voxel grid and the penetration loss built on it -- drop-in for the
reference's `sdf` extension (pose_data_optimize/sdf/sdf/sdf.py:8-35 `SDFFunction` / `SDF` / `sdf`, sdf_loss.py:7-103
`SDFLoss`), whose CUDA kernel is the only native code of the reference.  The voxeliser is the HIP kernel
csrc/rih_sdf.hip; like the reference's it has no gradient (phi is used as a constant field that other meshes' vertices
sample).

`TwoHandSDFLoss` / `FusedTwoHandSDFLoss` are drop-ins for the class the pose optimiser actually calls,
pose_data_optimize/code_sdf/sdf_template.py:19-157 `NewLoss` (hocontact/postprocess/geo_optimizer_both_batch.py:46,634-636):
the first a plain-torch mirror built from `sdf` and `grid_sample`, the second the same computation on csrc/rih_sdf_loss.hip
and the sparse voxeliser of csrc/rih_sdf.hip (four launches forward, one backward, no host sync).  Quirks of the reference
that both keep:
  * vertices [bs, 2, V, 3]: index 0 is the RIGHT hand, index 1 the LEFT; the returned per-vertex tensors come left first.
  * three return shapes: `loss [bs]`; `(loss, left [bs,V], right [bs,V])`; `(loss, per_vert [bs,2V], [left_oriscale,
    right_oriscale])`.
  * boxes, centres, scales, the normalised vertices and phi carry no gradient (`@torch.no_grad()` / `with torch.no_grad()`
    there); the only gradient path is (v_other - centre) / scale -> grid_sample.
  * centre = (lo + hi) / 2; scale = ((1 + scale_factor) * 0.5) * max axis of (hi - lo): the product of Python floats first,
    then applied to the fp32 tensor; normalisation DIVIDES by the scale (no reciprocal).
  * the voxeliser puts voxel i at -1 + (i + 0.5) * 2 / (G - 1), the sampler (align_corners=True, zero padding) puts sample
    index i at -1 + i * 2 / (G - 1): half a voxel apart, as in the reference, not reconciled.
  * left-hand vertices sample the RIGHT hand's cube and field and the other way round; one face list serves both hands (the
    reference loads right.npy twice).
  * the 16 hand parts overlap (934 entries for 778 vertices in the reference's part_vert.npy) and are accumulated with `+=`:
    a vertex in k parts counts k times (within one part an index counts once, as an indexed `+=` does).  Kept as an
    integer weight per vertex, derived once in the constructor.  The table is reference data: the caller supplies it.
  * loss = (left + right).sum(1), both sides divided by num_hand ** 2 = 4; the original-scale outputs are multiplied by
    boxes_scale[:, h, 0], the scale of the cube that was SAMPLED (left_oriscale by the right hand's scale).
  * `robustifier` is stored and never used, there and here.
NOT reproduced: the reference's `assert`s (normalised vertices within [-1, 1], phi >= 0) -- each is a device-to-host sync,
and both hold by construction; the hard-coded 778 (V and F follow the inputs).
"""
import os

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .ops import check


def sdf(faces, vertices, grid_size=32):
    """faces [F,3] int32, vertices [B,V,3] fp32 inside [-1,1]^3 (GPU) -> phi [B,G,G,G] indexed [b][z][y][x]."""
    ops._chk(vertices)
    ops._chk(faces, dtype=torch.int32)
    vertices, faces = vertices.contiguous(), faces.contiguous()
    B, V, _ = vertices.shape
    phi = torch.empty((B, grid_size, grid_size, grid_size), device=vertices.device, dtype=torch.float32)
    check(ops._L().rih_sdf(phi.data_ptr(), faces.data_ptr(), vertices.data_ptr(), B, faces.shape[0], V, grid_size,
                           ops._stream()), 'rih_sdf')
    return phi


class SDF(nn.Module):
    def forward(self, faces, vertices, grid_size=32):
        with torch.no_grad():
            return sdf(faces, vertices.detach(), grid_size)


class SDFLoss(nn.Module):
    """sdf_loss.py:7-103: every mesh ("person" there, hand here) is voxelised in its own padded bounding cube; the vertices of
    the other meshes sample that field (trilinear `grid_sample`); positive samples = penetration depth."""

    def __init__(self, faces, grid_size=32, robustifier=None):
        super().__init__()
        self.sdf = SDF()
        self.register_buffer('faces', torch.as_tensor(np.asarray(faces).astype(np.int32)))
        self.grid_size, self.robustifier = grid_size, robustifier

    def forward(self, vertices, translation, scale_factor=0.2):
        n = vertices.shape[0]
        vertices = vertices + translation.unsqueeze(dim=1)
        loss = torch.tensor(0., device=vertices.device)
        if n == 1:
            return loss
        with torch.no_grad():
            lo, hi = vertices.min(dim=1)[0], vertices.max(dim=1)[0]                          # [n,3] bounding boxes
            apart = ((lo[:, None] > hi[None]) | (lo[None] > hi[:, None])).any(-1)             # [n,n] boxes i, j disjoint
            apart = apart | torch.eye(n, dtype=torch.bool, device=vertices.device)
            isolated = (apart.sum(1) - 1) > 0                                                 # sic: ANY disjoint partner
            keep = ~isolated
        if keep.sum() == 0:
            return loss
        vertices = vertices[keep].contiguous()
        lo, hi = lo[keep], hi[keep]
        center = ((lo + hi) / 2).unsqueeze(1)
        scale = ((1 + scale_factor) * 0.5 * (hi - lo).max(dim=-1)[0])[:, None, None]
        with torch.no_grad():
            phi = self.sdf(self.faces, (vertices - center) / scale, self.grid_size)
        m = vertices.shape[0]
        for i in range(m):
            w = torch.ones(m, 1, device=vertices.device)
            w[i, 0] = 0.
            local = ((vertices - center[i].unsqueeze(0)) / scale[i].unsqueeze(0)).view(1, -1, 1, 1, 3)
            val = nn.functional.grid_sample(phi[i][None, None], local, align_corners=False).view(m, -1)
            cur = w * val
            if self.robustifier:
                frac = (cur / self.robustifier) ** 2
                cur = frac / (frac + 1)
            loss = loss + cur.sum() / m ** 2
        return loss


def part_weights(part_vert, V):
    """How many of the hand parts hold each vertex -> int32 [V].  `part_vert`: the reference's dict {part: vertex indices},
    the path of its part_vert.npy (a pickled 0-d object array, loaded as the reference loads it), or a ready [V] vector."""
    if isinstance(part_vert, (str, os.PathLike)):
        part_vert = np.load(part_vert, allow_pickle=True)[()]
    if isinstance(part_vert, dict):
        w = np.zeros(V, np.int64)
        for key in part_vert:
            idx = np.unique(np.asarray(list(part_vert[key]), np.int64))
            if idx.size and (idx.min() < 0 or idx.max() >= V):
                raise ValueError('part_vert names vertex %d of %d' % (idx.max(), V))
            w[idx] += 1
    else:
        w = (part_vert.detach().cpu().numpy() if torch.is_tensor(part_vert) else np.asarray(part_vert)).reshape(-1)
        if w.shape[0] != V or (w != np.round(w)).any() or (w < 0).any():
            raise ValueError('part_vert: expected %d non-negative integer weights' % V)
    return torch.as_tensor(w.astype(np.int32))


class TwoHandSDFLoss(nn.Module):
    """sdf_template.py:19-157 `NewLoss` in plain torch (see the module docstring for the quirks kept)."""

    def __init__(self, part_vert, faces=None, grid_size=32, robustifier=None):
        super().__init__()
        if faces is None:
            from . import assets
            faces = assets.hand_faces('right')
        faces = np.asarray(faces.detach().cpu() if torch.is_tensor(faces) else faces).astype(np.int32)
        self.register_buffer('faces', torch.as_tensor(faces))
        V = int(faces.max()) + 1 if isinstance(part_vert, (dict, str, os.PathLike)) else len(part_vert)
        self.register_buffer('weight', part_weights(part_vert, V))
        self.grid_size, self.robustifier = grid_size, robustifier           # robustifier: kept, unused (as in the reference)
        self.sdf = SDF()

    def _check(self, vertices):
        if vertices.dim() != 4 or vertices.shape[1] != 2 or vertices.shape[3] != 3 or vertices.shape[2] != self.weight.shape[0]:
            raise ValueError('vertices must be [bs, 2, %d, 3]; got %s' % (self.weight.shape[0], tuple(vertices.shape)))

    @staticmethod
    def _returns(loss, pv, ori, return_per_vert_loss, return_origin_scale_loss):
        if not return_per_vert_loss:
            return loss
        if not return_origin_scale_loss:
            return loss, pv[:, 0], pv[:, 1]
        return loss, pv.reshape(pv.shape[0], -1), [ori[:, 0], ori[:, 1]]

    def forward(self, vertices, scale_factor=0.1, return_per_vert_loss=False, return_origin_scale_loss=False):
        self._check(vertices)
        bs, _, V, _ = vertices.shape
        G = self.grid_size
        with torch.no_grad():
            lo, hi = vertices.min(dim=2)[0], vertices.max(dim=2)[0]                          # [bs,2,3]
            center = ((lo + hi) / 2).unsqueeze(2)                                              # [bs,2,1,3]
            scale = ((1 + scale_factor) * 0.5 * (hi - lo).max(dim=-1)[0])[:, :, None, None]    # [bs,2,1,1]
            normed = ((vertices - center) / scale).reshape(bs * 2, V, 3)
            phi = self.sdf(self.faces, normed, G).view(bs, 2, G, G, G)
        w = self.weight.to(vertices.dtype)
        pv, ori = [], []
        for h in (0, 1):                                   # the cube and field of hand h, sampled by the other hand
            local = ((vertices[:, 1 - h] - center[:, h]) / scale[:, h]).view(bs, V, 1, 1, 3)
            val = nn.functional.grid_sample(phi[:, h].unsqueeze(1), local, align_corners=True).view(bs, V) * w
            pv.append(val / 4)
            ori.append(val * scale[:, h, 0])
        pv, ori = torch.stack(pv, 1), torch.stack(ori, 1)
        loss = (pv[:, 0] + pv[:, 1]).sum(dim=1)
        return self._returns(loss, pv, ori, return_per_vert_loss, return_origin_scale_loss)


# RIH_SDF_SPARSE=0: the fused loss voxelises every voxel (rih_sdf) instead of the sampled ones (rih_sdf_sparse) -- for
# same-box A/B runs; the outputs are bit-identical.  Read at import.
SPARSE = os.environ.get('RIH_SDF_SPARSE', '1') != '0'


class _TwoHandSDF(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, faces, weight, G, scale_mul, sparse, debug):
        ops._chk(vertices)
        ops._chk(faces, weight, dtype=torch.int32)
        v = vertices.detach().contiguous()
        bs, _, V, _ = v.shape
        dev, L, st = v.device, ops._L(), ops._stream()
        vox, F = G ** 3, faces.shape[0]
        cap = min(vox, 8 * V)
        f32 = dict(device=dev, dtype=torch.float32)
        box, vnorm = torch.empty((bs, 2, 4), **f32), torch.empty((bs * 2, V, 3), **f32)
        flags = torch.empty((bs, 2, G, G, G), device=dev, dtype=torch.uint8)
        lst = torch.empty((bs * 2, cap), device=dev, dtype=torch.int32)
        count = torch.empty((bs * 2,), device=dev, dtype=torch.int32)
        phi = torch.empty((bs, 2, G, G, G), **f32)
        pv, ori = torch.empty((bs, 2, V), **f32), torch.empty((bs, 2, V), **f32)
        grad, loss = torch.empty((bs, 2, V, 3), **f32), torch.empty((bs,), **f32)
        check(L.rih_two_hand_prep(v.data_ptr(), scale_mul, box.data_ptr(), vnorm.data_ptr(), flags.data_ptr(), lst.data_ptr(),
                                  count.data_ptr(), bs, V, G, cap, st), 'rih_two_hand_prep')
        if sparse:
            check(L.rih_sdf_sparse(phi.data_ptr(), faces.data_ptr(), vnorm.data_ptr(), lst.data_ptr(), count.data_ptr(), cap,
                                   bs * 2, F, V, G, st), 'rih_sdf_sparse')
        else:
            check(L.rih_sdf(phi.data_ptr(), faces.data_ptr(), vnorm.data_ptr(), bs * 2, F, V, G, st), 'rih_sdf')
        check(L.rih_two_hand_sample(phi.data_ptr(), v.data_ptr(), box.data_ptr(), weight.data_ptr(), pv.data_ptr(),
                                    ori.data_ptr(), grad.data_ptr(), loss.data_ptr(), bs, V, G, st), 'rih_two_hand_sample')
        ctx.save_for_backward(grad, box)
        ctx.set_materialize_grads(False)
        if debug is not None:
            debug.update(phi=phi, flags=flags, box=box, count=count, list=lst, vnorm=vnorm)
        return loss, pv, ori

    @staticmethod
    def backward(ctx, g_loss, g_pv, g_ori):
        grad, box = ctx.saved_tensors
        bs, _, V, _ = grad.shape
        out = torch.empty_like(grad)
        gs = [None if g is None else g.contiguous() for g in (g_loss, g_pv, g_ori)]
        ops._chk(*gs)
        check(ops._L().rih_two_hand_bwd(grad.data_ptr(), box.data_ptr(), ops._p(gs[0]), ops._p(gs[1]), ops._p(gs[2]),
                                        out.data_ptr(), bs, V, ops._stream()), 'rih_two_hand_bwd')
        return out, None, None, None, None, None, None


class FusedTwoHandSDFLoss(TwoHandSDFLoss):
    """`TwoHandSDFLoss` on the HIP kernels: rih_two_hand_prep -> rih_sdf_sparse (rih_sdf with RIH_SDF_SPARSE=0) ->
    rih_two_hand_sample, and rih_two_hand_bwd for the gradient.  No host sync: usable under graph capture.  With
    `keep_debug = True` the last forward's phi [bs,2,G,G,G], flags (the voxels that were sampled, hence voxelised), box
    (centre, scale), count and list stay in `self.debug`."""

    def __init__(self, part_vert, faces=None, grid_size=32, robustifier=None, sparse=None):
        super().__init__(part_vert, faces, grid_size, robustifier)
        self.sparse = SPARSE if sparse is None else bool(sparse)
        self.keep_debug, self.debug = False, {}

    def forward(self, vertices, scale_factor=0.1, return_per_vert_loss=False, return_origin_scale_loss=False):
        self._check(vertices)
        self.debug = {} if self.keep_debug else None
        loss, pv, ori = _TwoHandSDF.apply(vertices, self.faces, self.weight, self.grid_size, (1 + scale_factor) * 0.5,
                                          self.sparse, self.debug)
        return self._returns(loss, pv, ori, return_per_vert_loss, return_origin_scale_loss)
