"""Hand-prior and contact terms of the pose optimiser's two-hand objective -- drop-ins for what `GeOptimizer.loss_fn`
(pose_data_optimize/hocontact/postprocess/geo_optimizer_both_batch.py:498-859, mode='both') adds to the penetration loss:
`HandLoss.batch_pose_quat_norm_loss`, `HandLoss.edge_len_loss`, `FieldLoss.batch_contact_loss` and
`HandLoss.hand_pose_ergonomics_loss` (hocontact/postprocess/geo_loss.py) with the axis conversion it needs,
`HandPoseConverter.mano_quat_2_mat_tensor` (scripts/HandPoseConverter.py).

The functions and `TwoHandPriorLoss` are plain-torch mirrors (CPU-capable, pinned to the reference by
tests/golden/pose_prior.npz); `FusedTwoHandPriorLoss` runs the same sum on csrc/rih_pose_prior.hip: rih_pose_prior_fwd (one
workgroup per (sample, hand)) + rih_pose_prior_reduce forward, rih_pose_prior_bwd backward.  GPU fp32 only, no atomics, no
host read of device memory: usable under graph capture, two evaluations are bit-identical.  Quirks of the reference that both
keep:
  * axis tables: the converter's MANO layer is centred on joint 9 and posed with identity quaternions and the converter's own
    hard-coded shape vector (HandPoseConverter.py:43-44), whatever hand is optimised; bones follow the joint list
    [5,6,7,9,10,11,17,18,19,13,14,15,1,2,3]; the left hand's up-axis base is the SECOND assignment (:92-93: (0,-1,0) for the
    fingers, (1,-1,-1) for the thumb), which overwrites the first; the left hand's root block is diag(1,-1,-1).
  * mano_quat_2_mat: left hand negates y and z on a copy; the conversion does not normalise (R = form / |q|^2; the optimiser
    passes normalised quaternions); left hand negates [:, 0, 1:, 1:] of the ROOT only; result invM_U_n_0^T R invU_M_n_1^T.
  * the quaternion-norm term sees the UN-normalised quaternions, all 16; the ergonomics term sees normalize_quaternion(q)
    and drops the root.
  * edges: unique undirected edges in first-seen order over the faces; the sub (left) hand's edges are built from the RIGHT
    hand's faces (geo_optimizer_both_batch.py:229); the static lengths come from each hand's own rest mesh (identity
    quaternions, zero betas, center_idx=0).
  * contact: `mask` enters only through its sum -- the product elastic * dist is NOT masked, so a masked-out entry with a
    nonzero elastic still pulls.
  * ergonomics: relative frames are zero_ja^T ja; step 1 over joints [1,2,4,5,10,11,7,8,13,14], step 2 (twist, antisymmetric
    part) over [0,3,9,6] plus the thumb's max(c - 0.5, 0)^2 at 12; step 3 hinges in DEGREES converted back to radians, one
    mean per joint added; step 4 after negative bends were set to 0 in place (zero gradient through a clamped bend);
    `target_second_bend_angle` is dead code and `side` is unused, there and here.
DELIBERATE DEVIATIONS: the reference reads `mask.sum() <= 0` on the host in every iteration and then returns a fresh [1]
tensor.  Here mask, anchor_id and elastic are constants given to `set_contacts`, the sum is taken there once, on host data, and
an empty mask gives an exact scalar 0 with zero gradients; `forward` never reads device memory.  The orientation of an edge
row is (smaller, larger) index; the reference's is the iteration order of a two-element Python set (the loss is symmetric).
`terms` of the fused class carries no gradient (the mirror's does).
Not reproduced: the terms loss_fn multiplies by 0 or has commented out, the single-hand / object mode.  NatureLoss is
renderih_amd/nature.py.  The Adam + ReduceLROnPlateau loop around this loss: renderih_amd/pose_opt.py.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .ops import check
from .quat_mano import PARENT, QuatManoLayer, normalize_quaternion, quaternion_to_rotation_matrix

JOINT_MAP = (5, 6, 7, 9, 10, 11, 17, 18, 19, 13, 14, 15, 1, 2, 3)
# HandPoseConverter.py:43-44: the shape the converter's own layer is posed with
CONVERTER_SHAPE = (0.5082395, -0.39488167, -1.7484332, 1.6630946, 0.34428665, -1.37387, 0.38293332, 1.196094, 0.6538949,
                   -0.94331187)
NO_TWIST_SPLAY = (1, 2, 4, 5, 10, 11, 7, 8, 13, 14)                  # step 1 (indices into the 15 finger joints)
NO_TWIST = (0, 3, 9, 6)                                              # step 2, plain squares
THUMB = 12                                                           # step 2, max(c - 0.5, 0)^2
SPLAY = {0: (-25, 15), 3: (-15, 15), 9: (-25, 15), 6: (-20, 30), 12: (-30, 30)}
BEND = {0: (-25, 70), 1: (-4, 110), 3: (-25, 80), 4: (-7, 100), 9: (-25, 70), 10: (-10, 100), 6: (-22, 70), 7: (-8, 90),
        12: (-20, 40), 13: (-35, 50), 14: (-10, 100), 2: (-8, 90), 5: (-8, 90), 11: (-8, 90), 8: (-8, 90)}
PINKY, RING = 10, 7                                                  # step 4: clamp(bend[10] - 3/4 bend[7], max=0)^2


def _np(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def axis_tables(side, mano):
    """(invM_U_n_0, invU_M_n_1), each [16,3,3] fp32: the once-per-construction part of the reference's HandPoseConverter
    (`__init__`, `axis_convert`, `init_convert_matrix`).  `mano`: the model dict or pickle path of `QuatManoLayer`."""
    if side not in ('right', 'left'):
        raise ValueError("side must be 'right' or 'left'; got %r" % (side,))
    layer = QuatManoLayer(mano, side=side, center_idx=9, return_transf=True)
    ident = torch.zeros(1, 16, 4)
    ident[..., 0] = 1.0
    with torch.no_grad():
        _, joints, transf = layer(ident, torch.tensor([CONVERTER_SHAPE], dtype=torch.float32))
    joints, m = joints[0].numpy(), transf[0, :, :3, :3].numpy()                      # fp32, as the reference holds them
    sign = 1 if side == 'right' else -1
    jm = np.asarray(JOINT_MAP)
    bone = (joints[jm] - joints[jm + 1]) * np.float32(sign)
    up = np.array([[0, sign, 0]] * 12 + [[1, sign, sign]] * 3)
    x = np.einsum('nji,nj->ni', m[1:], bone)                                          # the bone in the joint's own frame
    z = np.cross(x, up)
    y = np.cross(z, x)
    x, y, z = (a / np.linalg.norm(a, axis=-1)[:, None] for a in (x, y, z))
    local = np.tile(np.eye(3), (16, 1, 1))
    local[1:] = np.stack([x, y, z], axis=-1)                                          # columns x, y, z
    if side == 'left':
        local[0] = np.diag([1.0, -1.0, -1.0])
    u = m @ local
    parent = [0] + PARENT[1:]
    inv_m_u_0 = np.stack([m[parent[a]].T @ u[parent[a]] for a in range(16)]).astype(np.float32)
    inv_u_m_1 = np.stack([u[a].T @ m[a] for a in range(16)]).astype(np.float32)
    return torch.from_numpy(inv_m_u_0), torch.from_numpy(inv_u_m_1)


def mano_quat_2_mat(q, tables, side):
    """q [B,16,4] -> [B,16,3,3]: HandPoseConverter.mano_quat_2_mat_tensor with the tables of `axis_tables`."""
    if q.dim() != 3 or tuple(q.shape[1:]) != (16, 4):
        raise ValueError('q must be [B,16,4]; got %s' % (tuple(q.shape),))
    t0, t1 = (t.to(device=q.device, dtype=q.dtype) for t in tables)
    if side == 'left':
        q = q * q.new_tensor([1.0, 1.0, -1.0, -1.0])
    R = quaternion_to_rotation_matrix(q)
    if side == 'left':
        flip = torch.ones(16, 3, 3, dtype=q.dtype, device=q.device)
        flip[0, 1:, 1:] = -1.0
        R = R * flip
    return t0.transpose(1, 2) @ R @ t1.transpose(1, 2)


def quat_norm_loss(q):
    """mean((|q|^2 - 1)^2) over [B,16], on the un-normalised quaternions."""
    return (((q * q).sum(-1) - 1.0) ** 2).mean()


def edge_index(faces):
    """faces [F,3] -> int64 [E,2]: the unique undirected edges in first-seen order over the faces (corners 0-1, 1-2, 0-2),
    as HandLoss.get_edge_idx finds them; each row (smaller, larger)."""
    seen, out = set(), []
    for a, b, c in _np(faces).astype(np.int64).reshape(-1, 3).tolist():
        for e in ((a, b), (b, c), (a, c)):
            e = (min(e), max(e))
            if e not in seen:
                seen.add(e)
                out.append(e)
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 2)


def edge_len_loss(verts, edges, static_len):
    """mean((|v_a - v_b| - static)^2) over [B,E]."""
    length = (verts[..., edges[:, 0], :] - verts[..., edges[:, 1], :]).norm(p=2, dim=-1)
    return ((length - static_len) ** 2).mean()


def edge_csr(edges, V):
    """For every vertex the (edge * 2 + end) entries that read it, ascending -> int32 vptr [V+1], vlist [2E].  Indices are
    range-checked here, on the host, once per edge table (the kernel trusts the lists)."""
    e = _np(edges).astype(np.int64).reshape(-1)
    if e.size == 0 or e.min() < 0 or e.max() >= V:
        raise ValueError('edges name vertex %d of %d' % (int(e.max()) if e.size else -1, V))
    order = np.argsort(e, kind='stable')
    vptr = np.zeros(V + 1, np.int64)
    np.cumsum(np.bincount(e, minlength=V), out=vptr[1:])
    return torch.from_numpy(vptr.astype(np.int32)), torch.from_numpy(order.astype(np.int32))


def batch_contact_loss(anchors_main, anchors_sub, anchor_id, mask, elastic):
    """sum(elastic * |anchors_main[b, anchor_id[b,i,d]] - anchors_sub[b,i]|^2) / mask.sum(); `mask` (a tensor, or its sum as a
    number) enters only through the sum, and a sum <= 0 gives 0."""
    msum = float(mask.sum()) if torch.is_tensor(mask) else float(mask)
    if msum <= 0:
        return (anchors_main.sum() + anchors_sub.sum()) * 0.0
    B, A, D = anchor_id.shape
    indexed = anchors_main[torch.arange(B, device=anchors_main.device)[:, None, None], anchor_id.long()]      # [B,A,D,3]
    dist = ((anchors_sub.unsqueeze(2) - indexed) ** 2).sum(-1)
    return (elastic * dist).sum() / msum


def _hinge(angle, lo, hi):
    return torch.max(torch.relu(angle - hi), torch.relu(lo - angle)) / 180 * math.pi


def ergonomics_loss(ja, zero_ja, side=None):
    """HandLoss.hand_pose_ergonomics_loss: ja, zero_ja [B,15,3,3] (the finger joints' converted frames and those of the
    identity pose) -> scalar."""
    rel = zero_ja.transpose(3, 2) @ ja
    col_x = rel[..., 0]                                                    # [B,15,3]: the first column
    s1 = list(NO_TWIST_SPLAY)
    res = (rel[:, s1, 2, 0] ** 2).mean() + (rel[:, s1, 2, 1] ** 2).mean() + ((rel[:, s1, 2, 2] - 1) ** 2).mean()
    twist = (rel[..., 2, 1] - rel[..., 1, 2]) / 2
    res = res + (twist[:, list(NO_TWIST)] ** 2).mean()
    res = res + (torch.relu(twist[:, THUMB] - 0.5) ** 2).mean()
    bend = torch.atan2(col_x[..., 1], col_x[..., 0]) * 180 / math.pi
    splay = torch.atan2(-col_x[..., 2], col_x[..., 0]) * 180 / math.pi
    for j, (lo, hi) in SPLAY.items():
        res = res + (_hinge(splay[:, j], lo, hi) ** 2).mean()
    for j, (lo, hi) in BEND.items():
        res = res + (_hinge(bend[:, j], lo, hi) ** 2).mean()
    pos = bend.clamp_min(0.0) / 180 * math.pi
    return res + (torch.clamp(pos[:, PINKY] - pos[:, RING] * 3 / 4, max=0) ** 2).mean()


def _identity_quats(n=1):
    q = torch.zeros(n, 16, 4)
    q[..., 0] = 1.0
    return q


class TwoHandPriorLoss(nn.Module):
    """The prior / contact part of `loss_fn` for mode='both' in plain torch:
        quat_norm(r) + quat_norm(l) + edge(r) + edge(l) + lambda_contact * contact + ergo(r) + ergo(l)
    with the right hand as the main hand (its anchors are indexed by `anchor_id`) and the left as the sub hand.
    `mano_right`, `mano_left`: model dicts or pickle paths as `QuatManoLayer` takes them; `faces` [F,3]: the face list the edges
    of BOTH hands are built from (default: the right model's).  `forward(q_r, q_l, verts_r, verts_l, anchors_r, anchors_l)`
    -> (loss, terms[7] in the order above, contact without its weight)."""

    def __init__(self, mano_right, mano_left, lambda_contact=10.0, faces=None):
        super().__init__()
        self.lambda_contact = float(lambda_contact)
        rest = {}
        for side, mano in (('right', mano_right), ('left', mano_left)):
            layer = QuatManoLayer(mano, side=side, center_idx=0)
            with torch.no_grad():
                rest[side] = layer(_identity_quats(), torch.zeros(1, 10))[0][0]
            if side == 'right' and faces is None:
                faces = layer.th_faces
            t0, t1 = axis_tables(side, mano)
            self.register_buffer('inv_m_u_0_' + side, t0)
            self.register_buffer('inv_u_m_1_' + side, t1)
            self.register_buffer('zero_ja_' + side, mano_quat_2_mat(_identity_quats(), (t0, t1), side)[:, 1:].contiguous())
        self._set_mesh(faces, rest['right'], rest['left'])
        self.mask_sum = None

    def _set_mesh(self, faces, rest_right, rest_left):
        edges = edge_index(faces)
        V = rest_right.shape[0]
        if rest_left.shape[0] != V:
            raise ValueError('the two rest meshes differ in size')
        self._edge_lists = edge_csr(edges, V)                                 # range check of the face list
        self.register_buffer('edges', edges)
        static = torch.stack([(r[edges[:, 0]] - r[edges[:, 1]]).norm(p=2, dim=-1) for r in (rest_right, rest_left)])
        self.register_buffer('static_len', static.float().contiguous())      # [2,E]: right, left

    def set_mesh(self, faces, rest_right, rest_left):
        """Another topology than the MANO model's (tests: a handful of vertices).  rest_* [V,3]."""
        self._set_mesh(faces, torch.as_tensor(rest_right).float().cpu(), torch.as_tensor(rest_left).float().cpu())
        dev = self.zero_ja_right.device
        self.edges, self.static_len = self.edges.to(dev), self.static_len.to(dev)

    def set_contacts(self, anchor_id, mask, elastic):
        """The contact constants of a batch: anchor_id [B,A,D] (indices into the MAIN hand's anchors), mask [B,A,D] (only its
        sum is used, taken here), elastic [B,A,D].  Host or device tensors; nothing is read from the device later."""
        anchor_id, mask, elastic = (torch.as_tensor(_np(x)) for x in (anchor_id, mask, elastic))
        if anchor_id.dim() != 3 or mask.shape != anchor_id.shape or elastic.shape != anchor_id.shape:
            raise ValueError('anchor_id, mask, elastic must share one shape [B,A,D]; got %s, %s, %s' %
                             (tuple(anchor_id.shape), tuple(mask.shape), tuple(elastic.shape)))
        if anchor_id.dtype.is_floating_point or anchor_id.dtype == torch.bool:
            raise ValueError('anchor_id must hold integers')
        B, A, D = anchor_id.shape
        if anchor_id.numel() and (int(anchor_id.min()) < 0 or int(anchor_id.max()) >= A):
            raise ValueError('anchor_id names anchor %d..%d of %d' % (int(anchor_id.min()), int(anchor_id.max()), A))
        dev = self.zero_ja_right.device
        self.mask_sum = float(mask.sum())
        self.register_buffer('anchor_id', anchor_id.to(torch.int32).contiguous().to(dev), persistent=False)
        self.register_buffer('elastic', elastic.float().contiguous().to(dev), persistent=False)
        return anchor_id

    def _check(self, q_r, q_l, verts_r, verts_l, anchors_r, anchors_l):
        if self.mask_sum is None:
            raise RuntimeError('call set_contacts(anchor_id, mask, elastic) first')
        B, A, D = self.anchor_id.shape
        V = int(self._edge_lists[0].shape[0]) - 1
        for name, t, shape in (('q_r', q_r, (B, 16, 4)), ('q_l', q_l, (B, 16, 4)), ('verts_r', verts_r, (B, V, 3)),
                               ('verts_l', verts_l, (B, V, 3)), ('anchors_r', anchors_r, (B, A, 3)),
                               ('anchors_l', anchors_l, (B, A, 3))):
            if tuple(t.shape) != shape:
                raise ValueError('%s must be %s; got %s' % (name, list(shape), tuple(t.shape)))
        return B, V, A, D

    def _ergo(self, q, side):
        tables = (getattr(self, 'inv_m_u_0_' + side), getattr(self, 'inv_u_m_1_' + side))
        ja = mano_quat_2_mat(normalize_quaternion(q), tables, side)[:, 1:]
        return ergonomics_loss(ja, getattr(self, 'zero_ja_' + side).to(q.dtype), side[0])

    def forward(self, q_r, q_l, verts_r, verts_l, anchors_r, anchors_l):
        self._check(q_r, q_l, verts_r, verts_l, anchors_r, anchors_l)
        static = self.static_len.to(verts_r.dtype)
        terms = torch.stack([
            quat_norm_loss(q_r), quat_norm_loss(q_l),
            edge_len_loss(verts_r, self.edges, static[0]), edge_len_loss(verts_l, self.edges, static[1]),
            batch_contact_loss(anchors_r, anchors_l, self.anchor_id, self.mask_sum, self.elastic.to(anchors_r.dtype)),
            self._ergo(q_r, 'right'), self._ergo(q_l, 'left')])
        weight = terms.new_tensor([1, 1, 1, 1, self.lambda_contact, 1, 1])
        return (terms * weight).sum(), terms


def contact_csr(anchor_id):
    """anchor_id [B,A,D] -> int32 cptr [B,A+1], clist [B,A*D]: per sample, for every MAIN-hand anchor the (i * D + d) entries
    that index it, ascending."""
    ids = _np(anchor_id).astype(np.int64)
    B, A, D = ids.shape
    flat = ids.reshape(B, A * D)
    if flat.size and (flat.min() < 0 or flat.max() >= A):
        raise ValueError('anchor_id names anchor %d..%d of %d' % (int(flat.min()), int(flat.max()), A))
    clist = np.argsort(flat, axis=1, kind='stable')
    cptr = np.zeros((B, A + 1), np.int64)
    for b in range(B):
        np.cumsum(np.bincount(flat[b], minlength=A), out=cptr[b, 1:])
    return torch.from_numpy(cptr.astype(np.int32)), torch.from_numpy(clist.astype(np.int32))


class _TwoHandPrior(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, q_r, q_l, verts_r, verts_l, anchors_r, anchors_l):
        ins = [t.detach().contiguous() for t in (q_r, q_l, verts_r, verts_l, anchors_r, anchors_l)]
        ops._chk(*ins)                                   # fp32 GPU tensors only: there is no CPU fallback
        c = mod._constants(ins[0].device)
        ops._chk(c['tables'], c['static_len'], c['elastic'])
        ops._chk(c['edges'], c['vptr'], c['vlist'], c['anchor_id'], c['cptr'], c['clist'], dtype=torch.int32)
        B, A, D = c['anchor_id'].shape
        V, E = ins[2].shape[1], c['edges'].shape[0]
        f32 = dict(device=ins[0].device, dtype=torch.float32)
        sizes = [t.numel() for t in ins]
        grads, partial = torch.empty((sum(sizes),), **f32), torch.empty((B, 2, 4), **f32)
        terms, loss = torch.empty((7,), **f32), torch.empty((), **f32)
        inv_mask = 1.0 / mod.mask_sum if mod.mask_sum > 0 else 0.0
        L, st = ops._L(), ops._stream()
        check(L.rih_pose_prior_fwd(*[t.data_ptr() for t in ins], c['tables'].data_ptr(), c['edges'].data_ptr(),
                                   c['static_len'].data_ptr(), c['vptr'].data_ptr(), c['vlist'].data_ptr(),
                                   c['anchor_id'].data_ptr(), c['elastic'].data_ptr(), c['cptr'].data_ptr(),
                                   c['clist'].data_ptr(), inv_mask, mod.lambda_contact, grads.data_ptr(), partial.data_ptr(),
                                   B, V, E, A, D, st), 'rih_pose_prior_fwd')
        check(L.rih_pose_prior_reduce(partial.data_ptr(), mod.lambda_contact, terms.data_ptr(), loss.data_ptr(), B, st),
              'rih_pose_prior_reduce')
        ctx.save_for_backward(grads)
        ctx.shapes = [tuple(t.shape) for t in ins]
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return loss, terms

    @staticmethod
    def backward(ctx, g_loss, g_terms):
        grads, = ctx.saved_tensors
        if g_loss is None:
            return (None,) * 7
        g = g_loss.contiguous()
        ops._chk(g)
        out = torch.empty_like(grads)
        check(ops._L().rih_pose_prior_bwd(grads.data_ptr(), g.data_ptr(), out.data_ptr(), grads.numel(), ops._stream()),
              'rih_pose_prior_bwd')
        views, at = [], 0
        for shape in ctx.shapes:
            n = int(np.prod(shape))
            views.append(out[at:at + n].view(shape))
            at += n
        return (None,) + tuple(views)


class FusedTwoHandPriorLoss(TwoHandPriorLoss):
    """`TwoHandPriorLoss` on csrc/rih_pose_prior.hip: rih_pose_prior_fwd (one workgroup per (sample, hand): the 15 finger
    joints' ergonomics with their analytic quaternion gradient on one lane per joint, the edges strided over the workgroup,
    the contact pairs; it writes per-(sample, hand) partial sums and the complete, already scaled gradients) ->
    rih_pose_prior_reduce (fixed-order sum into terms[7] and the loss); rih_pose_prior_bwd scales the saved gradients by the
    upstream scalar in one launch.  Vertex and main-hand anchor gradients gather through host-built, range-checked lists
    (`edge_csr`, `contact_csr`): no atomics, exact zeros for a vertex without an edge.  `terms` carries no gradient."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._const = {}

    def set_mesh(self, faces, rest_right, rest_left):
        super().set_mesh(faces, rest_right, rest_left)
        self._const = {}

    def set_contacts(self, anchor_id, mask, elastic):
        ids = super().set_contacts(anchor_id, mask, elastic)
        self._csr = contact_csr(ids)
        self._const = {}

    def _joint_tables(self):
        """[2,15,18] fp32 per hand and finger joint: Lm = zero_ja^T invM_U_n_0^T and Rm = invU_M_n_1^T, so that the relative
        frame is Lm R(q) Rm (products taken in fp64)."""
        out = []
        for side in ('right', 'left'):
            t0, t1, z = (getattr(self, n + side).double().cpu()
                         for n in ('inv_m_u_0_', 'inv_u_m_1_', 'zero_ja_'))
            lm = z.reshape(15, 3, 3).transpose(1, 2) @ t0[1:].transpose(1, 2)
            out.append(torch.cat([lm.reshape(15, 9), t1[1:].transpose(1, 2).reshape(15, 9)], 1))
        return torch.stack(out).float().contiguous()

    def _constants(self, device):
        key = str(device)
        if key not in self._const:
            cptr, clist = self._csr
            vptr, vlist = self._edge_lists
            self._const[key] = dict(
                tables=self._joint_tables().to(device), edges=self.edges.to(torch.int32).contiguous().to(device),
                static_len=self.static_len.contiguous().to(device), vptr=vptr.to(device), vlist=vlist.to(device),
                anchor_id=self.anchor_id.contiguous().to(device), elastic=self.elastic.contiguous().to(device),
                cptr=cptr.contiguous().to(device), clist=clist.contiguous().to(device))
        return self._const[key]

    def forward(self, q_r, q_l, verts_r, verts_l, anchors_r, anchors_l):
        self._check(q_r, q_l, verts_r, verts_l, anchors_r, anchors_l)
        return _TwoHandPrior.apply(self, q_r, q_l, verts_r, verts_l, anchors_r, anchors_l)
