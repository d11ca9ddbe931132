"""Training loss of the graph model as plain torch ops on the GPU (host-side mirror of core/Loss.py).

SURVEY.md 8a row a15 / 8f-2: the loss sits right after the hot path; its FLOPs are negligible, so round 1 keeps it
as PyTorch elementwise ops (fusing it into HIP kernels is the "next" row).  Semantics follow
core/Loss.py:20-164 (GraphLoss) and :201-277 (calc_loss_GCN): SmoothL1 on 3-D vertices and regressed joints,
MSE on normalised 2-D vertices, face-normal and edge-length terms, the same at the coarse (252-vertex) level, aux
(hms/mask/dense) loss disabled unless `aux=` hands in a renderih_amd.aux_heads loss, edge term gated by epoch >= NORM_EPOCH,
right hand shifted by root_rel.

MANO-head loss (core/Loss_mano.py: ManoLoss :62-219, mano_loss_GCN :245-335; the loss of `load_new_model`), reproduced with
its quirks by `ManoLoss` / `mano_loss_GCN` (torch mirror) and `FusedManoLoss` / `mano_loss_GCN_fused` (csrc/rih_mano_loss.hip):
  * L1 = SmoothL1 (beta 1), L2 = MSE, both means over all elements; 21-joint regressor with tips 745, 317, 444, 556, 673.
  * per hand, then averaged over the two hands: vert2d, vert3d, joint, norm, edge (as GraphLoss, no coarse terms),
    pose = MSE over [B,16,3,3] of batch_rodrigues(pred) against batch_rodrigues(label), shape = MSE over [B,10].
  * batch_rodrigues as written: angle |a + 1e-8|, axis a / angle (unshifted a), q = [cos(angle/2), sin(angle/2) axis],
    q normalised again, quat2mat; differentiated through that chain (finite at a = 0, as torch autograd).
  * the right-hand ground truth is shifted by the root_rel label before any term.
  * rootrel = MANO_REL * MSE(otherInfo['root_rel'], root_rel), not halved; regularize = 0.005 (sum left_shape^2 +
    sum right_shape^2), a sum over the batch, not halved, not configurable.
  * upsample_norm = SmoothL1(w - w0) when the trainer passes w (`.weight.data`: value only, no gradient), else zeros.
  * total = LABEL_3D (vert3d + joint) + LABEL_2D vert2d + NORMAL norm + alpha EDGE edge + MANO_POSE pose + MANO_SHAPE shape
    + rootrel + regularize + UPSAMPLE upsample_norm, alpha = 0 if epoch < NORM_EPOCH else 1; weights from cfg.LOSS_WEIGHT
    (utils/defaults.yaml layout).  Returns (total, {'total_loss': 0}, mano_loss_dict with ten terms, {}).
"""
import numpy as np
import torch
import torch.nn.functional as F

NEW_ORDER = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]
TIPS = [745, 317, 444, 556, 673]

DEFAULT_WEIGHTS = {'LABEL_3D': 100.0, 'LABEL_2D': 50.0, 'NORMAL': 10.0, 'EDGE': 2000.0, 'NORM_EPOCH': 50,
                   'UPSAMPLE': 1.0}


def joint_regressor_21(J_regressor):
    """core/Loss.py:38-53: 16 MANO joints + 5 one-hot finger tips, reordered to the 21-joint convention."""
    tips = torch.zeros((5, J_regressor.shape[1]), dtype=J_regressor.dtype, device=J_regressor.device)
    for i, v in enumerate(TIPS):
        tips[i, v] = 1.0
    return torch.cat([J_regressor, tips], 0)[NEW_ORDER].contiguous()


class GraphLoss:
    def __init__(self, J_regressor, faces, level=4, device='cuda', upsample_weight=None):
        self.device = device
        self.level = level + 1
        self.J_regressor = joint_regressor_21(J_regressor.clone().detach().float()).to(device)
        self.faces = torch.from_numpy(np.asarray(faces).astype(np.int64)).to(device)
        self.upsample_weight = None if upsample_weight is None else upsample_weight.to(device)

    @staticmethod
    def _edges(v, faces):
        t = v[:, faces]                                             # B x F x 3 x 3
        return torch.stack([t[:, :, 0] - t[:, :, 1], t[:, :, 1] - t[:, :, 2], t[:, :, 2] - t[:, :, 0]], dim=2)

    def norm_loss(self, pred, gt):
        eg, ep = self._edges(gt, self.faces), self._edges(pred, self.faces)
        n = F.normalize(torch.cross(eg[:, :, 0], eg[:, :, 1], dim=-1), dim=-1).unsqueeze(2)
        d = torch.sum(F.normalize(ep, dim=-1) * n, dim=-1)
        return F.smooth_l1_loss(d, torch.zeros_like(d))

    def edge_loss(self, pred, gt):
        lg = torch.linalg.norm(self._edges(gt, self.faces), dim=-1)
        lp = torch.linalg.norm(self._edges(pred, self.faces), dim=-1)
        return F.smooth_l1_loss(lp, lg)

    def calc_mano_loss(self, v3d_pred, v2d_pred, v3d_gt, v2d_gt, img_size):
        return {'vert2d_loss': F.mse_loss(v2d_pred / img_size * 2 - 1, v2d_gt / img_size * 2 - 1),
                'vert3d_loss': F.smooth_l1_loss(v3d_pred, v3d_gt),
                'joint_loss': F.smooth_l1_loss(torch.matmul(self.J_regressor, v3d_pred),
                                               torch.matmul(self.J_regressor, v3d_gt)),
                'norm_loss': self.norm_loss(v3d_pred, v3d_gt),
                'edge_loss': self.edge_loss(v3d_pred, v3d_gt)}

    @staticmethod
    def _down(x, p=2):
        B, V, D = x.shape
        return x[:, :V // p * p].reshape(B, V // p, p, D).mean(2)   # AvgPool1d(p) along V (floor, like torch)

    def calc_loss(self, converter, v3d_gt, v2d_gt, v3d_pred, v2d_pred, v3dList, v2dList, img_size):
        mano = self.calc_mano_loss(v3d_pred, v2d_pred, v3d_gt, v2d_gt, img_size)
        g3, g2 = converter.vert_to_GCN(v3d_gt), converter.vert_to_GCN(v2d_gt)
        l3, l2 = [], []
        for _ in range(self.level):
            l3.append(g3)
            l2.append(g2)
            g3, g2 = self._down(g3), self._down(g2)
        coarse = {'v3d_loss': [], 'v2d_loss': []}
        for p3, p2 in zip(v3dList, v2dList):
            j = [t.shape[1] for t in l3].index(p3.shape[1])
            coarse['v3d_loss'].append(F.smooth_l1_loss(p3, l3[j]))
            coarse['v2d_loss'].append(F.mse_loss(p2 / img_size * 2 - 1, l2[j] / img_size * 2 - 1))
        return mano, coarse


def calc_loss_GCN(weights, epoch, loss_left, loss_right, converter_left, converter_right, result, paramsDict,
                  handDictList, otherInfo, v2d_l, v2d_r, v3d_l, v3d_r, root_rel, img_size=256, upsample_weight=None,
                  aux=None, mask=None, dense=None, hms=None, joints2d=None, sigma=None):
    """core/Loss.py:201-277 (aux loss disabled there, :211).  aux: an aux_heads.AuxLoss / FusedAuxLoss switches that line on --
    calc_aux_loss on otherInfo's 'mask', 'dense', 'hms' against the labels mask, dense and hms (or joints2d with sigma) -- and
    the call then returns (total, mano, aux_lost_dict) with the aux total inside the total."""
    w = dict(DEFAULT_WEIGHTS)
    w.update(weights or {})
    v3d_r = v3d_r + root_rel.unsqueeze(1)
    out = {}
    for side, gl, conv, v3, v2 in (('left', loss_left, converter_left, v3d_l, v2d_l),
                                   ('right', loss_right, converter_right, v3d_r, v2d_r)):
        out[side] = gl.calc_loss(conv, v3, v2, result['verts3d'][side], result['verts2d'][side],
                                 [h['verts3d'][side] for h in handDictList],
                                 [h['verts2d'][side] for h in handDictList], img_size)
    mano = {k: (out['left'][0][k] + out['right'][0][k]) / 2 for k in out['left'][0]}
    alpha = 0 if epoch < w['NORM_EPOCH'] else 1
    total = w['LABEL_3D'] * mano['vert3d_loss'] + w['LABEL_2D'] * mano['vert2d_loss'] + \
        w['LABEL_3D'] * mano['joint_loss'] + w['NORMAL'] * mano['norm_loss'] + alpha * w['EDGE'] * mano['edge_loss']
    for i in range(len(out['left'][1]['v3d_loss'])):
        total = total + w['LABEL_3D'] * (out['left'][1]['v3d_loss'][i] + out['right'][1]['v3d_loss'][i]) / 2 \
            + w['LABEL_2D'] * (out['left'][1]['v2d_loss'][i] + out['right'][1]['v2d_loss'][i]) / 2
    if upsample_weight is not None and loss_left.upsample_weight is not None:
        total = total + w['UPSAMPLE'] * F.smooth_l1_loss(upsample_weight - loss_left.upsample_weight,
                                                         torch.zeros_like(upsample_weight))
    if aux is not None:
        return _with_aux(total, mano, aux, otherInfo, mask, dense, hms, joints2d, sigma)
    return total, mano


def _with_aux(total, mano, aux, otherInfo, mask, dense, hms, joints2d, sigma):
    """The un-commented core/Loss.py:211: aux_lost_dict = calc_aux_loss(cfg, graph_loss_left, otherInfo, mask, dense, hms)."""
    heads = {k: otherInfo[k] for k in ('mask', 'dense', 'hms') if k in otherInfo}
    aux_total, aux_lost_dict = aux(heads, mask, dense, hms=hms, joints2d=joints2d, sigma=sigma)
    return total + aux_total, mano, aux_lost_dict


# ------------------------------------------------------------------------------------------------ MANO-head loss (mirror)
MANO_DEFAULT_WEIGHTS = {'LABEL_3D': 100.0, 'LABEL_2D': 50.0, 'MANO_POSE': 0.5, 'MANO_SHAPE': 0.01, 'MANO_REL': 1.0,
                        'NORMAL': 10.0, 'EDGE': 2000.0, 'NORM_EPOCH': 50, 'UPSAMPLE': 1.0}
MANO_TERMS = ['vert2d_loss', 'vert3d_loss', 'joint_loss', 'norm_loss', 'edge_loss', 'pose_loss', 'shape_loss',
              'rootrel_loss', 'regularize_loss', 'upsample_norm_loss']


def mano_loss_weights(weights=None):
    """Flat weights of the MANO-head recipe.  `weights`: None (utils/defaults.yaml), a flat dict with the keys of
    MANO_DEFAULT_WEIGHTS, or the reference's nested cfg.LOSS_WEIGHT (DATA.*, GRAPH.NORM.*, NORM.UPSAMPLE), flattened
    explicitly key by key."""
    w = dict(MANO_DEFAULT_WEIGHTS)
    if weights is None:
        return w
    get = weights.get if isinstance(weights, dict) else (lambda k, d=None: getattr(weights, k, d))
    if get('DATA') is not None or get('GRAPH') is not None:
        def sub(node, *path):
            for k in path:
                if node is None:
                    return None
                node = node.get(k) if isinstance(node, dict) else getattr(node, k, None)
            return node
        for key, path in (('LABEL_3D', ('DATA', 'LABEL_3D')), ('LABEL_2D', ('DATA', 'LABEL_2D')),
                          ('MANO_POSE', ('DATA', 'MANO_POSE')), ('MANO_SHAPE', ('DATA', 'MANO_SHAPE')),
                          ('MANO_REL', ('DATA', 'MANO_REL')), ('NORMAL', ('GRAPH', 'NORM', 'NORMAL')),
                          ('EDGE', ('GRAPH', 'NORM', 'EDGE')), ('NORM_EPOCH', ('GRAPH', 'NORM', 'NORM_EPOCH')),
                          ('UPSAMPLE', ('NORM', 'UPSAMPLE'))):
            v = sub(weights, *path)
            if v is not None:
                w[key] = v
        return w
    unknown = set(weights) - set(w)
    if unknown:
        raise KeyError('unknown MANO loss weights %s' % sorted(unknown))
    w.update(weights)
    return w


def quat2mat(quat):
    """core/Loss_mano.py:18-46: [N,4] (w, x, y, z), normalised again, -> [N,3,3]."""
    q = quat / quat.norm(p=2, dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    w2, x2, y2, z2 = w.pow(2), x.pow(2), y.pow(2), z.pow(2)
    wx, wy, wz = w * x, w * y, w * z
    xy, xz, yz = x * y, x * z, y * z
    return torch.stack([w2 + x2 - y2 - z2, 2 * xy - 2 * wz, 2 * wy + 2 * xz, 2 * wz + 2 * xy, w2 - x2 + y2 - z2,
                        2 * yz - 2 * wx, 2 * xz - 2 * wy, 2 * wx + 2 * yz, w2 - x2 - y2 + z2], dim=1).view(-1, 3, 3)


def batch_rodrigues(axisang):
    """core/Loss_mano.py:48-59 as written: angle |a + 1e-8|, axis a / angle (unshifted a), half-angle quaternion -> [N,9]."""
    angle = torch.norm(axisang + 1e-8, p=2, dim=1).unsqueeze(-1)
    axis = torch.div(axisang, angle)
    angle = angle * 0.5
    quat = torch.cat([torch.cos(angle), torch.sin(angle) * axis], dim=1)
    return quat2mat(quat).view(-1, 9)


class ManoLoss(GraphLoss):
    """core/Loss_mano.py:62-219 (the loss the reference trains `load_new_model` with).  `upsample_weight`: the initial
    up-sampling matrix w0 of misc/upsample.pkl (the reference loads it in __init__; None = renderih_amd.assets' stand-in)."""

    def __init__(self, J_regressor, faces, level=4, device='cuda', upsample_weight=None):
        if upsample_weight is None:
            from . import assets
            upsample_weight = torch.from_numpy(assets.synthetic_upsample_weight())
        super().__init__(J_regressor, faces, level=level, device=device, upsample_weight=upsample_weight)

    def calc_mano_loss(self, v3d_pred, v2d_pred, v3d_gt, v2d_gt, img_size, pred_pose, pred_shape, lp_gt, ls_gt):
        d = GraphLoss.calc_mano_loss(self, v3d_pred, v2d_pred, v3d_gt, v2d_gt, img_size)
        d['pose_loss'] = F.mse_loss(batch_rodrigues(pred_pose.reshape(-1, 3)).reshape(-1, 16, 3, 3),
                                    batch_rodrigues(lp_gt.reshape(-1, 3)).reshape(-1, 16, 3, 3))
        d['shape_loss'] = F.mse_loss(pred_shape, ls_gt)
        return d

    def calc_loss(self, converter, v3d_gt, v2d_gt, v3d_pred, v2d_pred, v3dList, v2dList, img_size, pred_pose, pred_shape,
                  lp_gt, ls_gt):
        """core/Loss_mano.py:173-206: the per-hand terms only (the coarse terms are commented out there)."""
        return self.calc_mano_loss(v3d_pred, v2d_pred, v3d_gt, v2d_gt, img_size, pred_pose, pred_shape, lp_gt, ls_gt)

    def upsample_weight_loss(self, w):
        x = w - self.upsample_weight
        return F.smooth_l1_loss(x, torch.zeros_like(x))

    def rel_loss(self, v1, v2, v1_gt, v2_gt):
        rel_gt = torch.linalg.norm(v1.unsqueeze(1) - v2.unsqueeze(2), dim=-1)
        rel_pred = torch.linalg.norm(v1_gt.unsqueeze(1) - v2_gt.unsqueeze(2), dim=-1)
        return F.smooth_l1_loss(rel_gt, rel_pred)

    def range_loss(self, label, Min, Max):
        z = lambda p: F.smooth_l1_loss(p, torch.zeros_like(p))        # noqa: E731
        return z(torch.clamp(Min - label, min=0.)) + z(torch.clamp(label - Max, min=0.))


def mano_loss_GCN(cfg, epoch, loss_left, loss_right, converter_left, converter_right, result, paramsDict, handDictList,
                  otherInfo, mask, dense, hms, v2d_l, j2d_l, v2d_r, j2d_r, v3d_l, j3d_l, v3d_r, j3d_r, root_rel, img_size,
                  lp_gt, ls_gt, rp_gt, rs_gt, upsample_weight=None):
    """core/Loss_mano.py:245-335.  cfg: the reference config (cfg.LOSS_WEIGHT is read), a weights dict, or None."""
    w = mano_loss_weights(getattr(cfg, 'LOSS_WEIGHT', cfg) if cfg is not None else None)
    mi = otherInfo['verts3d_MANO_list']
    left_pose, left_shape = mi['left']['mano_pose'], mi['left']['mano_shape']
    right_pose, right_shape = mi['right']['mano_pose'], mi['right']['mano_shape']
    v3d_r = v3d_r + root_rel.unsqueeze(1)
    dl = loss_left.calc_loss(converter_left, v3d_l, v2d_l, result['verts3d']['left'], result['verts2d']['left'], [], [],
                             img_size, left_pose, left_shape, lp_gt, ls_gt)
    dr = loss_right.calc_loss(converter_right, v3d_r, v2d_r, result['verts3d']['right'], result['verts2d']['right'], [], [],
                              img_size, right_pose, right_shape, rp_gt, rs_gt)
    d = {k: (dl[k] + dr[k]) / 2 for k in dl}
    alpha = 0 if epoch < w['NORM_EPOCH'] else 1
    if upsample_weight is not None:
        d['upsample_norm_loss'] = loss_left.upsample_weight_loss(upsample_weight)
    else:
        d['upsample_norm_loss'] = torch.zeros_like(d['vert3d_loss'])
    d['rootrel_loss'] = w['MANO_REL'] * F.mse_loss(otherInfo['root_rel'], root_rel)
    d['regularize_loss'] = 0.005 * torch.mean(torch.sum(left_shape ** 2) + torch.sum(right_shape ** 2))
    total = w['LABEL_3D'] * d['vert3d_loss'] + w['LABEL_2D'] * d['vert2d_loss'] + w['LABEL_3D'] * d['joint_loss'] + \
        w['NORMAL'] * d['norm_loss'] + alpha * w['EDGE'] * d['edge_loss'] + w['MANO_POSE'] * d['pose_loss'] + \
        w['MANO_SHAPE'] * d['shape_loss'] + d['rootrel_loss'] + d['regularize_loss']
    total = total + w['UPSAMPLE'] * d['upsample_norm_loss']
    return total, {'total_loss': 0}, d, {}


# ------------------------------------------------------------------------------------------------ fused HIP loss
class _FusedLoss:
    """What FusedMeshLoss and FusedManoLoss share: the constant topology of both hands (faces, vertex->face adjacency,
    21-joint regressor) on the host and, once per device, on the device; and the term weights that the kernels read at
    run time.  A subclass gives `weights(B)` -> (weights[NW], counts[7]) and, for a coarse level, `_coarse()`."""
    NW = None           # number of weights in front of the seven counts in the device slot

    def __init__(self, w, loss_left, loss_right, img_size):
        self.w = w
        self.img_size = img_size
        self.epoch = 0
        self._host = {}
        for side, gl in (('left', loss_left), ('right', loss_right)):
            faces = gl.faces.detach().cpu().numpy().astype(np.int32)
            V = gl.J_regressor.shape[1]
            order = np.argsort(faces.reshape(-1), kind='stable')            # entries (face*3 + corner) grouped by vertex
            counts = np.bincount(faces.reshape(-1), minlength=V)
            vptr = np.zeros(V + 1, np.int32)
            vptr[1:] = np.cumsum(counts)
            self._host[side] = dict(faces=faces, vptr=vptr, vlist=order.astype(np.int32),
                                    J=gl.J_regressor.detach().cpu().float().contiguous(), V=V, F=faces.shape[0],
                                    NJ=gl.J_regressor.shape[0])
        self._dev = {}

    def device_weights(self, B, device):
        """(weights[NW], counts[7]) as views of one device tensor that the kernels read at run time.  The tensor is
        rewritten IN PLACE (outside any stream capture) only when the values change -- batch size, or the epoch gate of
        the edge term (core/Loss.py:211-220, NORM_EPOCH) -- so a hipGraph captured at epoch 0 picks the edge term up
        when the trainer calls `set_epoch()` (or this loss eagerly) at a later epoch."""
        w, cnt = self.weights(B)
        vals = tuple(w) + tuple(cnt)
        # one slot per (device, batch size): evaluating this loss on another batch size between two replays of a captured
        # step must not rewrite the weights / counts that the graph reads
        key = ('wdev', device, B)
        if key not in self._dev:
            self._dev[key] = [torch.zeros(self.NW + 7, device=device, dtype=torch.float32), None]
        slot = self._dev[key]
        if slot[1] != vals:
            if torch.cuda.is_available() and device.type == 'cuda' and torch.cuda.is_current_stream_capturing():
                raise RuntimeError('%s: the term weights changed during stream capture (epoch gate or batch '
                                   'size); call set_epoch() / run one eager step before capturing' % type(self).__name__)
            slot[0].copy_(torch.tensor(vals, dtype=torch.float32))
            slot[1] = vals
        return slot[0][:self.NW], slot[0][self.NW:]

    def set_epoch(self, epoch, B=None, device=None):
        """Move the epoch gate (edge term on from NORM_EPOCH).  With a replayed hipGraph pass the captured batch size and
        device so that the device-resident weights are refreshed in place (without them: every slot that exists)."""
        self.epoch = epoch
        if B is not None and device is not None:
            self.device_weights(B, torch.device(device))
        else:                                       # all captured batch sizes / devices
            for key in [k for k in self._dev if k[0] == 'wdev']:
                self.device_weights(key[2], key[1])

    def _coarse(self, h, device):
        """(perm on the device, Vc, pool) of the coarse level; none here."""
        return None, 0, 0

    def topo(self, side, device):
        from ._lib import MeshTopo
        key = (side, device)
        if key not in self._dev:
            h = self._host[side]
            t = {k: torch.as_tensor(h[k], device=device) for k in ('faces', 'vptr', 'vlist')}
            t['J'] = h['J'].to(device)
            t['perm'], Vc, pool = self._coarse(h, device)
            self._dev[key] = (t, MeshTopo(t['faces'].data_ptr(), t['vptr'].data_ptr(), t['vlist'].data_ptr(),
                                          t['J'].data_ptr(), None if t['perm'] is None else t['perm'].data_ptr(),
                                          h['V'], h['F'], h['NJ'], Vc, pool))
        return self._dev[key][1]


def _scaled(ctx, g_total):
    """The backward of both fused losses: the kernels already produced the gradients, scale them by the incoming one.  Out
    of place: the saved gradients may be read again (retain_graph); ONE multi-tensor launch instead of a clone per tensor."""
    return tuple(torch._foreach_mul(list(ctx.saved_tensors), g_total))


class _MeshLossFn(torch.autograd.Function):
    """Total loss of calc_loss_GCN for both hands in three launches (rih_mesh_loss x 2 + rih_mesh_loss_final); the
    kernel already produced the gradients, backward only scales them by the incoming gradient."""

    @staticmethod
    def forward(ctx, fused, v3l, v2l, c3l, c2l, v3r, v2r, c3r, c2r, gt3l, gt2l, gt3r, gt2r, root_rel):
        import ctypes as C
        from . import _lib
        from .ops import _stream, check
        lib = _lib.load()
        B = v3l.shape[0]
        wa, ca = fused.device_weights(B, v3l.device)     # device-resident: a captured graph follows set_epoch()
        preds = [t.contiguous() for t in (v3l, v2l, c3l, c2l, v3r, v2r, c3r, c2r)]
        grads = [torch.empty_like(t) for t in preds]
        parts = torch.empty((2, B, 8), device=v3l.device, dtype=torch.float32)
        out = torch.empty((8,), device=v3l.device, dtype=torch.float32)
        for h, (gt3, gt2, shift) in enumerate(((gt3l, gt2l, None), (gt3r, gt2r, root_rel))):
            p, g = preds[4 * h:4 * h + 4], grads[4 * h:4 * h + 4]
            topo = fused.topo('left' if h == 0 else 'right', v3l.device)
            check(lib.rih_mesh_loss(C.byref(topo), p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), p[3].data_ptr(),
                                    gt3.contiguous().data_ptr(), gt2.contiguous().data_ptr(),
                                    0 if shift is None else shift.contiguous().data_ptr(), wa.data_ptr(),
                                    float(fused.img_size),
                                    g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(),
                                    parts[h].data_ptr(), B, _stream()), 'rih_mesh_loss')
        check(lib.rih_mesh_loss_final(parts[0].data_ptr(), parts[1].data_ptr(), B, wa.data_ptr(), ca.data_ptr(),
                                      out.data_ptr(), _stream()),
              'rih_mesh_loss_final')
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        return (None,) + _scaled(ctx, g_total) + (None,) * 5


class FusedMeshLoss(_FusedLoss):
    """GPU drop-in for `calc_loss_GCN` (same arguments and total) on the fused HIP kernel.  Holds the constant
    topology of both hands on the device: faces, vertex->face adjacency, 21-joint regressor, graph permutation."""

    NW = 7

    def __init__(self, loss_left, loss_right, converter_left, converter_right, weights=None, img_size=256):
        w = dict(DEFAULT_WEIGHTS)
        w.update(weights or {})
        super().__init__(w, loss_left, loss_right, img_size)
        for side, conv in (('left', converter_left), ('right', converter_right)):
            self._host[side]['perm'] = np.asarray(conv.graph_perm, dtype=np.int32)
        self.Vc = None

    def weights(self, B):
        h = self._host['left']
        V, F, NJ, Vc = h['V'], h['F'], h['NJ'], self.Vc
        cnt = [B * V * 2, B * V * 3, B * NJ * 3, B * F * 3, B * F * 3, B * Vc * 3, B * Vc * 2]
        alpha = 0.0 if self.epoch < self.w['NORM_EPOCH'] else 1.0
        lw = [self.w['LABEL_2D'], self.w['LABEL_3D'], self.w['LABEL_3D'], self.w['NORMAL'], alpha * self.w['EDGE'],
              self.w['LABEL_3D'], self.w['LABEL_2D']]
        return [0.5 * a / c for a, c in zip(lw, cnt)], [float(c) for c in cnt]

    def set_epoch(self, epoch, B=None, device=None):
        """As _FusedLoss.set_epoch; before the first call of this loss the coarse size, hence the counts, are unknown and
        no slot exists: only the gate moves."""
        if self.Vc is None:
            self.epoch = epoch
        else:
            super().set_epoch(epoch, B, device)

    def _coarse(self, h, device):
        pool = h['perm'].shape[0] // self.Vc
        assert pool * self.Vc == h['perm'].shape[0] and pool & (pool - 1) == 0
        return torch.as_tensor(h['perm'], device=device), self.Vc, pool

    def __call__(self, epoch, result, handDictList, v2d_l, v2d_r, v3d_l, v3d_r, root_rel):
        """Returns (total, terms) with terms = [total, vert2d, vert3d, joint, norm, edge, coarse3d, coarse2d].
        epoch=None keeps the gate where `set_epoch()` put it (what a `loss_fn` handed to TrainStep should pass: a literal 0
        there would switch the edge term off again on every eager step)."""
        if epoch is not None:
            self.epoch = epoch
        assert len(handDictList) == 1, 'one coarse level (the reference decoder emits exactly one)'
        hd = handDictList[0]
        Vc = hd['verts3d']['left'].shape[1]
        if self.Vc not in (None, Vc):
            self._dev = {k: v for k, v in self._dev.items() if k[0] == 'wdev'}
            for v in self._dev.values():
                v[1] = None
        self.Vc = Vc
        total, terms = _MeshLossFn.apply(self, result['verts3d']['left'], result['verts2d']['left'], hd['verts3d']['left'],
                                         hd['verts2d']['left'], result['verts3d']['right'], result['verts2d']['right'],
                                         hd['verts3d']['right'], hd['verts2d']['right'], v3d_l, v2d_l, v3d_r, v2d_r, root_rel)
        return total, terms


def calc_loss_GCN_fused(fused, epoch, result, paramsDict, handDictList, otherInfo, v2d_l, v2d_r, v3d_l, v3d_r, root_rel,
                        upsample_weight=None, upsample_target=None, aux=None, mask=None, dense=None, hms=None, joints2d=None,
                        sigma=None):
    """`calc_loss_GCN` on the fused kernel: same total; the mano dict carries the reference's five terms.  aux (an
    aux_heads.FusedAuxLoss or AuxLoss) with the labels mask, dense and hms / joints2d: as in calc_loss_GCN, three values return.
    `upsample_weight` / `upsample_target`: the trainable up-sampling matrix and its initial value -- the UPSAMPLE term of
    core/Loss.py:222-224, which the reference adds when the up-sampling layer is not frozen (a tiny torch expression on
    one 778x252 matrix; with the default frozen layer both are None and the term is absent, as in the reference)."""
    if (upsample_weight is None) != (upsample_target is None):
        raise ValueError('calc_loss_GCN_fused: pass upsample_weight and upsample_target together (or neither)')
    total, terms = fused(epoch, result, handDictList, v2d_l, v2d_r, v3d_l, v3d_r, root_rel)
    if upsample_weight is not None:
        total = total + fused.w['UPSAMPLE'] * F.smooth_l1_loss(upsample_weight - upsample_target,
                                                                torch.zeros_like(upsample_weight))
    mano = {'vert2d_loss': terms[1], 'vert3d_loss': terms[2], 'joint_loss': terms[3], 'norm_loss': terms[4],
            'edge_loss': terms[5]}
    if aux is not None:
        return _with_aux(total, mano, aux, otherInfo, mask, dense, hms, joints2d, sigma)
    return total, mano


# ------------------------------------------------------------------------------------------------ fused MANO-head loss
class _ManoLossFn(torch.autograd.Function):
    """Total of mano_loss_GCN (without the value-only up-sampling term) in three launches (rih_mano_loss x 2 +
    rih_mano_loss_final); the kernels already produced the gradients, backward only scales them by the incoming one."""

    @staticmethod
    def forward(ctx, fused, img_size, v3l, v2l, pl, sl, v3r, v2r, pr, sr, rel, gt3l, gt2l, gpl, gsl, gt3r, gt2r, gpr, gsr,
                root_rel):
        import ctypes as C
        from . import _lib
        from .ops import _stream, check
        lib = _lib.load()
        B = v3l.shape[0]
        wa, ca = fused.device_weights(B, v3l.device)     # device-resident: a captured graph follows set_epoch()
        flat = lambda t: t.reshape(B, -1).contiguous()                          # noqa: E731
        preds = [v3l.contiguous(), v2l.contiguous(), flat(pl), flat(sl), v3r.contiguous(), v2r.contiguous(), flat(pr),
                 flat(sr), rel.contiguous()]
        labels = [gt3l.contiguous(), gt2l.contiguous(), flat(gpl), flat(gsl), gt3r.contiguous(), gt2r.contiguous(),
                  flat(gpr), flat(gsr)]
        from . import ops
        ops._chk(*preds, *labels, root_rel)              # HIP kernels only: GPU float32 tensors
        for t in preds + labels + [root_rel]:
            if t.dtype != torch.float32 or t.device != v3l.device or t.shape[0] != B:
                raise ValueError('mano_loss_GCN_fused: every input must be float32 on %s with batch size %d' % (v3l.device, B))
        V = fused._host['left']['V']
        want = [(B, V, 3), (B, V, 2)] * 2
        for t, shp in zip(preds[0:2] + preds[4:6] + labels[0:2] + labels[4:6], want + want):
            if tuple(t.shape) != shp:
                raise ValueError('mano_loss_GCN_fused: a mesh tensor has shape %s, expected %s' % (tuple(t.shape), shp))
        if tuple(rel.shape) != (B, 3) or tuple(root_rel.shape) != (B, 3):
            raise ValueError('mano_loss_GCN_fused: root_rel must be [B, 3]')
        grads = [torch.empty_like(t) for t in preds]
        parts = torch.empty((2, B, 8), device=v3l.device, dtype=torch.float32)
        out = torch.empty((10,), device=v3l.device, dtype=torch.float32)
        rr = root_rel.contiguous()
        for h, side in enumerate(('left', 'right')):
            p, g, lab = preds[4 * h:4 * h + 4], grads[4 * h:4 * h + 4], labels[4 * h:4 * h + 4]
            check(lib.rih_mano_loss(C.byref(fused.topo(side, v3l.device)), p[0].data_ptr(), p[1].data_ptr(),
                                    p[2].data_ptr(), p[3].data_ptr(), lab[0].data_ptr(), lab[1].data_ptr(),
                                    lab[2].data_ptr(), lab[3].data_ptr(), 0 if h == 0 else rr.data_ptr(),
                                    p[2].shape[1], p[3].shape[1], wa.data_ptr(), float(img_size), g[0].data_ptr(),
                                    g[1].data_ptr(), g[2].data_ptr(), g[3].data_ptr(), parts[h].data_ptr(), B, _stream()),
                  'rih_mano_loss')
        check(lib.rih_mano_loss_final(parts[0].data_ptr(), parts[1].data_ptr(), preds[8].data_ptr(), rr.data_ptr(), B,
                                      wa.data_ptr(), ca.data_ptr(), grads[8].data_ptr(), out.data_ptr(), _stream()),
              'rih_mano_loss_final')
        grads = [g.view(t.shape) for g, t in zip(grads, (v3l, v2l, pl, sl, v3r, v2r, pr, sr, rel))]
        ctx.save_for_backward(*grads)
        ctx.mark_non_differentiable(out)
        return out[0], out

    @staticmethod
    def backward(ctx, g_total, _g_terms):
        return (None, None) + _scaled(ctx, g_total) + (None,) * 9


class FusedManoLoss(_FusedLoss):
    """GPU drop-in for `mano_loss_GCN` (same total, terms and gradients) on the fused HIP kernel
    (csrc/rih_mano_loss.hip).  `loss_left` / `loss_right`: the ManoLoss (or GraphLoss) of each hand, whose faces, 21-joint
    regressor and up-sampling matrix w0 are held on the device.  `weights`: None, a flat dict, or the reference's nested
    cfg.LOSS_WEIGHT (see mano_loss_weights)."""

    NW = 9

    def __init__(self, loss_left, loss_right, weights=None, img_size=256):
        super().__init__(mano_loss_weights(weights), loss_left, loss_right, img_size)
        w0 = getattr(loss_left, 'upsample_weight', None)
        self.upsample_target = None if w0 is None else w0.detach()

    def weights(self, B):
        """(weights[9], counts[7]): the weight of each raw sum the kernels form, and the element counts of the seven
        per-hand terms."""
        h = self._host['left']
        V, F, NJ = h['V'], h['F'], h['NJ']
        cnt = [B * V * 2, B * V * 3, B * NJ * 3, B * F * 3, B * F * 3, B * 16 * 9, B * 10]
        alpha = 0.0 if self.epoch < self.w['NORM_EPOCH'] else 1.0
        lw = [self.w['LABEL_2D'], self.w['LABEL_3D'], self.w['LABEL_3D'], self.w['NORMAL'], alpha * self.w['EDGE'],
              self.w['MANO_POSE'], self.w['MANO_SHAPE']]
        w = [0.5 * a / c for a, c in zip(lw, cnt)] + [self.w['MANO_REL'] / (3.0 * B), 0.005]
        return w, [float(c) for c in cnt]

    def __call__(self, epoch, result, otherInfo, v2d_l, v2d_r, v3d_l, v3d_r, root_rel, lp_gt, ls_gt, rp_gt, rs_gt,
                 img_size=None, upsample_weight=None):
        """Returns (total, terms): the reference's mano_loss_dict (ten 0-d tensors; not differentiable on their own, the
        total is).  epoch=None keeps the gate where `set_epoch()` put it (what a `loss_fn` handed to TrainStep should pass).
        upsample_weight: the decoder's up-sampling matrix, as the reference trainer passes it (`.weight.data`): the term
        adds to the value and sends no gradient."""
        if epoch is not None:
            self.epoch = epoch
        mi = otherInfo['verts3d_MANO_list']
        total, out = _ManoLossFn.apply(
            self, self.img_size if img_size is None else img_size,
            result['verts3d']['left'], result['verts2d']['left'], mi['left']['mano_pose'], mi['left']['mano_shape'],
            result['verts3d']['right'], result['verts2d']['right'], mi['right']['mano_pose'], mi['right']['mano_shape'],
            otherInfo['root_rel'], v3d_l, v2d_l, lp_gt, ls_gt, v3d_r, v2d_r, rp_gt, rs_gt, root_rel)
        terms = {k: out[1 + i] for i, k in enumerate(MANO_TERMS[:9])}
        if upsample_weight is not None:
            if self.upsample_target is None:
                raise ValueError('FusedManoLoss: an upsample_weight was passed but the hand losses hold no w0')
            x = upsample_weight.detach() - self.upsample_target.to(upsample_weight.device)
            terms['upsample_norm_loss'] = F.smooth_l1_loss(x, torch.zeros_like(x))
            total = total + self.w['UPSAMPLE'] * terms['upsample_norm_loss']
        else:
            terms['upsample_norm_loss'] = torch.zeros_like(out[2])
        return total, terms


def mano_loss_GCN_fused(fused, epoch, loss_left, loss_right, converter_left, converter_right, result, paramsDict,
                        handDictList, otherInfo, mask, dense, hms, v2d_l, j2d_l, v2d_r, j2d_r, v3d_l, j3d_l, v3d_r, j3d_r,
                        root_rel, img_size, lp_gt, ls_gt, rp_gt, rs_gt, upsample_weight=None):
    """`mano_loss_GCN` on the fused kernel: the argument list of core/Loss_mano.py:245 with the FusedManoLoss in the place
    of cfg (it holds cfg.LOSS_WEIGHT); returns the same (total, {'total_loss': 0}, mano_loss_dict, {})."""
    total, terms = fused(epoch, result, otherInfo, v2d_l, v2d_r, v3d_l, v3d_r, root_rel, lp_gt, ls_gt, rp_gt, rs_gt,
                         img_size=img_size, upsample_weight=upsample_weight)
    return total, {'total_loss': 0}, terms, {}
