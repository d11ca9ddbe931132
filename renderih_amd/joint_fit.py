"""Fitting MANO pose and shape to 3-D joints -- the stage of the reference's utils/mano_from_3djoint/ (AIK.py `adaptive_IK`,
utils.py `mat2aa`, convert2mano.py:158-240) that turns mocap joints into MANO parameters, batched over hands.

Mirrors in plain torch (any device, fp32 or fp64):
  `adaptive_ik(template, joints, normalize=True, dtype=torch.float64)`   AIK.py:16-104 for [B,21,3] joints -> [B,16,3,3]
  `mat2aa(R)`                                                            utils.py:198-216 as an autograd.Function, [N,3,3] -> [N,3]
  `ManoJointFitter(mano, lr=1e-1, n_iter=200, select='last')`            convert2mano.py:158-240
On the HIP kernels of csrc/rih_joint_fit.hip (fp32): `fused_adaptive_ik`, `FusedMat2AA.apply`, `FusedManoJointFitter`.

`fit(joints [B,21,3])` takes joints in any unit, in the reference's order (wrist, then thumb, index, middle, ring, little) and
returns a dict of device tensors: `pose_R` [B,16,3,3] and `beta` [B,10] (the optimised parameters), `ori_pose` [B,48] (`mat2aa`
of the root, then `mat2aa(pose_R[:, 1:]) @ hands_components`, i.e. `pca2axis(.) - hands_mean`: the pose of an axis-angle MANO
layer with flat_hand_mean=False, convert2mano.py:226-231), `verts` [B,778,3] and `joints` [B,21,3] of a final forward, both
relative to joint 0 (:216-217), `loss` [B] of the returned parameters, `loss_history` [n_iter,B] (the loss each iteration
started from) and `init_R`, the IK result.  `start(joints)`, `run(k)`, `result()` are the three parts of `fit`, so that a fit
can be run in pieces.  B hands are B independent copies of the reference's B = 1 fit: the loss is the per-hand mean summed over
hands, so one hand's gradients do not depend on B.

`FusedManoJointFitter`: one iteration is seven launches -- rih_mat2aa_fwd, rih_mano_fwd, rih_joint_l1, rih_mano_bwd,
rih_mat2aa_bwd, rih_adam_dev, rih_lr_linear_step (eight with select='best': rih_fit_select after the loss) -- on static
buffers, captured once per batch shape in a `torch.cuda.graph` and replayed; `graph=False` launches the same kernels without
capture.  Step count, learning rate, base rate and n_iter live in device memory, so another `lr` or `n_iter` replays the same
graph (the history buffer is captured with room for max(n_iter, 256) rows; a longer fit recaptures).  `start` writes joints,
the IK result, fresh moments and a fresh state block into the static buffers; the device is read only by the caller.

Quirks of the reference that both classes keep:
  * the 15 finger rotations are fed to a `use_pca=True`, `center_idx=9` layer as 45 PCA COEFFICIENTS: their axis-angles are
    multiplied by `hands_components` and `hands_mean` is added.  The IK template is that layer's joints at zero coefficients.
  * the 16 matrices are unconstrained 3x3 parameters, never re-orthogonalised; the root matrix enters the skinning as it is.
  * the target is `(joints - joints[0]) / unit` with unit = 100 (the reference's mocap is in centimetres).
  * the learning rate of iteration i + 1 is `lr * (n_iter - i) / n_iter`: the first two iterations run at `lr`.
  * the last iterate is returned, not the best.  `select='best'` (off by default, the one extension) returns the parameters
    with the lowest loss in `loss_history` instead.
  * the caller flips `shapedirs` for the left hand, as convert2mano.py:135 does.
DELIBERATE DEVIATIONS of `adaptive_ik` / rih_aik from AIK.py: (a) the root rotation is always the proper rotation maximising
tr(R H) -- where V U^T has determinant -1 and no singular value is below 1e-4 the reference returns a reflection; (b) a bone
whose cross product with its template bone is exactly zero gets the identity swing (the reference divides 0 by 0: NaN); (c) the
cosine is clamped to [-1, 1] before arccos; (d) the twist angle is always 0, so D_tw = I is not computed.  The parent
rotation is inverted by transposition (the reference calls a general inverse on it).
`mat2aa` where torch's autograd through the reference gives NaN: the derivative is that of the selected branch only; at
sin^2 = 0 it is that of aa = 2 (x, y, z); where the forward result is NaN or the term under the square root is not positive
(the optimised matrices are not rotations) output and gradient are 0 -- the reference would carry NaN into Adam and lose the
hand.  Not reproduced: the csv / BVH readers, the plots and the .obj files of convert2mano.py.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .manolayer import ManoLayer
from .pose_opt import ADAM_EPS, BETAS, DeviceAdamPlateau, _bytes_tensor

KNUCKLES = (1, 5, 9, 13, 17)                # first joint of thumb, index, middle, ring, little; the other parents are k - 1
FINGER_SLOT = (13, 1, 4, 10, 7)             # slot of each finger's first bone rotation among the 16 matrices
HIST_MIN_ROWS = 256
KEYS = ('pose_R', 'beta', 'ori_pose', 'verts', 'joints', 'loss', 'loss_history', 'init_R')


# ---------------------------------------------------------------------------------------------------- inverse kinematics
def _axis_angle_matrix(axis, angle):
    """Rodrigues' formula for unit axes [...,3] and angles [...]."""
    x, y, z = axis.unbind(-1)
    c, s = torch.cos(angle), torch.sin(angle)
    C1 = 1 - c
    return torch.stack([x * x * C1 + c, x * y * C1 - z * s, z * x * C1 + y * s,
                        x * y * C1 + z * s, y * y * C1 + c, y * z * C1 - x * s,
                        z * x * C1 - y * s, y * z * C1 + x * s, z * z * C1 + c], -1).reshape(axis.shape[:-1] + (3, 3))


def adaptive_ik(template, joints, normalize=True, dtype=torch.float64):
    """`adaptive_IK(template, joints[b])` for every hand, with the module docstring's deviations; -> [B,16,3,3] in `dtype`."""
    T = torch.as_tensor(template).to(dtype)
    P = torch.as_tensor(joints).to(device=T.device, dtype=dtype)
    if tuple(T.shape) != (21, 3) or P.dim() != 3 or tuple(P.shape[1:]) != (21, 3):
        raise ValueError('template must be [21,3] and joints [B,21,3]; got %s and %s' % (tuple(T.shape), tuple(P.shape)))
    B = P.shape[0]
    if normalize:
        P = P * ((T[9] - T[0]).norm() / (P[:, 9] - P[:, 0]).norm(dim=-1)).view(B, 1, 1)
        P = P - P[:, :1] + T[0]
    base = list(KNUCKLES)
    H = torch.einsum('ka,bkc->bac', T[base] - T[0], P[:, base] - P[:, :1])
    U, _, Vh = torch.linalg.svd(H)
    V = Vh.transpose(1, 2)
    fix = torch.ones((B, 3), dtype=dtype, device=T.device)
    fix[:, 2] = torch.linalg.det(V @ U.transpose(1, 2)).sign()
    R0 = (V * fix.unsqueeze(1)) @ U.transpose(1, 2)
    out = torch.zeros((B, 16, 3, 3), dtype=dtype, device=T.device)
    out[:, 0] = R0
    eye = torch.eye(3, dtype=dtype, device=T.device)
    Rpa = R0.unsqueeze(1).expand(B, 5, 3, 3)
    qpa = torch.einsum('bfac,fc->bfa', Rpa, T[base] - T[0]) + T[0]
    for s in range(3):
        k = [b + 1 + s for b in base]
        dt = (T[k] - T[[i - 1 for i in k]]).unsqueeze(0).expand(B, 5, 3)
        dp = torch.einsum('bfca,bfc->bfa', Rpa, P[:, k] - qpa)
        ax = torch.cross(dt, dp, dim=-1)
        zero = (ax == 0).all(-1)
        ax = ax / (ax.norm(dim=-1, keepdim=True) + 1e-8)
        ax = ax / ax.norm(dim=-1, keepdim=True)
        cos = (dt * dp).sum(-1) / ((dt.norm(dim=-1) + 1e-8) * (dp.norm(dim=-1) + 1e-8))
        D = _axis_angle_matrix(torch.where(zero.unsqueeze(-1), eye[0], ax), torch.acos(cos.clamp(-1.0, 1.0)))
        D = torch.where(zero.view(B, 5, 1, 1), eye, D)
        for f, slot in enumerate(FINGER_SLOT):
            out[:, slot + s] = D[:, f]
        Rpa = Rpa @ D
        qpa = torch.einsum('bfac,bfc->bfa', Rpa, dt) + qpa
    return out


def _refuse(t, shape, what):
    if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError('%s must be a contiguous fp32 tensor' % what)
    if len(shape) != t.dim() or any(s is not None and s != d for s, d in zip(shape, t.shape)):
        raise ValueError('%s must be %s; got %s' % (what, list(shape), tuple(t.shape)))


def fused_adaptive_ik(template, joints, normalize=True):
    """rih_aik: contiguous fp32 `template` [21,3] and `joints` [B,21,3] on the GPU -> [B,16,3,3]."""
    _refuse(template, (21, 3), 'template')
    _refuse(joints, (None, 21, 3), 'joints')
    if joints.shape[0] < 1:
        raise ValueError('joints must hold at least one hand')
    ops._chk(template, joints)
    out = torch.empty((joints.shape[0], 16, 3, 3), dtype=torch.float32, device=joints.device)
    ops.check(ops._L().rih_aik(template.data_ptr(), joints.data_ptr(), 1 if normalize else 0, out.data_ptr(), joints.shape[0],
                               ops._stream()), 'rih_aik')
    return out


# ---------------------------------------------------------------------------------------------------- matrix -> axis-angle
# numerator (w, x, y, z) of mat2quat's four branches as rows over the row-major matrix; the component that is the trace term
# t (1 + its row . r) per branch
_SEL = np.zeros((4, 4, 9))
for _b, _rows in enumerate(((((7, 1), (5, -1)), ((0, 1), (4, -1), (8, -1)), ((3, 1), (1, 1)), ((2, 1), (6, 1))),
                            (((2, 1), (6, -1)), ((3, 1), (1, 1)), ((0, -1), (4, 1), (8, -1)), ((7, 1), (5, 1))),
                            (((3, 1), (1, -1)), ((2, 1), (6, 1)), ((7, 1), (5, 1)), ((0, -1), (4, -1), (8, 1))),
                            (((0, 1), (4, 1), (8, 1)), ((7, 1), (5, -1)), ((2, 1), (6, -1)), ((3, 1), (1, -1))))):
    for _c, _terms in enumerate(_rows):
        for _i, _s in _terms:
            _SEL[_b, _c, _i] = _s
_TCOMP = (1, 2, 3, 0)


def _mat2aa_parts(R):
    r = R.reshape(-1, 9)
    d2, d01, d0n1 = r[:, 8] < 1e-6, r[:, 0] > r[:, 4], r[:, 0] < -r[:, 4]
    branch = torch.where(d2, torch.where(d01, 0, 1), torch.where(d0n1, 2, 3))
    one = torch.ones_like(r[:, 0])
    ts = torch.stack([one + r[:, 0] - r[:, 4] - r[:, 8], one - r[:, 0] + r[:, 4] - r[:, 8],
                      one - r[:, 0] - r[:, 4] + r[:, 8], one + r[:, 0] + r[:, 4] + r[:, 8]], 1)
    t = ts.gather(1, branch.unsqueeze(1))[:, 0]
    A = torch.as_tensor(_SEL, dtype=R.dtype, device=R.device)[branch]                  # [N,4,9]
    tcomp = torch.as_tensor(_TCOMP, device=R.device)[branch]
    n = torch.einsum('nci,ni->nc', A, r)           # pairs: one rounding, as the reference's sums and differences
    n = n.scatter(1, tcomp.unsqueeze(1), t.unsqueeze(1))
    q = n / torch.sqrt(t).unsqueeze(1) * 0.5
    s2 = q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3]
    s, c = torch.sqrt(s2), q[:, 0]
    two_theta = 2.0 * torch.where(c < 0, torch.atan2(-s, -c), torch.atan2(s, c))
    k = torch.where(s2 > 0, two_theta / s, 2.0 * torch.ones_like(s))
    aa = q[:, 1:] * k.unsqueeze(1)
    return A, tcomp, n, t, q, s2, two_theta, k, aa


class _Mat2AA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, R):
        aa = _mat2aa_parts(R)[-1]
        ctx.save_for_backward(R)
        return torch.where(torch.isnan(aa), torch.zeros_like(aa), aa)

    @staticmethod
    def backward(ctx, ga):
        R, = ctx.saved_tensors
        A, tcomp, n, t, q, s2, two_theta, k, aa = _mat2aa_parts(R)
        alive = ~torch.isnan(aa).any(1) & (t > 0)
        pos = s2 > 0
        s, c = torch.sqrt(s2), q[:, 0]
        s_ = torch.where(pos, s, torch.ones_like(s))
        s2_ = torch.where(pos, s2, torch.ones_like(s))
        nn = s2 + c * c
        gk = (ga * q[:, 1:]).sum(1)
        gtt = gk / s_
        gs = gtt * (2.0 * c / nn) - gk * two_theta / s2_
        gq = torch.cat([(gtt * (-2.0 * s / nn)).unsqueeze(1), ga * k.unsqueeze(1) + gs.unsqueeze(1) * (q[:, 1:] / s_.unsqueeze(1))], 1)
        gq = torch.where(pos.unsqueeze(1), gq, torch.cat([torch.zeros_like(ga[:, :1]), 2.0 * ga], 1))
        rt = torch.sqrt(t)
        gn = 0.5 * gq / rt.unsqueeze(1)
        gt = -0.25 * (gq * n).sum(1) / (t * rt)
        gn = gn.scatter_add(1, tcomp.unsqueeze(1), gt.unsqueeze(1))
        gr = torch.einsum('nc,nci->ni', gn, A)
        return torch.where(alive.unsqueeze(1), gr, torch.zeros_like(gr)).reshape(R.shape)


def mat2aa(R):
    """`mat2aa` of utils.py for [N,3,3] matrices, with the module docstring's gradient rules."""
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3):
        raise ValueError('mat2aa expects [N,3,3]; got %s' % (tuple(R.shape),))
    return _Mat2AA.apply(R)


class FusedMat2AA(torch.autograd.Function):
    """`mat2aa` on rih_mat2aa_fwd / rih_mat2aa_bwd: `FusedMat2AA.apply(R)` for a contiguous fp32 GPU tensor [N,3,3]."""

    @staticmethod
    def forward(ctx, R):
        _refuse(R, (None, 3, 3), 'R')
        if R.shape[0] < 1:
            raise ValueError('R must hold at least one matrix')
        ops._chk(R)
        aa = torch.empty((R.shape[0], 3), dtype=torch.float32, device=R.device)
        ops.check(ops._L().rih_mat2aa_fwd(R.data_ptr(), aa.data_ptr(), 0, R.shape[0], 0, 0, ops._stream()), 'rih_mat2aa_fwd')
        ctx.save_for_backward(R)
        return aa

    @staticmethod
    def backward(ctx, ga):
        R, = ctx.saved_tensors
        ga = ga.contiguous()
        ops._chk(ga)
        gR = torch.empty_like(R)
        ops.check(ops._L().rih_mat2aa_bwd(R.data_ptr(), ga.data_ptr(), 0, gR.data_ptr(), R.shape[0], 0, 0, ops._stream()),
                  'rih_mat2aa_bwd')
        return gR


# ---------------------------------------------------------------------------------------------------- the mirror fit
def _mano_mirror(c, root, pose, shape):
    """The reference's `ManoLayer.forward` (models/manolayer.py:250-322) with use_pca=True and center_idx=9, in plain torch on the
    constants `c`; -> verts [B,778,3], joints [B,21,3]."""
    B = root.shape[0]
    axis = (pose @ c['hands_components'] + c['hands_mean']).reshape(-1, 3)
    angle = axis.norm(dim=1, keepdim=True) + 1e-8
    a = axis / angle
    z = torch.zeros_like(a[:, 0])
    K = torch.stack([z, -a[:, 2], a[:, 1], a[:, 2], z, -a[:, 0], -a[:, 1], a[:, 0], z], 1).view(-1, 3, 3)
    eye = torch.eye(3, dtype=root.dtype, device=root.device)
    rot = (eye + torch.sin(angle).unsqueeze(2) * K + (1 - torch.cos(angle)).unsqueeze(2) * (K @ K)).view(B, 15, 3, 3)
    v_shaped = c['v_template'] + torch.einsum('vck,bk->bvc', c['shapedirs'], shape)
    j = c['J_regressor'] @ v_shaped
    v_t = v_shaped + torch.einsum('vck,bk->bvc', c['posedirs'], (rot - eye).reshape(B, 135))
    Rs, ts = [root], [j[:, 0] - torch.einsum('bac,bc->ba', root, j[:, 0])]
    for i in range(1, 16):
        p, Rl = c['parent'][i], rot[:, i - 1]
        tl = j[:, i] - torch.einsum('bac,bc->ba', Rl, j[:, i])
        Rs.append(Rs[p] @ Rl)
        ts.append(torch.einsum('bac,bc->ba', Rs[p], tl) + ts[p])
    jl = [j[:, 0]] + [torch.einsum('bac,bc->ba', Rs[c['parent'][i]], j[:, i]) + ts[c['parent'][i]] for i in range(1, 16)]
    Rv = torch.einsum('vk,bkac->bvac', c['weights'], torch.stack(Rs, 1))
    tv = torch.einsum('vk,bka->bva', c['weights'], torch.stack(ts, 1))
    v = torch.einsum('bvac,bvc->bva', Rv, v_t) + tv
    jo = torch.stack(jl + [v[:, t] for t in (745, 317, 444, 556, 673)], 1)[:, c['new_order']]
    ctr = jo[:, 9:10]
    return v - ctr, jo - ctr


class ManoJointFitter:
    """convert2mano.py:158-240 in plain torch, batched; see the module docstring.  `mano`: a `ManoLayer` (its buffers are read
    when a fit starts) or what its constructor takes (a model dict or a pickle path)."""

    def __init__(self, mano, lr=1e-1, n_iter=200, select='last', unit=100.0, device='cpu', dtype=torch.float32):
        if select not in ('last', 'best'):
            raise ValueError("select must be 'last' or 'best'; got %r" % (select,))
        self.layer = mano if isinstance(mano, ManoLayer) else ManoLayer(mano, center_idx=9, use_pca=True)
        self.device, self.dtype = torch.device(device), dtype
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.layer.to(self.device)
        self.lr, self.n_iter, self.select, self.unit = float(lr), int(n_iter), select, float(unit)
        self.batch_size = None

    # ------------------------------------------------------------------ shared
    def _check(self, joints):
        if int(self.n_iter) < 1:
            raise ValueError('n_iter must be at least 1; got %r' % (self.n_iter,))
        if not torch.is_tensor(joints) or joints.dim() != 3 or tuple(joints.shape[1:]) != (21, 3) or joints.shape[0] < 1:
            raise ValueError('joints must be a [B,21,3] tensor; got %s'
                             % (tuple(joints.shape) if torch.is_tensor(joints) else type(joints).__name__,))

    def _constants(self):
        L = self.layer
        c = {k: getattr(L, k).to(device=self.device, dtype=self.dtype)
             for k in ('hands_components', 'hands_mean', 'shapedirs', 'posedirs', 'v_template', 'J_regressor', 'weights')}
        c['parent'], c['new_order'] = L.parent, L.new_order
        return c

    def _ori_pose(self, P):
        aa = self._mat2aa(P.reshape(-1, 3, 3)).reshape(-1, 48)
        return torch.cat([aa[:, :3], aa[:, 3:] @ self.layer.hands_components.to(aa.dtype)], 1)

    _mat2aa = staticmethod(mat2aa)

    # ------------------------------------------------------------------ the loop
    def _forward(self, P, beta):
        B = P.shape[0]
        return _mano_mirror(self.c, P[:, 0], mat2aa(P[:, 1:].reshape(-1, 3, 3)).reshape(B, 45), beta)

    def start(self, joints):
        """The IK initialisation and fresh optimiser state for these joints."""
        self._check(joints)
        joints = joints.detach().to(device=self.device, dtype=self.dtype)
        B = joints.shape[0]
        self.c = self._constants()
        eye = torch.eye(3, dtype=self.dtype, device=self.device)
        with torch.no_grad():
            self.template = self._forward(eye.repeat(B, 16, 1, 1)[:1], torch.zeros((1, 10), dtype=self.dtype, device=self.device))[1][0]
            self.init_R = adaptive_ik(self.template, joints, True, torch.float64).to(self.dtype)
        self.target = (joints - joints[:, :1]) / self.unit
        self.P = self.init_R.clone().requires_grad_(True)
        self.beta = torch.zeros((B, 10), dtype=self.dtype, device=self.device, requires_grad=True)
        self.optimizer = torch.optim.Adam([self.P, self.beta], lr=self.lr, betas=BETAS, eps=ADAM_EPS)
        self.history = torch.zeros((int(self.n_iter), B), dtype=self.dtype, device=self.device)
        self.best = (torch.full((B,), float('inf'), dtype=self.dtype, device=self.device), self.P.detach().clone(),
                     self.beta.detach().clone())
        self.batch_size, self.done = B, 0

    def _losses(self, P, beta):
        j = self._forward(P, beta)[1]
        return ((j - j[:, :1]) - self.target).abs().mean((1, 2))

    def run(self, k):
        """k more iterations (the history holds n_iter of them)."""
        if self.batch_size is None:
            raise RuntimeError('call start(joints) first')
        n = int(self.n_iter)
        for _ in range(int(k)):
            per = self._losses(self.P, self.beta)
            if self.done < self.history.shape[0]:
                self.history[self.done] = per.detach()
            if self.select == 'best':
                better = per.detach() < self.best[0]
                self.best = (torch.where(better, per.detach(), self.best[0]),
                             torch.where(better.view(-1, 1, 1, 1), self.P.detach(), self.best[1]),
                             torch.where(better.view(-1, 1), self.beta.detach(), self.best[2]))
            self.optimizer.zero_grad()
            per.sum().backward()
            self.optimizer.step()
            for group in self.optimizer.param_groups:
                group['lr'] = self.lr * (n - self.done) / n
            self.done += 1

    def result(self):
        with torch.no_grad():
            P, beta = (self.best[1], self.best[2]) if self.select == 'best' else (self.P.detach(), self.beta.detach())
            v, j = self._forward(P, beta)
            jr = j - j[:, :1]
            return dict(zip(KEYS, (P.clone(), beta.clone(), self._ori_pose(P), v - j[:, :1], jr,
                                   (jr - self.target).abs().mean((1, 2)), self.history.clone(), self.init_R.clone())))

    def fit(self, joints):
        self.start(joints)
        self.run(self.n_iter)
        return self.result()


# ---------------------------------------------------------------------------------------------------- the fused fit
class DeviceAdamLinear(DeviceAdamPlateau):
    """`DeviceAdamPlateau`'s table, moments and state block with the reference's linear schedule in the scheduler's place:
    rih_adam_dev, then rih_lr_linear_step on a device block of the base rate and n_iter."""

    def __init__(self, params, lr, n_iter):
        self.sched = torch.zeros(C.sizeof(_lib.LrLinear), dtype=torch.uint8, device=params[0]['p'].device)
        self.n_iter = int(n_iter)
        super().__init__(params, [lr])

    def reset(self, lr=None, n_iter=None):
        if lr is not None:
            self.lrs = [float(lr)]
        if n_iter is not None:
            self.n_iter = int(n_iter)
        super().reset()
        self.sched.copy_(_bytes_tensor(_lib.LrLinear(base_lr=self.lrs[0], n_iter=self.n_iter), 'cpu'))

    def step(self, loss=None):
        self.adam()
        ops.check(ops._L().rih_lr_linear_step(self.state.data_ptr(), self.sched.data_ptr(), ops._stream()), 'rih_lr_linear_step')


class FusedManoJointFitter(ManoJointFitter):
    """`ManoJointFitter` on the HIP kernels, one iteration = one replayed graph; see the module docstring.  fp32 only."""

    def __init__(self, mano, lr=1e-1, n_iter=200, select='last', unit=100.0, device='cuda', graph=True):
        super().__init__(mano, lr, n_iter, select, unit, device, torch.float32)
        self.graph = bool(graph)
        if self.graph and self.device.type != 'cuda':
            raise ValueError('graph=True needs a GPU device')
        self._B = self._graph = None
        self.launches_per_iteration = 8 if select == 'best' else 7

    _mat2aa = staticmethod(FusedMat2AA.apply)

    def _allocate(self, B, rows):
        f = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.device)
        L = ops._L()
        self.joints_in, self.target, self.init_R = f(B, 21, 3), f(B, 21, 3), f(B, 16, 3, 3)
        self.P, self.beta = f(B, 16, 3, 3), f(B, 10)
        self.root, self.pose = f(B, 9), f(B, 45)
        self.v, self.j, self.dv, self.dj = f(B, 778, 3), f(B, 21, 3), f(B, 778, 3), f(B, 21, 3)       # dv stays zero
        self.ws, self.wsb = f(int(L.rih_mano_ws_floats(B))), f(int(L.rih_mano_bwd_ws_floats(B)))
        self.d_root, self.d_pose, self.g_beta, self.g_P = f(B, 9), f(B, 45), f(B, 10), f(B, 16, 3, 3)
        self.loss, self.total, self.history = f(B), f(1), f(rows, B)
        self.best_loss, self.best_P, self.best_beta = f(B), f(B, 16, 3, 3), f(B, 10)
        self.stepper = DeviceAdamLinear([{'p': self.P, 'group': 0}, {'p': self.beta, 'group': 0}], self.lr, self.n_iter)
        self.stepper.set_grads([self.g_P, self.g_beta])
        self._B, self._graph = B, None

    def _template(self):
        """The layer's joints at identity rotations, zero coefficients and zero shape (convert2mano.py:165-166)."""
        eye = torch.eye(3, dtype=torch.float32, device=self.device)
        with torch.no_grad():
            return self.layer(eye.view(1, 3, 3), torch.zeros((1, 45), device=self.device),
                              torch.zeros((1, 10), device=self.device))[1][0].contiguous()

    def _mano_forward(self, ws):
        layer, B = self.layer, self._B
        mm = layer._model_struct()
        ops.check(ops._L().rih_mano_fwd(C.byref(mm), layer._packed_basis(mm).data_ptr(), self.root.data_ptr(), self.pose.data_ptr(),
                                        45, self.beta.data_ptr(), 0, 0, 9, 0, self.v.data_ptr(), self.j.data_ptr(),
                                        0 if ws is None else ws.data_ptr(), B, 0, ops._stream()), 'rih_mano_fwd')
        return mm

    def _loss_launch(self, history):
        ops.check(ops._L().rih_joint_l1(self.j.data_ptr(), self.target.data_ptr(), self.stepper.state.data_ptr(),
                                        self.loss.data_ptr(), self.total.data_ptr(), self.dj.data_ptr(),
                                        history.data_ptr() if history is not None else 0,
                                        history.shape[0] if history is not None else 0, self._B, ops._stream()), 'rih_joint_l1')

    def _iteration(self):
        L, st, B = ops._L(), ops._stream(), self._B
        ops.check(L.rih_mat2aa_fwd(self.P.data_ptr(), self.pose.data_ptr(), self.root.data_ptr(), 16 * B, 16, 1, st), 'rih_mat2aa_fwd')
        mm = self._mano_forward(self.ws)
        self._loss_launch(self.history)
        if self.select == 'best':
            ops.check(L.rih_fit_select(self.loss.data_ptr(), self.P.data_ptr(), self.beta.data_ptr(), self.best_loss.data_ptr(),
                                       self.best_P.data_ptr(), self.best_beta.data_ptr(), B, st), 'rih_fit_select')
        ops.check(L.rih_mano_bwd(C.byref(mm), self.layer._packed_basis(mm).data_ptr(), self.root.data_ptr(), self.pose.data_ptr(), 45,
                                 self.beta.data_ptr(), 0, 0, 9, 0, self.dv.data_ptr(), self.dj.data_ptr(), self.ws.data_ptr(),
                                 self.d_root.data_ptr(), self.d_pose.data_ptr(), self.g_beta.data_ptr(), 0, 0, self.wsb.data_ptr(),
                                 B, st), 'rih_mano_bwd')
        ops.check(L.rih_mat2aa_bwd(self.P.data_ptr(), self.d_pose.data_ptr(), self.d_root.data_ptr(), self.g_P.data_ptr(), 16 * B,
                                   16, 1, st), 'rih_mat2aa_bwd')
        self.stepper.step()

    def _statics(self):
        return [self.P, self.beta, self.history, self.best_loss, self.best_P, self.best_beta, self.stepper.state] + \
               [e[k] for e in self.stepper.params for k in ('m', 'v')]

    def _capture(self):
        """One warm-up iteration on a side stream, undone afterwards, then the capture of one iteration."""
        saved = [t.clone() for t in self._statics()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._iteration()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            self._iteration()
        with torch.no_grad():
            for t, s in zip(self._statics(), saved):
                t.copy_(s)
        self._graph = graph

    def start(self, joints):
        self._check(joints)
        _refuse(joints, (None, 21, 3), 'joints')
        ops._chk(joints)
        if joints.device != self.device:
            raise ValueError('joints are on %s, the fitter on %s' % (joints.device, self.device))
        B, rows = joints.shape[0], max(int(self.n_iter), HIST_MIN_ROWS)
        if self._B != B or self.history.shape[0] < int(self.n_iter):
            self._allocate(B, rows)
        with torch.no_grad():
            self.joints_in.copy_(joints)
            torch.sub(joints, joints[:, :1], out=self.target)
            self.target.div_(self.unit)
            self.history.zero_()
            self.best_loss.fill_(float('inf'))
        self.template = self._template()
        ops.check(ops._L().rih_aik(self.template.data_ptr(), self.joints_in.data_ptr(), 1, self.init_R.data_ptr(), B, ops._stream()),
                  'rih_aik')
        with torch.no_grad():
            self.P.copy_(self.init_R)
            self.best_P.copy_(self.init_R)
            self.beta.zero_()
            self.best_beta.zero_()
        self.stepper.reset(self.lr, self.n_iter)
        self.batch_size, self.done = B, 0

    def run(self, k):
        if self.batch_size is None:
            raise RuntimeError('call start(joints) first')
        if self.graph:
            if self._graph is None:
                self._capture()
            for _ in range(int(k)):
                self._graph.replay()
        else:
            for _ in range(int(k)):
                self._iteration()
        self.done += int(k)

    def result(self):
        B, n = self._B, int(self.n_iter)
        P, beta = (self.best_P, self.best_beta) if self.select == 'best' else (self.P, self.beta)
        keep = (self.P.clone(), self.beta.clone())
        with torch.no_grad():
            if self.select == 'best':                  # the final forward reads the parameter buffers
                self.P.copy_(P), self.beta.copy_(beta)
            ops.check(ops._L().rih_mat2aa_fwd(self.P.data_ptr(), self.pose.data_ptr(), self.root.data_ptr(), 16 * B, 16, 1,
                                              ops._stream()), 'rih_mat2aa_fwd')
            self._mano_forward(None)
            self._loss_launch(None)
            j0 = self.j[:, :1]
            out = dict(zip(KEYS, (self.P.clone(), self.beta.clone(), self._ori_pose(self.P), self.v - j0, self.j - j0,
                                  self.loss.clone(), self.history[:n].clone(), self.init_R.clone())))
            self.P.copy_(keep[0]), self.beta.copy_(keep[1])
        return out
