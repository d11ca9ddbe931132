"""The pose-data stages around the two-hand pose optimiser -- drop-ins for pose_data_optimize's scripts/HandPoseConverter.py
(annotation <-> MANO quaternion <-> "mocap" Euler degrees, `trans` <-> `loc`), scripts/HandPoseArguer.py and
Ver2Code/NatureJudge/PoseArgue.py (`argue_pose`), Ver2Code/ValidJudge/ValidJudger.py with GetValidRate.py, and the dict
handling of data/template_0_pose_convert.py, template_1_pose_argue.py, template_3_pose_reconvert.py and
batch_optimize_mocap_origin.py:41-46, 385-388, 579-585.

`PoseConverter`, `PoseAugmenter`, `PoseValidJudge` are plain-torch mirrors (fp64 or fp32, any device; pinned to the reference's
own program by tests/golden/pose_convert.npz); `FusedPoseConverter`, `FusedPoseAugmenter`, `FusedPoseValidJudge` are the same
surfaces on rih_pose_convert (csrc/rih_pose_convert.hip): ONE launch per call, fp32 GPU tensors only, nothing read back by the
host, capturable in a `torch.cuda.graph`.  Conventions (DESIGN.md 3.18 has them in full):
  * quaternions are (w, x, y, z); the ones emitted are unit with w >= 0 (scipy's sign is an artefact of its algorithm).
  * Euler angles are scipy's lower-case 'xyz' (extrinsic) in degrees: E = Rz(c) Ry(b) Rx(a) -- NOT the pytorch3d 'XYZ' of
    `nature.quaternion_to_euler_xyz`.  Back: c = atan2(E10, E00), b = atan2(-E20, |(E00, E10)|) (= -asin(E20), without its loss
    of digits next to +-90 degrees), a = atan2(s E02 - k E12, k E11 - s E01) with (k, s) = (E00, E10) / |(E00, E10)| (=
    atan2(E21, E22) for an exact rotation, and still a rotation that reproduces E when cos b goes to 0).  At gimbal lock c = 0
    and a takes the whole in-plane angle.
  * Euler -> MANO quaternion (`euler_2_mano_quat`): M = invM_U_n_0[j] E invU_M_n_1[j]; left hand: the ROOT matrix is
    pre-multiplied by diag(1, -1, -1), and y, z of all 16 quaternions are negated.  MANO quaternion -> Euler
    (`mano_quat_2_euler`) is the inverse with the transposed tables.  Tables: `pose_prior.axis_tables`.
  * annotation -> quaternion (`axis_angle_2_mano_quat(flat_hand=False)`): hands_mean is added to the 15 finger joints, rotation
    vector -> quaternion, left hand: y, z negated.  Back (`mano_quat_flat_2_normal(return_type='aa')`): the angle is in [0, pi],
    the series near 0 as scipy's.
  * `loc` is joint 0 of the layer with center_idx=None plus `trans`; joint 0 is J_regressor[0] (v_template + shapedirs beta),
    whatever the pose (manopth/manopth/manolayer.py:277), so trans <-> loc is one 10 -> 3 affine map per side.
  * augmentation (`argue_pose`): per joint d_bend uniform in [neg, pos], pos = max(min(max_bend, hi - bend), 0), neg =
    min(max(-max_bend, lo - bend), 0), bend the ORIGINAL euler[j, 2]; d_splay alike from the ORIGINAL euler[j, 1];
    E' = E Rz(d_bend) Ry(d_splay); joints without a range (the root among them) do not move; output row m = n * A + a.
  * validity (`ValidationJudge`): for joints 1..15 rel = zero_frame^T frame (frames of `pose_prior.mano_quat_2_mat`), bend =
    atan2(x1, x0), splay = atan2(-x2, x0) of rel's first column in degrees, residual = the largest excess over
    `pose_prior.SPLAY` / `pose_prior.BEND` in radians.
DELIBERATE DEVIATIONS: inputs are never written (the reference's `mano_quat_2_euler` and `mano_quat_flat_2_normal` negate the
caller's left-hand array in place).  The augmenter does not go matrix -> Euler -> matrix between its two products (the identity
up to rounding).  Draws come from the counter hash of csrc/rih_hash.h, u = (rih_hash(seed, ((m * 16 + j) * 2 + which)) >> 8) *
2^-24 (which: 0 bend, 1 splay), or from explicit `uniforms` [M,16,2]; the reference consumes numpy's global stream.  Steps 1
and 2 of the judge are computed and then commented out of its result there; they are left out here.  Not reproduced: `mode=1`
of template_3's `data_loader` (no caller uses it), the 5000-frame file splitting and every file write of the templates,
scripts/Interpolation.py, every open3d visualisation.
"""
import copy
import math
import pickle

import numpy as np
import torch

from . import ops
from .ops import check
from .pose_prior import BEND, SPLAY, axis_tables, mano_quat_2_mat
from .quat_mano import QuatManoLayer, quaternion_to_rotation_matrix

TAB = 44                                             # = RIH_POSE_TAB: floats per joint row of the kernel's table
AA, EULER, QUAT, VALID = 0, 1, 2, 3                  # in_fmt; out_fmt is (EULER, QUAT, AA, VALID) -> 0, 1, 2, 3
_OUT = {'euler': 0, 'quat': 1, 'aa': 2}
THRESHOLD = 0.1 / 180 * math.pi                      # ValidJudger.ComputeValidation

# scripts/HandPoseArguer.py:117-146 (what data/template_1_pose_argue.py runs) and Ver2Code/NatureJudge/PoseArgue.py:118-147;
# joint -> (lo, hi) in degrees, joints numbered 0..15 as the converter's axis order
_BEND_SCRIPT = {2: (-8, 110), 5: (-8, 110), 11: (-8, 110), 8: (-8, 110), 13: (-20, 40), 14: (-8, 50), 3: (-8, 90), 6: (-8, 90),
                12: (-8, 90), 9: (-8, 90), 15: (-8, 90), 1: (-25, 70), 4: (-25, 70), 10: (-25, 70), 7: (-25, 70)}
SCRIPT_RANGES = {'bend': _BEND_SCRIPT, 'splay': {1: (-6, 20), 4: (-10, 10), 10: (-15, 6), 7: (-35, 6), 13: (-9, 80)}}
VER2_RANGES = {'bend': {j: ((-8, 95) if j in (3, 6, 12, 9, 15) else r) for j, r in _BEND_SCRIPT.items()},
               'splay': {1: (-25, 15), 4: (-15, 15), 10: (-25, 15), 7: (-20, 30), 13: (-30, 30)}}


def _side(side):
    if side not in ('right', 'left'):
        raise ValueError("side must be 'right' or 'left'; got %r" % (side,))
    return side


def _mano_dict(mano):
    if isinstance(mano, dict):
        return mano
    with open(mano, 'rb') as f:
        return pickle.load(f, encoding='latin1')


def _rows(x, width, name):
    """[N,16,width] or [N,16*width] -> [N,16,width], N >= 1."""
    if not torch.is_tensor(x) or not x.is_floating_point():
        raise ValueError('%s must be a floating-point tensor; got %r' % (name, type(x)))
    if x.dim() == 2 and x.shape[1] == 16 * width:
        x = x.reshape(-1, 16, width)
    if x.dim() != 3 or tuple(x.shape[1:]) != (16, width) or x.shape[0] < 1:
        raise ValueError('%s must be [N,16,%d] with N >= 1; got %s' % (name, width, tuple(x.shape)))
    return x


# ------------------------------------------------------------------------------------------------ per-joint rotations
def rotvec_to_quat(v):
    """[...,3] -> unit (w, x, y, z) with w >= 0; scipy's series below 1e-3."""
    n2 = (v * v).sum(-1, keepdim=True)
    n = n2.sqrt()
    small = n <= 1e-3
    k = torch.where(small, 0.5 - n2 / 48 + n2 * n2 / 3840, torch.sin(0.5 * n) / torch.where(small, torch.ones_like(n), n))
    q = torch.cat([torch.cos(0.5 * n), k * v], -1)
    return torch.where(q[..., :1] < 0, -q, q)


def quat_to_rotvec(q):
    """(w, x, y, z) of any norm > 0 -> rotation vector with its angle in [0, pi]; scipy's series below 1e-3."""
    q = q / q.norm(dim=-1, keepdim=True)
    q = torch.where(q[..., :1] < 0, -q, q)
    n = q[..., 1:].norm(dim=-1, keepdim=True)
    angle = 2 * torch.atan2(n, q[..., :1])
    small = angle <= 1e-3
    a2 = angle * angle
    k = torch.where(small, 2 + a2 / 12 + 7 * a2 * a2 / 2880, angle / torch.where(small, torch.ones_like(n), n))
    return k * q[..., 1:]


def mat_to_quat(R):
    """[...,3,3] -> unit (w, x, y, z) with w >= 0; the largest of (trace, R00, R11, R22) picks the component taken from a root."""
    r = [[R[..., i, j] for j in range(3)] for i in range(3)]
    tr = r[0][0] + r[1][1] + r[2][2]
    cand = (torch.stack([1 + tr, r[2][1] - r[1][2], r[0][2] - r[2][0], r[1][0] - r[0][1]], -1),
            torch.stack([r[2][1] - r[1][2], 1 + r[0][0] - r[1][1] - r[2][2], r[0][1] + r[1][0], r[0][2] + r[2][0]], -1),
            torch.stack([r[0][2] - r[2][0], r[0][1] + r[1][0], 1 - r[0][0] + r[1][1] - r[2][2], r[1][2] + r[2][1]], -1),
            torch.stack([r[1][0] - r[0][1], r[0][2] + r[2][0], r[1][2] + r[2][1], 1 - r[0][0] - r[1][1] + r[2][2]], -1))
    first = (tr >= r[0][0]) & (tr >= r[1][1]) & (tr >= r[2][2])
    second = (r[0][0] >= r[1][1]) & (r[0][0] >= r[2][2])
    third = r[1][1] >= r[2][2]
    q = torch.where(first[..., None], cand[0], torch.where(second[..., None], cand[1],
                                                           torch.where(third[..., None], cand[2], cand[3])))
    q = q / q.norm(dim=-1, keepdim=True)
    return torch.where(q[..., :1] < 0, -q, q)


def polar(E):
    """The nearest rotation to a matrix that is one to about 1e-7: one Newton step of the polar decomposition,
    (E + E^-T) / 2, which leaves the square of that distance."""
    return 0.5 * (E + torch.linalg.inv(E).transpose(-1, -2))


def euler_to_mat(e):
    """Euler degrees [...,3] (scipy 'xyz') -> E = Rz(c) Ry(b) Rx(a) [...,3,3]."""
    r = e * (math.pi / 180)
    (sa, sb, sc), (ca, cb, cc) = torch.sin(r).unbind(-1), torch.cos(r).unbind(-1)
    rows = [cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa,
            sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa,
            -sb, cb * sa, cb * ca]
    return torch.stack(rows, -1).reshape(e.shape[:-1] + (3, 3))


def mat_to_euler(E):
    """[...,3,3] -> Euler degrees [...,3]; see the module docstring (c = 0 at gimbal lock)."""
    h = (E[..., 0, 0] ** 2 + E[..., 1, 0] ** 2).sqrt()
    lock = h < 8 * torch.finfo(E.dtype).eps
    safe = torch.where(lock, torch.ones_like(h), h)
    k = torch.where(lock, torch.ones_like(h), E[..., 0, 0] / safe)
    s = torch.where(lock, torch.zeros_like(h), E[..., 1, 0] / safe)
    a = torch.atan2(s * E[..., 0, 2] - k * E[..., 1, 2], k * E[..., 1, 1] - s * E[..., 0, 1])
    b = torch.atan2(-E[..., 2, 0], h)
    c = torch.where(lock, torch.zeros_like(h), torch.atan2(E[..., 1, 0], E[..., 0, 0]))
    return torch.stack([a, b, c], -1) * (180 / math.pi)


def hash_uniforms(seed, M, row_offset=0):
    """float32 numpy [M,16,2]: the draws of the seeded kernel, u = (rih_hash(seed, (((row_offset + m) * 16 + j) * 2 + which))
    >> 8) * 2^-24 -- csrc/rih_hash.h restated in numpy for the mirror."""
    m32 = np.uint64(0xFFFFFFFF)

    def mix(x, kb=None):
        x = np.asarray(x, np.uint64) & m32
        x = x ^ (x >> np.uint64(16))
        x = (x * np.uint64(0x7feb352d)) & m32
        x = x ^ (x >> np.uint64(15))
        if kb is not None:
            x = (x + kb) & m32
        x = (x * np.uint64(0x846ca68b)) & m32
        return x ^ (x >> np.uint64(16))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    ka = mix(lo) ^ mix(hi ^ np.uint64(0x9E3779B9))
    kb = (mix(lo ^ np.uint64(0x85EBCA6B)) + mix((hi + np.uint64(0xC2B2AE35)) & m32)) & m32
    idx = np.arange(int(row_offset) * 32, (int(row_offset) + int(M)) * 32, dtype=np.uint64)
    word = (idx & m32) ^ ka ^ (((idx >> np.uint64(32)) * np.uint64(0x85EBCA6B)) & m32)
    h = mix(word, kb)
    return ((h >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(int(M), 16, 2)


# ------------------------------------------------------------------------------------------------ the kernel's table
def _table(side, tables, hands_mean, ranges=None, caps=(0.0, 0.0)):
    """float32 numpy [16,TAB]: a hand's rows of rih_pose_convert's table (include/renderih_amd.h)."""
    t0, t1 = (t.float() for t in tables)
    ident = torch.zeros(1, 16, 4)
    ident[..., 0] = 1.0
    zero = mano_quat_2_mat(ident, (t0, t1), side)[0]                          # fp32, as the judge holds it
    rows = np.zeros((16, TAB), np.float32)
    rows[:, 0:9], rows[:, 9:18], rows[:, 18:27] = (x.reshape(16, 9).numpy() for x in (t0, t1, zero))
    rows[1:, 27:30] = np.asarray(hands_mean, np.float32).reshape(15, 3)
    rows[:, 36], rows[:, 37], rows[:, 38], rows[:, 39] = -np.inf, np.inf, -np.inf, np.inf
    for j, (lo, hi) in BEND.items():
        rows[j + 1, 36:38] = lo, hi
    for j, (lo, hi) in SPLAY.items():
        rows[j + 1, 38:40] = lo, hi
    if ranges is not None:
        for at, name, cap in ((30, 'bend', caps[0]), (33, 'splay', caps[1])):
            for j, (lo, hi) in ranges[name].items():
                rows[j, at:at + 3] = lo, hi, cap
    rows[:, 40] = 1.0 if side == 'right' else -1.0
    return rows


def _launch(x, second, out, table, uniforms, seed, row0, M, A, in_fmt, mid, out_fmt):
    ops._chk(x, second, out, table, uniforms)                  # fp32 GPU tensors only: there is no CPU fallback
    for t in (x, second, out):
        if t is not None and t.data_ptr() % 16:
            raise ValueError('renderih_amd.pose_convert: tensors must be 16-byte aligned')
    check(ops._L().rih_pose_convert(x.data_ptr(), ops._p(second), out.data_ptr(), table.data_ptr(), ops._p(uniforms),
                                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(row0), int(M), int(A), in_fmt, mid, out_fmt,
                                    ops._stream()), 'rih_pose_convert')
    return out


def _fp32(x):
    if x.dtype != torch.float32:
        raise ValueError('the fused pose conversion is fp32 only; got %s' % x.dtype)
    return x.detach().contiguous()


class _DeviceTable:
    """The kernel's table per device, uploaded on first use."""

    def _device_table(self, device):
        key = str(device)
        if key not in self._tables:
            self._tables[key] = torch.from_numpy(self._table_rows).to(device).contiguous()
        return self._tables[key]


# ------------------------------------------------------------------------------------------------ converter
class PoseConverter:
    """HandPoseConverter in plain torch; see the module docstring.  `side`: 'right' or 'left'; `mano`: the model dict or pickle
    path of `QuatManoLayer`.  Every method takes a tensor of any floating dtype on any device, works in that dtype and leaves
    it untouched: annotation [N,16,3] (or [N,48]) axis-angle, quat [N,16,4], euler [N,16,3] degrees, shape [N,10], trans and
    loc [N,3]."""

    def __init__(self, side, mano, tables=None):
        """`tables`: (invM_U_n_0, invU_M_n_1) [16,3,3] each, to use instead of `pose_prior.axis_tables(side, mano)` (which runs
        the hand model in fp32 and so differs in the last bits from one machine's CPU to another's)."""
        self.side = _side(side)
        data = _mano_dict(mano)
        if tables is None:
            tables = axis_tables(side, data)                                    # fp32, as the reference holds them
        self.tables = tuple(torch.as_tensor(np.asarray(t)).float().reshape(16, 3, 3).contiguous() for t in tables)
        mean = data['hands_mean']
        self.hands_mean = torch.from_numpy(np.asarray(mean.r if hasattr(mean, 'r') else mean, np.float32).reshape(15, 3).copy())
        layer = QuatManoLayer(data, side=side, center_idx=None)                # the left hand's shapedirs flip is in here
        reg = layer.th_J_regressor[0].double()
        self.loc_base = reg @ layer.th_v_template[0].double()                   # [3]
        self.loc_shape = torch.einsum('v,vck->ck', reg, layer.th_shapedirs.double())      # [3,10]
        self._sign = 1.0 if side == 'right' else -1.0

    # the two middle forms: Q, the MANO quaternion after the left hand's y, z flip, and E, the finger-frame rotation
    def _flip(self, q):
        return q * q.new_tensor([1.0, 1.0, self._sign, self._sign])

    def _root(self, R):
        if self.side == 'right':
            return R
        d = torch.ones(16, 3, 1, dtype=R.dtype, device=R.device)
        d[0, 1:] = -1.0
        return R * d                                                            # diag(1, -1, -1) R on the root

    def _t(self, like):
        return tuple(t.to(device=like.device, dtype=like.dtype) for t in self.tables)

    def _q_to_e(self, Q):
        """The tables are fp32, orthogonal to 1e-7 only, and so is the product; scipy's `Rotation.from_matrix` inside
        `rotation_2_euler` replaces it by the nearest rotation before it reads the angles, and so does this."""
        t0, t1 = self._t(Q)
        E = t0.transpose(1, 2) @ self._root(quaternion_to_rotation_matrix(Q)) @ t1.transpose(1, 2)
        return polar(E)

    def _e_to_q(self, E):
        t0, t1 = self._t(E)
        return mat_to_quat(self._root(polar(t0 @ E @ t1)))                       # scipy's from_matrix, as in _q_to_e

    def _mean(self, like):
        mean = like.new_zeros(16, 3)
        mean[1:] = self.hands_mean.to(device=like.device, dtype=like.dtype)
        return mean

    def annotation_to_quat(self, annotation):
        aa = _rows(annotation, 3, 'annotation')
        return self._flip(rotvec_to_quat(aa + self._mean(aa)))

    def quat_to_annotation(self, quat):
        q = _rows(quat, 4, 'quat')
        return quat_to_rotvec(self._flip(q)) - self._mean(q)

    def euler_to_quat(self, euler):
        return self._flip(self._e_to_q(euler_to_mat(_rows(euler, 3, 'euler'))))

    def quat_to_euler(self, quat):
        return mat_to_euler(self._q_to_e(self._flip(_rows(quat, 4, 'quat'))))

    def annotation_to_euler(self, annotation):
        """template_0's composition `mano_quat_2_euler(axis_angle_2_mano_quat(aa))`."""
        aa = _rows(annotation, 3, 'annotation')
        return mat_to_euler(self._q_to_e(rotvec_to_quat(aa + self._mean(aa))))

    def euler_to_annotation(self, euler):
        """template_3's composition `mano_quat_flat_2_normal(euler_2_mano_quat(rot), return_type='aa')`."""
        e = _rows(euler, 3, 'euler')
        return quat_to_rotvec(self._e_to_q(euler_to_mat(e))) - self._mean(e)

    def _joint0(self, shape):
        if not torch.is_tensor(shape) or shape.dim() != 2 or shape.shape[1] != 10:
            raise ValueError('shape must be [N,10]; got %s' % (tuple(getattr(shape, 'shape', ())),))
        k = dict(device=shape.device, dtype=shape.dtype)
        return self.loc_base.to(**k) + shape @ self.loc_shape.to(**k).t()

    def _vec3(self, x, shape, name):
        if not torch.is_tensor(x) or tuple(x.shape) != (shape.shape[0], 3):
            raise ValueError('%s must be [N,3] with the N of shape; got %s' % (name, tuple(getattr(x, 'shape', ()))))
        return x

    def trans_to_loc(self, shape, trans):
        """`trans_2_loc(..., loc_center_idx=0)`: joint 0 of the layer with center_idx=None, plus trans."""
        return self._joint0(shape) + self._vec3(trans, shape, 'trans')

    def loc_to_trans(self, shape, loc):
        return self._vec3(loc, shape, 'loc') - self._joint0(shape)


class FusedPoseConverter(PoseConverter, _DeviceTable):
    """`PoseConverter` on rih_pose_convert: one launch per conversion (the two compositions included), fp32 GPU tensors only.
    `trans_to_loc` / `loc_to_trans` are the mirror's (one small matrix product)."""

    def __init__(self, side, mano, tables=None):
        super().__init__(side, mano, tables)
        self._table_rows = _table(side, self.tables, self.hands_mean)
        self._tables = {}

    def _run(self, x, width, name, in_fmt, out):
        x = _fp32(_rows(x, width, name))
        res = torch.empty((x.shape[0], 16, 4 if out == 'quat' else 3), device=x.device, dtype=torch.float32)
        return _launch(x, None, res, self._device_table(x.device), None, 0, 0, x.shape[0], 1, in_fmt, 0, _OUT[out])

    def annotation_to_quat(self, annotation):
        return self._run(annotation, 3, 'annotation', AA, 'quat')

    def quat_to_annotation(self, quat):
        return self._run(quat, 4, 'quat', QUAT, 'aa')

    def euler_to_quat(self, euler):
        return self._run(euler, 3, 'euler', EULER, 'quat')

    def quat_to_euler(self, quat):
        return self._run(quat, 4, 'quat', QUAT, 'euler')

    def annotation_to_euler(self, annotation):
        return self._run(annotation, 3, 'annotation', AA, 'euler')

    def euler_to_annotation(self, euler):
        return self._run(euler, 3, 'euler', EULER, 'aa')


# ------------------------------------------------------------------------------------------------ augmenter
def _ranges(ranges):
    try:
        out = {name: {int(j): (float(lo), float(hi)) for j, (lo, hi) in ranges[name].items()} for name in ('bend', 'splay')}
    except (KeyError, TypeError, ValueError, AttributeError):
        raise ValueError("ranges must be {'bend': {joint: (lo, hi)}, 'splay': {joint: (lo, hi)}}")
    for table in out.values():
        for j, (lo, hi) in table.items():
            if not 1 <= j <= 15 or not lo <= hi:
                raise ValueError('ranges name joints 1..15 with lo <= hi; got %d: (%g, %g)' % (j, lo, hi))
    return out


class PoseAugmenter:
    """`argue_pose(pose_type='euler')` in plain torch; see the module docstring.  `ranges`: `SCRIPT_RANGES` (scripts/
    HandPoseArguer.py, with its max_bend=120, max_splay=30: what template_1 runs) or `VER2_RANGES` (Ver2Code/NatureJudge/
    PoseArgue.py; `ver2(side, mano, level)` also sets its max_bend = 120 * level, max_splay = 45 * level).
    __call__(euler [N,16,3], argue_size, seed=None, uniforms=None, out='euler', row_offset=0) -> [N*A,16,3] Euler degrees, or
    with out='quat' the MANO quaternions [N*A,16,4] of the variants (what the optimiser takes).  Exactly one of `seed` (the
    draws of `hash_uniforms(seed, N*A, row_offset)`) and `uniforms` ([N*A,16,2] in [0,1): [..., 0] bend, [..., 1] splay).
    `row_offset` numbers the output rows from there on, so a sequence augmented in pieces draws what it draws in one call."""

    def __init__(self, side, mano, ranges=SCRIPT_RANGES, max_bend=120, max_splay=30, tables=None):
        self.converter = PoseConverter(side, mano, tables)
        self.side = self.converter.side
        self.ranges = _ranges(ranges)
        self.max_bend, self.max_splay = float(max_bend), float(max_splay)
        if not (self.max_bend >= 0 and self.max_splay >= 0):
            raise ValueError('max_bend and max_splay must be >= 0; got %r, %r' % (max_bend, max_splay))
        limits = np.zeros((16, 6), np.float64)                                  # bend lo, hi, cap; splay lo, hi, cap
        for at, name, cap in ((0, 'bend', self.max_bend), (3, 'splay', self.max_splay)):
            for j, (lo, hi) in self.ranges[name].items():
                limits[j, at:at + 3] = lo, hi, cap
        self.limits = torch.from_numpy(limits)

    @classmethod
    def ver2(cls, side, mano, level=1.0, tables=None):
        return cls(side, mano, VER2_RANGES, 120 * level, 45 * level, tables)

    def _args(self, euler, argue_size, seed, uniforms, out, row_offset):
        e = _rows(euler, 3, 'euler')
        A = int(argue_size)
        if A < 1 or A != argue_size:
            raise ValueError('argue_size must be a whole number >= 1; got %r' % (argue_size,))
        if out not in ('euler', 'quat'):
            raise ValueError("out must be 'euler' or 'quat'; got %r" % (out,))
        if (seed is None) == (uniforms is None):
            raise ValueError('give exactly one of seed and uniforms')
        if int(row_offset) < 0:
            raise ValueError('row_offset must be >= 0; got %r' % (row_offset,))
        M = e.shape[0] * A
        if uniforms is not None and (not torch.is_tensor(uniforms) or tuple(uniforms.shape) != (M, 16, 2)):
            raise ValueError('uniforms must be a tensor [%d,16,2]; got %s' % (M, tuple(getattr(uniforms, 'shape', ()))))
        return e, A, M

    def __call__(self, euler, argue_size, seed=None, uniforms=None, out='euler', row_offset=0):
        e, A, M = self._args(euler, argue_size, seed, uniforms, out, row_offset)
        if uniforms is None:
            uniforms = torch.from_numpy(hash_uniforms(seed, M, row_offset))
        u = uniforms.to(device=e.device, dtype=e.dtype)
        lim = self.limits.to(device=e.device, dtype=e.dtype)
        zero = e.new_zeros(())

        def delta(angle, lo, hi, cap, u):
            pos = torch.maximum(torch.minimum(cap, hi - angle), zero)
            neg = torch.minimum(torch.maximum(-cap, lo - angle), zero)
            return (pos - neg) * u + neg
        rep = e.repeat_interleave(A, 0)                                         # np.repeat order: m = n * A + a
        bend = delta(rep[..., 2], lim[:, 0], lim[:, 1], lim[:, 2], u[..., 0])
        splay = delta(rep[..., 1], lim[:, 3], lim[:, 4], lim[:, 5], u[..., 1])
        turn = torch.zeros_like(rep)
        turn[..., 2] = bend
        rz = euler_to_mat(turn)
        turn = torch.zeros_like(rep)
        turn[..., 1] = splay
        E = euler_to_mat(rep) @ rz @ euler_to_mat(turn)
        return mat_to_euler(E) if out == 'euler' else self.converter._flip(self.converter._e_to_q(E))


class FusedPoseAugmenter(PoseAugmenter, _DeviceTable):
    """`PoseAugmenter` on rih_pose_convert: Euler in, the variants' Euler angles or quaternions out, ONE launch, no bytes of
    traffic for the draws when seeded.  fp32 GPU tensors only; `result=` is a buffer to write into (for a captured graph)."""

    def __init__(self, side, mano, ranges=SCRIPT_RANGES, max_bend=120, max_splay=30, tables=None):
        super().__init__(side, mano, ranges, max_bend, max_splay, tables)
        self._table_rows = _table(self.side, self.converter.tables, self.converter.hands_mean, self.ranges,
                                  (self.max_bend, self.max_splay))
        self._tables = {}

    def __call__(self, euler, argue_size, seed=None, uniforms=None, out='euler', row_offset=0, result=None):
        e, A, M = self._args(euler, argue_size, seed, uniforms, out, row_offset)
        e = _fp32(e)
        if uniforms is not None:
            uniforms = _fp32(uniforms)
        shape = (M, 16, 4 if out == 'quat' else 3)
        if result is None:
            result = torch.empty(shape, device=e.device, dtype=torch.float32)
        elif not torch.is_tensor(result) or tuple(result.shape) != shape or result.dtype != torch.float32 or \
                not result.is_contiguous():
            raise ValueError('result must be a contiguous fp32 tensor %s' % (list(shape),))
        return _launch(e, None, result, self._device_table(e.device), uniforms, 0 if seed is None else seed, row_offset, M, A,
                       EULER, 1 if uniforms is None else 2, _OUT[out])


# ------------------------------------------------------------------------------------------------ validity judge
class PoseValidJudge:
    """ValidJudger in plain torch.  __call__(left_quat [N,16,4], right_quat [N,16,4]) -> (residual [N,2] in radians: column 0
    the left hand, column 1 the right; invalid bool [N] = a residual above 0.1 degrees).  The reference's `ComputeValidation`
    writes `((r > t) + l > t) > 0`; `l` is a residual, so l >= 0 and (0 or 1) + l > t holds exactly when r > t or l > t: that
    is what `invalid` is.  The number the reference prints and calls the valid rate is the share of INVALID frames; `rate()`
    returns that share over all calls since construction or `reset()` (one host read, there only; the count is `torch.sum` of
    the flags)."""

    def __init__(self, mano_left, mano_right=None, tables=None):
        """`mano_left`, `mano_right`: model dicts or pickle paths; one argument {'left': ..., 'right': ...} is taken apart.
        `tables`: {'left': (t0, t1), 'right': (t0, t1)} as `PoseConverter` takes them."""
        if mano_right is None and isinstance(mano_left, dict) and set(mano_left) == {'left', 'right'}:
            mano_left, mano_right = mano_left['left'], mano_left['right']
        if mano_right is None:
            raise ValueError("the judge needs both hands' models: (mano_left, mano_right) or {'left': ..., 'right': ...}")
        tables = tables or {}
        self.converters = {'left': PoseConverter('left', mano_left, tables.get('left')),
                           'right': PoseConverter('right', mano_right, tables.get('right'))}
        self.zero = {s: self._zero(s, torch.float32) for s in self.converters}
        lim = np.zeros((15, 4), np.float64)
        lim[:, 0], lim[:, 1], lim[:, 2], lim[:, 3] = -np.inf, np.inf, -np.inf, np.inf
        for j, (lo, hi) in BEND.items():
            lim[j, 0:2] = lo, hi
        for j, (lo, hi) in SPLAY.items():
            lim[j, 2:4] = lo, hi
        self.limits = torch.from_numpy(lim)
        self.reset()

    def _zero(self, side, dtype, device='cpu'):
        """The identity pose's frames [1,15,3,3], computed in the working precision as the reference's `zero_mat_` is."""
        ident = torch.zeros(1, 16, 4, dtype=dtype, device=device)
        ident[..., 0] = 1.0
        return mano_quat_2_mat(ident, self.converters[side].tables, side)[:, 1:]

    def reset(self):
        self.frames, self._invalid = 0, None

    def rate(self):
        """The reference's "valid rate": invalid frames / frames, over the calls so far."""
        if not self.frames:
            raise RuntimeError('no frame has been judged yet')
        return float(self._invalid) / self.frames

    def _count(self, invalid):
        n = torch.sum(invalid)
        self._invalid = n if self._invalid is None else self._invalid + n.to(self._invalid.device)
        self.frames += invalid.shape[0]

    def _check(self, left_quat, right_quat):
        lq, rq = _rows(left_quat, 4, 'left_quat'), _rows(right_quat, 4, 'right_quat')
        if lq.shape[0] != rq.shape[0] or lq.dtype != rq.dtype or lq.device != rq.device:
            raise ValueError('left_quat and right_quat must share N, dtype and device')
        return lq, rq

    def residual(self, quat, side):
        """One hand's residual [N]."""
        q = _rows(quat, 4, 'quat')
        ja = mano_quat_2_mat(q, self.converters[side].tables, side)[:, 1:]
        x = (self._zero(side, q.dtype, q.device).transpose(3, 2) @ ja)[..., 0]                                 # [N,15,3]
        bend = torch.atan2(x[..., 1], x[..., 0]) * 180 / math.pi
        splay = torch.atan2(-x[..., 2], x[..., 0]) * 180 / math.pi
        lim = self.limits.to(device=q.device, dtype=q.dtype)
        over = torch.maximum(torch.maximum(torch.relu(bend - lim[:, 1]), torch.relu(lim[:, 0] - bend)),
                             torch.maximum(torch.relu(splay - lim[:, 3]), torch.relu(lim[:, 2] - splay)))
        return (over / 180 * math.pi).amax(1)

    def __call__(self, left_quat, right_quat):
        lq, rq = self._check(left_quat, right_quat)
        res = torch.stack([self.residual(lq, 'left'), self.residual(rq, 'right')], 1)
        invalid = (res > THRESHOLD).any(1)
        self._count(invalid)
        return res, invalid


class FusedPoseValidJudge(PoseValidJudge, _DeviceTable):
    """`PoseValidJudge` on rih_pose_convert: both hands in ONE launch (the per-frame maximum is a reduction over the 16 lanes
    of a sample), the flags and their `torch.sum` in torch.  fp32 GPU tensors only."""

    def __init__(self, mano_left, mano_right=None, tables=None):
        super().__init__(mano_left, mano_right, tables)
        self._table_rows = np.stack([_table(s, self.converters[s].tables, self.converters[s].hands_mean)
                                     for s in ('left', 'right')])
        self._tables = {}

    def __call__(self, left_quat, right_quat):
        lq, rq = self._check(left_quat, right_quat)
        lq, rq = _fp32(lq), _fp32(rq)
        res = torch.empty((lq.shape[0], 2), device=lq.device, dtype=torch.float32)
        _launch(lq, rq, res, self._device_table(lq.device), None, 0, 0, lq.shape[0], 1, QUAT, 0, VALID)
        invalid = (res > THRESHOLD).any(1)
        self._count(invalid)
        return res, invalid


# ------------------------------------------------------------------------------------------------ dict-level glue (host side)
def _tensor(a, like):
    return torch.as_tensor(np.asarray(a, np.float64)).to(device=like['device'], dtype=like['dtype'])


def _np(t):
    return t.detach().cpu().numpy()


def _pair(things, what):
    if not isinstance(things, dict) or set(things) != {'left', 'right'}:
        raise ValueError("%s must be {'left': ..., 'right': ...}" % what)
    return things


def annotations_to_mocap(frames, converters, dtype=torch.float32, device='cpu'):
    """data/template_0_pose_convert.py without its file handling: `frames` is a sequence of annotation dicts
    (frame['mano_params'][side] = {'oripose' (or 'pose') 48 axis-angle values, 'trans' [1,3], 'shape' [1,10]}); `converters` =
    {'left': ..., 'right': ...} of either converter class, run in `dtype` on `device`.  -> the mocap dict {'right': {'rot'
    [N,16,3] Euler degrees, 'loc' [N,3] in cm (x 100), 'shape' [N,1,10]}, 'left': {...}, 'capture_frame_id' arange(N)}."""
    _pair(converters, 'converters')
    frames = list(frames)
    if not frames:
        raise ValueError('no frames')
    like = dict(dtype=dtype, device=device)
    out = {}
    for side in ('right', 'left'):
        p = [f['mano_params'][side] for f in frames]
        aa = _tensor([np.asarray(q['oripose'] if 'oripose' in q else q['pose']).reshape(16, 3) for q in p], like)
        shape = np.stack([np.asarray(q['shape']).reshape(1, 10) for q in p])
        trans = _tensor([np.asarray(q['trans']).reshape(3) for q in p], like)
        c = converters[side]
        out[side] = {'rot': _np(c.annotation_to_euler(aa)),
                     'loc': _np(c.trans_to_loc(_tensor(shape[:, 0], like), trans)) * 100, 'shape': shape}
    out['capture_frame_id'] = np.arange(len(frames))
    return out


def augment_mocap(data, argue_size, seed, augmenters, dtype=torch.float32, device='cpu'):
    """data/template_1_pose_argue.py without `add_origin` and the 5000-frame file splitting: 'rot' goes through the side's
    augmenter (`augmenters` = {'left': ..., 'right': ...}; the right hand draws from `seed` * 2, the left from `seed` * 2 + 1),
    'loc', 'shape' and 'capture_frame_id' are repeated `argue_size` times (np.repeat).  `data` is left untouched."""
    _pair(augmenters, 'augmenters')
    like = dict(dtype=dtype, device=device)
    out = {}
    for k, side in enumerate(('right', 'left')):
        rot = augmenters[side](_tensor(data[side]['rot'], like), argue_size, seed=int(seed) * 2 + k)
        out[side] = {'rot': _np(rot), 'loc': np.repeat(np.asarray(data[side]['loc']), argue_size, axis=0),
                     'shape': np.repeat(np.asarray(data[side]['shape']), argue_size, axis=0)}
    out['capture_frame_id'] = np.repeat(np.asarray(data['capture_frame_id']), argue_size)
    return out


def _shape10(a):
    return np.asarray(a, np.float32).reshape(-1, 10)


def mocap_to_optimizer(data, mocap_scale, converters, dtype=torch.float32, device='cpu'):
    """batch_optimize_mocap_origin.py:41-46, 385-393: -> {'right_quat', 'right_loc', 'left_quat', 'left_loc', 'hand_shape'
    [N,20] (right then left)}, CPU tensors, the five sequences `pose_driver.optimize_sequence` takes; loc = loc / 100 *
    mocap_scale."""
    _pair(converters, 'converters')
    like = dict(dtype=dtype, device=device)
    out = {}
    for side in ('right', 'left'):
        out[side + '_quat'] = converters[side].euler_to_quat(_tensor(data[side]['rot'], like)).detach().cpu()
        out[side + '_loc'] = torch.as_tensor(np.asarray(data[side]['loc'], np.float64) / 100 * mocap_scale).to(dtype)
    out['hand_shape'] = torch.from_numpy(np.concatenate([_shape10(data['right']['shape']), _shape10(data['left']['shape'])], 1))
    return out


def optimizer_to_mocap(result, data, converters, dtype=torch.float32, device='cpu'):
    """batch_optimize_mocap_origin.py:579-585: `result` = what `optimize_sequence` returns ({'right': {'rot' quaternions,
    'loc'}, 'left': {...}}); -> a deep copy of `data` with 'rot' = the quaternions' Euler degrees and 'loc' = loc * 100."""
    _pair(converters, 'converters')
    like = dict(dtype=dtype, device=device)
    out = copy.deepcopy(data)
    for side in ('right', 'left'):
        rot = torch.as_tensor(result[side]['rot']).detach().to(**like)
        out[side]['rot'] = _np(converters[side].quat_to_euler(rot))
        out[side]['loc'] = _np(torch.as_tensor(result[side]['loc']).detach().double()) * 100
    return out


def mocap_to_annotations(data, converters, dtype=torch.float32, device='cpu'):
    """data/template_3_pose_reconvert.py (`data_loader` with mode 0 and scale 1.0) without its file writing: -> a list of N
    frames {'mano_params': {side: {'pose' [16,3] axis-angle, 'trans' [1,3], 'shape' [1,10]}}, 'capture_frame_id': id}."""
    _pair(converters, 'converters')
    like = dict(dtype=dtype, device=device)
    per = {}
    for side in ('right', 'left'):
        c = converters[side]
        shape = _shape10(data[side]['shape'])
        loc = _tensor(np.asarray(data[side]['loc'], np.float64) * 1.0 / 100, like)
        per[side] = (_np(c.euler_to_annotation(_tensor(data[side]['rot'], like))),
                     _np(c.loc_to_trans(_tensor(shape, like), loc)), shape)
    ids = np.asarray(data['capture_frame_id'])
    return [{'mano_params': {side: {'pose': per[side][0][i], 'trans': per[side][1][i:i + 1], 'shape': per[side][2][i:i + 1]}
                             for side in ('left', 'right')}, 'capture_frame_id': ids[i]} for i in range(len(ids))]
