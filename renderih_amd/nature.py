"""The pose optimiser's NatureLoss -- drop-ins for `GeOptimizer.NatureLoss`
(pose_data_optimize/hocontact/postprocess/geo_optimizer_both_batch.py:110-132), which `loss_fn` computes on every iteration
(:802) and adds with weight 1 (:824): a pose discriminator (`Pos2dDiscriminator(num_joints=15, hid_dim=512)` of
Ver2Code/Discriminator/discrim.py:66-105, weights `Ver2Code/Discriminator/discrim.pth`) judges the 15 finger quaternions of
each hand, and the hands it does not take for real enough are pushed towards "real" by a binary cross-entropy.

`Pos2dDiscriminator` mirrors the network with the reference's `state_dict` keys; `TwoHandNatureLoss` is the plain-torch mirror
(any dtype, CPU-capable, pinned to the reference by tests/golden/nature_loss.npz); `FusedTwoHandNatureLoss` runs the same sum on
csrc/rih_nature.hip: rih_nature_fwd (one workgroup per tile of rows) + rih_nature_reduce forward, rih_nature_bwd backward.  GPU
fp32 only, no atomics, no host read of device memory: usable under graph capture, two evaluations are bit-identical.
What the reference does, and both keep:
  * `forward(q_r, q_l)` takes the UN-normalised assembled poses [B,16,4]; they are normalised as manopth's
    `normalize_quaternion` does and the root is dropped (`loss_fn` :708, :736, :802).
  * quaternion -> matrix divides by |q|^2 once more (utlize.py:41-69: two_s = 2 / sum(q^2)), then
    `matrix_to_euler_angles(., 'XYZ')` = (atan2(-m12, m22), asin(m02), atan2(-m01, m00)): 45 inputs per hand.
  * d1 = relu(layer_1(x)); d2 = relu(layer_2(d1)); d3 = relu(layer_3(d2) + d1); d4 = layer_4(d3) WITHOUT activation;
    d_last = relu(layer_last(d4)); softmax(layer_pred(d_last)); `relu` is LeakyReLU(0.01).  The network's `dropout` argument is
    unused.
  * per side, only the rows with p1 < 1.5 p0 (p1 < 0.6) enter `binary_cross_entropy(out[mask], (0, 1))`, a mean over
    2 * count elements with torch's log floor of -100; a side without such a row adds exactly 0.  The mask carries no gradient.
  * the loss is right + left.
DELIBERATE DEVIATIONS of the fused class (the mirror is exactly the reference's):
  * asin's argument is clamped to [-1, 1] and a clamped angle has a zero derivative: the reference feeds asin the raw m02, where
    one rounding above 1 gives NaN, and a NaN poisons Adam's moments for the rest of a replayed run.  atan2(0, 0) (gimbal lock)
    passes no gradient either.
  * the reference reads `mask.sum() > 0` on the host; here the counts, the means and the per-row scale 1 / count stay on the
    device (rih_nature_reduce), so nothing is baked into a captured graph.
  * summation order: per row (l0 + l1) / 2, summed over the masked rows of a side in a fixed order, divided by the count
    (the reference: one mean over the 2 * count elements).  `terms` carries no gradient (the mirror's does).
Not reproduced: training the discriminator, the single-hand and object modes.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .ops import check
from .quat_mano import normalize_quaternion

KEYS = tuple('%s.%s' % (layer, p) for layer in ('pose_layer_1', 'pose_layer_2', 'pose_layer_3', 'pose_layer_4', 'layer_last',
                                                'layer_pred') for p in ('weight', 'bias'))
NUM_JOINTS = 15
THRESHOLD = 1.5                                                       # the mask: p1 < 1.5 * p0


def synthetic_state_dict(seed, hid_dim=512, pred_scale=1.0):
    """A reproducible stand-in for discrim.pth (tests, the golden generator, the bench): numpy `RandomState(seed)`, every
    tensor uniform in +-1/sqrt(fan_in) drawn in `KEYS` order as float64 and stored as fp32, `layer_pred.weight` multiplied by
    `pred_scale` (a larger scale spreads the two probabilities, so that rows fall on both sides of the mask)."""
    rng = np.random.RandomState(seed)
    shapes = {'pose_layer_1': (hid_dim, 3 * NUM_JOINTS), 'layer_pred': (2, hid_dim)}
    out = {}
    for key in KEYS:
        layer, kind = key.split('.')
        o, i = shapes.get(layer, (hid_dim, hid_dim))
        bound = 1.0 / math.sqrt(i)
        a = rng.uniform(-bound, bound, size=(o, i) if kind == 'weight' else (o,))
        if key == 'layer_pred.weight':
            a = a * pred_scale
        out[key] = torch.from_numpy(a.astype(np.float32))
    return out


def load_weights(weights):
    """A path (`torch.load(..., map_location='cpu')`) or a state dict -> (dict of the twelve fp32 CPU tensors, hid_dim)."""
    sd = torch.load(weights, map_location='cpu') if isinstance(weights, (str, bytes)) or hasattr(weights, '__fspath__') \
        else weights
    missing = [k for k in KEYS if k not in sd]
    if missing:
        raise ValueError('the discriminator state dict lacks %s' % (missing,))
    sd = {k: torch.as_tensor(sd[k]).detach().to('cpu', torch.float32).contiguous() for k in KEYS}
    H = int(sd['pose_layer_1.weight'].shape[0])
    want = {'pose_layer_1': (H, 3 * NUM_JOINTS), 'layer_pred': (2, H)}
    for key in KEYS:
        layer, kind = key.split('.')
        o, i = want.get(layer, (H, H))
        if tuple(sd[key].shape) != ((o, i) if kind == 'weight' else (o,)):
            raise ValueError('%s must be %s; got %s' % (key, [o, i] if kind == 'weight' else [o], tuple(sd[key].shape)))
    return sd, H


def quaternion_to_euler_xyz(q):
    """[..., 4] (w, x, y, z) -> [..., 3]: the reference's quaternion -> matrix (its own 2 / |q|^2) -> XYZ Euler angles."""
    w, x, y, z = q.unbind(-1)
    s = 2.0 / (q * q).sum(-1)
    m00, m01, m02 = 1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)
    m12, m22 = s * (y * z - x * w), 1 - s * (x * x + y * y)
    return torch.stack([torch.atan2(-m12, m22), torch.asin(m02), torch.atan2(-m01, m00)], -1)


class Pos2dDiscriminator(nn.Module):
    """The reference's pose discriminator: [N, 15 * 4] normalised quaternions -> softmax probabilities [N, 2]."""

    def __init__(self, num_joints=NUM_JOINTS, hid_dim=512):
        super().__init__()
        self.pose_layer_1 = nn.Linear(num_joints * 3, hid_dim)
        self.pose_layer_2 = nn.Linear(hid_dim, hid_dim)
        self.pose_layer_3 = nn.Linear(hid_dim, hid_dim)
        self.pose_layer_4 = nn.Linear(hid_dim, hid_dim)
        self.layer_last = nn.Linear(hid_dim, hid_dim)
        self.layer_pred = nn.Linear(hid_dim, 2)
        self.relu = nn.LeakyReLU()
        self.hid_dim = hid_dim

    def forward(self, x):
        n = x.shape[0]
        x = quaternion_to_euler_xyz(x.reshape(-1, 4)).reshape(n, -1)
        d1 = self.relu(self.pose_layer_1(x))
        d2 = self.relu(self.pose_layer_2(d1))
        d3 = self.relu(self.pose_layer_3(d2) + d1)
        d4 = self.pose_layer_4(d3)
        d_last = self.relu(self.layer_last(d4))
        return torch.softmax(self.layer_pred(d_last), dim=1)


def _check_poses(q_r, q_l):
    B = int(q_r.shape[0]) if q_r.dim() == 3 else -1
    for name, q in (('q_r', q_r), ('q_l', q_l)):
        if q.dim() != 3 or tuple(q.shape) != (B, 16, 4) or B < 1:
            raise ValueError('%s must be [B,16,4] with B >= 1; got %s' % (name, tuple(q.shape)))
    return B


class TwoHandNatureLoss(nn.Module):
    """`GeOptimizer.NatureLoss` for both hands in plain torch, written as the reference writes it (boolean indexing and the
    host-side `if` included).  `weights`: a path or a state dict (`load_weights`).  `forward(q_r, q_l)` with the UN-normalised
    poses [B,16,4] -> (loss, terms[4] = nature_r, nature_l, n_r, n_l).  `outputs` holds the discriminator's two outputs
    [2,B,2] of the last call."""

    def __init__(self, weights):
        super().__init__()
        sd, self.hid_dim = load_weights(weights)
        self.disc = Pos2dDiscriminator(NUM_JOINTS, self.hid_dim)
        self.disc.load_state_dict(sd)
        self.disc.eval()
        for p in self.disc.parameters():
            p.requires_grad_(False)
        self.outputs = None

    def forward(self, q_r, q_l):
        B = _check_poses(q_r, q_l)
        real = torch.cat([q_r.new_zeros(B, 1), q_r.new_ones(B, 1)], 1)
        losses, counts, outs = [], [], []
        for q in (q_r, q_l):
            out = self.disc(normalize_quaternion(q)[:, 1:].reshape(B, -1))
            mask = out[:, 1] < THRESHOLD * out[:, 0]
            loss = q.new_zeros(())
            if mask.sum() > 0:
                loss = torch.nn.functional.binary_cross_entropy(out[mask], real[mask])
            losses.append(loss), counts.append(mask.sum().to(q.dtype)), outs.append(out.detach())
        self.outputs = torch.stack(outs)
        return losses[0] + losses[1], torch.stack(losses + counts)


class _TwoHandNature(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mod, q_r, q_l):
        q_r, q_l = q_r.detach().contiguous(), q_l.detach().contiguous()
        ops._chk(q_r, q_l)                              # fp32 GPU tensors only: there is no CPU fallback
        packed = mod._packed_on(q_r.device)
        B, H = q_r.shape[0], mod.hid_dim
        L, st = ops._L(), ops._stream()
        f32 = dict(device=q_r.device, dtype=torch.float32)
        ws = torch.empty((int(L.rih_nature_ws_floats(B, H)),), **f32)
        loss, terms = torch.empty((), **f32), torch.empty((4,), **f32)
        check(L.rih_nature_fwd(packed.data_ptr(), q_r.data_ptr(), q_l.data_ptr(), ws.data_ptr(), B, H, st), 'rih_nature_fwd')
        check(L.rih_nature_reduce(ws.data_ptr(), loss.data_ptr(), terms.data_ptr(), B, H, st), 'rih_nature_reduce')
        ctx.save_for_backward(packed, q_r, q_l, ws)
        ctx.H = H
        ctx.mark_non_differentiable(terms)
        ctx.set_materialize_grads(False)
        return loss, terms

    @staticmethod
    def backward(ctx, g_loss, g_terms):
        if g_loss is None:
            return None, None, None
        packed, q_r, q_l, ws = ctx.saved_tensors
        g = g_loss.contiguous()
        ops._chk(g)
        dq = torch.empty((2,) + tuple(q_r.shape), device=q_r.device, dtype=torch.float32)
        check(ops._L().rih_nature_bwd(packed.data_ptr(), q_r.data_ptr(), q_l.data_ptr(), ws.data_ptr(), g.data_ptr(),
                                      dq[0].data_ptr(), dq[1].data_ptr(), q_r.shape[0], ctx.H, ops._stream()), 'rih_nature_bwd')
        return None, dq[0], dq[1]


class FusedTwoHandNatureLoss(TwoHandNatureLoss):
    """`TwoHandNatureLoss` on csrc/rih_nature.hip, three launches: rih_nature_fwd (tiles of rows through the six layers with the
    activations in LDS) -> rih_nature_reduce (counts, means and row scales on the device) forward, rih_nature_bwd backward.
    The weights are packed once per device (rih_nature_pack).  DEVIATION from the mirror: asin's argument is clamped to
    [-1, 1] with a zero derivative when clamped (the mirror, like the reference, returns NaN one rounding above 1); see the
    module docstring.  GPU fp32 only; `terms` carries no gradient; `outputs` is not kept."""

    def __init__(self, weights):
        super().__init__(weights)
        if self.hid_dim % 64 or not 64 <= self.hid_dim <= 512:
            raise ValueError('the fused NatureLoss takes a hidden width that is a multiple of 64 in [64, 512]; got %d'
                             % self.hid_dim)
        self._packed = {}

    def _packed_on(self, device):
        key = str(device)
        if key not in self._packed:
            L = ops._L()
            sd = self.disc.state_dict()
            src = [sd[k].detach().to(device=device, dtype=torch.float32).contiguous() for k in KEYS]
            ops._chk(*src)
            packed = torch.empty((int(L.rih_nature_pack_floats(self.hid_dim)),), device=device, dtype=torch.float32)
            check(L.rih_nature_pack(*[t.data_ptr() for t in src], packed.data_ptr(), self.hid_dim, ops._stream()),
                  'rih_nature_pack')
            if packed.is_cuda:
                torch.cuda.current_stream().synchronize()           # `src` is released on return
            self._packed[key] = packed
        return self._packed[key]

    def forward(self, q_r, q_l):
        _check_poses(q_r, q_l)
        return _TwoHandNature.apply(self, q_r, q_l)
