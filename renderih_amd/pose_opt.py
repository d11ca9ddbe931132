"""The two-hand pose optimiser -- drop-ins for `GeOptimizer` of pose_data_optimize/hocontact/postprocess/
geo_optimizer_both_batch.py in mode='both': `set_opt_val(...)`, a mutable `coef_val` and `n_iter`, `optimize()`.

`TwoHandPoseOptimizer` is the plain-torch mirror (fp64 with dtype=torch.float64): two `QuatManoLayer`, `AnchorLayer`,
`TwoHandSDFLoss` (whose voxel field comes from rih_sdf in fp32, as that mirror takes it: on CPU tensors it needs the
host-compiled kernels of the tests), `TwoHandPriorLoss`, `torch.optim.Adam` over the reference's four groups (translations of the right and the
left hand at 0.01 lr, their 15 finger quaternions at lr) and `ReduceLROnPlateau(mode='min', factor=0.5, patience=20,
min_lr=1e-5)`.  The objective is `loss_fn` :805-825 without the terms that are 0 in this mode:
    quat_norm + edge + lambda_contact * contact + 0.02 * lambda_repulsion * penetration.mean() + ergonomics + 1 * nature
`nature` is the reference's NatureLoss (renderih_amd.nature: `TwoHandNatureLoss` in the mirror, `FusedTwoHandNatureLoss` in the
fused class), present only when the constructor is given `nature=` the discriminator's weights (the reference's
Ver2Code/Discriminator/discrim.pth as a path, or a state dict).  With `nature=None`, the default, the term is absent: the same
launches, the same graph and the same results as before the argument existed, and NOT the reference's objective.

`FusedTwoHandPoseOptimizer` has the same surface on the fused modules.  One iteration -- both hands, anchors, penetration +
prior, `torch.autograd.grad` to quaternions and translations, rih_adam_dev, rih_plateau_step (csrc/rih_pose_opt.hip) -- is
captured once per (batch shape, coef_val) in a `torch.cuda.graph` and replayed `n_iter` times; learning rates, step count, best
loss and bad-epoch counter live in a device block (`DeviceAdamPlateau`), so `optimize()` reads the device only at its end.
Changing `coef_val` or the batch shape recaptures, changing `n_iter` does not, and `set_opt_val` writes into the static
buffers.  `graph=False` launches the same kernels without capture.  `last_loss` (0-dim) and `last_terms` (a dict: 'prior' the
seven terms of `TwoHandPriorLoss`, 'penetration' [B], and with weights 'nature' [4]: the two sides' means and their counts of
judged rows) are device tensors of the last iteration, in place of the reference's per-iteration `.item()` dictionary.  The
NatureLoss mask and its counts live on the device, so they are not part of the graph key.

Quirks of the reference that both keep:
  * the shape (`hand_shape_init` [B,20], right then left) is never optimised: `optimize_hand_shape` is False on every path
    that the driver takes, so it is in no parameter group.
  * the root quaternion is a constant (`hand_pose_gt=([0], q[:, 0:1])`): it comes back bit-equal to the input.
  * `optimized_hand_pose` / `optimized_sub_hand_pose` are the assembled poses from BEFORE the last Adam step -- the assembly is a
    copy made inside `loss_fn` -- while the two translations are the parameters from after it.
  * the returned quaternions are not normalised.
  * `set_opt_val` creates fresh optimiser and scheduler state; a second `optimize()` without it continues.
DELIBERATE DEVIATIONS: the loss is summed as prior + 0.02 * lambda_repulsion * penetration.mean() (the reference adds the
penetration term before the ergonomics term: another rounding order), and the NatureLoss term is added last, as the
reference does, each side's mean taken as renderih_amd.nature describes.  The fused class hands the contact term elastic / mask.sum()
and a mask sum of 1, so that the sum -- a launch argument of rih_pose_prior_fwd -- is not baked into the captured graph and
another batch's contacts replay the same graph (one more rounding per contact pair; an empty mask still gives an exact 0).
The driver's numpy code (`update_scene`, `search_anchors`) and its attempt loop are renderih_amd.contact_search and
renderih_amd.pose_driver.  Not reproduced: the single-hand and object modes, progress bars; `n_iter` < 1 raises (the reference
fails on its missing snapshot).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, ops
from .nature import FusedTwoHandNatureLoss, TwoHandNatureLoss
from .pose_prior import FusedTwoHandPriorLoss, TwoHandPriorLoss
from .quat_mano import AnchorLayer, FusedAnchorLayer, FusedQuatManoLayer, QuatManoLayer
from .sdf import FusedTwoHandSDFLoss, TwoHandSDFLoss, sdf

# torch.optim.lr_scheduler.ReduceLROnPlateau as geo_optimizer_both_batch.py:430 builds it (threshold, cooldown, eps: defaults)
SCHEDULER = dict(mode='min', factor=0.5, patience=20, threshold=1e-4, threshold_mode='rel', cooldown=0, min_lr=1e-5, eps=1e-8)
BETAS, ADAM_EPS = (0.9, 0.999), 1e-8                  # torch.optim.Adam's defaults, which the reference takes
REPULSION_SCALE = 0.02                                # loss_fn :816
KEYS = ('optimized_hand_pose', 'optimized_hand_tsl', 'optimized_sub_hand_pose', 'optimized_sub_hand_tsl')


# ---------------------------------------------------------------------------------------------------- device-state stepper
def _bytes_tensor(struct, device):
    return torch.frombuffer(bytearray(bytes(struct)), dtype=torch.uint8).to(device)


class DeviceAdamPlateau:
    """Adam + ReduceLROnPlateau over a few small fp32 tensors with all optimiser scalars in a device block
    (rih_adam_dev, rih_plateau_step).  `params`: a list of dicts `{'p': tensor, 'group': int, 'period': int, 'skip': int,
    'prev': tensor or None}` -- element i of p is frozen when (i % period) < skip; prev receives p from before each step.
    `lrs`: the initial learning rate of every group.  Buffers are allocated once; `reset()` rewrites them in place."""

    def __init__(self, params, lrs, betas=BETAS, eps=ADAM_EPS, factor=0.5, patience=20, threshold=1e-4, min_lr=1e-5,
                 eps_lr=1e-8):
        if not params or not 1 <= len(lrs) <= len(_lib.OptState().lr):
            raise ValueError('1..%d parameter groups and at least one tensor' % len(_lib.OptState().lr))
        self.params, self.lrs = [dict(p) for p in params], [float(x) for x in lrs]
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.settings = dict(factor=float(factor), patience=int(patience), threshold=float(threshold), min_lr=float(min_lr),
                             eps_lr=float(eps_lr))
        dev = self.params[0]['p'].device
        for e in self.params:
            p, prev = e['p'], e.get('prev')
            e.setdefault('period', 0), e.setdefault('skip', 0)
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                raise ValueError('parameters must be contiguous fp32 tensors on one device')
            if prev is not None and (prev.shape != p.shape or prev.dtype != p.dtype or not prev.is_contiguous()):
                raise ValueError('prev must match its parameter')
            if not 0 <= int(e['group']) < len(self.lrs) or int(e['period']) < 0 or not 0 <= int(e['skip']) <= max(int(e['period']), 0):
                raise ValueError('bad group or frozen pattern: %r' % ({k: e[k] for k in ('group', 'period', 'skip')},))
            e['m'], e['v'] = torch.zeros_like(p), torch.zeros_like(p)
        self.max_n = max(e['p'].numel() for e in self.params)
        self.state = torch.zeros(C.sizeof(_lib.OptState), dtype=torch.uint8, device=dev)
        self.table = torch.zeros(len(self.params) * C.sizeof(_lib.AdamDevEntry), dtype=torch.uint8, device=dev)
        self.reset()

    def reset(self):
        """Fresh Adam moments and scheduler state, written into the existing buffers."""
        st = _lib.OptState(best=float('inf'), step=0, num_bad_epochs=0, ngroups=len(self.lrs), **self.settings)
        for i, lr in enumerate(self.lrs):
            st.lr[i] = lr
        self.state.copy_(_bytes_tensor(st, 'cpu'))
        for e in self.params:
            e['m'].zero_()
            e['v'].zero_()

    def set_grads(self, grads):
        """Point the launch table at these gradient tensors (one per parameter, kept alive by the caller)."""
        rows = (_lib.AdamDevEntry * len(self.params))()
        for r, e, g in zip(rows, self.params, grads):
            if g.shape != e['p'].shape or g.dtype != torch.float32 or not g.is_contiguous() or g.device != e['p'].device:
                raise ValueError('a gradient must match its parameter: contiguous fp32 of shape %s' % (tuple(e['p'].shape),))
            r.p, r.g, r.m, r.v = e['p'].data_ptr(), g.data_ptr(), e['m'].data_ptr(), e['v'].data_ptr()
            r.prev = None if e.get('prev') is None else e['prev'].data_ptr()
            r.n, r.group, r.period, r.skip = e['p'].numel(), int(e['group']), int(e['period']), int(e['skip'])
        self.table.copy_(_bytes_tensor(rows, 'cpu'))

    def adam(self):
        """optimizer.step() alone (rih_adam_dev): the state block is read, not written.  A scheduler kernel follows it --
        `step` here, rih_lr_linear_step in renderih_amd.joint_fit."""
        ops._chk(*[e['p'] for e in self.params])
        ops.check(ops._L().rih_adam_dev(self.table.data_ptr(), len(self.params), self.max_n, self.state.data_ptr(),
                                        self.betas[0], self.betas[1], self.eps, ops._stream()), 'rih_adam_dev')

    def step(self, loss):
        """optimizer.step(); scheduler.step(loss) with `loss` a device fp32 scalar: two launches, no host read."""
        ops._chk(loss)
        self.adam()
        ops.check(ops._L().rih_plateau_step(self.state.data_ptr(), loss.data_ptr(), ops._stream()), 'rih_plateau_step')

    def read_state(self):
        """The device block as a dict (a host read: for tests and reports)."""
        st = _lib.OptState.from_buffer_copy(self.state.cpu().numpy().tobytes())
        return dict(step=int(st.step), best=float(st.best), num_bad_epochs=int(st.num_bad_epochs),
                    lr=[float(st.lr[i]) for i in range(len(self.lrs))])


# ---------------------------------------------------------------------------------------------------- the mirror
class _WidenedVoxeliser(torch.nn.Module):
    """The voxeliser of `TwoHandSDFLoss` for a mirror in another dtype: rih_sdf is fp32 (and has no gradient), so the normalised
    vertices are narrowed for it and the field is widened afterwards."""

    def forward(self, faces, vertices, grid_size=32):
        with torch.no_grad():
            return sdf(faces, vertices.detach().float(), grid_size).to(vertices.dtype)


def _as(x, device, dtype):
    return torch.as_tensor(x.detach() if torch.is_tensor(x) else np.asarray(x)).to(device=device, dtype=dtype)


class TwoHandPoseOptimizer:
    """`GeOptimizer(mode='both')` in plain torch; see the module docstring.  `mano_right`, `mano_left`: model dicts or pickle
    paths as `QuatManoLayer` takes them; `anchor`: the anchor directory (or arrays) of `AnchorLayer`; `part_vert`, `faces`: the
    hand-part table and the face list of `TwoHandSDFLoss` (faces=None: its default, the right hand's); `nature`: the pose
    discriminator's weights (a path or a state dict) for the NatureLoss term, None: no such term."""
    _classes = (QuatManoLayer, AnchorLayer, TwoHandSDFLoss, TwoHandPriorLoss)
    _nature_class = TwoHandNatureLoss

    def __init__(self, mano_right, mano_left, anchor, part_vert, lr=1e-2, n_iter=2500, lambda_contact_loss=10.0,
                 lambda_repulsion_loss=0.5, grid_size=32, faces=None, device='cpu', dtype=torch.float32, nature=None):
        mano_cls, anchor_cls, sdf_cls, prior_cls = self._classes
        self.device, self.dtype = torch.device(device), dtype
        self.lr, self.n_iter = float(lr), int(n_iter)
        self.coef_val = {'lambda_contact_loss': lambda_contact_loss, 'lambda_repulsion_loss': lambda_repulsion_loss}
        self.hands = [mano_cls(m, side=s, center_idx=0) for s, m in (('right', mano_right), ('left', mano_left))]
        self.anchor_layer = anchor_cls(anchor)
        self.sdf_loss = sdf_cls(part_vert, faces=faces, grid_size=grid_size)
        self.prior = prior_cls(mano_right, mano_left, lambda_contact=lambda_contact_loss)
        if dtype != torch.float32:
            self.sdf_loss.sdf = _WidenedVoxeliser()
        self.nature = None if nature is None else self._nature_class(nature)
        self.modules = self.hands + [self.anchor_layer, self.sdf_loss, self.prior] + ([] if nature is None else [self.nature])
        for m in self.modules:
            m.to(device=self.device, dtype=dtype) if dtype != torch.float32 else m.to(self.device)
        self.batch_size = None
        self.last_loss = self.last_terms = None

    # ------------------------------------------------------------------ inputs
    def _inputs(self, anchor_id, anchor_elasti, anchor_padding_mask, hand_shape_init, hand_tsl_init, obj_tsl_init, hand_pose_gt,
                hand_pose_init, obj_pose_gt, obj_pose_init, batch_size):
        """Shape checks of the reference's call -> B, the two full poses [B,16,4], the two translations, the shape."""
        poses = []
        for name, gt, init in (('hand_pose', hand_pose_gt, hand_pose_init), ('obj_pose', obj_pose_gt, obj_pose_init)):
            if gt is None or init is None or list(gt[0]) != [0] or list(init[0]) != list(range(1, 16)):
                raise ValueError("%s_gt must be ([0], q[:, 0:1]) and %s_init (range(1, 16), q[:, 1:])" % (name, name))
            root, var = gt[1], init[1]
            B = int(root.shape[0])
            if tuple(root.shape) != (B, 1, 4) or tuple(var.shape) != (B, 15, 4):
                raise ValueError('%s: expected [B,1,4] and [B,15,4]; got %s and %s' % (name, tuple(root.shape), tuple(var.shape)))
            poses.append(torch.cat([_as(root, self.device, self.dtype), _as(var, self.device, self.dtype)], 1))
        B = poses[0].shape[0]
        if batch_size is not None and int(batch_size) != B or poses[1].shape[0] != B:
            raise ValueError('batch_size %r does not match the poses (%d, %d)' % (batch_size, B, poses[1].shape[0]))
        for name, t, shape in (('hand_shape_init', hand_shape_init, (B, 20)), ('hand_tsl_init', hand_tsl_init, (B, 3)),
                               ('obj_tsl_init', obj_tsl_init, (B, 3))):
            if t is None or tuple(t.shape) != shape:
                raise ValueError('%s must be %s; got %s' % (name, list(shape), None if t is None else tuple(t.shape)))
        for name, t in (('anchor_id', anchor_id), ('anchor_elasti', anchor_elasti), ('anchor_padding_mask', anchor_padding_mask)):
            if t is None or len(t.shape) != 3 or t.shape[0] != B or tuple(t.shape) != tuple(anchor_id.shape):
                raise ValueError('%s must be [B,A,D] like anchor_id; got %s' % (name, None if t is None else tuple(t.shape)))
        return (B, poses, [_as(hand_tsl_init, self.device, self.dtype), _as(obj_tsl_init, self.device, self.dtype)],
                _as(hand_shape_init, self.device, self.dtype))

    def set_opt_val(self, anchor_id=None, anchor_elasti=None, anchor_padding_mask=None, hand_shape_init=None, hand_tsl_init=None,
                    obj_tsl_init=None, hand_pose_gt=None, hand_pose_init=None, obj_pose_gt=None, obj_pose_init=None,
                    batch_size=None, **ignored):
        """The arguments of the reference's call (batch_optimize_mocap_origin.py:706-736) that mode='both' uses; the others
        (vertex_contact, contact_region, obj_anchors, obj_normals, optimize_it, consistent_mask, runtime_vis, ...) are
        accepted and ignored.  Fresh optimiser and scheduler state."""
        B, poses, tsl, shape = self._inputs(anchor_id, anchor_elasti, anchor_padding_mask, hand_shape_init, hand_tsl_init,
                                            obj_tsl_init, hand_pose_gt, hand_pose_init, obj_pose_gt, obj_pose_init, batch_size)
        self.prior.set_contacts(anchor_id, anchor_padding_mask, anchor_elasti)
        self.batch_size, self.shape = B, shape
        self.roots = [p[:, :1].clone() for p in poses]
        self.tsl = [t.clone().requires_grad_(True) for t in tsl]
        self.var = [p[:, 1:].clone().requires_grad_(True) for p in poses]
        self.optimizer = torch.optim.Adam([{'params': [self.tsl[0]], 'lr': 0.01 * self.lr}, {'params': [self.tsl[1]], 'lr': 0.01 * self.lr},
                                           {'params': [self.var[0]], 'lr': self.lr}, {'params': [self.var[1]], 'lr': self.lr}],
                                          lr=self.lr, betas=BETAS, eps=ADAM_EPS)
        self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(self.optimizer, **SCHEDULER)
        self.snapshot = None

    # ------------------------------------------------------------------ objective
    def _objective(self, q_r, q_l, t_r, t_l):
        """-> loss, the terms (the prior's seven, the penetration loss per sample, with weights NatureLoss's four)."""
        vr = self.hands[0](q_r, self.shape[:, :10])[0] + t_r.unsqueeze(1)
        vl = self.hands[1](q_l, self.shape[:, 10:])[0] + t_l.unsqueeze(1)
        pen = self.sdf_loss(torch.stack([vr, vl], 1))
        prior, terms = self.prior(q_r, q_l, vr, vl, self.anchor_layer(vr), self.anchor_layer(vl))
        loss = prior + (REPULSION_SCALE * float(self.coef_val['lambda_repulsion_loss'])) * pen.mean()
        terms = {'prior': terms.detach(), 'penetration': pen.detach()}
        if self.nature is not None:
            nature, counts = self.nature(q_r, q_l)
            loss, terms['nature'] = loss + 1.0 * nature, counts.detach()
        return loss, terms

    def _ready(self):
        if self.batch_size is None:
            raise RuntimeError('call set_opt_val(...) first')
        if int(self.n_iter) < 1:
            raise ValueError('n_iter must be at least 1; got %r' % (self.n_iter,))
        self.prior.lambda_contact = float(self.coef_val['lambda_contact_loss'])

    def _result(self, poses):
        """The reference's dict: four CPU tensors (copies, also where the optimiser itself runs on the CPU)."""
        return {k: x.detach().to('cpu', copy=True) for k, x in zip(KEYS, (poses[0], self.tsl[0], poses[1], self.tsl[1]))}

    def optimize(self, progress=False):
        self._ready()
        for _ in range(int(self.n_iter)):
            self.optimizer.zero_grad()
            q = [torch.cat([r, v], 1) for r, v in zip(self.roots, self.var)]           # the reference's assembled copies
            loss, terms = self._objective(q[0], q[1], self.tsl[0], self.tsl[1])
            loss.backward()
            self.optimizer.step()
            self.scheduler.step(loss.detach())
            self.snapshot = [x.detach() for x in q]
            self.last_loss, self.last_terms = loss.detach(), terms
        return self._result(self.snapshot)


# ---------------------------------------------------------------------------------------------------- the fused loop
class FusedTwoHandPoseOptimizer(TwoHandPoseOptimizer):
    """`TwoHandPoseOptimizer` on the HIP kernels, one iteration = one replayed graph; see the module docstring.  GPU fp32 only."""
    _classes = (FusedQuatManoLayer, FusedAnchorLayer, FusedTwoHandSDFLoss, FusedTwoHandPriorLoss)
    _nature_class = FusedTwoHandNatureLoss
    _CONTACT_CONSTANTS = ('anchor_id', 'elastic', 'cptr', 'clist')

    def __init__(self, *args, graph=True, device='cuda', **kwargs):
        if kwargs.get('dtype', torch.float32) != torch.float32:
            raise ValueError('the fused optimiser is fp32 only')
        super().__init__(*args, device=device, **kwargs)
        self.graph = bool(graph)
        if self.graph and self.device.type != 'cuda':
            raise ValueError('graph=True needs a GPU device')
        self._shape_key = self._graph = self._graph_key = None
        self._capturing = False

    def _allocate(self, B, A, D):
        f32 = dict(device=self.device, dtype=torch.float32)
        self.q = [torch.zeros((B, 16, 4), **f32).requires_grad_(True) for _ in range(2)]
        self.tsl = [torch.zeros((B, 3), **f32).requires_grad_(True) for _ in range(2)]
        self.prev = [torch.zeros((B, 16, 4), **f32) for _ in range(2)]
        self.shape = torch.zeros((B, 20), **f32)
        params = [{'p': self.tsl[0].detach(), 'group': 0}, {'p': self.tsl[1].detach(), 'group': 1},
                  {'p': self.q[0].detach(), 'group': 2, 'period': 64, 'skip': 4, 'prev': self.prev[0]},
                  {'p': self.q[1].detach(), 'group': 3, 'period': 64, 'skip': 4, 'prev': self.prev[1]}]
        self.stepper = DeviceAdamPlateau(params, [0.01 * self.lr, 0.01 * self.lr, self.lr, self.lr],
                                         **{('eps_lr' if k == 'eps' else k): SCHEDULER[k]
                                            for k in ('factor', 'patience', 'threshold', 'min_lr', 'eps')})
        self._contacts = None
        self._shape_key, self._graph, self._graph_key = (B, A, D), None, None

    def _set_contacts(self, anchor_id, mask, elastic):
        """The prior's contact constants with 1 / mask.sum() folded into elastic, copied into the tensors of the first call
        for this shape so that a captured graph keeps reading them."""
        msum = float(np.asarray(mask.detach().cpu() if torch.is_tensor(mask) else mask).sum())
        elastic = np.asarray(elastic.detach().cpu() if torch.is_tensor(elastic) else elastic, np.float64)
        one = np.zeros(elastic.shape, np.int64)
        one.reshape(-1)[0] = 1
        self.prior.set_contacts(anchor_id, one, (elastic / msum if msum > 0 else elastic * 0.0).astype(np.float32))
        fresh = self.prior._constants(self.device)
        if self._contacts is None:
            self._contacts = fresh
        else:
            with torch.no_grad():
                for k in self._CONTACT_CONSTANTS:
                    self._contacts[k].copy_(fresh[k])
            self.prior._const[str(self.device)] = self._contacts

    def set_opt_val(self, anchor_id=None, anchor_elasti=None, anchor_padding_mask=None, hand_shape_init=None, hand_tsl_init=None,
                    obj_tsl_init=None, hand_pose_gt=None, hand_pose_init=None, obj_pose_gt=None, obj_pose_init=None,
                    batch_size=None, **ignored):
        B, poses, tsl, shape = self._inputs(anchor_id, anchor_elasti, anchor_padding_mask, hand_shape_init, hand_tsl_init,
                                            obj_tsl_init, hand_pose_gt, hand_pose_init, obj_pose_gt, obj_pose_init, batch_size)
        if self._shape_key != (B,) + tuple(anchor_id.shape[1:]):
            self._allocate(B, *anchor_id.shape[1:])
        self._set_contacts(anchor_id, anchor_padding_mask, anchor_elasti)
        with torch.no_grad():
            for dst, src in zip(self.q + self.prev + self.tsl + [self.shape], poses + poses + tsl + [shape]):
                dst.copy_(src)
        self.stepper.reset()
        self.batch_size = B

    def _iteration(self):
        loss, terms = self._objective(self.q[0], self.q[1], self.tsl[0], self.tsl[1])
        grads = [g if g.is_contiguous() else g.contiguous() for g in torch.autograd.grad(loss, self.tsl + self.q)]
        if not self._capturing:                                     # under capture the table is filled afterwards
            self.stepper.set_grads(grads)
        self.stepper.step(loss)
        self._grads = grads                                         # the launch table points at them
        self.last_loss, self.last_terms = loss.detach(), terms

    def _capture(self, key):
        """Warm up on a side stream (on copies of the state: the warm-up iteration is undone), capture one iteration, then
        point the launch table at the gradient tensors the capture allocated."""
        statics = [t.detach() for t in self.q + self.tsl + self.prev] + [self.stepper.state] + \
                  [e[k] for e in self.stepper.params for k in ('m', 'v')]
        saved = [t.clone() for t in statics]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            self._iteration()
        torch.cuda.current_stream().wait_stream(side)
        with torch.no_grad():
            for t, s in zip(statics, saved):
                t.copy_(s)
        self._graph = torch.cuda.CUDAGraph()
        self._capturing = True
        try:
            with torch.cuda.graph(self._graph):
                self._iteration()
        finally:
            self._capturing = False
        self.stepper.set_grads(self._grads)
        self._graph_key = key

    def optimize(self, progress=False):
        self._ready()
        if self.graph:
            key = (float(self.coef_val['lambda_contact_loss']), float(self.coef_val['lambda_repulsion_loss']))
            if self._graph is None or self._graph_key != key:
                self._capture(key)
            for _ in range(int(self.n_iter)):
                self._graph.replay()
        else:
            for _ in range(int(self.n_iter)):
                self._iteration()
        return self._result(self.prev)
