"""The sequence driver of the two-hand pose optimiser: the attempt loop of pose_data_optimize/batch_optimize_mocap_origin.py
`main` (:460-560) with `update_scene` (:227-317) and `run_sample` (:654-738) folded in, over an optimiser of
renderih_amd.pose_opt and a search of renderih_amd.contact_search.

`REFERENCE_SCHEDULE` restates :460-479 -- per attempt (factor on lambda_repulsion_loss, factor on lambda_contact_loss, n_iter,
fresh search); the factors scale the `coef_val` found at entry.  Per attempt `optimize_sequence`
  1. computes both hands' meshes of all N frames with `optimizer.hands`, adds the translations (no gradient);
  2. on a fresh attempt searches all N frames anew (:484-500); attempts 1 and 2 keep the ids of attempt 0;
  3. refreshes the weights of the current ids on the current meshes (:522-532, `update_scene(anchor_id=...)`);
  4. per batch of `batch_size` frames (the last one shorter) calls `set_opt_val` with the arguments `run_sample` builds
     (:706-734), `optimize()`, and writes the four results back into the sequence (:555-558).
The batches of one attempt are disjoint, and a frame's tables depend on that frame alone, so searching all N frames before the
first batch computes what the reference's per-batch search does.

DELIBERATE DEVIATIONS: `coef_val` and `n_iter` are restored on exit (the reference leaves the last attempt's).  `obj_anchors`
and `obj_normals` are not handed to `set_opt_val` (mode='both' ignores them, and the fused search keeps them in LDS).  Not
reproduced, all dead under the driver's `discrete_optimize = True`: the anchor similarity with `filter_anchor_id` (:277-287,
:503-504), `get_joint_change` (:596-623; multiplied by 0 at :509-511, so `consistent_mask` is handed over as zeros), the file
output (:593), and every visualisation.  The Euler input (:385-388) and output (:579-585) around the loop are
`pose_convert.mocap_to_optimizer` and `pose_convert.optimizer_to_mocap`.
"""
import torch

# (repulsion factor, contact factor, n_iter, fresh search)        batch_optimize_mocap_origin.py:460-479, :484
REFERENCE_SCHEDULE = ((1.0, 1.0, 50, True), (0.1, 15.0, 40, False), (30.0, 0.1, 75, False), (1.0, 5.0, 50, True))
FINGERS = list(range(1, 16))


def _sequence(x, shape, dtype, name):
    x = torch.as_tensor(x).detach().to('cpu', dtype, copy=True)
    if tuple(x.shape[1:]) != shape:
        raise ValueError('%s must be [N,%s]; got %s' % (name, ','.join(map(str, shape)), tuple(x.shape)))
    return x


def scene_meshes(optimizer, right_quat, right_loc, left_quat, left_loc, hand_shape):
    """Both hands' translated vertices [N,V,3] on the optimiser's device (update_scene :246-257)."""
    dev = optimizer.device
    with torch.no_grad():
        shape = hand_shape.to(dev)
        vm = optimizer.hands[0](right_quat.to(dev), shape[:, :10])[0] + right_loc.to(dev).unsqueeze(1)
        vs = optimizer.hands[1](left_quat.to(dev), shape[:, 10:])[0] + left_loc.to(dev).unsqueeze(1)
    return vm, vs


def opt_val_kwargs(tables, start, stop, right_quat, right_loc, left_quat, left_loc, hand_shape):
    """The arguments of `set_opt_val` for the frames [start, stop) as run_sample :706-734 builds them."""
    cut = slice(start, stop)
    rq, lq = right_quat[cut], left_quat[cut]
    n = stop - start
    return dict(vertex_contact=tables['vertex_contact'][cut], contact_region=torch.zeros_like(tables['vertex_contact'][cut]),
                anchor_id=tables['anchor_id'][cut], anchor_elasti=tables['anchor_elasti'][cut],
                anchor_padding_mask=tables['anchor_padding_mask'][cut],
                hand_shape_init=hand_shape[cut], hand_tsl_init=right_loc[cut],
                hand_pose_gt=([0], rq[:, 0:1]), hand_pose_init=(FINGERS, rq[:, 1:]), runtime_vis=None,
                obj_tsl_init=left_loc[cut], obj_pose_gt=([0], lq[:, 0:1]), obj_pose_init=(FINGERS, lq[:, 1:]),
                optimize_it=tables['optimize_it'][cut], batch_size=n,
                consistent_mask=[torch.zeros(n, 16), torch.zeros(n, 16)])


def optimize_sequence(optimizer, search, right_quat, right_loc, left_quat, left_loc, hand_shape, batch_size,
                      schedule=REFERENCE_SCHEDULE):
    """Optimise a sequence of N frames; see the module docstring.  `optimizer`: a `TwoHandPoseOptimizer` or
    `FusedTwoHandPoseOptimizer`; `search`: a `TwoHandContactSearch` or `FusedTwoHandContactSearch` on the optimiser's device.
    right_quat, left_quat [N,16,4] (w, x, y, z), right_loc, left_loc [N,3], hand_shape [N,20] (right then left): arrays or
    tensors, left untouched.  -> {'right': {'rot' [N,16,4], 'loc' [N,3]}, 'left': {...}} as CPU tensors."""
    dtype = optimizer.dtype
    rq, lq = _sequence(right_quat, (16, 4), dtype, 'right_quat'), _sequence(left_quat, (16, 4), dtype, 'left_quat')
    rl, ll = _sequence(right_loc, (3,), dtype, 'right_loc'), _sequence(left_loc, (3,), dtype, 'left_loc')
    shape = _sequence(hand_shape, (20,), dtype, 'hand_shape')
    N, batch_size = rq.shape[0], int(batch_size)
    if N < 1 or any(x.shape[0] != N for x in (lq, rl, ll, shape)):
        raise ValueError('the five sequences must have one length N >= 1; got %s' % [x.shape[0] for x in (rq, rl, lq, ll, shape)])
    if batch_size < 1:
        raise ValueError('batch_size must be at least 1; got %r' % (batch_size,))
    schedule = [(float(r), float(c), int(n), bool(f)) for r, c, n, f in schedule]
    if not schedule or not schedule[0][3]:
        raise ValueError('the first attempt of a schedule must search afresh: there are no ids to refresh yet')
    entry_coef, entry_n_iter = dict(optimizer.coef_val), optimizer.n_iter
    ids = None
    try:
        for repulsion, contact, n_iter, fresh in schedule:
            optimizer.coef_val['lambda_repulsion_loss'] = entry_coef['lambda_repulsion_loss'] * repulsion
            optimizer.coef_val['lambda_contact_loss'] = entry_coef['lambda_contact_loss'] * contact
            optimizer.n_iter = n_iter
            vm, vs = scene_meshes(optimizer, rq, rl, lq, ll, shape)
            if fresh:
                ids = search(vm, vs)['anchor_id']
            tables = search(vm, vs, ids)
            for start in range(0, N, batch_size):
                stop = min(start + batch_size, N)
                optimizer.set_opt_val(**opt_val_kwargs(tables, start, stop, rq, rl, lq, ll, shape))
                res = optimizer.optimize(progress=False)
                rq[start:stop], rl[start:stop] = res['optimized_hand_pose'], res['optimized_hand_tsl']
                lq[start:stop], ll[start:stop] = res['optimized_sub_hand_pose'], res['optimized_sub_hand_tsl']
    finally:
        optimizer.coef_val.clear()
        optimizer.coef_val.update(entry_coef)
        optimizer.n_iter = entry_n_iter
    return {'right': {'rot': rq, 'loc': rl}, 'left': {'rot': lq, 'loc': ll}}
