"""The two-hand pose optimiser (renderih_amd.pose_opt; reference hocontact/postprocess/geo_optimizer_both_batch.py, mode='both')
on the CPU: the step kernels (csrc/rih_pose_opt.hip) through the host-compiled library, teacher-forced against torch's own Adam
and ReduceLROnPlateau; the fused loop (eager, on the host shim) against the mirror loop; the surface.
tests/test_gpu_pose_opt.py shares the helpers.

Bars (none of them taken from the code under test):
  scheduler   learning rates, num_bad_epochs, best: EQUAL to torch's ReduceLROnPlateau after every iteration (double arithmetic
              on both sides; the crafted losses are a factor 2 away from the threshold either way).
  parameters  the project's convention (testing.assert_fp32_equivalent, k = 4, floor 0): the kernel's deviation from torch's
              fp64 Adam is at most 4 x the deviation of torch's own fp32 Adam (run on the device under test) from it, per tensor,
              relative to the largest |parameter|.  Found (profiles/pose_optimizer/deviation_{cpu,gpu}.log): see there.
  loop        over the first K iterations the fused loop's losses and parameters deviate from the fp64 mirror loop by at most
              4 x what the fp32 mirror loop does.  K = 12, the length of the runs here: on the CPU the fp32 mirror stays within
              1e-5 of the largest parameter change over these 12 and over the 16 iterations that were measured, far below the
              1e-3 that ends the prefix (asserted below; figures in the same logs).  Poses: chain_poses(LOOP_SEED[B], B) --
              with seeds 1 and 5 at B = 1 a first-step gradient changes sign between fp32 and fp64 and the mirrors alone
              separate by 0.3 and 6e-3 of the largest change, so those are not used.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

from quat_mano_cases import ANCHOR_DIR, mano_dict  # noqa: E402
from renderih_amd import testing  # noqa: E402
from test_gpu_quat_mano import chain_poses  # noqa: E402
from test_two_hand_sdf import PART_VERT  # noqa: E402

T, PATIENCE = 70, 3
G, D = 8, 4
K = 12                                    # compared prefix of the loops (>= 10); see the module docstring
LOOP_SEED = {1: 3, 2: 1}                  # chain_poses seeds per batch size for which the mirrors alone keep that prefix
KEYS = ('optimized_hand_pose', 'optimized_hand_tsl', 'optimized_sub_hand_pose', 'optimized_sub_hand_tsl')


# ------------------------------------------------------------------------------------------------ step kernels, teacher-forced
def crafted_losses():
    """T fp32 losses for patience = 3: ten clear improvements; eight flat values (two reductions); three improvements by a
    factor 1 - 5e-5 of the best (bad epochs); three by 1 - 2e-4 (good ones); a NaN; flat values until the translation groups
    sit at min_lr and stop changing."""
    seq, x = [], 10.0
    for _ in range(10):
        x *= 0.8
        seq.append(x)
    seq += [x] * 8
    seq += [x * (1 - 5e-5)] * 3
    for _ in range(3):
        x *= 1 - 2e-4
        seq.append(x)
    seq.append(float('nan'))
    seq += [x] * (T - len(seq))
    assert len(seq) == T
    return np.asarray(seq, np.float32)


def teacher_case(B, seed=0):
    """Parameters, per-tensor (group, period, skip, lr) and T seeded gradient sets: the optimiser's four tensors (roots frozen)
    plus an unaligned 5-element tensor (tail path) and a 1030-element one (two chunks)."""
    rs = np.random.RandomState(100 + 17 * B + seed)
    shapes = [(B, 3), (B, 3), (B, 16, 4), (B, 16, 4), (5,), (1030,)]
    lrs = [1e-4, 1e-4, 1e-2, 1e-2, 1e-2, 1e-3]
    pattern = [(0, 0), (0, 0), (64, 4), (64, 4), (0, 0), (0, 0)]
    params = [rs.randn(*s).astype(np.float32) for s in shapes]
    grads = [[(rs.randn(*s) * rs.uniform(0.01, 3.0)).astype(np.float32) for s in shapes] for _ in range(T)]
    for gs in grads:                                       # elements whose gradient is zero throughout
        gs[0][0, 1] = 0.0
        gs[5][7] = 0.0
        gs[5][1029] = 0.0
    return params, grads, lrs, pattern


def torch_reference(params, grads, lrs, pattern, losses, dtype, device='cpu'):
    """torch.optim.Adam + ReduceLROnPlateau(patience=3) on the same gradients (frozen elements: gradient zeroed, so torch
    leaves them alone) -> per iteration (lrs, num_bad, best) and the parameters after iterations 10, 20, ..., T."""
    ps = [torch.tensor(p, dtype=dtype, device=device, requires_grad=True) for p in params]
    opt = torch.optim.Adam([{'params': [p], 'lr': lr} for p, lr in zip(ps, lrs)])
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode='min', factor=0.5, patience=PATIENCE, min_lr=1e-5)
    trace, snaps = [], {}
    for it in range(T):
        for p, g, (period, skip) in zip(ps, grads[it], pattern):
            g = torch.tensor(g, dtype=dtype, device=device)
            if period:
                g.view(-1, period)[:, :skip] = 0
            p.grad = g
        opt.step()
        sched.step(torch.tensor(losses[it]))
        trace.append(([float(g['lr']) for g in opt.param_groups], int(sched.num_bad_epochs), float(sched.best)))
        if (it + 1) % 10 == 0:
            snaps[it + 1] = [p.detach().clone() for p in ps]
    return trace, snaps


def run_step_kernels(B, device, log=print):
    """The teacher-forced run of rih_adam_dev + rih_plateau_step on `device` with every assertion of the issue's check 1."""
    from renderih_amd.pose_opt import DeviceAdamPlateau
    params, grads, lrs, pattern = teacher_case(B)
    losses = crafted_losses()
    want_trace, want64 = torch_reference(params, grads, lrs, pattern, losses, torch.float64)
    _, want32 = torch_reference(params, grads, lrs, pattern, losses, torch.float32, device)
    store = torch.zeros(6, device=device)                              # the 5-element tensor starts 4 bytes off alignment
    ps = [torch.tensor(p, device=device) for p in params]
    store[1:].copy_(ps[4])
    ps[4] = store[1:]
    assert ps[4].data_ptr() % 16 == 4
    prev = [None, None, torch.zeros_like(ps[2]), None, None, None]
    entries = [dict(p=p, group=i, period=pat[0], skip=pat[1], prev=pv) for i, (p, pat, pv) in enumerate(zip(ps, pattern, prev))]
    stepper = DeviceAdamPlateau(entries, lrs, patience=PATIENCE)
    start = [p.clone() for p in ps]
    worst = {}
    for it in range(T):
        gs = [torch.tensor(g, device=device) for g in grads[it]]
        before = ps[2].clone()
        stepper.set_grads(gs)
        stepper.step(torch.tensor(losses[it], device=device))
        st = stepper.read_state()
        want_lr, want_bad, want_best = want_trace[it]
        assert st['lr'] == want_lr and st['num_bad_epochs'] == want_bad and st['step'] == it + 1, (it, st, want_trace[it])
        assert st['best'] == want_best, (it, st['best'], want_best)
        assert torch.equal(prev[2], before)                             # the snapshot is the parameter from before the step
        if (it + 1) % 10 == 0:
            for i, (p, w32, w64) in enumerate(zip(ps, want32[it + 1], want64[it + 1])):
                e_got, e_ref = testing.assert_fp32_equivalent(p, w32, w64, k=4.0, floor=0.0, what='tensor %d after %d' % (i, it + 1))
                log('step kernels B=%d on %s: tensor %d after %2d iterations: kernel vs fp64 %.3g, torch fp32 vs fp64 %.3g'
                    % (B, device, i, it + 1, e_got, e_ref))
                worst[i] = max(worst.get(i, (0, 0)), (e_got, e_ref))
    lr_trace = np.asarray([t[0] for t in want_trace])
    assert (lr_trace[-9:, 0] == 1e-5).all() and lr_trace[17, 2] == 2.5e-3 and lr_trace[9, 2] == 1e-2      # the sequence did its job
    assert [t[1] for t in want_trace[18:25]] == [1, 2, 3, 0, 0, 0, 1]            # 1 - 5e-5: bad; 1 - 2e-4: good; NaN: bad
    for i in (2, 3):                                                              # frozen roots, moments included
        e = stepper.params[i]
        assert torch.equal(ps[i][:, 0], start[i][:, 0]) and not e['m'][:, 0].any() and not e['v'][:, 0].any()
        assert not torch.equal(ps[i][:, 1:], start[i][:, 1:])
    for i, idx in ((0, (0, 1)), (5, (7,)), (5, (1029,))):                       # all-zero gradient history
        assert ps[i][idx].item() == start[i][idx].item() and stepper.params[i]['m'][idx].item() == 0
    return worst


@pytest.mark.parametrize('B', [1, 3])
def test_step_kernels_follow_torch_adam_and_plateau_on_cpu(B):
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        run_step_kernels(B, 'cpu')


def test_step_kernels_refuse_bad_arguments():
    from host_kernels import host_kernels_abi, load
    from renderih_amd.pose_opt import DeviceAdamPlateau
    lib = load()
    buf = np.zeros(64, np.float64)
    p = buf.ctypes.data
    einval = lib.rih_anchor_fwd(None, p, p, p, 1, 4, 1, None)
    ok = [p, 1, 4, p, 0.9, 0.999, 1e-8, None]
    for i, bad in ((0, None), (3, None), (1, 0), (2, 0), (4, 1.0), (4, -0.1), (5, 1.0), (6, -1.0), (6, float('nan'))):
        assert lib.rih_adam_dev(*(ok[:i] + [bad] + ok[i + 1:])) == einval, i
    assert lib.rih_plateau_step(None, p, None) == einval and lib.rih_plateau_step(p, None, None) == einval
    x = torch.zeros(4, 16, 4)
    for bad in (dict(p=x, group=1), dict(p=x, group=0, period=4, skip=5), dict(p=x.double(), group=0),
                dict(p=x, group=0, prev=torch.zeros(3))):
        with pytest.raises(ValueError):
            DeviceAdamPlateau([bad], [1e-2])
    with pytest.raises(ValueError):
        DeviceAdamPlateau([dict(p=x, group=0)], [1e-2] * 9)
    with host_kernels_abi():
        stepper = DeviceAdamPlateau([dict(p=x, group=0)], [1e-2])
        with pytest.raises(ValueError):
            stepper.set_grads([torch.zeros(4, 16, 3)])
    with pytest.raises(RuntimeError):                                            # GPU fp32 only: no CPU fallback
        stepper.step(torch.zeros(()))


# ------------------------------------------------------------------------------------------------ the loops
def opt_case(seed, B):
    """The arguments of `set_opt_val` for the interpenetrating hands of `chain_poses`, with random contact tables."""
    q, t = chain_poses(seed, B)
    from renderih_amd.quat_mano import AnchorLayer
    rs = np.random.RandomState(50 + seed)
    A = AnchorLayer(ANCHOR_DIR).face_vert_idx.shape[1]
    q, t = torch.from_numpy(q), torch.from_numpy(t)
    return dict(anchor_id=torch.from_numpy(rs.randint(0, A, size=(B, A, D))), anchor_elasti=torch.from_numpy(rs.rand(B, A, D).astype(np.float32)),
                anchor_padding_mask=torch.from_numpy((rs.rand(B, A, D) < 0.5).astype(np.int64)),
                hand_shape_init=torch.from_numpy((0.3 * rs.randn(B, 20)).astype(np.float32)), hand_tsl_init=t[0], obj_tsl_init=t[1],
                hand_pose_gt=([0], q[0][:, 0:1]), hand_pose_init=(list(range(1, 16)), q[0][:, 1:]),
                obj_pose_gt=([0], q[1][:, 0:1]), obj_pose_init=(list(range(1, 16)), q[1][:, 1:]), batch_size=B,
                vertex_contact=None, runtime_vis=None)                # two of the arguments that are accepted and ignored


def make(cls, device='cpu', **kw):
    kw.setdefault('grid_size', G)
    return cls(mano_dict('right'), mano_dict('left'), ANCHOR_DIR, PART_VERT, device=device, **kw)


def trajectory(opt, case, n):
    """`n` single-iteration calls of optimize() -> per iteration the loss and the parameters AFTER it as float64 numpy
    (poses from the NEXT snapshot are not needed: the translations and the snapshot of the call are compared)."""
    opt.set_opt_val(**case)
    opt.n_iter = 1
    out = []
    for _ in range(n):
        res = opt.optimize()
        out.append(dict(loss=float(opt.last_loss), pen=opt.last_terms['penetration'].double().cpu().numpy(),
                        q=np.stack([res[KEYS[0]].double().numpy(), res[KEYS[2]].double().numpy()]),
                        t=np.stack([res[KEYS[1]].double().numpy(), res[KEYS[3]].double().numpy()])))
    return out


def deviation(got, want, upto):
    """Largest deviation over the first `upto` iterations: of the loss (relative), of the quaternions and of the translations
    (each relative to the largest change of that kind in `want` since its first entry)."""
    loss = max(abs(g['loss'] - w['loss']) / abs(w['loss']) for g, w in zip(got[:upto], want[:upto]))
    par = 0.0
    for k in ('q', 't'):
        change = max(np.abs(w[k] - want[0][k]).max() for w in want[1:upto])
        par = max(par, max(np.abs(g[k] - w[k]).max() for g, w in zip(got[:upto], want[:upto])) / change)
    return loss, par


_REF = {}


def mirror_reference(device='cpu', B=1, n=K):
    """The fp64 and the fp32 mirror loops on `device`, computed once (the mirror's voxeliser is the HIP kernel: on the CPU
    the caller is inside host_kernels_abi())."""
    from renderih_amd.pose_opt import TwoHandPoseOptimizer
    key = (str(device), B, n)
    if key not in _REF:
        case = opt_case(LOOP_SEED[B], B)
        _REF[key] = (trajectory(make(TwoHandPoseOptimizer, device, dtype=torch.float64), case, n),
                     trajectory(make(TwoHandPoseOptimizer, device), case, n))
    return _REF[key]


def check_loop_against_mirror(got, device, B, upto=K, log=print):
    want64, want32 = mirror_reference(device, B)
    ref_loss, ref_par = deviation(want32, want64, upto)
    got_loss, got_par = deviation(got, want64, upto)
    log('loop B=%d on %s, first %d iterations: fp32 mirror vs fp64 mirror: loss %.3g parameters %.3g; fused vs fp64 mirror: loss %.3g '
        'parameters %.3g' % (B, device, upto, ref_loss, ref_par, got_loss, got_par))
    log('losses fp64 %s' % [round(w['loss'], 6) for w in want64])
    assert (want64[0]['pen'] > 1e-3).all() and got[0]['pen'].min() > 1e-3              # the penetration term is active
    assert want64[upto - 1]['loss'] < want64[0]['loss'] and got[upto - 1]['loss'] < got[0]['loss']
    assert got_loss <= 4 * ref_loss and got_par <= 4 * ref_par


def test_mirror_loop_descends_and_fp32_tracks_fp64_over_the_prefix():
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        want64, want32 = mirror_reference()
    loss, par = deviation(want32, want64, K)
    print('mirror loops B=1 on cpu, K = %d: fp32 vs fp64 loss %.3g, parameters %.3g of the largest change' % (K, loss, par))
    assert K >= 10 and par < 1e-3
    assert (want64[0]['pen'] > 1e-3).all() and want64[-1]['loss'] < want64[0]['loss']


def test_fused_loop_matches_mirror_loop_on_cpu():
    """Three eager iterations through the host-compiled kernels (about 2 s each there); the GPU file runs all K."""
    from host_kernels import host_kernels_abi
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    with host_kernels_abi():
        case = opt_case(LOOP_SEED[1], 1)
        got = trajectory(make(FusedTwoHandPoseOptimizer, graph=False), case, 3)
        check_loop_against_mirror(got, 'cpu', 1, upto=3)
    for k, name in ((0, 'hand_pose'), (1, 'obj_pose')):
        assert np.array_equal(got[2]['q'][k][:, 0], case[name + '_gt'][1][:, 0].double().numpy())      # the root never moves


# ------------------------------------------------------------------------------------------------ surface
def check_surface(cls, device, **kw):
    case = opt_case(2, 3)
    opt = make(cls, device, n_iter=3, **kw)
    with pytest.raises(RuntimeError):
        opt.optimize()
    opt.set_opt_val(**case)
    opt.n_iter = 2
    first = opt.optimize()
    opt.n_iter = 1
    res = opt.optimize()                                                      # continues: the third iteration
    assert tuple(res) == KEYS
    for k, shape in zip(KEYS, ((3, 16, 4), (3, 3)) * 2):
        assert tuple(res[k].shape) == shape and res[k].dtype == torch.float32 and res[k].device.type == 'cpu'
        assert not res[k].requires_grad
    q0 = [torch.cat([case[n + '_gt'][1], case[n + '_init'][1]], 1) for n in ('hand_pose', 'obj_pose')]
    for k, q in zip((KEYS[0], KEYS[2]), q0):
        assert torch.equal(res[k][:, 0], q[:, 0]) and not torch.equal(res[k][:, 1:], q[:, 1:])     # constant root, moving fingers
    # the snapshot quirk: the pose of this call is the parameter state the PREVIOUS call left; the translations moved on
    whole = make(cls, device, n_iter=3, **kw)
    whole.set_opt_val(**case)
    three = whole.optimize()
    before = [(x.detach().clone() if x.shape[1] == 15 else x.detach()[:, 1:].clone()) for x in getattr(whole, 'var', None) or whole.q]
    whole.n_iter = 1
    four = whole.optimize()
    for k, kt, b, t in zip((KEYS[0], KEYS[2]), (KEYS[1], KEYS[3]), before, whole.tsl):
        assert torch.equal(four[k][:, 1:], b.cpu()) and torch.equal(four[kt], t.detach().cpu())
    now = [x.detach() if x.shape[1] == 15 else x.detach()[:, 1:] for x in getattr(whole, 'var', None) or whole.q]
    assert not torch.equal(now[0], before[0])
    for k in KEYS:
        assert torch.equal(res[k], three[k])                                 # 2 + 1 iterations = 3
    assert not torch.equal(four[KEYS[0]], three[KEYS[0]]) and not torch.equal(first[KEYS[1]], res[KEYS[1]])
    assert not torch.equal(first[KEYS[0]], res[KEYS[0]])
    whole.set_opt_val(**case)                                                # fresh state: the same three iterations again
    whole.n_iter = 3
    again = whole.optimize()
    for k in KEYS:
        assert torch.equal(again[k], three[k])
    whole.set_opt_val(**case)
    whole.coef_val['lambda_contact_loss'] = 150.0
    other = whole.optimize()
    assert not torch.equal(other[KEYS[0]], three[KEYS[0]])
    assert whole.last_loss.shape == () and whole.last_terms['prior'].shape == (7,) and whole.last_terms['penetration'].shape == (3,)
    for bad in (dict(hand_shape_init=case['hand_shape_init'][:, :10]), dict(hand_tsl_init=case['hand_tsl_init'][:2]),
                dict(hand_pose_gt=([1], case['hand_pose_gt'][1])), dict(obj_pose_init=(list(range(1, 16)), case['obj_pose_init'][1][:, :14])),
                dict(anchor_elasti=case['anchor_elasti'][:, :, :2]), dict(batch_size=4), dict(obj_pose_gt=None)):
        with pytest.raises(ValueError):
            whole.set_opt_val(**dict(case, **bad))
    whole.n_iter = 0
    with pytest.raises(ValueError):
        whole.optimize()
    return three


def test_surface_of_the_mirror():
    from host_kernels import host_kernels_abi
    from renderih_amd.pose_opt import TwoHandPoseOptimizer
    with host_kernels_abi():
        check_surface(TwoHandPoseOptimizer, 'cpu')


def test_fused_optimiser_refuses_what_it_cannot_run():
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer
    with pytest.raises(ValueError):
        make(FusedTwoHandPoseOptimizer, 'cpu', graph=True)
    with pytest.raises(ValueError):
        make(FusedTwoHandPoseOptimizer, 'cpu', graph=False, dtype=torch.float64)
    opt = make(FusedTwoHandPoseOptimizer, 'cpu', graph=False, n_iter=1)
    opt.set_opt_val(**opt_case(2, 1))
    with pytest.raises(RuntimeError):                                            # GPU fp32 only: no CPU fallback
        opt.optimize()
