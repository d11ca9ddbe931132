"""The sequence driver (renderih_amd.pose_driver.optimize_sequence; reference batch_optimize_mocap_origin.py `main` :460-560,
`run_sample` :706-734) on the CPU: its bookkeeping with a recording stub in place of the optimiser and the search, and the real
mirror optimiser with the mirror search against the same loop written out below.  Optimiser trajectories are never compared
across implementations (they separate after about a dozen iterations): the driver and the written-out loop run
the SAME objects, so their results are bit-equal.  tests/test_gpu_pose_driver.py shares the helpers."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

from quat_mano_cases import ANCHOR_DIR  # noqa: E402
from test_gpu_quat_mano import chain_poses  # noqa: E402
from test_pose_opt import KEYS, make  # noqa: E402

SHORT_SCHEDULE = ((1.0, 1.0, 2, True), (0.1, 15.0, 1, False), (30.0, 0.1, 1, False), (1.0, 5.0, 2, True))
A, D, V = 6, 4, 5


# ------------------------------------------------------------------------------------------------ bookkeeping, on a stub
class StubSearch:
    """Records every call; the ids of a fresh search are its call number, so that whoever receives them can be told."""

    def __init__(self):
        self.calls = []

    def __call__(self, vm, vs, prev=None):
        n = len(self.calls)
        self.calls.append((vm.clone(), vs.clone(), None if prev is None else prev.clone()))
        B = vm.shape[0]
        ids = torch.full((B, A, D), n, dtype=torch.int64) if prev is None else prev
        contact = torch.zeros(B, A, dtype=torch.int64)
        contact[::2, 0] = 1
        return {'vertex_contact': contact, 'anchor_id': ids, 'anchor_elasti': torch.full((B, A, D), 0.5 + n),
                'anchor_padding_mask': torch.ones(B, A, D, dtype=torch.int64), 'optimize_it': contact.any(1)}


class StubOptimizer:
    """The surface the driver uses.  `optimize()` turns every finger quaternion by +1 and every translation by +0.5 (right) and
    -0.5 (left); the 'mesh' of a hand is its translation-free marker: V copies of (sum of the quaternions, shape[0], side)."""

    def __init__(self):
        self.device, self.dtype = torch.device('cpu'), torch.float32
        self.coef_val = {'lambda_contact_loss': 10.0, 'lambda_repulsion_loss': 0.5, 'other': 7}
        self.n_iter = 100
        self.hands = [self._hand(0), self._hand(1)]
        self.log = []

    @staticmethod
    def _hand(side):
        def forward(q, betas):
            marker = torch.stack([q.sum((1, 2)), betas[:, 0], torch.full((q.shape[0],), float(side))], 1)
            return marker[:, None].repeat(1, V, 1), None, None
        return forward

    def set_opt_val(self, **kw):
        def copy(x):                                  # the driver hands over views of its sequence and writes into it afterwards
            return x.clone() if torch.is_tensor(x) else type(x)(copy(y) for y in x) if isinstance(x, (tuple, list)) else x
        self.kw = {k: copy(v) for k, v in kw.items()}

    def optimize(self, progress=False):
        kw = self.kw
        self.log.append(dict(kw=kw, coef=dict(self.coef_val), n_iter=self.n_iter))
        poses = [torch.cat([kw[n + '_gt'][1], kw[n + '_init'][1] + 1.0], 1) for n in ('hand_pose', 'obj_pose')]
        return dict(zip(KEYS, (poses[0], kw['hand_tsl_init'] + 0.5, poses[1], kw['obj_tsl_init'] - 0.5)))


def near(a, b, atol=1e-5):
    """Equal up to the roundings of a few additions of 0.5 or 1 to numbers of unit size."""
    return a.shape == b.shape and torch.allclose(a, b, rtol=0, atol=atol)


def stub_sequence(N=5):
    rs = np.random.RandomState(3)
    return [rs.randn(N, 16, 4).astype(np.float32), rs.randn(N, 3).astype(np.float32), rs.randn(N, 16, 4).astype(np.float32),
            rs.randn(N, 3).astype(np.float32), rs.randn(N, 20).astype(np.float32)]


def test_driver_bookkeeping_on_a_recording_stub():
    from renderih_amd.pose_driver import REFERENCE_SCHEDULE, optimize_sequence
    assert REFERENCE_SCHEDULE == ((1.0, 1.0, 50, True), (0.1, 15.0, 40, False), (30.0, 0.1, 75, False), (1.0, 5.0, 50, True))
    opt, search, seq = StubOptimizer(), StubSearch(), stub_sequence()
    kept = [x.copy() for x in seq]
    out = optimize_sequence(opt, search, *seq, batch_size=2)
    for x, k in zip(seq, kept):
        assert np.array_equal(x, k)                                                    # the inputs are left untouched
    # the schedule: factors on the coef_val found at entry, n_iter, three batches (2 + 2 + 1) per attempt
    assert len(opt.log) == 12
    for a, (rep, con, n_iter, _) in enumerate(REFERENCE_SCHEDULE):
        for b, (start, stop) in enumerate(((0, 2), (2, 4), (4, 5))):
            e = opt.log[3 * a + b]
            assert e['coef'] == {'lambda_contact_loss': 10.0 * con, 'lambda_repulsion_loss': 0.5 * rep, 'other': 7} and e['n_iter'] == n_iter
            kw = e['kw']
            assert kw['batch_size'] == stop - start and kw['anchor_id'].shape == (stop - start, A, D)
            # the frames of this batch as the attempts before left them: fingers + a, translations +- a / 2; the root constant
            assert list(kw['hand_pose_gt'][0]) == [0] and list(kw['obj_pose_init'][0]) == list(range(1, 16))
            assert torch.equal(kw['hand_pose_gt'][1], torch.from_numpy(kept[0][start:stop, 0:1]))
            assert near(kw['hand_pose_init'][1], torch.from_numpy(kept[0][start:stop, 1:]) + a)
            assert torch.equal(kw['obj_pose_gt'][1], torch.from_numpy(kept[2][start:stop, 0:1]))
            assert near(kw['obj_pose_init'][1], torch.from_numpy(kept[2][start:stop, 1:]) + a)
            assert near(kw['hand_tsl_init'], torch.from_numpy(kept[1][start:stop]) + 0.5 * a)
            assert near(kw['obj_tsl_init'], torch.from_numpy(kept[3][start:stop]) - 0.5 * a)
            assert torch.equal(kw['hand_shape_init'], torch.from_numpy(kept[4][start:stop]))
            # the tables: the ids of the latest fresh search (calls 0 and 4), the weights of this attempt's refresh
            fresh_call, refresh_call = (0, 0, 0, 4)[a], (1, 2, 3, 5)[a]
            assert (kw['anchor_id'] == fresh_call).all() and (kw['anchor_elasti'] == 0.5 + refresh_call).all()
            assert kw['optimize_it'].tolist() == [True, False, True, False, True][start:stop]
            assert kw['vertex_contact'].shape == (stop - start, A) and not kw['contact_region'].any()
            assert [tuple(m.shape) for m in kw['consistent_mask']] == [(stop - start, 16)] * 2 and not kw['consistent_mask'][0].any()
            assert kw['runtime_vis'] is None
    # the searches: fresh ones on attempts 0 and 3 only, every refresh gets the current ids, all on the current meshes
    assert [c[2] is None for c in search.calls] == [True, False, False, False, True, False]
    for call, ids in zip((1, 2, 3, 5), (0, 0, 0, 4)):
        assert search.calls[call][2].shape == (5, A, D) and (search.calls[call][2] == ids).all()
    for call, a in zip(range(6), (0, 0, 1, 2, 3, 3)):
        vm, vs, _ = search.calls[call]
        assert vm.shape == (5, V, 3) and vs.shape == (5, V, 3) and torch.equal(vm[:, 0], vm[:, V - 1])
        rl, ll = torch.from_numpy(kept[1]) + 0.5 * a, torch.from_numpy(kept[3]) - 0.5 * a      # marker + translation, 60 turned numbers
        assert near(vm[:, 0, 0], torch.from_numpy(kept[0]).sum((1, 2)) + 60 * a + rl[:, 0], 1e-4)
        assert near(vs[:, 0, 0], torch.from_numpy(kept[2]).sum((1, 2)) + 60 * a + ll[:, 0], 1e-4)
        assert near(vm[:, 0, 1], torch.from_numpy(kept[4][:, 0]) + rl[:, 1]) and near(vs[:, 0, 1], torch.from_numpy(kept[4][:, 10]) + ll[:, 1])
        assert near(vm[:, 0, 2], rl[:, 2]) and near(vs[:, 0, 2], 1.0 + ll[:, 2])
    # the results are written back; coef_val and n_iter are restored
    assert tuple(out) == ('right', 'left') and all(tuple(out[s]) == ('rot', 'loc') for s in out)
    assert torch.equal(out['right']['rot'][:, 0], torch.from_numpy(kept[0][:, 0])) and near(out['right']['rot'][:, 1:], torch.from_numpy(kept[0][:, 1:]) + 4)
    assert near(out['left']['rot'][:, 1:], torch.from_numpy(kept[2][:, 1:]) + 4)
    assert near(out['right']['loc'], torch.from_numpy(kept[1]) + 2.0) and near(out['left']['loc'], torch.from_numpy(kept[3]) - 2.0)
    assert all(out[s][k].device.type == 'cpu' and out[s][k].dtype == torch.float32 for s in out for k in out[s])
    assert opt.coef_val == {'lambda_contact_loss': 10.0, 'lambda_repulsion_loss': 0.5, 'other': 7} and opt.n_iter == 100


def test_driver_restores_the_settings_after_a_failure_and_refuses_bad_input():
    from renderih_amd.pose_driver import optimize_sequence
    opt, seq = StubOptimizer(), stub_sequence()

    def broken(*a, **k):
        raise RuntimeError('boom')
    opt.optimize = broken
    with pytest.raises(RuntimeError):
        optimize_sequence(opt, StubSearch(), *seq, batch_size=2)
    assert opt.coef_val == {'lambda_contact_loss': 10.0, 'lambda_repulsion_loss': 0.5, 'other': 7} and opt.n_iter == 100
    opt = StubOptimizer()
    for bad in (dict(batch_size=0), dict(schedule=()), dict(schedule=((1.0, 1.0, 2, False),))):
        with pytest.raises(ValueError):
            optimize_sequence(opt, StubSearch(), *seq, **dict(dict(batch_size=2), **bad))
    for i, cut in ((0, np.s_[:, :15]), (1, np.s_[:4]), (4, np.s_[:, :10])):
        with pytest.raises(ValueError):
            optimize_sequence(opt, StubSearch(), *[x[cut] if j == i else x for j, x in enumerate(seq)], batch_size=2)
    assert not opt.log


# ------------------------------------------------------------------------------------------------ the real components
def real_sequence(N=3, seed=1):
    q, t = chain_poses(seed, N)
    shape = (0.3 * np.random.RandomState(70 + seed).randn(N, 20)).astype(np.float32)
    return [q[0], t[0], q[1], t[1], shape]


def written_out_loop(opt, search, seq, batch, schedule):
    """What the driver is specified to do, step by step, over the same optimiser and search."""
    rq, rl, lq, ll, shape = (torch.from_numpy(x.copy()) for x in seq)
    N = rq.shape[0]
    contact0, repulsion0 = opt.coef_val['lambda_contact_loss'], opt.coef_val['lambda_repulsion_loss']
    ids = None
    for repulsion, contact, n_iter, fresh in schedule:
        opt.coef_val['lambda_repulsion_loss'] = repulsion0 * repulsion
        opt.coef_val['lambda_contact_loss'] = contact0 * contact
        opt.n_iter = n_iter
        with torch.no_grad():
            dev = opt.device
            vm = opt.hands[0](rq.to(dev), shape[:, :10].to(dev))[0] + rl.to(dev)[:, None]
            vs = opt.hands[1](lq.to(dev), shape[:, 10:].to(dev))[0] + ll.to(dev)[:, None]
        if fresh:
            ids = search(vm, vs)['anchor_id']
        t = search(vm, vs, ids)
        start = 0
        while start < N:
            n = min(batch, N - start)
            s = slice(start, start + n)
            opt.set_opt_val(vertex_contact=t['vertex_contact'][s], anchor_id=t['anchor_id'][s], anchor_elasti=t['anchor_elasti'][s],
                            anchor_padding_mask=t['anchor_padding_mask'][s], hand_shape_init=shape[s], hand_tsl_init=rl[s],
                            hand_pose_gt=([0], rq[s][:, 0:1]), hand_pose_init=(list(range(1, 16)), rq[s][:, 1:]),
                            obj_tsl_init=ll[s], obj_pose_gt=([0], lq[s][:, 0:1]), obj_pose_init=(list(range(1, 16)), lq[s][:, 1:]),
                            optimize_it=t['optimize_it'][s], batch_size=n)
            res = opt.optimize()
            rq[s], rl[s], lq[s], ll[s] = (res[k] for k in KEYS)
            start += n
    opt.coef_val['lambda_contact_loss'], opt.coef_val['lambda_repulsion_loss'] = contact0, repulsion0
    return rq, rl, lq, ll


def run_real(opt_cls, search_cls, device, log=print, **kw):
    """The driver against the written-out loop on the same objects: bit-equal; finite; both roots bit-equal to the inputs."""
    from renderih_amd.pose_driver import optimize_sequence
    opt = make(opt_cls, device, **kw)
    search = search_cls(ANCHOR_DIR).to(device)
    seq = real_sequence()
    got = optimize_sequence(opt, search, *seq, batch_size=2, schedule=SHORT_SCHEDULE)
    assert opt.coef_val == {'lambda_contact_loss': 10.0, 'lambda_repulsion_loss': 0.5}
    want = written_out_loop(opt, search, seq, 2, SHORT_SCHEDULE)
    for name, g, w, x in zip(('right rot', 'right loc', 'left rot', 'left loc'),
                             (got['right']['rot'], got['right']['loc'], got['left']['rot'], got['left']['loc']), want, seq):
        assert g.shape == x.shape and g.device.type == 'cpu' and torch.isfinite(g).all(), name
        assert torch.equal(g, w), name
        assert not torch.equal(g, torch.from_numpy(x)), name                            # the optimiser moved it
        log('%s: moved by at most %.3g' % (name, float((g - torch.from_numpy(x)).abs().max())))
    assert torch.equal(got['right']['rot'][:, 0], torch.from_numpy(seq[0][:, 0]))
    assert torch.equal(got['left']['rot'][:, 0], torch.from_numpy(seq[2][:, 0]))
    return opt


def test_driver_equals_the_written_out_loop_on_the_mirrors():
    from host_kernels import host_kernels_abi
    from renderih_amd.contact_search import TwoHandContactSearch
    from renderih_amd.pose_opt import TwoHandPoseOptimizer
    with host_kernels_abi():
        run_real(TwoHandPoseOptimizer, TwoHandContactSearch, 'cpu')
