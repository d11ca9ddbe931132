"""Cases and bars of the pose-data converter, augmenter and validity judge (renderih_amd.pose_convert, csrc/rih_pose_convert.hip),
shared by tests/test_pose_convert.py (mirror, and the kernel through the host-compiled library) and
tests/test_gpu_pose_convert.py (the same on the device).  Reference: tests/golden/pose_convert.npz, written by
tests/golden/make_pose_convert_golden.py from the reference's own HandPoseConverter, HandPoseArguer, PoseArguer and ValidJudger.

BARS.  The fp64 mirror meets the fixture at 1e-8 (degrees, quaternion components, radians); where the reference itself rounds
its result to fp32 (the quaternions of `axis_angle_2_mano_quat` and `euler_2_mano_quat`) the mirror's result is rounded the same
way first.  Quaternions compare up to sign per joint.  For fp32 (the mirror in fp32, the kernel on the host and on the device)
the bar per quantity is 4 x the worst error of the fp32 MIRROR against the fixture on the CPU (the device's sincos, atan2 and
asin differ from libm by a few ulp), measured once and written down here -- it does not come from the kernel:
    quantity              fp32 mirror, worst   bar (x 4)    kernel on the host, worst
    Euler degrees         1.962e-05            7.848e-05    1.892e-05
    quaternion component  1.491e-07            5.964e-07    1.788e-07
    axis-angle, radians   2.654e-07            1.062e-06    2.928e-07
    residual, radians     6.460e-07            2.584e-06    2.393e-07
(the fp64 mirror's worst: 4.1e-13 degrees, 0 on the rounded quaternions, 8.9e-16 radians).
`invalid` flags compare exactly (the generator keeps every angle 0.05 degrees away from a limit and from a limit +- the
threshold).  Rotation matrices rebuilt from quaternions (round trips) get 4 x the quaternion bar: R is quadratic in a unit q
with coefficients summing to at most 4 per entry.  Tail shapes and seeded inputs use the same bars: their inputs keep |R20| <
0.98 and rotation angles inside [0.05, 3.0] like the fixture's, except where a test says it sits AT a singular pose.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
from renderih_amd import assets, pose_convert as pc  # noqa: E402
from renderih_amd.quat_mano import QuatManoLayer, quaternion_to_rotation_matrix  # noqa: E402

FIX = np.load(os.path.join(HERE, 'golden', 'pose_convert.npz'))
SIDES = ('right', 'left')
PRESETS = ('script', 'ver2')
FP64_BAR = 1e-8
# worst error of the fp32 mirror against the fixture on the CPU (profiles/pose_convert/pytest_cpu.log), and 4 x that
MIRROR_FP32 = {'euler': 1.962e-5, 'quat': 1.491e-7, 'aa': 2.654e-7, 'residual': 6.460e-7}
BARS = {k: 4 * v for k, v in MIRROR_FP32.items()}
TAILS = (1, 3, 4, 5, 35)
_MANO = {}


def mano(side):
    """The synthetic model the fixture was made with, with the fixture's grid-rounded hands_mean (see the generator)."""
    if side not in _MANO:
        d = dict(assets.synthetic_mano_dict(side, seed=0))
        d['hands_mean'] = FIX[side + '/hands_mean'].reshape(45).astype(np.float64)
        _MANO[side] = d
    return _MANO[side]


_OBJ = {}


def tables(side):
    """The axis tables the fixture was made with: both sides of every comparison run on identical fp32 tables
    (`pose_prior.axis_tables` runs the hand model in fp32; its last bits differ from one CPU to another)."""
    return FIX[side + '/inv_m_u_0'], FIX[side + '/inv_u_m_1']


def make(cls, *args):
    key = (cls, args)
    if key not in _OBJ:
        if cls in (pc.PoseValidJudge, pc.FusedPoseValidJudge):
            _OBJ[key] = cls(mano('left'), mano('right'), tables={s: tables(s) for s in SIDES})
        elif args[1:] == ('ver2',):
            _OBJ[key] = cls.ver2(args[0], mano(args[0]), tables=tables(args[0]))
        else:                                                                  # converters, and the 'script' preset (the default)
            _OBJ[key] = cls(args[0], mano(args[0]), tables=tables(args[0]))
    return _OBJ[key]


def run_tables():
    """What the classes build by default is the fixture's tables up to the fp32 rounding of the hand model behind them."""
    for side in SIDES:
        for got, want in zip(pc.PoseConverter(side, mano(side)).tables, tables(side)):
            assert err(got, want) <= 2e-5, side


def classes(fused):
    return (pc.FusedPoseConverter, pc.FusedPoseAugmenter, pc.FusedPoseValidJudge) if fused else \
        (pc.PoseConverter, pc.PoseAugmenter, pc.PoseValidJudge)


def T(a, device, dtype):
    return torch.as_tensor(np.asarray(a)).to(device=device, dtype=dtype)


def err(got, want):
    return float((got.detach().double().cpu() - torch.as_tensor(np.asarray(want)).double()).abs().max())


def qerr(got, want, round_fp32=False):
    got = got.detach().cpu()
    if round_fp32:
        got = got.float()
    got, want = got.double(), torch.as_tensor(np.asarray(want)).double()
    return float(torch.minimum((got - want).abs().amax(-1), (got + want).abs().amax(-1)).max())


def fixture_errors(fused, device, dtype):
    """Worst error per quantity over both sides and every comparison the fixture holds; flags are asserted here."""
    Conv, Aug, Judge = classes(fused)
    worst = {k: 0.0 for k in MIRROR_FP32}

    def note(k, e):
        worst[k] = max(worst[k], e)
    r64 = dtype == torch.float64
    for side in SIDES:
        f = lambda name: FIX[side + '/' + name]       # noqa: E731
        c = make(Conv, side)
        note('quat', qerr(c.annotation_to_quat(T(f('aa'), device, dtype)), f('quat'), r64))
        note('aa', err(c.quat_to_annotation(T(f('quat'), device, dtype)), f('aa_back')))
        note('euler', err(c.quat_to_euler(T(f('quat'), device, dtype)), f('euler')))
        note('quat', qerr(c.euler_to_quat(T(f('euler'), device, dtype)), f('quat_from_euler'), r64))
        # template_0's composition goes through the reference's fp32-rounded quaternions; the one-launch form does not round,
        # so it is held against the same class's two steps
        aa = T(f('aa'), device, dtype)
        note('euler', err(c.annotation_to_euler(aa), c.quat_to_euler(c.annotation_to_quat(aa)).detach().cpu()))
        for preset in PRESETS:
            a = make(Aug, side, preset)
            u, e_in = T(f(preset + '/uniforms'), device, dtype), T(f('argue_in'), device, dtype)
            note('euler', err(a(e_in, 3, uniforms=u), f(preset + '/euler')))
            note('quat', qerr(a(e_in, 3, uniforms=u, out='quat'), f(preset + '/quat'), r64))
    j = make(Judge)
    j.reset()
    res, invalid = j(T(FIX['left/judge_quat'], device, dtype), T(FIX['right/judge_quat'], device, dtype))
    want = np.stack([FIX['left/residual'], FIX['right/residual']], 1)
    note('residual', err(res, want))
    flags = (want > pc.THRESHOLD).any(1)
    assert np.array_equal(invalid.cpu().numpy(), flags), (invalid, flags)
    assert abs(j.rate() - float(FIX['invalid_rate'])) < 1e-12 and 0 < j.rate() < 1
    return worst


def check_bars(worst, dtype, label):
    for k, e in worst.items():
        bar = FP64_BAR if dtype == torch.float64 else BARS[k]
        print('%s %s: worst %.3e, bar %.3e' % (label, k, e, bar))
    for k, e in worst.items():
        assert e <= (FP64_BAR if dtype == torch.float64 else BARS[k]), (label, k, e)


def run_fixture(fused, device, dtype=torch.float32):
    check_bars(fixture_errors(fused, device, dtype), dtype, '%s %s' % ('fused' if fused else 'mirror', dtype))


# ------------------------------------------------------------------------------------------------ seeded inputs, tail shapes
def seeded_euler(M, seed, splay=25.0):
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(M, 16, 3, generator=g, dtype=torch.float64)
    e = (u - 0.5) * torch.tensor([40.0, 2 * splay, 200.0], dtype=torch.float64)
    e[..., 2] += 30.0
    return e


def judge_frames(M, side):
    """M frames in fp64, cycling (violation on joint 15 only, valid, violation on joint 1 only); -> quat, residual, invalid."""
    c = make(pc.PoseConverter, side)
    j = make(pc.PoseValidJudge)
    zero = torch.eye(3, dtype=torch.float64).repeat(16, 1, 1)
    zero[1:] = j.zero[side][0].double()
    bend = torch.zeros(M, 16, dtype=torch.float64)
    for k, (lo, hi) in pc.BEND.items():
        bend[:, k + 1] = 0.5 * (lo + hi)
    want = torch.zeros(M, dtype=torch.float64)
    for m in range(M):
        if m % 3 == 0:
            bend[m, 15], want[m] = pc.BEND[14][1] + 10.0, np.radians(10.0)
        elif m % 3 == 2:
            bend[m, 1], want[m] = pc.BEND[0][0] - 7.0, np.radians(7.0)
    e = torch.zeros(M, 16, 3, dtype=torch.float64)
    e[..., 2] = bend
    quat = c._flip(c._e_to_q(zero @ pc.euler_to_mat(e)))
    res = j.residual(quat, side)                                               # the fp64 mirror; the crafted excess to 1e-5
    assert float((res - want).abs().max()) < 1e-5
    return quat, res, want > pc.THRESHOLD


def run_tail(fused, device, M, dtype=torch.float32):
    """Every kernel form at M samples against the fp64 mirror, both sides."""
    Conv, Aug, Judge = classes(fused)
    N, A = (5, 7) if M == 35 else (M, 1)
    worst = {k: 0.0 for k in MIRROR_FP32}
    quats = {}
    for si, side in enumerate(SIDES):
        ref, c = make(pc.PoseConverter, side), make(Conv, side)
        e = seeded_euler(M, 100 * M + si)
        q = ref.euler_to_quat(e)
        aa = ref.quat_to_annotation(q)
        d = lambda x: x.to(device=device, dtype=dtype)       # noqa: E731
        worst['quat'] = max(worst['quat'], qerr(c.euler_to_quat(d(e)), q), qerr(c.annotation_to_quat(d(aa)), q))
        worst['euler'] = max(worst['euler'], err(c.quat_to_euler(d(q)), e), err(c.annotation_to_euler(d(aa)), e))
        worst['aa'] = max(worst['aa'], err(c.quat_to_annotation(d(q)), aa), err(c.euler_to_annotation(d(e)), aa))
        for preset in PRESETS:
            a_ref, a = make(pc.PoseAugmenter, side, preset), make(Aug, side, preset)
            want_e, want_q = a_ref(e[:N], A, seed=M + si), a_ref(e[:N], A, seed=M + si, out='quat')
            assert tuple(want_e.shape) == (M, 16, 3)
            worst['euler'] = max(worst['euler'], err(a(d(e[:N]), A, seed=M + si), want_e))
            worst['quat'] = max(worst['quat'], qerr(a(d(e[:N]), A, seed=M + si, out='quat'), want_q))
        quats[side] = judge_frames(M, side)
    res, invalid = make(Judge)(quats['left'][0].to(device=device, dtype=dtype), quats['right'][0].to(device=device, dtype=dtype))
    assert tuple(res.shape) == (M, 2) and tuple(invalid.shape) == (M,)
    want = torch.stack([quats['left'][1], quats['right'][1]], 1)
    worst['residual'] = err(res, want)
    assert torch.equal(invalid.cpu(), quats['left'][2] | quats['right'][2])
    # one hand's violation must not leak into the other hand's column or into a neighbouring sample's group of 16 lanes
    lone = make(Judge)(quats['left'][0].to(device=device, dtype=dtype),
                       judge_frames(2, 'right')[0][1:2].expand(M, 16, 4).to(device=device, dtype=dtype))[0]
    assert float(lone[:, 1].abs().max()) <= (FP64_BAR if dtype == torch.float64 else BARS['residual'])
    check_bars(worst, dtype, 'tail M=%d' % M)


def rot(q):
    return quaternion_to_rotation_matrix(q.detach().double().cpu())


def run_round_trips(fused, device, dtype=torch.float32):
    Conv = classes(fused)[0]
    bar = 4 * (FP64_BAR if dtype == torch.float64 else BARS['quat'])
    for side in SIDES:
        c, ref = make(Conv, side), make(pc.PoseConverter, side)
        e = seeded_euler(8, 77)
        e[0, 0], e[1, 0], e[2, 0] = torch.tensor([[30.0, 90.0, -50.0], [-100.0, -90.0, 20.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
        e[3] = 0.0
        q = ref.euler_to_quat(e).to(device=device, dtype=dtype)                # the root AT gimbal lock, a frame at the identity
        back = c.quat_to_euler(q)
        assert torch.isfinite(back).all()
        assert float(back[0, 0, 2].abs()) == 0.0 and float(back[1, 0, 2].abs()) == 0.0      # c = 0 at lock
        e1 = float((rot(c.euler_to_quat(back)) - rot(q)).abs().max())
        aa = ref.quat_to_annotation(q.double().cpu())
        aa[4] = -ref._mean(aa)                                                  # every joint AT the identity
        aa[5, 0] = torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64) * np.pi   # the root AT angle pi
        aa = aa.to(device=device, dtype=dtype)
        q2 = c.annotation_to_quat(aa)
        aa2 = c.quat_to_annotation(q2)
        assert torch.isfinite(aa2).all()
        e2 = float((rot(c.annotation_to_quat(aa2)) - rot(q2)).abs().max())
        ident = q2[4].detach().double().cpu()
        assert float((ident[:, 0] - 1).abs().max()) <= bar and float(ident[:, 1:].abs().max()) <= bar
        print('round trip %s: quat-euler-quat %.3e, aa-quat-aa %.3e, bar %.3e' % (side, e1, e2, bar))
        assert e1 <= bar and e2 <= bar, (side, e1, e2)


def run_seeded(device, hash_np):
    """The seeded kernel: equal to the kernel fed with uniforms built from the tests' own hash mirror, bit for bit."""
    for side in SIDES:
        a = make(pc.FusedPoseAugmenter, side, 'script')
        e = seeded_euler(5, 9).to(device=device, dtype=torch.float32)
        M, seed = 35, 0x1234567890ABCDEF
        idx = np.arange(M * 32, dtype=np.uint64)
        u = ((hash_np(seed, idx) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(M, 16, 2)
        assert np.array_equal(u, pc.hash_uniforms(seed, M))
        for out in ('euler', 'quat'):
            seeded = a(e, 7, seed=seed, out=out)
            assert torch.equal(seeded, a(e, 7, uniforms=torch.from_numpy(u).to(device), out=out))
            assert not torch.equal(seeded, a(e, 7, seed=seed + 1, out=out))
            parts = torch.cat([a(e[:2], 7, seed=seed, out=out), a(e[2:], 7, seed=seed, out=out, row_offset=14)])
            assert torch.equal(seeded, parts)
        assert torch.equal(a(e, 7, seed=seed)[:, 0], a(e, 7, seed=seed + 1)[:, 0])          # the root never moves


def run_in_range(fused, device, dtype=torch.float32):
    """Wherever the input was inside its range the adjusted angle stays inside it (a = 0 and, for the bend, b = 0, so that the
    Euler angle the adjustment turns about is the one read back; the splay alone with max_bend = 0)."""
    Aug = classes(fused)[1]
    slack = FP64_BAR if dtype == torch.float64 else BARS['euler']
    for side in SIDES:
        for preset, ranges in (('script', pc.SCRIPT_RANGES), ('ver2', pc.VER2_RANGES)):
            g = torch.Generator().manual_seed(5)
            e = torch.zeros(6, 16, 3, dtype=torch.float64)
            for j, (lo, hi) in ranges['bend'].items():
                e[:, j, 2] = lo + (hi - lo) * torch.rand(6, generator=g, dtype=torch.float64)
            out = make(Aug, side, preset)(e.to(device=device, dtype=dtype), 4, seed=3).double().cpu()
            moved = False
            for j, (lo, hi) in ranges['bend'].items():
                if j not in ranges['splay']:
                    assert float(out[:, j, 2].min()) >= lo - slack and float(out[:, j, 2].max()) <= hi + slack, (side, preset, j)
                    moved = moved or float((out[:, j, 2] - e[:, j, 2].repeat_interleave(4)).abs().max()) > 1.0
            assert moved
            splay_only = Aug(side, mano(side), ranges, 0, 30, tables=tables(side))
            e = torch.zeros(6, 16, 3, dtype=torch.float64)
            e[..., 2] = 20.0
            for j, (lo, hi) in ranges['splay'].items():
                e[:, j, 1] = lo + (hi - lo) * torch.rand(6, generator=g, dtype=torch.float64)
            out = splay_only(e.to(device=device, dtype=dtype), 4, seed=4).double().cpu()
            for j, (lo, hi) in ranges['splay'].items():
                assert float(out[:, j, 1].min()) >= lo - slack and float(out[:, j, 1].max()) <= hi + slack, (side, preset, j)
            assert float((out[..., 2] - 20.0).abs().max()) <= slack


def run_untouched(fused, device):
    Conv, Aug, Judge = classes(fused)
    c = make(Conv, 'left')
    q = T(FIX['left/quat'], device, torch.float32)
    aa, e = T(FIX['left/aa'], device, torch.float32), T(FIX['left/euler'], device, torch.float32)
    keep = [x.clone() for x in (q, aa, e)]
    c.quat_to_euler(q), c.quat_to_annotation(q), c.annotation_to_quat(aa), c.euler_to_quat(e)
    make(Aug, 'left', 'script')(e, 2, seed=1)
    make(Judge)(q, q)
    for x, k in zip((q, aa, e), keep):
        assert torch.equal(x, k)


def run_bad_input(fused, device):
    import pytest
    Conv, Aug, Judge = classes(fused)
    with pytest.raises(ValueError):
        Conv('middle', mano('right'))
    c, a, j = make(Conv, 'right'), make(Aug, 'right', 'script'), make(Judge)
    z = lambda *s: torch.zeros(*s, device=device)       # noqa: E731
    for call in (lambda: c.quat_to_euler(z(2, 16, 3)), lambda: c.euler_to_quat(z(2, 16, 4)), lambda: c.annotation_to_quat(z(2, 15, 3)),
                 lambda: c.quat_to_annotation(z(16, 4)), lambda: c.quat_to_euler(z(0, 16, 4)),
                 lambda: c.trans_to_loc(z(2, 9), z(2, 3)), lambda: c.loc_to_trans(z(2, 10), z(3, 3)),
                 lambda: a(z(2, 16, 3), 0, seed=1), lambda: a(z(2, 16, 3), 2), lambda: a(z(2, 16, 3), 2, seed=1, uniforms=z(4, 16, 2)),
                 lambda: a(z(2, 16, 3), 2, uniforms=z(2, 16, 2)), lambda: a(z(2, 16, 3), 2, seed=1, out='aa'),
                 lambda: a(z(2, 16, 4), 2, seed=1), lambda: j(z(2, 16, 4), z(3, 16, 4)), lambda: j(z(2, 16, 3), z(2, 16, 3)),
                 lambda: Aug('right', mano('right'), {'bend': {0: (0, 1)}, 'splay': {}}),
                 lambda: Aug('right', mano('right'), {'bend': {}})):
        with pytest.raises(ValueError):
            call()
    if fused:
        with pytest.raises(ValueError):
            c.quat_to_euler(z(2, 16, 4).double())                               # fp32 only


def run_einval(lib, ptr, stream=0):
    args = dict(inp=ptr, second=0, out=ptr, tab=ptr, u=0, seed=0, row0=0, M=1, A=1, fi=2, mid=0, fo=0)
    for bad in (dict(inp=0), dict(out=0), dict(tab=0), dict(M=0), dict(M=(1 << 27) + 1), dict(A=0), dict(A=2), dict(row0=-1),
                dict(fi=3), dict(fi=-1), dict(mid=3), dict(fo=4), dict(mid=2, fi=1), dict(second=ptr)):
        a = dict(args, **bad)
        assert lib.rih_pose_convert(a['inp'], a['second'], a['out'], a['tab'], a['u'], a['seed'], a['row0'], a['M'], a['A'],
                                    a['fi'], a['mid'], a['fo'], stream) == -1, bad


def run_loc_trans(device, dtype=torch.float64):
    g = torch.Generator().manual_seed(3)
    for side in SIDES:
        c = make(pc.PoseConverter, side)
        shape = torch.randn(4, 10, generator=g, dtype=torch.float64).to(device=device, dtype=dtype)
        trans = (torch.randn(4, 3, generator=g, dtype=torch.float64) * 0.3).to(device=device, dtype=dtype)
        q = c.euler_to_quat(seeded_euler(4, 5).to(device=device, dtype=dtype))
        layer = QuatManoLayer(mano(side), side=side, center_idx=None).to(device=device, dtype=dtype)
        joints = layer(q, shape, trans)[1]
        loc = c.trans_to_loc(shape, trans)
        # the layer regresses its joints in its own order of sums: 1e-12 of fp64 rounding on values of order 1
        bar = 1e-12 if dtype == torch.float64 else 1e-5
        assert err(loc, joints[:, 0].detach().cpu()) <= bar
        assert err(c.loc_to_trans(shape, loc), trans.cpu()) <= bar


def run_glue(fused, device, dtype=torch.float32):
    Conv, Aug, _ = classes(fused)
    conv = {s: make(Conv, s) for s in SIDES}
    rs = np.random.RandomState(11)
    frames = []
    for n in range(2):
        p = {}
        for side in SIDES:
            aa = FIX[side + '/aa'][n].reshape(48).astype(np.float64)
            p[side] = {'oripose': aa, 'trans': rs.randn(1, 3) * 0.2, 'shape': rs.randn(1, 10)}
        frames.append({'mano_params': p})
    k = dict(dtype=dtype, device=device)
    mocap = pc.annotations_to_mocap(frames, conv, **k)
    assert mocap['right']['rot'].shape == (2, 16, 3) and mocap['left']['shape'].shape == (2, 1, 10)
    assert np.array_equal(mocap['capture_frame_id'], [0, 1])
    seq = pc.mocap_to_optimizer(mocap, 1.0, conv, **k)
    assert tuple(seq['right_quat'].shape) == (2, 16, 4) and tuple(seq['hand_shape'].shape) == (2, 20)
    result = {s: {'rot': seq[s + '_quat'], 'loc': seq[s + '_loc']} for s in SIDES}
    back = pc.mocap_to_annotations(pc.optimizer_to_mocap(result, mocap, conv, **k), conv, **k)
    fp64 = dtype == torch.float64
    for n in range(2):
        assert back[n]['capture_frame_id'] == n
        for side in SIDES:
            got, want = back[n]['mano_params'][side], frames[n]['mano_params'][side]
            # pose through two Euler passages: the aa bar twice over; trans through loc in cm and back
            assert np.abs(got['pose'].reshape(48) - want['oripose']).max() <= (1e-7 if fp64 else 4 * BARS['aa'])
            assert got['trans'].shape == (1, 3) and np.abs(got['trans'] - want['trans']).max() <= (1e-9 if fp64 else 1e-5)
            assert np.array_equal(got['shape'], want['shape'].astype(np.float32))
    aug = {s: make(Aug, s, 'script') for s in SIDES}
    more = pc.augment_mocap(mocap, 3, 7, aug, **k)
    assert more['right']['rot'].shape == (6, 16, 3) and more['left']['loc'].shape == (6, 3)
    assert np.array_equal(more['capture_frame_id'], [0, 0, 0, 1, 1, 1]) and mocap['right']['rot'].shape == (2, 16, 3)
    assert np.array_equal(more['right']['loc'][:3], np.repeat(mocap['right']['loc'][:1], 3, 0))
