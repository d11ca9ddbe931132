#!/usr/bin/env python
"""Golden vectors of the pose-data converter, augmenter and validity judge from the REFERENCE's own program:
pose_data_optimize/scripts/HandPoseConverter.py (`HandPoseConverter`, data_type='np', both sides), scripts/HandPoseArguer.py
(`HandPoseArguer.argue_pose`), Ver2Code/NatureJudge/PoseArgue.py (`PoseArguer.argue_pose`) and Ver2Code/ValidJudge/
ValidJudger.py (`ValidationJudge`, `ComputeValidation`), imported from a reference checkout at generation time and run
unmodified on the CPU.

Imports: `reference_modules` of make_quat_mano_golden.py (synthetic MANO through the stubbed chumpy loader, the checkout's
manopth first on sys.path), then pose_data_optimize/, its scripts/, Ver2Code/NatureJudge and Ver2Code/ValidJudge on the path
(the Ver2 files import `HandPoseConverter` as a top-level module), and EMPTY stand-in modules for open3d, trimesh, pycocotools
(with a `coco.COCO` name) and tqdm: all imported at module top there, none used by these functions, none installed here.

What is arranged around the reference's code, none of it an edit of it:
  * `np.random.rand` is wrapped for the duration of an `argue_pose` call: every call is recorded, and the draws are rounded to
    fp32-representable values, so that the fp64 mirror, the fp32 mirror and the kernel consume identical uniforms.  The recorded
    calls are laid out as the kernel's [M,16,2] (which 0 = bend, 1 = splay) by replaying the call order of `bend_argue` and
    `splank_argue`.
  * `ValidJudger.__init__` builds its converters on the default device string 'cuda:0'; the judge is therefore put together
    by hand -- `ValidJudger.__new__`, device='cpu', the two `HandPoseConverter(data_type='tensor', device='cpu')` and the two
    zero frames exactly as `__init__` computes them -- with the converters' tables cast to fp64 (the same fp32 values), so that
    `ValidationJudge` and `ComputeValidation` run in fp64 on fp64 copies of the fp32 quaternions (torch's default dtype is
    fp64 for the duration of those two calls: the judge builds its unit vectors with torch.tensor([1.0, ...])).
  * `axis_angle_2_mano_quat` adds hands_mean to the annotation in fp32.  The converter's `th_hands_mean` (data it read from the
    synthetic model) is rounded to multiples of 2^-12 and stored here as 'hands_mean', and the annotations lie on the same
    grid, so that fp32 sum is exact and an fp64 restatement sees the same rotation vector; a test gives its converter the
    stored hands_mean.  The quaternions it and `euler_2_mano_quat` return are rounded to fp32 by the reference itself; they are
    stored as they come.

Writes tests/golden/pose_convert.npz, N = 6 frames, A = 3 variants.  Per side: aa -> quat (`axis_angle_2_mano_quat`), quat ->
aa_back (`mano_quat_flat_2_normal(return_type='aa')`), quat -> euler (`mano_quat_2_euler`), euler -> quat_from_euler
(`euler_2_mano_quat`); the augmenters' input argue_in, per preset ('script': HandPoseArguer, 'ver2': PoseArguer with
random_level=1) the uniforms, the output Euler angles and `euler_2_mano_quat` of them; the judge's quaternions judge_quat and
residual.  'invalid_rate' is `ComputeValidation(left, right)`.

Asserted here (another seed is tried until they hold; nothing is excused at test time): every Euler output has |R20| < 0.98;
every rotation-vector angle lies in [0.05, 3.0]; no bend or splay angle of the judge within 0.05 degrees of a range limit or of
a limit +- the 0.1 degree threshold; no augmenter input within 0.05 degrees of a limit; on each side and for each preset an input
angle already outside its range on either side (pos resp. neg clamps to 0) and a cap that binds, for bend and for splay; at
least one invalid and one valid frame per hand; two runs write identical arrays.
       python tests/golden/make_pose_convert_golden.py <reference checkout>"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_quat_mano_golden import reference_modules  # noqa: E402

N, A = 6, 3
ROOT = 'mano/models'
# the judge's ranges (ValidJudger.py:80-98), joints numbered 0..14
SPLAY = {0: (-25, 15), 3: (-15, 15), 9: (-25, 15), 6: (-20, 30), 12: (-30, 30)}
BEND = {0: (-25, 70), 1: (-4, 110), 3: (-25, 80), 4: (-7, 100), 9: (-25, 70), 10: (-10, 100), 6: (-22, 70), 7: (-8, 90),
        12: (-20, 40), 13: (-35, 50), 14: (-10, 100), 2: (-8, 90), 5: (-8, 90), 11: (-8, 90), 8: (-8, 90)}
# the augmenters' call order and ranges (HandPoseArguer.py:117-146, PoseArgue.py:118-147), joints numbered 0..15
BEND_ORDER = [2, 5, 11, 8, 13, 14, 3, 6, 12, 9, 15, 1, 4, 10, 7]
SPLAY_ORDER = [1, 4, 10, 7, 13]


def argue_ranges(preset):
    normal = (-8, 90) if preset == 'script' else (-8, 95)
    bend = {j: (-8, 110) for j in (2, 5, 11, 8)}
    bend.update({13: (-20, 40), 14: (-8, 50)})
    bend.update({j: normal for j in (3, 6, 12, 9, 15)})
    bend.update({j: (-25, 70) for j in (1, 4, 10, 7)})
    if preset == 'script':
        return bend, {1: (-6, 20), 4: (-10, 10), 10: (-15, 6), 7: (-35, 6), 13: (-9, 80)}, 120.0, 30.0
    return bend, {1: (-25, 15), 4: (-15, 15), 10: (-25, 15), 7: (-20, 30), 13: (-30, 30)}, 120.0, 45.0


def load(ref):
    reference_modules(ref)
    base = os.path.join(ref, 'pose_data_optimize')
    for p in (base, os.path.join(base, 'scripts'), os.path.join(base, 'Ver2Code', 'NatureJudge'),
              os.path.join(base, 'Ver2Code', 'ValidJudge')):
        sys.path.insert(1, p)
    for name in ('open3d', 'trimesh', 'pycocotools', 'pycocotools.coco', 'tqdm'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['pycocotools.coco'].COCO = object
    from scripts.HandPoseArguer import HandPoseArguer
    from scripts.HandPoseConverter import HandPoseConverter
    from PoseArgue import PoseArguer
    from ValidJudger import ValidJudger
    return HandPoseConverter, HandPoseArguer, PoseArguer, ValidJudger


class RecordedRand:
    """np.random.rand for the duration of a `with`: fp32-representable draws from a seeded stream, every call kept."""

    def __init__(self, seed):
        self.rs, self.calls = np.random.RandomState(seed), []

    def __call__(self, *shape):
        u = self.rs.rand(*shape).astype(np.float32).astype(np.float64)
        u = np.minimum(u, np.float64(np.float32(1.0) - np.float32(2.0 ** -24)))          # rounding may not reach 1
        self.calls.append(u)
        return u

    def __enter__(self):
        self.saved, np.random.rand = np.random.rand, self
        return self

    def __exit__(self, *exc):
        np.random.rand = self.saved

    def layout(self):
        """The calls in the kernel's [M,16,2] layout: bend_argue runs frame by frame over BEND_ORDER, then splank_argue over
        SPLAY_ORDER; a call holds the A draws of one (frame, joint)."""
        assert len(self.calls) == N * (len(BEND_ORDER) + len(SPLAY_ORDER)) and all(c.shape == (A,) for c in self.calls)
        u, calls = np.zeros((N * A, 16, 2)), iter(self.calls)
        for which, order in ((0, BEND_ORDER), (1, SPLAY_ORDER)):
            for n in range(N):
                for j in order:
                    u[n * A:(n + 1) * A, j, which] = next(calls)
        return u


def exact_annotation(rs, mean):
    """[N,16,3] fp32 whose fp32 sum with hands_mean (finger joints) is exact; rotation angles of the sum in [0.05, 3.0]."""
    full = np.concatenate([np.zeros((1, 3), np.float32), mean.reshape(15, 3)])
    aa = np.zeros((N, 16, 3), np.float32)
    for n in range(N):
        for j in range(16):
            while True:
                axis = rs.randn(3)
                target = axis / np.linalg.norm(axis) * rs.uniform(0.1, 2.9 if j else 3.0)
                v = (np.round((target - full[j]) * 4096) / 4096).astype(np.float32)
                assert (np.float64(v + full[j]) == np.float64(v) + np.float64(full[j])).all()
                if 0.05 <= np.linalg.norm(v.astype(np.float64) + full[j]) <= 3.0:
                    break
            aa[n, j] = v
    return aa


def sin_b(euler):
    return np.abs(np.sin(np.radians(euler[..., 1])))


def rotvec_angles(q):
    q = q.astype(np.float64)
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    return 2 * np.arctan2(np.linalg.norm(q[..., 1:], axis=-1), np.abs(q[..., 0]))


def argue_input(rs):
    e = np.zeros((N, 16, 3))
    e[..., 0] = rs.uniform(-20, 20, size=(N, 16))
    e[..., 1] = rs.uniform(-50, 50, size=(N, 16))
    e[..., 2] = rs.uniform(-70, 140, size=(N, 16))
    e[:, 0] = np.stack([rs.uniform(-170, 170, N), rs.uniform(-60, 60, N), rs.uniform(-170, 170, N)], -1)
    return e


def argue_conditions(e, preset):
    bend, splay, cap_b, cap_s = argue_ranges(preset)
    ok = True
    for table, angle, cap in ((bend, e[..., 2], cap_b), (splay, e[..., 1], cap_s)):
        above = below = binds = False
        for j, (lo, hi) in table.items():
            a = angle[:, j]
            ok = ok and (np.abs(a - lo) > 0.05).all() and (np.abs(a - hi) > 0.05).all()
            above, below = above or (a > hi).any(), below or (a < lo).any()
            binds = binds or (hi - a > cap).any() or (lo - a < -cap).any()
        ok = ok and above and below and binds
    return bool(ok)


def judge_quats(rs, hpc, zero):
    """[N,16,4] fp32: frames 0..2 drawn inside the ranges, frames 3..5 with a wider spread; through the converter's own
    `rotation_2_euler` and `euler_2_mano_quat`, so that joint j's frame is zero[j] @ rel[j]."""
    euler = np.zeros((N, 16, 3))
    euler[:, 0] = np.stack([rs.uniform(-170, 170, N), rs.uniform(-60, 60, N), rs.uniform(-170, 170, N)], -1)
    for n in range(N):
        wide = n >= 3
        for j in range(15):
            lo, hi = BEND[j]
            slo, shi = SPLAY.get(j, (-8, 8))
            if wide and rs.rand() < 0.25:
                b = rs.choice([lo - rs.uniform(0.5, 30), hi + rs.uniform(0.5, 30)])
            else:
                b = rs.uniform(lo + 1, hi - 1)
            if wide and j in SPLAY and rs.rand() < 0.25:
                s = rs.choice([slo - rs.uniform(0.5, 20), shi + rs.uniform(0.5, 20)])
            else:
                s = rs.uniform(slo + 1, shi - 1) * (0.5 if j in SPLAY else 1.0)
            rel = hpc.euler_2_rotation(np.array([rs.uniform(-5, 5), s, b]))
            euler[n, j + 1] = hpc.rotation_2_euler(zero[j + 1] @ rel)
    return hpc.euler_2_mano_quat(euler), euler


def judge_conditions(rel):
    x = rel[..., 0]
    bend = np.degrees(np.arctan2(x[..., 1], x[..., 0]))
    splay = np.degrees(np.arctan2(-x[..., 2], x[..., 0]))
    ok = True
    for table, angle in ((SPLAY, splay), (BEND, bend)):
        for j, limits in table.items():
            for lim in limits:
                for edge in (lim - 0.1, lim, lim + 0.1):
                    ok = ok and (np.abs(angle[:, j] - edge) > 0.05).all()
    return bool(ok)


def in_fp64(fn, *args):
    """`fn(*args)` with torch's default dtype at fp64: `ValidationJudge` builds its unit vectors with torch.tensor([1.0, ...])."""
    saved = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return fn(*args)
    finally:
        torch.set_default_dtype(saved)


def generate(ref):
    HandPoseConverter, HandPoseArguer, PoseArguer, ValidJudger = load(ref)
    out = {}
    ident = torch.zeros(1, 16, 4)
    ident[..., 0] = 1.0
    judge = ValidJudger.__new__(ValidJudger)
    judge.device = 'cpu'
    for si, side in enumerate(('right', 'left')):
        k = side + '/'
        hpc = HandPoseConverter(side=side, root=ROOT)
        hpc.th_hands_mean = (np.round(hpc.th_hands_mean * 4096) / 4096).astype(np.float32)
        hpc_t = HandPoseConverter(side=side, root=ROOT, data_type='tensor', device='cpu')
        hpc_t.invM_U_n_0, hpc_t.invU_M_n_1 = hpc_t.invM_U_n_0.double(), hpc_t.invU_M_n_1.double()
        zero_t = hpc_t.mano_quat_2_mat_tensor(ident.double())
        if side == 'right':
            judge.rhpc, judge.zero_mat_ = hpc_t, zero_t
        else:
            judge.lhpc, judge.sub_zero_mat_ = hpc_t, zero_t
        arguers = {'script': HandPoseArguer(side=side, root=ROOT), 'ver2': PoseArguer(side=side, root=ROOT)}
        for seed in range(7300 + 1000 * si, 7300 + 1000 * si + 500):
            rs = np.random.RandomState(seed)
            aa = exact_annotation(rs, hpc.th_hands_mean)
            quat = hpc.axis_angle_2_mano_quat(aa.copy(), flat_hand=False)
            aa_back = hpc.mano_quat_flat_2_normal(quat.copy(), return_type='aa')
            euler = hpc.mano_quat_2_euler(quat.copy())
            quat_from_euler = hpc.euler_2_mano_quat(euler.copy())
            if sin_b(euler).max() >= 0.98:
                continue
            angles = np.concatenate([rotvec_angles(quat).ravel(), rotvec_angles(quat_from_euler).ravel()])
            if angles.min() < 0.05 or angles.max() > 3.0:
                continue
            argue_in = argue_input(rs)
            if not (argue_conditions(argue_in, 'script') and argue_conditions(argue_in, 'ver2')):
                continue
            argued, good = {}, True
            for pi, (preset, arguer) in enumerate(arguers.items()):
                with RecordedRand(seed * 10 + pi) as rand:
                    e = arguer.argue_pose(argue_in.copy(), argue_size=A, pose_type='euler')
                good = good and sin_b(e).max() < 0.98
                argued[preset] = (rand.layout(), e, hpc.euler_2_mano_quat(e.copy()))
            if not good:
                continue
            jq, _ = judge_quats(rs, hpc, zero_t[0].numpy())
            ja = hpc_t.mano_quat_2_mat_tensor(torch.from_numpy(jq).double())
            rel = (zero_t[:, 1:].transpose(3, 2) @ ja[:, 1:]).numpy()
            res = in_fp64(judge.ValidationJudge, ja[:, 1:], zero_t[:, 1:], side[0]).numpy()
            bad = res > 0.1 / 180 * np.pi
            if judge_conditions(rel) and bad.any() and not bad.all():
                break
        else:
            raise AssertionError('no seed meets the conditions for the %s hand' % side)
        out[k + 'seed'] = np.int32(seed)
        out[k + 'inv_m_u_0'], out[k + 'inv_u_m_1'], out[k + 'hands_mean'] = hpc.invM_U_n_0, hpc.invU_M_n_1, hpc.th_hands_mean[0]
        out[k + 'aa'], out[k + 'quat'], out[k + 'aa_back'] = aa, quat, aa_back
        out[k + 'euler'], out[k + 'quat_from_euler'] = euler, quat_from_euler
        out[k + 'argue_in'] = argue_in
        for preset, (u, e, q) in argued.items():
            out[k + preset + '/uniforms'], out[k + preset + '/euler'], out[k + preset + '/quat'] = u, e, q
        out[k + 'judge_quat'], out[k + 'residual'] = jq, res
    rate = in_fp64(judge.ComputeValidation, torch.from_numpy(out['left/judge_quat']).double(),
                   torch.from_numpy(out['right/judge_quat']).double())
    out['invalid_rate'] = np.float64(rate)
    return out


def main(ref):
    out = generate(ref)
    again = generate(ref)
    assert set(out) == set(again) and all(np.array_equal(out[k], again[k]) for k in out), 'two runs differ'
    path = os.path.join(HERE, 'pose_convert.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes; seeds', int(out['right/seed']), int(out['left/seed']))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
