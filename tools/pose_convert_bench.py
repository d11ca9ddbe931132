#!/usr/bin/env python
"""The pose-data stages of renderih_amd.pose_convert, per call on M samples of 16 joints: (a) `fused` -- one launch of
rih_pose_convert; (b) `mirror` -- the plain-torch classes on the device; (c) `host` -- a numpy / scipy restatement, written
here, of the reference's per-frame loop (HandPoseArguer.argue_pose with its ~20 `angle_random_adjust` calls per frame and
scipy `Rotation` objects in fp64; `mano_quat_2_euler`; `ValidationJudge` is torch in the reference, so its host column is the
mirror on the CPU), run on min(M, --host-frames) frames (default 4096 = 2^12) and reported per frame.
Three ops: `augment_quat` (Euler in, A = --argue-size variants out as quaternions; M counts OUTPUT rows), `quat_to_euler`, `judge`
(both hands).  Inputs: the synthetic MANO model, seeded angles inside +-60 degrees of splay.

  us        microseconds per call at M in --sizes (default 2^10 2^15 2^20): HIP events around --reps calls; the variants
            alternate, --rounds windows each after a warm-up; medians and every variant's own max - min.
  launches  kernels per call, counted by torch's profiler over one call.
  bytes     the model: in + out bytes of the fused call (augment_quat: 12 / A in, 16 out per joint; quat_to_euler: 16 + 12;
            judge: 2 x 16 in per joint, 8 out per sample) and the GB/s the fused median achieves on it.

Prints one JSON line and writes it to <profile-dir>/pose_convert_bench.json (the same line and the windows to .log).
    python tools/pose_convert_bench.py [--profile-dir profiles/pose_convert]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
OPS = ('augment_quat', 'quat_to_euler', 'judge')


def device_window(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def host_argue(euler, A, ranges, caps, rs):
    """argue_pose(pose_type='euler') as the reference runs it: per frame and joint group a draw, then scipy Rotations."""
    from scipy.spatial.transform import Rotation
    N = euler.shape[0]
    adjust = np.zeros((2, N * A, 16))
    for which, (name, col) in enumerate((('bend', 2), ('splay', 1))):
        for i in range(N):
            for j, (lo, hi) in ranges[name].items():
                angle = euler[i, j, col]
                pos = max(min(caps[which], hi - angle), 0)
                neg = min(max(-caps[which], lo - angle), 0)
                adjust[which, i * A:(i + 1) * A, j] = (pos - neg) * rs.rand(A) + neg
    out = np.repeat(euler, A, axis=0)
    for which, col in ((0, 2), (1, 1)):
        turn = np.zeros((N * A * 16, 3))
        turn[:, col] = adjust[which].reshape(-1)
        rot = Rotation.from_euler('xyz', out.reshape(-1, 3), True).as_matrix() @ Rotation.from_euler('xyz', turn, True).as_matrix()
        out = Rotation.from_matrix(rot).as_euler('xyz', degrees=True).reshape(-1, 16, 3)
    return out


def host_quat_to_euler(quat, tables):
    from scipy.spatial.transform import Rotation
    t0, t1 = (t.numpy().astype(np.float64) for t in tables)
    mat = Rotation.from_quat(quat.reshape(-1, 4)[:, [1, 2, 3, 0]]).as_matrix().reshape(-1, 16, 3, 3)
    mat = t0.swapaxes(1, 2) @ mat @ t1.swapaxes(1, 2)
    out = np.zeros(quat.shape[:2] + (3,))
    for j in range(16):
        out[:, j] = Rotation.from_matrix(mat[:, j]).as_euler('xyz', True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'pose_convert'))
    ap.add_argument('--sizes', type=int, nargs='+', default=[1 << 10, 1 << 15, 1 << 20])
    ap.add_argument('--argue-size', type=int, default=8)
    ap.add_argument('--host-frames', type=int, default=1 << 12)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    args = ap.parse_args()
    os.makedirs(args.profile_dir, exist_ok=True)
    from renderih_amd import assets, pose_convert as pc
    dev = torch.device('cuda:0')
    mano = {s: assets.synthetic_mano_dict(s, seed=0) for s in ('left', 'right')}
    A = args.argue_size
    aug = {'fused': pc.FusedPoseAugmenter('right', mano['right']), 'mirror': pc.PoseAugmenter('right', mano['right'])}
    conv = {'fused': pc.FusedPoseConverter('right', mano['right']), 'mirror': pc.PoseConverter('right', mano['right'])}
    judge = {'fused': pc.FusedPoseValidJudge(mano['left'], mano['right']), 'mirror': pc.PoseValidJudge(mano['left'], mano['right'])}
    lines, result = [], {'argue_size': A, 'host_frames': args.host_frames, 'sizes': {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)
    for M in args.sizes:
        g = torch.Generator().manual_seed(M)
        euler = ((torch.rand(M, 16, 3, generator=g) - 0.5) * torch.tensor([40.0, 120.0, 200.0])).to(dev)
        quat = conv['fused'].euler_to_quat(euler)
        N = max(M // A, 1)
        calls = {'augment_quat': {k: (lambda k=k: aug[k](euler[:N], A, seed=1, out='quat')) for k in aug},
                 'quat_to_euler': {k: (lambda k=k: conv[k].quat_to_euler(quat)) for k in conv},
                 'judge': {k: (lambda k=k: judge[k](quat, quat)) for k in judge}}
        rows = N * A
        model = {'augment_quat': rows * 16 * 16 + N * 16 * 12, 'quat_to_euler': M * 16 * 28, 'judge': M * (2 * 16 * 16 + 8)}
        per = {}
        for op in OPS:
            windows = {k: [] for k in calls[op]}
            for fn in calls[op].values():
                fn()
            for _ in range(args.rounds):
                for k, fn in calls[op].items():
                    windows[k].append(device_window(fn, args.reps if k == 'fused' or M < (1 << 20) else 3))
            med = {k: float(np.median(v)) for k, v in windows.items()}
            per[op] = {'us': med, 'spread': {k: float(max(v) - min(v)) for k, v in windows.items()},
                       'launches': {k: launches(fn) for k, fn in calls[op].items()}, 'bytes': model[op],
                       'fused_GBps': model[op] / med['fused'] / 1e3, 'mirror_over_fused': med['mirror'] / med['fused']}
            say('M=%d %s: fused %.1f us (spread %.1f, %d launches, %.1f GB/s on %d bytes), mirror %.1f us (spread %.1f, %d launches), '
                'ratio %.1f' % (M, op, med['fused'], per[op]['spread']['fused'], per[op]['launches']['fused'], per[op]['fused_GBps'],
                                model[op], med['mirror'], per[op]['spread']['mirror'], per[op]['launches']['mirror'],
                                per[op]['mirror_over_fused']))
        result['sizes'][str(M)] = per
    # the reference's per-frame loop on the host, restated above: microseconds per frame (input frame for the augmenter)
    H = min(max(args.sizes), args.host_frames)
    rs = np.random.RandomState(0)
    e_host = ((rs.rand(H, 16, 3) - 0.5) * np.array([40.0, 120.0, 200.0]))
    q_host = conv['mirror'].euler_to_quat(torch.from_numpy(e_host)).numpy()
    t0 = time.perf_counter()
    host_argue(e_host, A, pc.SCRIPT_RANGES, (120.0, 30.0), rs)
    t1 = time.perf_counter()
    host_quat_to_euler(q_host, conv['mirror'].tables)
    t2 = time.perf_counter()
    judge['mirror'](torch.from_numpy(q_host), torch.from_numpy(q_host))
    t3 = time.perf_counter()
    result['host_us_per_frame'] = {'augment (A variants, Euler out)': (t1 - t0) * 1e6 / H, 'quat_to_euler': (t2 - t1) * 1e6 / H,
                                   'judge (torch on the CPU)': (t3 - t2) * 1e6 / H}
    say('host loop on %d frames, us per frame: %s' % (H, json.dumps(result['host_us_per_frame'])))
    line = json.dumps(result)
    print(line)
    with open(os.path.join(args.profile_dir, 'pose_convert_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'pose_convert_bench.log'), 'w') as fh:
        fh.write('\n'.join(lines + [line]) + '\n')


if __name__ == '__main__':
    main()
