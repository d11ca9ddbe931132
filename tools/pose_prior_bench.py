#!/usr/bin/env python
"""Hand-prior and contact terms of the pose optimiser's two-hand objective, forward + backward: (a) the fused HIP path
(renderih_amd.pose_prior.FusedTwoHandPriorLoss), (b) the torch mirror (TwoHandPriorLoss), on one build in one process.
Prints one JSON line and writes it to <profile-dir>/pose_prior_bench.json (the same line and the windows to .log).

  us        microseconds per evaluation at B in --batches (default 1 32): forward of the seven-term sum, then backward to
            both hands' quaternions, vertices and anchors (778 vertices, 32 anchors, D = 4).  HIP events on the current stream
            after a warm-up; the two variants alternate, --rounds windows of --iters evaluations each; medians, and every
            variant's own max - min over its windows.  The claim "fused is faster" holds where the mirror's median exceeds
            the fused one by more than the mirror's own spread.
  launches  kernel launches per evaluation at the largest batch: each variant runs under `rocprofv3 --kernel-trace --stats`
            (tracing only, the program after `--`) in fresh child processes with 2 and with 12 evaluations; the difference of
            the call counts / 10.  The stats tables of the 12-evaluation runs are kept in the profile directory.

    python tools/pose_prior_bench.py [--profile-dir profiles/pose_prior] [--no-launch-count]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
KINDS = ('fused', 'mirror')
NAMES = ('q_r', 'q_l', 'verts_r', 'verts_l', 'anchors_r', 'anchors_l')
A, D = 32, 4


def variants(dev):
    from renderih_amd import assets
    from renderih_amd.pose_prior import FusedTwoHandPriorLoss, TwoHandPriorLoss
    r, l = assets.synthetic_mano_dict('right', seed=0), assets.synthetic_mano_dict('left', seed=0)
    return {'fused': FusedTwoHandPriorLoss(r, l).to(dev), 'mirror': TwoHandPriorLoss(r, l).to(dev)}


def inputs(B, mods, dev, seed=0):
    """Rotations by up to ~80 degrees with |q| in [0.7, 1.4], vertices near the rest meshes, random contact tables."""
    rs = np.random.RandomState(seed)
    axis = rs.randn(2, B, 16, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * rs.uniform(0.0, 1.4, size=(2, B, 16, 1))
    q = np.concatenate([np.cos(half), np.sin(half) * axis], -1) * rs.uniform(0.7, 1.4, size=(2, B, 16, 1))
    from renderih_amd import assets
    from renderih_amd.quat_mano import QuatManoLayer
    ident = torch.zeros(1, 16, 4)
    ident[..., 0] = 1.0
    with torch.no_grad():
        rest = [QuatManoLayer(assets.synthetic_mano_dict(s, seed=0), side=s, center_idx=0)(ident, torch.zeros(1, 10))[0][0].numpy()
                for s in ('right', 'left')]
    arrays = [q[0], q[1], rest[0] + 3e-4 * rs.randn(B, 778, 3), rest[1] + 3e-4 * rs.randn(B, 778, 3),
              0.02 * rs.randn(B, A, 3), 0.02 * rs.randn(B, A, 3)]
    contacts = (rs.randint(0, A, size=(B, A, D)), (rs.rand(B, A, D) < 0.6).astype(np.int64), rs.rand(B, A, D).astype(np.float32))
    for m in mods.values():
        m.set_contacts(*contacts)
    return [torch.from_numpy(np.asarray(a, np.float32)).to(dev).requires_grad_(True) for a in arrays]


def step(mod, x):
    for t in x:
        t.grad = None
    mod(*x)[0].backward()


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def timed(mods, x, iters, rounds):
    for m in mods.values():
        for _ in range(3):
            step(m, x)
    torch.cuda.synchronize()
    win = {k: [] for k in mods}
    for _ in range(rounds):
        for k, m in mods.items():
            win[k].append(round(window(lambda: step(m, x), iters), 1))
    return win


def count_launches(args):
    """Call counts of the rocprofv3 stats tables of 2 and 12 evaluations of each variant -> launches per evaluation."""
    out = {}
    B = max(args.batches)
    tmp = os.path.join(args.profile_dir, 'rocprof_tmp')
    for kind in KINDS:
        calls = {}
        for n in (2, 12):
            d = os.path.join(tmp, '%s_%d' % (kind, n))
            cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--',
                   sys.executable, os.path.abspath(__file__), '--count-launches', kind, '--evals', str(n), '--batches', str(B)]
            with open(os.path.join(args.profile_dir, 'rocprofv3_%s_x%d.log' % (kind, n)), 'w') as log:
                r = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=300)
            if r.returncode != 0:
                raise RuntimeError('rocprofv3 run of %s x %d ended with %d' % (kind, n, r.returncode))
            tables = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
            if len(tables) != 1:
                raise RuntimeError('expected one kernel stats table under %s, found %s' % (d, tables))
            with open(tables[0]) as fh:
                calls[n] = sum(int(row['Calls']) for row in csv.DictReader(fh))
            if n == 12:
                shutil.copyfile(tables[0], os.path.join(args.profile_dir, 'kernel_stats_%s_B%d_x12.csv' % (kind, B)))
        out[kind] = (calls[12] - calls[2]) / 10.0
    shutil.rmtree(tmp, ignore_errors=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'pose_prior'))
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--count-launches', choices=KINDS)
    ap.add_argument('--evals', type=int, default=10)
    args = ap.parse_args()
    from renderih_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda', 0)
    mods = variants(dev)
    if args.count_launches:
        x = inputs(args.batches[0], mods, dev)
        for _ in range(args.evals):
            step(mods[args.count_launches], x)
        torch.cuda.synchronize()
        print(json.dumps({'count_launches': args.count_launches, 'evaluations': args.evals, 'batch': args.batches[0]}))
        return
    os.makedirs(args.profile_dir, exist_ok=True)
    res = {'tool': 'pose_prior_bench', 'iters': args.iters, 'rounds': args.rounds,
           'what': 'both hands, seven terms, forward + backward; us per evaluation, median of the windows', 'batch': {}}
    for B in args.batches:
        x = inputs(B, mods, dev)
        grads = {}
        for k, m in mods.items():                                    # faster and different is not faster
            step(m, x)
            grads[k] = [t.grad.clone() for t in x]
        win = timed(mods, x, args.iters, args.rounds)
        med = {k: float(np.median(w)) for k, w in win.items()}
        spread = {k: round(max(w) - min(w), 1) for k, w in win.items()}
        gain = med['mirror'] - med['fused']
        res['batch'][str(B)] = {
            'us': med, 'windows': win, 'spread_us': spread, 'fused_gain_over_mirror_us': round(gain, 1),
            'fused_beats_mirror_by_more_than_its_spread': bool(gain > spread['mirror']),
            'speedup_fused_vs_mirror': round(med['mirror'] / med['fused'], 2),
            'max_rel_grad_diff_fused_vs_mirror': {n: float((a - b).abs().max() / b.abs().max())
                                                  for n, a, b in zip(NAMES, grads['fused'], grads['mirror'])}}
    if not args.no_launch_count:
        res['launches_per_evaluation'] = count_launches(args)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.profile_dir, 'pose_prior_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'pose_prior_bench.log'), 'w') as fh:
        fh.write('python tools/pose_prior_bench.py --batches %s --iters %d --rounds %d\n' %
                 (' '.join(map(str, args.batches)), args.iters, args.rounds))
        for B, r in res['batch'].items():
            for k in KINDS:
                fh.write('B=%s %-6s median %.1f us, windows %s, spread %.1f us\n' % (B, k, r['us'][k], r['windows'][k], r['spread_us'][k]))
            fh.write('B=%s fused gain over mirror %.1f us (mirror spread %.1f us): %s\n' %
                     (B, r['fused_gain_over_mirror_us'], r['spread_us']['mirror'],
                      'holds' if r['fused_beats_mirror_by_more_than_its_spread'] else 'does NOT hold'))
        if 'launches_per_evaluation' in res:
            fh.write('launches per evaluation at B=%d: %s\n' % (max(args.batches), res['launches_per_evaluation']))


if __name__ == '__main__':
    main()
