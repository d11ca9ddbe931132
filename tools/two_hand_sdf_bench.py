#!/usr/bin/env python
"""Two-hand penetration loss of the pose optimiser: the fused HIP path (renderih_amd.sdf.FusedTwoHandSDFLoss) with the sparse
voxeliser, the same with the dense voxeliser (what RIH_SDF_SPARSE=0 selects), and the torch mirror (TwoHandSDFLoss), on one
build in one process.  Prints one JSON line.

  us        microseconds per evaluation, forward + backward of loss.sum(), at bs in --batches (default 1 32), G = 32,
            V = 778 (the hand templates, posed so that the fingers interpenetrate).  HIP events on the current stream after a
            warm-up; the three variants alternate, --rounds windows of --iters evaluations each; medians.  The mirror's
            windows also give its own run-to-run spread (max - min over the windows), against which the fused gain is held.
  launches  kernel launches per evaluation at the largest batch: each variant runs under `rocprofv3 --kernel-trace --stats`
            in fresh child processes with 2 and with 12 evaluations; the difference of the call counts / 10.  The stats
            tables of the 12-evaluation runs are kept in --profile-dir.

    python tools/two_hand_sdf_bench.py --part-vert tests/golden/part_vert.npy [--profile-dir DIR] [--json out.json]
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
KINDS = ('fused_sparse', 'fused_dense', 'mirror')


def rot(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    t = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def posed_hands(bs, seed=0):
    """[bs,2,778,3]: the right template and the left template moved onto it with a seeded rotation and offset."""
    from renderih_amd import assets
    rs = np.random.RandomState(seed)
    right, left = assets.obj_template('right').astype(np.float64), assets.obj_template('left').astype(np.float64)
    cr, cl = (right.min(0) + right.max(0)) / 2, (left.min(0) + left.max(0)) / 2
    out = []
    for _ in range(bs):
        R = rot(rs.randn(3), rs.uniform(20, 60))
        out.append(np.stack([right, (left - cl) @ R.T + cr + rs.uniform(-0.02, 0.02, 3)]))
    return np.stack(out).astype(np.float32)


def criteria(part_vert, G, dev):
    from renderih_amd.sdf import FusedTwoHandSDFLoss, TwoHandSDFLoss
    return {'fused_sparse': FusedTwoHandSDFLoss(part_vert, grid_size=G, sparse=True).to(dev),
            'fused_dense': FusedTwoHandSDFLoss(part_vert, grid_size=G, sparse=False).to(dev),
            'mirror': TwoHandSDFLoss(part_vert, grid_size=G).to(dev)}


def step(crit, v):
    v.grad = None
    crit(v).sum().backward()


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def timed(crits, v, iters, rounds):
    for c in crits.values():
        for _ in range(3):
            step(c, v)
    torch.cuda.synchronize()
    win = {k: [] for k in crits}
    for _ in range(rounds):
        for k, c in crits.items():
            win[k].append(round(window(lambda: step(c, v), iters), 1))
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
                   sys.executable, os.path.abspath(__file__), '--part-vert', args.part_vert, '--grid', str(args.grid),
                   '--count-launches', kind, '--evals', str(n), '--batches', str(B)]
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
    ap.add_argument('--part-vert', required=True, help="the reference's part_vert.npy (or a copy of it)")
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--grid', type=int, default=32)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--profile-dir')
    ap.add_argument('--count-launches', choices=KINDS)
    ap.add_argument('--evals', type=int, default=10)
    ap.add_argument('--json')
    args = ap.parse_args()
    from renderih_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda', 0)
    crits = criteria(args.part_vert, args.grid, dev)
    if args.count_launches:
        v = torch.from_numpy(posed_hands(args.batches[0])).to(dev).requires_grad_(True)
        for _ in range(args.evals):
            step(crits[args.count_launches], v)
        torch.cuda.synchronize()
        print(json.dumps({'count_launches': args.count_launches, 'evaluations': args.evals, 'batch': args.batches[0]}))
        return
    res = {'tool': 'two_hand_sdf_bench', 'grid': args.grid, 'V': 778, 'iters': args.iters, 'rounds': args.rounds,
           'what': 'forward + backward of loss.sum(); us per evaluation, median of the windows', 'batch': {}}
    for B in args.batches:
        v = torch.from_numpy(posed_hands(B)).to(dev).requires_grad_(True)
        ref = {}
        for k, c in crits.items():                                  # faster and different is not faster
            step(c, v)
            ref[k] = (c(v).detach().clone(), v.grad.clone())
        assert torch.equal(ref['fused_sparse'][0], ref['fused_dense'][0]) and torch.equal(ref['fused_sparse'][1], ref['fused_dense'][1])
        win = timed(crits, v, args.iters, args.rounds)
        med = {k: float(np.median(w)) for k, w in win.items()}
        spread = max(win['mirror']) - min(win['mirror'])
        crits['fused_sparse'].keep_debug = True
        crits['fused_sparse'](v)
        count = crits['fused_sparse'].debug['count'].float().mean().item()
        crits['fused_sparse'].keep_debug = False
        res['batch'][str(B)] = {
            'us': med, 'windows': win, 'mirror_spread_us': round(spread, 1),
            'fused_gain_over_mirror_us': round(med['mirror'] - med['fused_sparse'], 1),
            'speedup_sparse_vs_mirror': round(med['mirror'] / med['fused_sparse'], 2),
            'speedup_sparse_vs_dense': round(med['fused_dense'] / med['fused_sparse'], 2),
            'voxels_voxelised_per_hand_mean': round(count, 1), 'voxels_dense': args.grid ** 3,
            'max_abs_loss_diff_fused_vs_mirror': float((ref['fused_sparse'][0] - ref['mirror'][0]).abs().max()),
            'loss_mean': float(ref['mirror'][0].mean())}
    if args.profile_dir:
        os.makedirs(args.profile_dir, exist_ok=True)
        res['launches_per_evaluation'] = count_launches(args)
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
