#!/usr/bin/env python
"""The joints -> MANO fit (renderih_amd.joint_fit), per iteration: (a) `graph` -- FusedManoJointFitter, one captured iteration
replayed n_iter times; (b) `eager` -- the same kernels launched without capture (graph=False); (c) `mirror` -- the plain-torch
ManoJointFitter on the device: the reference's own shape of work (convert2mano.py:183-203), batched.  The reference's file itself
cannot be timed: it needs transforms3d, pandas and its csv, none of which is present.  One build, one process.  Prints one JSON
line and writes it to <profile-dir>/joint_fit_bench.json (the same line and the windows to .log).

  us        microseconds per iteration at B in --batches (default 1 32 1024), n_iter = --n-iter (200): HIP events around one
            fit() (IK, fresh state, the loop, the final forward), divided by n_iter.  The variants alternate, --rounds windows
            each; medians, and every variant's own max - min over its windows.  "The graph is faster" holds where the other
            loop's median exceeds the graph's by more than that loop's own spread.
  launches  kernel launches per iteration of (a) at every batch: `rocprofv3 --kernel-trace --stats` (tracing only, the program
            after `--`) on fresh child processes with 2 and with 12 iterations; the difference of the call counts / 10.  The
            table of the 12-iteration run is kept as kernel_stats_graph_B<B>_x12.csv.

    python tools/joint_fit_bench.py [--profile-dir profiles/joint_fit] [--no-launch-count]
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
KINDS = ('graph', 'eager', 'mirror')


def variants(dev, kinds=KINDS):
    from renderih_amd import assets
    from renderih_amd.joint_fit import FusedManoJointFitter, ManoJointFitter
    d = assets.synthetic_mano_dict('right', seed=0)
    make = {'graph': lambda: FusedManoJointFitter(d, device=dev, graph=True),
            'eager': lambda: FusedManoJointFitter(d, device=dev, graph=False),
            'mirror': lambda: ManoJointFitter(d, device=dev)}
    return {k: make[k]() for k in kinds}


def inputs(fitter, B, dev, seed=0):
    """Mocap-like joints in centimetres: the layer's joints at a random root rotation, pose and shape, times 110, plus an offset."""
    from renderih_amd.manolayer import rodrigues_batch
    g = torch.Generator().manual_seed(seed)
    root = rodrigues_batch(torch.randn(B, 3, generator=g) * 0.8).to(dev)
    pose, beta = (torch.randn(B, 45, generator=g) * 0.6).to(dev), (torch.randn(B, 10, generator=g) * 0.5).to(dev)
    with torch.no_grad():
        j = fitter.layer(root, pose, beta)[1]
    return (j * 110 + (torch.randn(B, 1, 3, generator=g) * 20).to(dev)).contiguous()


def window(fitter, joints, n_iter):
    fitter.n_iter = n_iter
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = fitter.fit(joints)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n_iter, res


def count_launches(args, B):
    """Call counts of the rocprofv3 stats tables of 2 and 12 iterations of the replayed graph -> launches per iteration."""
    tmp = os.path.join(args.profile_dir, 'rocprof_tmp')
    calls = {}
    for n in (2, 12):
        d = os.path.join(tmp, 'graph_B%d_%d' % (B, n))
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--count-launches', '--n-iter', str(n), '--batches', str(B)]
        with open(os.path.join(args.profile_dir, 'rocprofv3_graph_B%d_x%d.log' % (B, n)), 'w') as log:
            r = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=300)
        if r.returncode != 0:
            raise RuntimeError('rocprofv3 run of %d iterations at B=%d ended with %d' % (n, B, r.returncode))
        tables = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if len(tables) != 1:
            raise RuntimeError('expected one kernel stats table under %s, found %s' % (d, tables))
        with open(tables[0]) as fh:
            calls[n] = sum(int(row['Calls']) for row in csv.DictReader(fh))
        if n == 12:
            shutil.copyfile(tables[0], os.path.join(args.profile_dir, 'kernel_stats_graph_B%d_x12.csv' % B))
    shutil.rmtree(tmp, ignore_errors=True)
    return (calls[12] - calls[2]) / 10.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32, 1024])
    ap.add_argument('--n-iter', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'joint_fit'))
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--count-launches', action='store_true')
    args = ap.parse_args()
    from renderih_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda', 0)
    if args.count_launches:
        f = variants(dev, ('graph',))['graph']
        window(f, inputs(f, args.batches[0], dev), args.n_iter)
        print(json.dumps({'count_launches': 'graph', 'iterations': args.n_iter, 'batch': args.batches[0]}))
        return
    os.makedirs(args.profile_dir, exist_ok=True)
    fit = variants(dev)
    res = {'tool': 'joint_fit_bench', 'n_iter': args.n_iter, 'rounds': args.rounds,
           'what': 'one fit() of n_iter iterations; us per iteration, median of the windows', 'batch': {}}
    for B in args.batches:
        joints = inputs(fit['graph'], B, dev)
        out = {k: window(f, joints, args.n_iter)[1] for k, f in fit.items()}                # warm-up (captures the graph)
        win = {k: [] for k in fit}
        for _ in range(args.rounds):
            for k, f in fit.items():
                win[k].append(round(window(f, joints, args.n_iter)[0], 1))
        med = {k: float(np.median(w)) for k, w in win.items()}
        spread = {k: round(max(w) - min(w), 1) for k, w in win.items()}
        res['batch'][str(B)] = {
            'us_per_iteration': med, 'windows': win, 'spread_us': spread,
            'graph_beats_eager_by_more_than_its_spread': bool(med['eager'] - med['graph'] > spread['eager']),
            'graph_beats_mirror_by_more_than_its_spread': bool(med['mirror'] - med['graph'] > spread['mirror']),
            'speedup_graph_vs_eager': round(med['eager'] / med['graph'], 2),
            'speedup_graph_vs_mirror': round(med['mirror'] / med['graph'], 2),
            'graph_equals_eager_bitwise': bool(all(torch.equal(out['graph'][k], out['eager'][k]) for k in out['graph'])),
            'final_loss_mean': {k: float(out[k]['loss'].mean()) for k in out}}
        if not args.no_launch_count:
            res['batch'][str(B)]['launches_per_iteration_graph'] = count_launches(args, B)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.profile_dir, 'joint_fit_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'joint_fit_bench.log'), 'w') as fh:
        fh.write('python tools/joint_fit_bench.py --batches %s --n-iter %d --rounds %d\n' %
                 (' '.join(map(str, args.batches)), args.n_iter, args.rounds))
        for B, r in res['batch'].items():
            for k in KINDS:
                fh.write('B=%s %-6s median %.1f us per iteration, windows %s, spread %.1f us\n' %
                         (B, k, r['us_per_iteration'][k], r['windows'][k], r['spread_us'][k]))
            for k in ('eager', 'mirror'):
                fh.write('B=%s graph faster than %s by more than that loop\'s spread: %s (x%.2f)\n' %
                         (B, k, 'holds' if r['graph_beats_%s_by_more_than_its_spread' % k] else 'does NOT hold',
                          r['speedup_graph_vs_' + k]))
            if 'launches_per_iteration_graph' in r:
                fh.write('B=%s launches per iteration of the replayed graph: %s\n' % (B, r['launches_per_iteration_graph']))


if __name__ == '__main__':
    main()
