#!/usr/bin/env python
"""The two-hand pose optimiser's loop, per iteration: (a) `graph` -- renderih_amd.pose_opt.FusedTwoHandPoseOptimizer, one captured
iteration replayed n_iter times, no host read inside the loop; (b) `eager` -- the loop a user had to write before it: the fused
modules, torch.optim.Adam over the four groups, ReduceLROnPlateau.step(loss) with its host read; (c) `mirror` -- the plain-torch
TwoHandPoseOptimizer.  One build, one process.  Prints one JSON line and writes it to <profile-dir>/pose_opt_bench.json (the
same line and the windows to .log).

  us        microseconds per iteration at B in --batches (default 1 32), G = --grid (32), n_iter = --n-iter (50): HIP events
            around one optimize() call (fresh state from set_opt_val before each, outside the window; the result's four small
            device-to-host copies inside, as a user pays them), divided by n_iter.  The variants alternate, --rounds windows
            each; medians, and every variant's own max - min over its windows.  The claim "the graph is faster" holds where the
            eager median exceeds the graph's by more than the eager loop's own spread.
  launches  kernel launches per iteration of (a) at the largest batch: `rocprofv3 --kernel-trace --stats` (tracing only, the
            program after `--`) on fresh child processes with 2 and with 12 iterations; the difference of the call counts / 10.

    python tools/pose_opt_bench.py [--profile-dir profiles/pose_optimizer] [--no-launch-count]
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
KEYS = ('optimized_hand_pose', 'optimized_hand_tsl', 'optimized_sub_hand_pose', 'optimized_sub_hand_tsl')
D = 4


def variants(dev, grid, kinds=KINDS):
    from renderih_amd import assets
    from renderih_amd.pose_opt import FusedTwoHandPoseOptimizer, TwoHandPoseOptimizer

    class EagerLoop(TwoHandPoseOptimizer):
        """The loop of the mirror on the fused modules: what the three loss kernels alone allowed."""
        _classes = FusedTwoHandPoseOptimizer._classes
    r, l = assets.synthetic_mano_dict('right', seed=0), assets.synthetic_mano_dict('left', seed=0)
    anchor = os.path.join(ROOT, 'tests', 'golden', 'anchor')
    part_vert = np.ones(778, np.int32)
    cls = {'graph': FusedTwoHandPoseOptimizer, 'eager': EagerLoop, 'mirror': TwoHandPoseOptimizer}
    return {k: cls[k](r, l, anchor, part_vert, grid_size=grid, device=dev) for k in kinds}


def inputs(B, A, seed=0):
    """Two interpenetrating hands: a free root rotation, fingers bent by a few degrees, the left hand pushed a fifth of its size
    into the right one; random contact tables."""
    rs = np.random.RandomState(seed)
    q = np.zeros((2, B, 16, 4))
    q[..., 0] = 1.0
    q[..., 1:] = 0.04 * rs.randn(2, B, 16, 3)
    q[:, :, 0, 1:] = 0.3 * rs.randn(2, B, 3)
    q *= rs.uniform(0.7, 1.5, size=(2, B, 16, 1))
    t = np.zeros((2, B, 3))
    t[1] = np.array([0.003, 0.004, 0.005]) + 0.001 * rs.randn(B, 3)
    q, t = torch.from_numpy(q.astype(np.float32)), torch.from_numpy(t.astype(np.float32))
    return dict(anchor_id=torch.from_numpy(rs.randint(0, A, size=(B, A, D))), anchor_elasti=torch.from_numpy(rs.rand(B, A, D).astype(np.float32)),
                anchor_padding_mask=torch.from_numpy((rs.rand(B, A, D) < 0.5).astype(np.int64)),
                hand_shape_init=torch.from_numpy((0.3 * rs.randn(B, 20)).astype(np.float32)), hand_tsl_init=t[0], obj_tsl_init=t[1],
                hand_pose_gt=([0], q[0][:, 0:1]), hand_pose_init=(list(range(1, 16)), q[0][:, 1:]),
                obj_pose_gt=([0], q[1][:, 0:1]), obj_pose_init=(list(range(1, 16)), q[1][:, 1:]), batch_size=B)


def window(opt, case, n_iter):
    opt.set_opt_val(**case)
    opt.n_iter = n_iter
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    res = opt.optimize()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n_iter, res


def count_launches(args):
    """Call counts of the rocprofv3 stats tables of 2 and 12 iterations of the replayed graph -> launches per iteration."""
    B = max(args.batches)
    tmp = os.path.join(args.profile_dir, 'rocprof_tmp')
    calls = {}
    for n in (2, 12):
        d = os.path.join(tmp, 'graph_%d' % n)
        cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--',
               sys.executable, os.path.abspath(__file__), '--count-launches', '--n-iter', str(n), '--batches', str(B),
               '--grid', str(args.grid)]
        with open(os.path.join(args.profile_dir, 'rocprofv3_graph_x%d.log' % n), 'w') as log:
            r = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=300)
        if r.returncode != 0:
            raise RuntimeError('rocprofv3 run of %d iterations ended with %d' % (n, r.returncode))
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
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--grid', type=int, default=32)
    ap.add_argument('--n-iter', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'pose_optimizer'))
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--count-launches', action='store_true')
    args = ap.parse_args()
    from renderih_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda', 0)
    if args.count_launches:
        opt = variants(dev, args.grid, ('graph',))['graph']
        A = opt.anchor_layer.face_vert_idx.shape[1]
        window(opt, inputs(args.batches[0], A), args.n_iter)
        print(json.dumps({'count_launches': 'graph', 'iterations': args.n_iter, 'batch': args.batches[0]}))
        return
    os.makedirs(args.profile_dir, exist_ok=True)
    opts = variants(dev, args.grid)
    A = opts['graph'].anchor_layer.face_vert_idx.shape[1]
    res = {'tool': 'pose_opt_bench', 'n_iter': args.n_iter, 'rounds': args.rounds, 'grid': args.grid,
           'what': 'one optimize() of n_iter iterations; us per iteration, median of the windows', 'batch': {}}
    for B in args.batches:
        case = inputs(B, A)
        out = {k: window(o, case, args.n_iter)[1] for k, o in opts.items()}             # warm-up (captures the graph)
        win = {k: [] for k in opts}
        for _ in range(args.rounds):
            for k, o in opts.items():
                win[k].append(round(window(o, case, args.n_iter)[0], 1))
        med = {k: float(np.median(w)) for k, w in win.items()}
        spread = {k: round(max(w) - min(w), 1) for k, w in win.items()}
        gain = med['eager'] - med['graph']
        res['batch'][str(B)] = {
            'us_per_iteration': med, 'windows': win, 'spread_us': spread, 'graph_gain_over_eager_us': round(gain, 1),
            'graph_beats_eager_by_more_than_its_spread': bool(gain > spread['eager']),
            'speedup_graph_vs_eager': round(med['eager'] / med['graph'], 2),
            'speedup_graph_vs_mirror': round(med['mirror'] / med['graph'], 2),
            # faster and different is not faster: the trajectories separate slowly (Adam divides by sqrt(v))
            'max_abs_diff_graph_vs_eager_after_n_iter': {k: float((out['graph'][k] - out['eager'][k]).abs().max()) for k in KEYS}}
    if not args.no_launch_count:
        res['launches_per_iteration_graph'] = count_launches(args)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.profile_dir, 'pose_opt_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'pose_opt_bench.log'), 'w') as fh:
        fh.write('python tools/pose_opt_bench.py --batches %s --grid %d --n-iter %d --rounds %d\n' %
                 (' '.join(map(str, args.batches)), args.grid, args.n_iter, args.rounds))
        for B, r in res['batch'].items():
            for k in KINDS:
                fh.write('B=%s %-6s median %.1f us per iteration, windows %s, spread %.1f us\n' %
                         (B, k, r['us_per_iteration'][k], r['windows'][k], r['spread_us'][k]))
            fh.write('B=%s graph gain over eager %.1f us (eager spread %.1f us): %s\n' %
                     (B, r['graph_gain_over_eager_us'], r['spread_us']['eager'],
                      'holds' if r['graph_beats_eager_by_more_than_its_spread'] else 'does NOT hold'))
        if 'launches_per_iteration_graph' in res:
            fh.write('launches per iteration of the replayed graph at B=%d: %s\n' % (max(args.batches), res['launches_per_iteration_graph']))


if __name__ == '__main__':
    main()
