#!/usr/bin/env python
"""Quaternion MANO layer of the pose optimiser, forward + backward of one hand: (a) the fused HIP path
(renderih_amd.quat_mano.FusedQuatManoLayer), (b) `quaternion_to_rotation_matrix` in torch followed by
renderih_amd.manolayer.ManoLayer on rotation matrices -- what could be assembled before the quaternion mode existed; it has
no transforms --, (c) the torch mirror (QuatManoLayer), on one build in one process.  Prints one JSON line.

  us        microseconds per evaluation at B in --batches (default 1 32): forward, then backward of a fixed weighting of
            verts, joints (and transf for a and c).  HIP events on the current stream after a warm-up; the three variants
            alternate, --rounds windows of --iters evaluations each; medians, and every variant's own max - min over its windows.
  launches  kernel launches per evaluation at the largest batch: each variant runs under `rocprofv3 --kernel-trace --stats`
            (tracing only, the program after `--`) in fresh child processes with 2 and with 12 evaluations; the difference of
            the call counts / 10.  The stats tables of the 12-evaluation runs are kept in --profile-dir.

    python tools/quat_mano_bench.py [--profile-dir DIR] [--json out.json]
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
KINDS = ('fused', 'torch_quat_plus_rotmat_layer', 'mirror')


def inputs(B, dev, seed=0):
    rs = np.random.RandomState(seed)
    q = rs.randn(B, 16, 4)
    q[..., 0] = np.abs(q[..., 0]) + 1.0
    q = q / np.linalg.norm(q, axis=-1, keepdims=True) * rs.uniform(0.5, 2.0, size=(B, 16, 1))
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev)
    return {'q': t(q).requires_grad_(True), 'betas': t(rs.randn(B, 10) * 0.8).requires_grad_(True),
            'wv': t(rs.rand(B, 778, 3)), 'wj': t(rs.rand(B, 21, 3)), 'wT': t(rs.rand(B, 16, 4, 4))}


def variants(dev):
    from renderih_amd import assets
    from renderih_amd.manolayer import ManoLayer
    from renderih_amd.quat_mano import FusedQuatManoLayer, QuatManoLayer, quaternion_to_rotation_matrix
    d = assets.synthetic_mano_dict('right', seed=0)
    fused = FusedQuatManoLayer(d, center_idx=0, return_transf=True).to(dev)
    mirror = QuatManoLayer(d, center_idx=0, return_transf=True).to(dev)
    rotmat = ManoLayer(d, center_idx=0, use_pca=False).to(dev)

    def with_transf(layer):
        def fn(x):
            v, j, T = layer(x['q'], x['betas'])
            return (x['wv'] * v).sum() + (x['wj'] * j).sum() + (x['wT'] * T).sum()
        return fn

    def assembled(x):
        R = quaternion_to_rotation_matrix(x['q'])
        v, j = rotmat(R[:, 0], R[:, 1:], x['betas'])
        return (x['wv'] * v).sum() + (x['wj'] * j).sum()
    return {'fused': with_transf(fused), 'torch_quat_plus_rotmat_layer': assembled, 'mirror': with_transf(mirror)}


def step(fn, x):
    x['q'].grad = x['betas'].grad = None
    fn(x).backward()


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def timed(fns, x, iters, rounds):
    for f in fns.values():
        for _ in range(3):
            step(f, x)
    torch.cuda.synchronize()
    win = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            win[k].append(round(window(lambda: step(f, x), iters), 1))
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
    ap.add_argument('--profile-dir')
    ap.add_argument('--count-launches', choices=KINDS)
    ap.add_argument('--evals', type=int, default=10)
    ap.add_argument('--json')
    args = ap.parse_args()
    from renderih_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda', 0)
    fns = variants(dev)
    if args.count_launches:
        x = inputs(args.batches[0], dev)
        for _ in range(args.evals):
            step(fns[args.count_launches], x)
        torch.cuda.synchronize()
        print(json.dumps({'count_launches': args.count_launches, 'evaluations': args.evals, 'batch': args.batches[0]}))
        return
    res = {'tool': 'quat_mano_bench', 'iters': args.iters, 'rounds': args.rounds,
           'what': 'one hand, forward + backward; us per evaluation, median of the windows', 'batch': {}}
    for B in args.batches:
        x = inputs(B, dev)
        grads = {}
        for k, f in fns.items():                                    # faster and different is not faster
            step(f, x)
            grads[k] = x['q'].grad.clone()
        win = timed(fns, x, args.iters, args.rounds)
        med = {k: float(np.median(w)) for k, w in win.items()}
        spread = {k: round(max(w) - min(w), 1) for k, w in win.items()}
        gain_b = med['torch_quat_plus_rotmat_layer'] - med['fused']
        res['batch'][str(B)] = {
            'us': med, 'windows': win, 'spread_us': spread,
            'fused_gain_over_assembled_us': round(gain_b, 1),
            'fused_beats_assembled_by_more_than_its_spread': bool(gain_b > spread['torch_quat_plus_rotmat_layer']),
            'speedup_fused_vs_mirror': round(med['mirror'] / med['fused'], 2),
            'speedup_fused_vs_assembled': round(med['torch_quat_plus_rotmat_layer'] / med['fused'], 2),
            'max_abs_quat_grad_diff_fused_vs_mirror': float((grads['fused'] - grads['mirror']).abs().max()),
            'max_abs_quat_grad_mirror': float(grads['mirror'].abs().max())}
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
