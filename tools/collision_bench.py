#!/usr/bin/env python
"""The two-hand collision count, per call on B frames of two 1538-face hands: (a) `fused` --
renderih_amd.collision.FusedTwoHandCollisionCount, one launch of rih_collision_count (and one memset); (b) `mirror` -- the
plain-torch TwoHandCollisionCount on the device.  The frames are the 8 of tests/golden/contact_search.npz (three near, one far
per set), tiled to B.  No timing of the reference exists: its collision gate needs trimesh and FCL, which are not available here.

  us        microseconds per call at B in --batches (default 1 32 256): HIP events around --reps calls of (a) and
            --mirror-reps calls of (b).  The variants alternate, --rounds windows each after a warm-up of every shape; medians,
            and every variant's own max - min.  The claim "the fused count is faster than the mirror" holds where the mirror's
            median exceeds the fused one's by more than the mirror's own spread.
  same      whether both give the same counts on the timed frames (they may differ on pairs within an fp32 rounding of flipping).
  kernel    the kernel's own time per launch at every B: `rocprofv3 --kernel-trace --stats` (tracing only, the program after
            `--`) on a fresh child process per B.
  gate      `filter_sequence` over N = --gate-frames frames in one batch beside ONE attempt of `optimize_sequence` (the
            reference schedule's first: n_iter 50, a fresh search) over the same frames, host clock around each (both end in
            copies to the host).

Prints one JSON line and writes it to <profile-dir>/collision_bench.json (the same line and the windows to .log).
    python tools/collision_bench.py [--profile-dir profiles/collision] [--no-kernel-trace]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
KINDS = ('fused', 'mirror')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'contact_search.npz')
ANCHOR = os.path.join(ROOT, 'tests', 'golden', 'anchor')
KERNEL = 'collision_count_kernel'


def frames(B, dev):
    z = np.load(GOLDEN)
    vm = np.concatenate([z['verts_main'], z['verts_main2']]).astype(np.float32)
    vs = np.concatenate([z['verts_sub'], z['verts_sub2']]).astype(np.float32)
    pick = np.arange(B) % vm.shape[0]
    return torch.from_numpy(vm[pick]).to(dev), torch.from_numpy(vs[pick]).to(dev)


def device_window(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def host_window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def kernel_time(args, B):
    """Mean time of the kernel per launch, in us, from the stats table of a traced child process that launches it 20 times."""
    d = os.path.join(args.profile_dir, 'rocprof_tmp', 'B%d' % B)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--',
           sys.executable, os.path.abspath(__file__), '--launch-only', '--batches', str(B)]
    with open(os.path.join(args.profile_dir, 'rocprofv3_B%d.log' % B), 'w') as log:
        r = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=300)
    if r.returncode != 0:
        raise RuntimeError('rocprofv3 run at B = %d ended with %d' % (B, r.returncode))
    tables = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if len(tables) != 1:
        raise RuntimeError('expected one kernel stats table under %s, found %s' % (d, tables))
    shutil.copyfile(tables[0], os.path.join(args.profile_dir, 'kernel_stats_B%d.csv' % B))
    with open(tables[0]) as fh:
        rows = [row for row in csv.DictReader(fh) if KERNEL in row['Name']]
    if len(rows) != 1:
        raise RuntimeError('expected one row of %s in %s' % (KERNEL, tables[0]))
    return {'calls': int(rows[0]['Calls']), 'mean_us': round(float(rows[0]['AverageNs']) / 1e3, 2),
            'min_us': round(float(rows[0]['MinNs']) / 1e3, 2), 'max_us': round(float(rows[0]['MaxNs']) / 1e3, 2)}


def gate(args, dev):
    from pose_opt_bench import variants
    from renderih_amd.collision import FusedTwoHandCollisionCount, filter_sequence
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    from renderih_amd.pose_driver import REFERENCE_SCHEDULE, optimize_sequence
    from pose_opt_bench import inputs
    N = args.gate_frames
    opt = variants(dev, 32, ('graph',))['graph']
    search, counter = FusedTwoHandContactSearch(ANCHOR).to(dev), FusedTwoHandCollisionCount().to(dev)
    case = inputs(N, 108)
    seq = [torch.cat([case['hand_pose_gt'][1], case['hand_pose_init'][1]], 1), case['hand_tsl_init'],
           torch.cat([case['obj_pose_gt'][1], case['obj_pose_init'][1]], 1), case['obj_tsl_init'], case['hand_shape_init']]
    runs = {'optimize_sequence_one_attempt': lambda: optimize_sequence(opt, search, *seq, batch_size=N, schedule=REFERENCE_SCHEDULE[:1]),
            'filter_sequence': lambda: filter_sequence(opt, counter, *seq, max_pairs=0, batch_size=N)}
    out = {k: f() for k, f in runs.items()}                                              # warm-up, the graph's capture
    win = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, f in runs.items():
            win[k].append(round(host_window(f), 1))
    med = {k: float(np.median(v)) for k, v in win.items()}
    return {'frames': N, 'us': med, 'windows': win, 'gate_share_of_one_attempt': round(med['filter_sequence'] / med['optimize_sequence_one_attempt'], 4),
            'pairs_per_frame_median': float(out['filter_sequence']['count'].double().median())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32, 256])
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--mirror-reps', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--gate-frames', type=int, default=32)
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'collision'))
    ap.add_argument('--no-kernel-trace', action='store_true')
    ap.add_argument('--launch-only', action='store_true')
    args = ap.parse_args()
    from renderih_amd import _lib
    from renderih_amd.collision import FusedTwoHandCollisionCount, TwoHandCollisionCount
    _lib.load()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda', 0)
    fused, mirror = FusedTwoHandCollisionCount().to(dev), TwoHandCollisionCount().to(dev)
    if args.launch_only:                        # the traced child: 20 launches at one B
        vm, vs = frames(args.batches[0], dev)
        for _ in range(20):
            fused(vm, vs)
        torch.cuda.synchronize()
        return
    os.makedirs(args.profile_dir, exist_ok=True)
    res = {'tool': 'collision_bench', 'reps': args.reps, 'mirror_reps': args.mirror_reps, 'rounds': args.rounds,
           'faces': int(fused.faces_main.shape[0]), 'what': 'us per call on B frames, median of the windows', 'batch': {}}
    lines = []
    for B in args.batches:
        vm, vs = frames(B, dev)
        calls = {'fused': lambda: fused(vm, vs), 'mirror': lambda: mirror(vm, vs)}
        out = {k: f() for k, f in calls.items()}                                         # warm-up of every shape
        win = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, f in calls.items():
                win[k].append(round(device_window(f, args.reps if k == 'fused' else args.mirror_reps), 1))
        med = {k: float(np.median(win[k])) for k in KINDS}
        spread = {k: round(max(win[k]) - min(win[k]), 1) for k in KINDS}
        gain = med['mirror'] - med['fused']
        count = out['fused']['count']
        entry = {'us_per_call': med, 'windows': win, 'spread_us': spread, 'fused_gain_over_mirror_us': round(gain, 1),
                 'fused_beats_mirror_by_more_than_its_spread': bool(gain > spread['mirror']),
                 'speedup_fused_vs_mirror': round(med['mirror'] / med['fused'], 1),
                 'frames_with_the_mirrors_count': float((count == out['mirror']['count']).float().mean()),
                 'pairs_per_frame': count[:8].tolist(), 'us_per_frame_fused': round(med['fused'] / B, 2)}
        if not args.no_kernel_trace:
            entry['kernel'] = kernel_time(args, B)
        for k in KINDS:
            lines.append('B=%d %-6s median %.1f us per call, windows %s, spread %.1f us' % (B, k, med[k], win[k], spread[k]))
        lines.append('B=%d fused gain over the mirror %.1f us (mirror spread %.1f us): %s' %
                     (B, gain, spread['mirror'], 'holds' if gain > spread['mirror'] else 'does NOT hold'))
        if 'kernel' in entry:
            lines.append('B=%d kernel alone (rocprofv3 --kernel-trace --stats, %d launches): mean %.2f us, min %.2f, max %.2f' %
                         (B, entry['kernel']['calls'], entry['kernel']['mean_us'], entry['kernel']['min_us'], entry['kernel']['max_us']))
        res['batch'][str(B)] = entry
    shutil.rmtree(os.path.join(args.profile_dir, 'rocprof_tmp'), ignore_errors=True)
    res['gate'] = gate(args, dev)
    lines.append('gate over %d frames: filter_sequence median %.1f us %s; one optimize_sequence attempt median %.1f us %s' %
                 (res['gate']['frames'], res['gate']['us']['filter_sequence'], res['gate']['windows']['filter_sequence'],
                  res['gate']['us']['optimize_sequence_one_attempt'], res['gate']['windows']['optimize_sequence_one_attempt']))
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.profile_dir, 'collision_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'collision_bench.log'), 'w') as fh:
        fh.write('python tools/collision_bench.py --batches %s --reps %d --mirror-reps %d --rounds %d --gate-frames %d\n' %
                 (' '.join(map(str, args.batches)), args.reps, args.mirror_reps, args.rounds, args.gate_frames))
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
