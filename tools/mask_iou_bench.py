#!/usr/bin/env python
"""The two-hand silhouette IoU, per call on B perspective scenes at S = 256 (the reference's IMG_SIZE): (a) `fused` --
renderih_amd.mask_iou.FusedTwoHandMaskIoU, one rih_render_setup launch and one rih_mask_iou call; (b) `mirror` -- TwoHandMaskIoU,
the reference's lines (utils/compute_maskiou.py:263-270) on this project's renderer: two renders of three launches each, the
division by 255, the threshold and the counts in torch on the device.  The mirror runs only kernels that existed before
rih_mask_iou, so it is the baseline; B = 1 is the reference's per-sample loop.  The hands are the MANO templates, rotated per
scene and placed so that they overlap in the image.

  us        microseconds per call at B in --batches (default 1 32 256): HIP events around --reps calls of (a) and
            --mirror-reps calls of (b).  The variants alternate, --rounds windows each after a warm-up of every shape; medians,
            and every variant's own max - min.  The claim "the fused call is faster than the mirror" holds where the mirror's
            median exceeds the fused one's by more than the mirror's own spread.
  same      whether both give the same counts on the timed scenes.
  kernels   per variant and B, a fresh child process under `rocprofv3 --kernel-trace --stats` (tracing only, the program after
            `--`) that makes 20 calls: launches per call (every kernel, torch's included) and the mean time of this project's
            kernels.
  bytes     a model from the shapes alone: what each variant moves per call beyond the face records, which both read alike.

Prints one JSON line and writes it to <profile-dir>/mask_iou_bench.json (the same line and the windows to .log).
    python tools/mask_iou_bench.py [--profile-dir profiles/mask_iou] [--no-kernel-trace]
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
OURS = ('setup_kernel', 'mask_zero_kernel', 'mask_iou_kernel', 'mask_ratio_kernel', 'raster_kernel', 'shade_kernel')
CALLS = 20                       # calls of the traced child


def rodrigues(a):
    t = np.linalg.norm(a) + 1e-12
    k = a / t
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K


def scenes(B, S, dev, seed=0):
    """Both hands half a metre in front of a pinhole camera, overlapping in the image: v3d_left, v3d_right [B, 778, 3], K."""
    from renderih_amd import assets
    rs = np.random.RandomState(seed)
    out = []
    for side, at in (('left', (-0.02, 0.0, 0.5)), ('right', (0.02, 0.0, 0.52))):
        vt = assets.obj_template(side)
        vt = vt - vt.mean(0)
        out.append(np.stack([vt @ rodrigues(rs.randn(3) * 0.3).T + np.array(at) + 0.01 * rs.randn(3) for _ in range(B)]))
    K = np.zeros((B, 3, 3))
    K[:, 0, 0] = K[:, 1, 1] = S * (1.1 + 0.2 * rs.rand(B))
    K[:, 0, 2] = S / 2 + rs.randn(B) * 2
    K[:, 1, 2] = S / 2 + rs.randn(B) * 2
    K[:, 2, 2] = 1
    return [torch.from_numpy(a.astype(np.float32)).to(dev) for a in (out[0], out[1], K)]


def device_window(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernel_trace(args, B, kind):
    """Launches per call and this project's kernels' mean times, from the stats table of a traced child making CALLS calls."""
    d = os.path.join(args.profile_dir, 'rocprof_tmp', '%s_B%d' % (kind, B))
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'run', '--',
           sys.executable, os.path.abspath(__file__), '--launch-only', kind, '--batches', str(B), '--size', str(args.size)]
    with open(os.path.join(args.profile_dir, 'rocprofv3_%s_B%d.log' % (kind, B)), 'w') as log:
        r = subprocess.run(cmd, stdout=log, stderr=subprocess.STDOUT, timeout=300)
    if r.returncode != 0:
        raise RuntimeError('rocprofv3 run of %s at B = %d ended with %d' % (kind, B, r.returncode))
    tables = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
    if len(tables) != 1:
        raise RuntimeError('expected one kernel stats table under %s, found %s' % (d, tables))
    shutil.copyfile(tables[0], os.path.join(args.profile_dir, 'kernel_stats_%s_B%d.csv' % (kind, B)))
    with open(tables[0]) as fh:
        rows = list(csv.DictReader(fh))
    ours = {}
    for row in rows:
        for name in OURS:
            if name in row['Name']:
                ours[name] = {'per_call': int(row['Calls']) / CALLS, 'mean_us': round(float(row['AverageNs']) / 1e3, 2)}
    total = sum(int(row['Calls']) for row in rows)
    return {'launches_per_call': total / CALLS, 'ours': ours,
            'our_kernels_us_per_call': round(sum(v['per_call'] * v['mean_us'] for v in ours.values()), 2),
            'all_kernels_us_per_call': round(sum(float(row['TotalDurationNs']) for row in rows) / 1e3 / CALLS, 2)}


def bytes_model(B, S, F):
    """Per call, beyond the face records (64 B each, written once by setup and read by every tile, alike in both variants --
    the mirror sets up and walks each hand's F / 2 records in a launch of its own): the mirror writes fragments (pix_to_face 4,
    zbuf 4, bary 12 = 20 B), re-reads 16 B of them in the shader and writes RGBA 16 B per pixel and hand, before torch's own
    passes (/255, slice, threshold, compares, sums), which are left out; the fused kernel writes three integers and a float."""
    return {'face_records_both': B * F * 64, 'mirror_fragments_and_rgba': 2 * B * S * S * (20 + 16 + 16),
            'fused_counts_and_iou': B * (12 + 12 + 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32, 256])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--mirror-reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'mask_iou'))
    ap.add_argument('--no-kernel-trace', action='store_true')
    ap.add_argument('--launch-only', choices=KINDS)
    args = ap.parse_args()
    from renderih_amd import _lib
    from renderih_amd.mask_iou import FusedTwoHandMaskIoU, TwoHandMaskIoU
    _lib.load()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda', 0)
    S = args.size
    variants = {'fused': FusedTwoHandMaskIoU(S, dev), 'mirror': TwoHandMaskIoU(S, dev)}
    if args.launch_only:                        # the traced child: CALLS calls of one variant at one B
        vl, vr, K = scenes(args.batches[0], S, dev)
        variants[args.launch_only](vl, vr, cameras=K)           # the topology's upload is not a call
        torch.cuda.synchronize()
        for _ in range(CALLS - 1):
            variants[args.launch_only](vl, vr, cameras=K)
        torch.cuda.synchronize()
        return
    os.makedirs(args.profile_dir, exist_ok=True)
    F = 2 * int(variants['fused'].faces_left.shape[0])
    res = {'tool': 'mask_iou_bench', 'size': S, 'reps': args.reps, 'mirror_reps': args.mirror_reps, 'rounds': args.rounds,
           'faces': F, 'what': 'us per call on B scenes, median of the windows', 'batch': {}}
    lines = []
    for B in args.batches:
        vl, vr, K = scenes(B, S, dev)
        calls = {k: (lambda v=v: v(vl, vr, cameras=K)) for k, v in variants.items()}
        out = {k: f() for k, f in calls.items()}                                         # warm-up of every shape
        win = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, f in calls.items():
                win[k].append(round(device_window(f, args.reps if k == 'fused' else args.mirror_reps), 1))
        med = {k: float(np.median(win[k])) for k in KINDS}
        spread = {k: round(max(win[k]) - min(win[k]), 1) for k in KINDS}
        gain = med['mirror'] - med['fused']
        entry = {'us_per_call': med, 'windows': win, 'spread_us': spread, 'fused_gain_over_mirror_us': round(gain, 1),
                 'fused_beats_mirror_by_more_than_its_spread': bool(gain > spread['mirror']),
                 'speedup_fused_vs_mirror': round(med['mirror'] / med['fused'], 1),
                 'same_counts': bool(torch.equal(out['fused'][1], out['mirror'][1])),
                 'same_iou': bool(torch.equal(out['fused'][0], out['mirror'][0])),
                 'iou_min_median_max': [round(float(x), 3) for x in (out['fused'][0].min(), out['fused'][0].median(),
                                                                     out['fused'][0].max())],
                 'us_per_sample_fused': round(med['fused'] / B, 2), 'bytes_model': bytes_model(B, S, F)}
        for k in KINDS:
            lines.append('B=%d %-6s median %.1f us per call, windows %s, spread %.1f us' % (B, k, med[k], win[k], spread[k]))
        lines.append('B=%d fused gain over the mirror %.1f us (mirror spread %.1f us): %s' %
                     (B, gain, spread['mirror'], 'holds' if gain > spread['mirror'] else 'does NOT hold'))
        if not args.no_kernel_trace:
            entry['kernels'] = {k: kernel_trace(args, B, k) for k in KINDS}
            for k in KINDS:
                e = entry['kernels'][k]
                lines.append('B=%d %-6s rocprofv3 --kernel-trace --stats, %d calls: %.1f launches per call, this project\'s '
                             'kernels %.2f us per call %s, all kernels %.2f us per call' %
                             (B, k, CALLS, e['launches_per_call'], e['our_kernels_us_per_call'],
                              {n: v['mean_us'] for n, v in e['ours'].items()}, e['all_kernels_us_per_call']))
        res['batch'][str(B)] = entry
    shutil.rmtree(os.path.join(args.profile_dir, 'rocprof_tmp'), ignore_errors=True)
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.profile_dir, 'mask_iou_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'mask_iou_bench.log'), 'w') as fh:
        fh.write('python tools/mask_iou_bench.py --batches %s --size %d --reps %d --mirror-reps %d --rounds %d\n' %
                 (' '.join(map(str, args.batches)), S, args.reps, args.mirror_reps, args.rounds))
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
