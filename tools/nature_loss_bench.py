#!/usr/bin/env python
"""The pose optimiser's NatureLoss, forward plus backward on B frames (2B hands) at the reference's hidden width 512:
(a) `fused` -- renderih_amd.nature.FusedTwoHandNatureLoss, three launches (rih_nature_fwd, rih_nature_reduce, rih_nature_bwd);
(b) `mirror` -- the plain-torch TwoHandNatureLoss on the device, boolean indexing and the host read of its `if` included.
Beside them: one replayed iteration of FusedTwoHandPoseOptimizer(graph=True) with and without the term, which is what the op
is for (reported, not gated).  Weights: `synthetic_state_dict(--seed, 512, --pred-scale)`; poses as the tests draw them.

  us        microseconds per forward + backward at B in --batches (default 1 32): HIP events around --reps calls.  The variants
            alternate, --rounds windows each after a warm-up of every shape; medians, and every variant's own max - min.  The
            claim "the fused op beats the mirror" holds where the mirror's median exceeds the fused one's by more than the
            mirror's own spread.
  launches  device kernels per forward + backward of each variant, counted by torch.profiler on one call (--no-launch-count
            skips it; the fused op's three are then taken from its source).
  iteration microseconds per iteration of one optimize() of --n-iter replayed iterations, with and without the term.

Prints one JSON line and writes it to <profile-dir>/nature_loss_bench.json (the same line and the windows to .log).
    python tools/nature_loss_bench.py [--profile-dir profiles/nature_loss]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
KINDS = ('fused', 'mirror')
H = 512


def poses(B, dev, seed=0):
    rs = np.random.RandomState(seed)
    axis = rs.randn(2, B, 16, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * rs.uniform(0.0, 1.4, size=(2, B, 16, 1))
    q = np.concatenate([np.cos(half), np.sin(half) * axis], -1) * rs.uniform(0.7, 1.4, size=(2, B, 16, 1))
    return [torch.from_numpy(q[i].astype(np.float32)).to(dev).requires_grad_(True) for i in (0, 1)]


def device_window(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def count_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and 'emcpy' not in e.name
               and 'emset' not in e.name]
    if not kernels:
        raise RuntimeError('the profiler saw no device kernel')
    return len(kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--n-iter', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--seed', type=int, default=2)
    ap.add_argument('--pred-scale', type=float, default=8.0)
    ap.add_argument('--no-launch-count', action='store_true')
    ap.add_argument('--no-optimizer', action='store_true')
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'nature_loss'))
    args = ap.parse_args()
    from renderih_amd import _lib
    from renderih_amd.nature import FusedTwoHandNatureLoss, TwoHandNatureLoss, synthetic_state_dict
    from pose_opt_bench import inputs, variants, window
    lib = _lib.load()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda', 0)
    os.makedirs(args.profile_dir, exist_ok=True)
    sd = synthetic_state_dict(args.seed, H, args.pred_scale)
    mods = {'fused': FusedTwoHandNatureLoss(sd).to(dev), 'mirror': TwoHandNatureLoss(sd).to(dev)}
    res = {'tool': 'nature_loss_bench', 'reps': args.reps, 'rounds': args.rounds, 'n_iter': args.n_iter, 'hid_dim': H,
           'tile_rows': int(lib.rih_nature_tile_rows()), 'seed': args.seed, 'pred_scale': args.pred_scale,
           'what': 'us per forward + backward on B frames, median of the windows', 'batch': {}}
    lines = []
    for B in args.batches:
        q = poses(B, dev)

        def call(kind):
            loss, _ = mods[kind](*q)
            return torch.autograd.grad(loss, q)
        out = {k: (mods[k](*q), call(k)) for k in KINDS}                                   # warm-up of every shape
        win = {k: [] for k in KINDS}
        for _ in range(args.rounds):
            for k in KINDS:
                win[k].append(round(device_window(lambda: call(k), args.reps), 1))
        med = {k: float(np.median(win[k])) for k in KINDS}
        spread = {k: round(max(win[k]) - min(win[k]), 1) for k in KINDS}
        gain = med['mirror'] - med['fused']
        (lf, tf), gf = out['fused']
        (lm, tm), gm = out['mirror']
        entry = {'us_per_call': med, 'windows': win, 'spread_us': spread, 'fused_gain_over_mirror_us': round(gain, 1),
                 'fused_beats_mirror_by_more_than_its_spread': bool(gain > spread['mirror']),
                 'speedup_fused_vs_mirror': round(med['mirror'] / med['fused'], 2),
                 'counts': tf[2:].tolist(), 'same_counts_as_mirror': bool(torch.equal(tf[2:], tm[2:].detach())),
                 'loss_rel_diff_vs_mirror': float((lf - lm).abs() / lm.abs().clamp_min(1e-30)),
                 'max_grad_diff_vs_mirror': float(max((a - b).abs().max() for a, b in zip(gf, gm)))}
        if not args.no_launch_count:
            entry['launches'] = {k: count_kernels(lambda: call(k)) for k in KINDS}
        else:
            entry['launches'] = {'fused': 3, 'mirror': None}
        for k in KINDS:
            lines.append('B=%d %-6s median %.1f us per forward + backward, windows %s, spread %.1f us, launches %s' %
                         (B, k, med[k], win[k], spread[k], entry['launches'][k]))
        lines.append('B=%d fused gain over the mirror %.1f us (mirror spread %.1f us): %s' %
                     (B, gain, spread['mirror'], 'holds' if gain > spread['mirror'] else 'does NOT hold'))
        if not args.no_optimizer:
            opts = {'without': variants(dev, 32, ('graph',))['graph']}
            opts['with'] = type(opts['without'])(*_optimizer_args(), grid_size=32, device=dev, nature=sd)
            case = inputs(B, opts['without'].anchor_layer.face_vert_idx.shape[1])
            for o in opts.values():
                window(o, case, args.n_iter)                                               # warm-up (captures the graph)
            wo = {k: [] for k in opts}
            for _ in range(args.rounds):
                for k, o in opts.items():
                    wo[k].append(round(window(o, case, args.n_iter)[0], 1))
            mo = {k: float(np.median(w)) for k, w in wo.items()}
            entry['optimizer_us_per_iteration'] = mo
            entry['optimizer_windows'] = wo
            entry['term_cost_in_the_iteration_us'] = round(mo['with'] - mo['without'], 1)
            entry['nature_terms_after_n_iter'] = opts['with'].last_terms['nature'].tolist()
            lines.append('B=%d one replayed iteration: without the term %.1f us %s, with it %.1f us %s: +%.1f us' %
                         (B, mo['without'], wo['without'], mo['with'], wo['with'], mo['with'] - mo['without']))
        res['batch'][str(B)] = entry
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.profile_dir, 'nature_loss_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'nature_loss_bench.log'), 'w') as fh:
        fh.write('python tools/nature_loss_bench.py --batches %s --reps %d --n-iter %d --rounds %d --seed %d --pred-scale %g '
                 '(tile of %d rows)\n' % (' '.join(map(str, args.batches)), args.reps, args.n_iter, args.rounds, args.seed,
                                          args.pred_scale, res['tile_rows']))
        fh.write('\n'.join(lines) + '\n')


def _optimizer_args():
    from renderih_amd import assets
    return (assets.synthetic_mano_dict('right', seed=0), assets.synthetic_mano_dict('left', seed=0),
            os.path.join(ROOT, 'tests', 'golden', 'anchor'), np.ones(778, np.int32))


if __name__ == '__main__':
    main()
