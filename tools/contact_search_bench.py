#!/usr/bin/env python
"""The contact search of the pose optimiser's driver, per call on B frames: (a) `fused` --
renderih_amd.contact_search.FusedTwoHandContactSearch, one launch of rih_contact_search; (b) `mirror` -- the plain-torch
TwoHandContactSearch on the device; (c) `numpy` -- the per-frame host loop that the reference's driver implies (one pass over the
A sub anchors per frame, each with a norm over the A main anchors and an argsort), restated here in this project's own words
since the reference is no part of this repository.  (c) starts from vertices that already are on the host, as the reference's
CPU hand model leaves them; (a) and (b) start from device vertices and leave their outputs on the device.  Beside them: one
`optimize()` of --n-iter iterations of FusedTwoHandPoseOptimizer(graph=True), which is what one search feeds.

  us     microseconds per call, fresh search and refresh, at B in --batches (default 1 32): HIP events around --reps calls for
         (a), (b) and the optimiser, a host clock around --numpy-reps calls of (c) (no device work in it).  The variants
         alternate, --rounds windows each after a warm-up of every shape; medians, and every variant's own max - min.  The
         claim "the fused search is faster than the mirror" holds where the mirror's median exceeds the fused one's by more than
         the mirror's own spread.
  same   the share of rows whose ids the fused search and the fp32 mirror choose alike on the timed inputs (they may differ
         where two distances are within an fp32 rounding), and the largest elastic difference on those rows.

Prints one JSON line and writes it to <profile-dir>/contact_search_bench.json (the same line and the windows to .log).
    python tools/contact_search_bench.py [--profile-dir profiles/contact_search]
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
sys.path.insert(0, HERE)
KINDS = ('fused', 'mirror', 'numpy')
MODES = ('fresh', 'refresh')
ANCHOR = os.path.join(ROOT, 'tests', 'golden', 'anchor')


def numpy_search(verts_main, verts_sub, fvi, aw, cls, prev=None, dim=4):
    """The host loop, frame by frame and sub anchor by sub anchor."""
    out = []
    for b in range(verts_main.shape[0]):
        geo = []
        for v, sign in ((verts_main[b], 1.0), (verts_sub[b], -1.0)):
            e1, e2 = v[fvi[:, 1]] - v[fvi[:, 0]], v[fvi[:, 2]] - v[fvi[:, 0]]
            n = np.cross(e1, e2)
            geo.append((aw[:, :1] * e1 + aw[:, 1:] * e2 + v[fvi[:, 0]], sign * n / np.linalg.norm(n, axis=-1, keepdims=True)))
        (main, n_main), (sub, n_sub) = geo
        radius = 0.015 if prev is None else 0.02
        facing_away = n_sub @ n_main.T > -0.6
        A = main.shape[0]
        ids, el = np.zeros((A, dim), np.int64), np.zeros((A, dim), np.float32)
        contact = np.zeros(A, np.int64)
        for i in range(A):
            dis = np.linalg.norm(sub[i] - main, axis=-1)
            if prev is None:
                dis[facing_away[i]] = 1000.0
                ids[i] = np.argsort(dis, kind='stable')[:dim]
                contact[i] = (dis < radius).any()
            else:
                ids[i] = prev[b, i]
                contact[i] = (dis[ids[i]] < radius).any()
            d = dis[ids[i]]
            el[i] = (d < radius) * np.cos(0.5 * np.pi * d / radius) ** 2
        mask = (el > 0).astype(np.int64)
        el[(cls[:, None] != 4) & (cls[ids] != 4)] *= 0.3
        out.append((contact, ids, el, mask))
    return [np.stack(x) for x in zip(*out)]


def scene(B, dev, seed=0):
    """Both hands' meshes of B frames (FusedQuatManoLayer on the synthetic model, the recipe of the golden's near frames)."""
    from pose_opt_bench import variants
    opt = variants(dev, 32, ('graph',))['graph']
    rs = np.random.RandomState(seed)
    q = np.zeros((2, B, 16, 4))
    q[..., 0] = 1.0
    q[..., 1:] = 0.04 * rs.randn(2, B, 16, 3)
    q[:, :, 0, 1:] = 0.3 * rs.randn(2, B, 3)
    q *= rs.uniform(0.7, 1.5, size=(2, B, 16, 1))
    d = rs.randn(B, 3)
    t = np.stack([np.zeros((B, 3)), 0.02 * d / np.linalg.norm(d, axis=-1, keepdims=True) + 0.002 * rs.randn(B, 3)])
    q, t = torch.from_numpy(q.astype(np.float32)).to(dev), torch.from_numpy(t.astype(np.float32)).to(dev)
    shape = torch.from_numpy((0.3 * rs.randn(B, 20)).astype(np.float32)).to(dev)
    with torch.no_grad():
        vm = opt.hands[0](q[0], shape[:, :10])[0] + t[0][:, None]
        vs = opt.hands[1](q[1], shape[:, 10:])[0] + t[1][:, None]
    return opt, vm.contiguous(), vs.contiguous()


def device_window(fn, reps):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def host_window(fn, reps):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) * 1e6 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--numpy-reps', type=int, default=2)
    ap.add_argument('--n-iter', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'contact_search'))
    args = ap.parse_args()
    from renderih_amd import _lib
    from renderih_amd.contact_search import FusedTwoHandContactSearch, TwoHandContactSearch
    from pose_opt_bench import inputs, window
    _lib.load()
    assert torch.cuda.is_available(), 'this benchmark needs a GPU'
    dev = torch.device('cuda', 0)
    os.makedirs(args.profile_dir, exist_ok=True)
    fused, mirror = FusedTwoHandContactSearch(ANCHOR).to(dev), TwoHandContactSearch(ANCHOR).to(dev)
    fvi, aw = fused.face_vert_idx.cpu().numpy(), fused.anchor_weight.double().cpu().numpy()
    cls = fused.class_type.cpu().numpy()
    res = {'tool': 'contact_search_bench', 'reps': args.reps, 'numpy_reps': args.numpy_reps, 'rounds': args.rounds,
           'n_iter': args.n_iter, 'what': 'us per call on B frames, median of the windows', 'batch': {}}
    lines = []
    for B in args.batches:
        opt, vm, vs = scene(B, dev)
        ids = fused(vm, vs)['anchor_id']
        hm, hs, hids = vm.cpu().numpy(), vs.cpu().numpy(), ids.cpu().numpy()
        calls = {('fused', 'fresh'): lambda: fused(vm, vs), ('fused', 'refresh'): lambda: fused(vm, vs, ids),
                 ('mirror', 'fresh'): lambda: mirror(vm, vs), ('mirror', 'refresh'): lambda: mirror(vm, vs, ids),
                 ('numpy', 'fresh'): lambda: numpy_search(hm, hs, fvi, aw, cls),
                 ('numpy', 'refresh'): lambda: numpy_search(hm, hs, fvi, aw, cls, hids)}
        case = inputs(B, 108)
        out = {k: f() for k, f in calls.items()}                                         # warm-up of every shape
        window(opt, case, args.n_iter)
        win = {k: [] for k in calls}
        win_opt = []
        for _ in range(args.rounds):
            for k, f in calls.items():
                w = host_window(f, args.numpy_reps) if k[0] == 'numpy' else device_window(f, args.reps)
                win[k].append(round(w, 1))
            win_opt.append(round(window(opt, case, args.n_iter)[0] * args.n_iter, 1))
        entry = {'optimize_us': float(np.median(win_opt)), 'optimize_windows': win_opt}
        for mode in MODES:
            med = {k: float(np.median(win[(k, mode)])) for k in KINDS}
            spread = {k: round(max(win[(k, mode)]) - min(win[(k, mode)]), 1) for k in KINDS}
            gain = med['mirror'] - med['fused']
            f, m, n = out[('fused', mode)], out[('mirror', mode)], out[('numpy', mode)]
            same = (f['anchor_id'] == m['anchor_id']).all(-1)
            same_np = torch.from_numpy(n[1]).to(dev).eq(f['anchor_id']).all(-1)
            entry[mode] = {
                'us_per_call': med, 'windows': {k: win[(k, mode)] for k in KINDS}, 'spread_us': spread,
                'fused_gain_over_mirror_us': round(gain, 1), 'fused_beats_mirror_by_more_than_its_spread': bool(gain > spread['mirror']),
                'speedup_fused_vs_mirror': round(med['mirror'] / med['fused'], 2),
                'speedup_fused_vs_numpy': round(med['numpy'] / med['fused'], 1),
                'searches_per_optimize': {k: round(med[k] / entry['optimize_us'], 4) for k in KINDS},
                'rows_with_the_mirrors_ids': float(same.float().mean()), 'rows_with_the_numpy_ids': float(same_np.float().mean()),
                'max_elastic_diff_on_those_rows': float((f['anchor_elasti'] - m['anchor_elasti'])[same].abs().max()),
                'rows_in_contact': int(f['vertex_contact'].sum())}
            for k in KINDS:
                lines.append('B=%d %-7s %-6s median %.1f us per call, windows %s, spread %.1f us' %
                             (B, mode, k, med[k], win[(k, mode)], spread[k]))
            lines.append('B=%d %-7s fused gain over the mirror %.1f us (mirror spread %.1f us): %s' %
                         (B, mode, gain, spread['mirror'], 'holds' if gain > spread['mirror'] else 'does NOT hold'))
        lines.append('B=%d one optimize() of %d iterations: median %.1f us, windows %s' % (B, args.n_iter, entry['optimize_us'], win_opt))
        res['batch'][str(B)] = entry
    line = json.dumps(res)
    print(line)
    with open(os.path.join(args.profile_dir, 'contact_search_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'contact_search_bench.log'), 'w') as fh:
        fh.write('python tools/contact_search_bench.py --batches %s --reps %d --numpy-reps %d --n-iter %d --rounds %d\n' %
                 (' '.join(map(str, args.batches)), args.reps, args.numpy_reps, args.n_iter, args.rounds))
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
