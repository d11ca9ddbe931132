#!/usr/bin/env python
"""The auxiliary heads of renderih_amd.aux_heads on the GPU.

  loss     calc_aux_loss at S = 64, Jh = 42, B in --batches (default 2 64), both heat-map label forms ('tensor': a label tensor
           is read; 'joints': the target is produced in the kernel): `fused` (rih_aux_loss + rih_aux_loss_final; backward =
           one torch._foreach_mul over the saved gradients) against `mirror` (the plain-torch AuxLoss on the device, autograd
           backward).  us per forward and per forward + backward: HIP events around a window of calls, the variants
           alternating, --rounds windows each after a warm-up; medians and each variant's own max - min.  A window holds as
           many calls as fill --window-ms (default 300 ms), counted from one short trial window per variant.  launches: kernels per forward +
           backward, counted by torch's profiler.  bytes: the model of the fused FORWARD (which also writes the gradients) --
           every prediction, label and gradient plane once, 4 B an element: (Jh + 8) + 5 [+ Jh] planes read, Jh + 8 written --
           and the GB/s the fused forward median achieves on it.
  decode   get_final_preds2 on 42 B maps of 64 x 64, kernel 5: `fused` (rih_hms_decode, one launch), `mirror` (vectorised torch
           on the device) and `host`, the reference's way restated here: the maps copied to the host, then a Python loop over
           the joints with np.matrix inverses (inference.py:51-69, 72-86 with the fixed 5-tap blur in numpy).
  step     one eager training step (forward, loss, backward, Adam) of the ResNet-50 model at B = --step-batch (default 64),
           with calc_loss_GCN_fused alone and with aux=FusedAuxLoss() (joints label), alternating.

Prints one JSON line and writes it to <profile-dir>/aux_heads_bench.json (the same line and the windows to .log).
    python tools/aux_heads_bench.py [--profile-dir profiles/aux_heads]

Kernel times (a run of its own, the profiler slows the host): --probe only issues the kernels -- 20 calls of the fused loss with
the tensor label, 20 of the decoder, 20 of the fused loss with the joints label, B = 64 -- and --summarize reads the trace:
    rocprofv3 --kernel-trace --stats -d <dir> -o aux -- python tools/aux_heads_bench.py --probe
    python tools/aux_heads_bench.py --summarize <dir>/aux_results.db       # writes <profile-dir>/kernel_trace.txt
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


def alternate(calls, window_ms, rounds):
    """{name: fn} -> ({name: median us}, {name: max - min}); every window lasts about window_ms."""
    windows = {k: [] for k in calls}
    reps = {}
    for k, fn in calls.items():
        fn()
        reps[k] = max(3, int(window_ms * 1e3 / device_window(fn, 5)) + 1)
    for _ in range(rounds):
        for k, fn in calls.items():
            windows[k].append(device_window(fn, reps[k]))
    return {k: float(np.median(v)) for k, v in windows.items()}, {k: float(max(v) - min(v)) for k, v in windows.items()}


def host_decode(hm_dev, kernel=5):
    """The reference's path: device -> host, blur per map, log, and a Python loop with np.matrix over every joint."""
    hm = hm_dev.detach().cpu().numpy().copy()
    N, J, H, W = hm.shape
    flat = hm.reshape(N, J, -1)
    idx, maxvals = flat.argmax(2), flat.max(2)
    coords = np.stack([idx % W, idx // W], -1).astype(np.float32) * (maxvals > 0)[..., None]
    taps, r = np.array([1, 4, 6, 4, 1]) / 16.0, kernel // 2
    for i in range(N):
        for j in range(J):
            m0 = hm[i, j].max()
            p = np.zeros((H + 4 * r, W + 4 * r))
            p[2 * r:-2 * r, 2 * r:-2 * r] = hm[i, j]
            rows = sum(taps[a] * p[:, a:a + W + 2 * r] for a in range(kernel))
            b = sum(taps[a] * rows[a:a + H + 2 * r] for a in range(kernel))[r:-r, r:-r]
            hm[i, j] = b * (m0 / b.max())
    hm = np.log(np.maximum(hm, 1e-10))
    for i in range(N):
        for j in range(J):
            m, px, py = hm[i, j], int(coords[i, j, 0]), int(coords[i, j, 1])
            if 1 < px < W - 2 and 1 < py < H - 2:
                dx, dy = 0.5 * (m[py][px + 1] - m[py][px - 1]), 0.5 * (m[py + 1][px] - m[py - 1][px])
                dxx = 0.25 * (m[py][px + 2] - 2 * m[py][px] + m[py][px - 2])
                dxy = 0.25 * (m[py + 1][px + 1] - m[py - 1][px + 1] - m[py + 1][px - 1] + m[py - 1][px - 1])
                dyy = 0.25 * (m[py + 2][px] - 2 * m[py][px] + m[py - 2][px])
                if dxx * dyy - dxy ** 2 != 0:
                    off = -np.matrix([[dxx, dxy], [dxy, dyy]]).I * np.matrix([[dx], [dy]])
                    coords[i, j] += np.squeeze(np.array(off.T), axis=0)
    return coords, maxvals


def probe_inputs(B, Jh, S, dev):
    from renderih_amd import aux_heads as ah
    g = torch.Generator().manual_seed(B)
    joints = torch.cat([S * torch.rand(B, Jh, 2, generator=g), torch.ones(B, Jh, 1)], -1).to(dev)
    t_hms = ah.FusedHeatmapGenerator(S, ah.HEATMAP_SIGMA)(joints)
    t_mask = (torch.rand(B, 2, S, S, generator=g) < 0.3).float().to(dev)
    t_dense = torch.rand(B, 3, S, S, generator=g).to(dev)
    pred = {'hms': t_hms + 0.1 * torch.randn(B, Jh, S, S, generator=g).to(dev),
            'mask': t_mask + 0.1 * torch.randn(B, 2, S, S, generator=g).to(dev), 'dense': torch.rand(B, 6, S, S, generator=g).to(dev)}
    return joints, t_hms, t_mask, t_dense, pred


def probe(B=64, calls=20):
    """The kernels alone, in an order --summarize relies on: loss (tensor label), decoder, loss (joints label)."""
    from renderih_amd import aux_heads as ah
    dev = torch.device('cuda:0')
    joints, t_hms, t_mask, t_dense, pred = probe_inputs(B, 42, ah.HEATMAP_SIZE, dev)
    loss, dec = ah.FusedAuxLoss(), ah.FusedHeatmapDecoder(ah.BLUR_KERNEL)
    for _ in range(calls):
        loss(pred, t_mask, t_dense, hms=t_hms)
    torch.cuda.synchronize()
    for _ in range(calls):
        dec(pred['hms'])
    torch.cuda.synchronize()
    for _ in range(calls):
        loss(pred, t_mask, t_dense, joints2d=joints, sigma=ah.HEATMAP_SIGMA)
    torch.cuda.synchronize()
    print('probe done: B = %d, %d calls each' % (B, calls))


def summarize(db, out):
    """Median / min / max duration per kernel of this file's three from a --probe trace (the first two calls left out)."""
    import collections
    import sqlite3
    rows = sqlite3.connect(db).execute('select name, start, end, grid_x, workgroup_x from kernels order by start').fetchall()
    agg, after_decoder = collections.OrderedDict(), False
    for name, start, end, gx, wx in rows:
        kind = next((k for k in ('aux_loss_final_kernel', 'aux_loss_kernel', 'decode_kernel') if k in name), None)
        if kind is None:
            continue
        after_decoder = after_decoder or kind == 'decode_kernel'
        label = ('joints label' if after_decoder else 'tensor label') if kind.startswith('aux_loss') else ''
        agg.setdefault((kind, label, gx // max(wx, 1)), []).append((end - start) / 1e3)
    lines = ['rocprofv3 --kernel-trace --stats of `tools/aux_heads_bench.py --probe`: B = 64, Jh = 42, S = 64; the first two calls left out']
    for (kind, label, wgs), v in agg.items():
        v = v[2:]
        lines.append('%-22s %-13s %5d workgroups, %2d calls: median %.2f us, min %.2f, max %.2f'
                     % (kind, label, wgs, len(v), float(np.median(v)), min(v), max(v)))
    with open(out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'aux_heads'))
    ap.add_argument('--batches', type=int, nargs='+', default=[2, 64])
    ap.add_argument('--step-batch', type=int, default=64)
    ap.add_argument('--window-ms', type=float, default=300.0)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--probe', action='store_true', help='only issue the kernels, for a kernel trace')
    ap.add_argument('--summarize', default=None, metavar='DB', help="a rocprofv3 results database of a --probe run")
    args = ap.parse_args()
    os.makedirs(args.profile_dir, exist_ok=True)
    if args.summarize:
        return summarize(args.summarize, os.path.join(args.profile_dir, 'kernel_trace.txt'))
    if args.probe:
        return probe()
    from renderih_amd import aux_heads as ah
    assert torch.cuda.is_available(), 'aux_heads_bench needs a GPU'
    dev = torch.device('cuda:0')
    S, Jh = ah.HEATMAP_SIZE, 42
    lines, result = [], {'S': S, 'Jh': Jh, 'loss': {}, 'decode': {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        joints = torch.cat([S * torch.rand(B, Jh, 2, generator=g), torch.ones(B, Jh, 1)], -1).to(dev)
        t_hms = ah.FusedHeatmapGenerator(S, ah.HEATMAP_SIGMA)(joints)
        t_mask = (torch.rand(B, 2, S, S, generator=g) < 0.3).float().to(dev)
        t_dense = torch.rand(B, 3, S, S, generator=g).to(dev)
        pred = {'hms': (t_hms + 0.1 * torch.randn(B, Jh, S, S, generator=g).to(dev)).requires_grad_(True),
                'mask': (t_mask + 0.1 * torch.randn(B, 2, S, S, generator=g).to(dev)).requires_grad_(True),
                'dense': torch.rand(B, 6, S, S, generator=g).to(dev).requires_grad_(True)}
        plist = list(pred.values())
        losses = {'fused': ah.FusedAuxLoss(), 'mirror': ah.AuxLoss()}
        plane = B * S * S * 4
        for form in ('tensor', 'joints'):
            kw = dict(hms=t_hms) if form == 'tensor' else dict(joints2d=joints, sigma=ah.HEATMAP_SIGMA)
            fwd = {k: (lambda k=k: losses[k](pred, t_mask, t_dense, **kw)[0]) for k in losses}
            both = {k: (lambda k=k: torch.autograd.grad(fwd[k](), plist)) for k in losses}
            a, b = fwd['fused']().item(), fwd['mirror']().item()
            assert abs(a - b) <= 1e-5 * abs(b), (a, b)
            f_us, f_sp = alternate(fwd, args.window_ms, args.rounds)
            b_us, b_sp = alternate(both, args.window_ms, args.rounds)
            read = (Jh + 8 + 5 + (Jh if form == 'tensor' else 0)) * plane
            written = (Jh + 8) * plane
            row = {'forward_us': f_us, 'forward_spread': f_sp, 'fwd_bwd_us': b_us, 'fwd_bwd_spread': b_sp,
                   'launches_fwd_bwd': {k: launches(fn) for k, fn in both.items()}, 'bytes_read': read, 'bytes_written': written,
                   'fused_forward_GBps': (read + written) / f_us['fused'] / 1e3, 'mirror_over_fused_fwd_bwd': b_us['mirror'] / b_us['fused']}
            result['loss']['B%d/%s' % (B, form)] = row
            say('loss B=%d %s label: forward fused %.1f us (spread %.1f; %.1f MB read + %.1f MB written = %.0f GB/s), mirror %.1f us; '
                'forward+backward fused %.1f us (spread %.1f, %d launches), mirror %.1f us (spread %.1f, %d launches), ratio %.1f'
                % (B, form, f_us['fused'], f_sp['fused'], read / 1e6, written / 1e6, row['fused_forward_GBps'], f_us['mirror'],
                   b_us['fused'], b_sp['fused'], row['launches_fwd_bwd']['fused'], b_us['mirror'], b_sp['mirror'],
                   row['launches_fwd_bwd']['mirror'], row['mirror_over_fused_fwd_bwd']))
        # ---- decoder on the network-like maps (the noisy labels)
        hm = pred['hms'].detach()
        dec = {'fused': (lambda: ah.FusedHeatmapDecoder(ah.BLUR_KERNEL)(hm)), 'mirror': (lambda: ah.decode_heatmaps(hm, ah.BLUR_KERNEL))}
        d_us, d_sp = alternate(dec, args.window_ms, args.rounds)
        t0 = time.perf_counter()
        want, _ = host_decode(hm, ah.BLUR_KERNEL)
        host_us = (time.perf_counter() - t0) * 1e6
        err = float(np.abs(dec['fused']()[0].cpu().numpy() - want).max())
        row = {'maps': B * Jh, 'us': d_us, 'spread': d_sp, 'host_loop_us': host_us, 'launches': {k: launches(fn) for k, fn in dec.items()},
               'bytes': B * Jh * S * S * 4, 'fused_GBps': B * Jh * S * S * 4 / d_us['fused'] / 1e3, 'max_abs_vs_host_px': err}
        result['decode']['B%d' % B] = row
        say('decode %d maps: fused %.1f us (spread %.1f, %d launch, %.0f GB/s on the maps), mirror %.1f us (%d launches), host loop '
            '%.0f us (one run, copy included); fused against the host loop: %.2e px'
            % (B * Jh, d_us['fused'], d_sp['fused'], row['launches']['fused'], row['fused_GBps'], d_us['mirror'],
               row['launches']['mirror'], host_us, err))

    # ---- one eager training step with and without the aux term
    from renderih_amd import assets, optim as rih_optim
    from renderih_amd.loss import FusedMeshLoss, GraphLoss, calc_loss_GCN_fused
    from renderih_amd.manolayer import ManoLayer
    from renderih_amd.model import build_model
    B = args.step_batch
    torch.manual_seed(0)
    model = build_model(dropout=0.05).to(dev).train()
    model.decoder.unsample_layer.weight.requires_grad_(False)
    opt = rih_optim.Adam([p for p in model.parameters() if p.requires_grad], lr=3e-4, weight_decay=1e-2)
    mano = {s: ManoLayer(assets.synthetic_mano_dict(s)) for s in ('left', 'right')}
    gl = {s: GraphLoss(mano[s].J_regressor, mano[s].get_faces(), level=4, device=dev) for s in ('left', 'right')}
    conv = model.decoder.converter
    mesh = FusedMeshLoss(gl['left'], gl['right'], conv['left'], conv['right'])
    aux = ah.FusedAuxLoss()
    g = torch.Generator().manual_seed(1)
    img = torch.randn(B, 3, 256, 256, generator=g).to(dev)
    lab = {'v3d_l': 0.05 * torch.randn(B, 778, 3, generator=g), 'v3d_r': 0.05 * torch.randn(B, 778, 3, generator=g),
           'v2d_l': 256 * torch.rand(B, 778, 2, generator=g), 'v2d_r': 256 * torch.rand(B, 778, 2, generator=g),
           'root_rel': 0.05 * torch.randn(B, 3, generator=g), 'mask': (torch.rand(B, 2, S, S, generator=g) < 0.3).float(),
           'dense': torch.rand(B, 3, S, S, generator=g), 'joints': torch.cat([S * torch.rand(B, 42, 2, generator=g), torch.ones(B, 42, 1)], -1)}
    lab = {k: v.to(dev) for k, v in lab.items()}

    def step(with_aux):
        opt.zero_grad(set_to_none=True)
        out = model(img)
        kw = dict(aux=aux, mask=lab['mask'], dense=lab['dense'], joints2d=lab['joints'], sigma=ah.HEATMAP_SIGMA) if with_aux else {}
        loss = calc_loss_GCN_fused(mesh, None, *out, lab['v2d_l'], lab['v2d_r'], lab['v3d_l'], lab['v3d_r'], lab['root_rel'], **kw)[0]
        loss.backward()
        opt.step()
    steps = {'mesh loss only': (lambda: step(False)), 'with the aux term': (lambda: step(True))}
    for fn in steps.values():
        fn()
        fn()
    s_us, s_sp = alternate(steps, args.window_ms, args.rounds)
    result['step'] = {'B': B, 'us': s_us, 'spread': s_sp, 'aux_cost_us': s_us['with the aux term'] - s_us['mesh loss only']}
    say('eager training step B=%d: mesh loss only %.0f us (spread %.0f), with the aux term %.0f us (spread %.0f): %+.0f us'
        % (B, s_us['mesh loss only'], s_sp['mesh loss only'], s_us['with the aux term'], s_sp['with the aux term'],
           result['step']['aux_cost_us']))
    line = json.dumps(result)
    print(line)
    with open(os.path.join(args.profile_dir, 'aux_heads_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'aux_heads_bench.log'), 'w') as fh:
        fh.write('\n'.join(lines + [line]) + '\n')


if __name__ == '__main__':
    main()
