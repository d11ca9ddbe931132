#!/usr/bin/env python
"""The demo's image-to-overlay glue (renderih_amd.demo) on the GPU: 480 x 640 frames -> input 256, render size 256 and 512,
B = 1 and 32.

  stages   prepare (fp32 NCHW, and fp16 NHWC8), compose over the frames as backgrounds, other view, smoother: `fused` (one
           launch of csrc/rih_demo.hip) against `mirror` (the same arithmetic in torch ops on the device), us per call: HIP
           events around a window of calls, the variants alternating, --rounds windows after a warm-up; medians and each
           variant's own max - min.  The frames are device-resident for both (the upload is the same 0.9 MB per frame either
           way).  launches: kernels per call, counted by torch's profiler.  bytes: the model of the fused kernel --
           prepare reads 3 (L / S)^2 bytes and writes 12 (fp32) or 16 (fp16) bytes per destination pixel, L = 640 the padded
           side; compose reads 16 (RGBA pitch: rgb 12 + mask 4) + 3 H W / R^2 and writes 3 bytes per pixel -- and the GB/s the
           fused median achieves on it.
  host     the reference's per-image path restated: numpy pad + table resize + normalise + upload for one frame; download of
           the fp32 render and mask + numpy resize of the frame + blend for one overlay.  One timed loop of --host-reps frames,
           host clock, ending in a device synchronise.
  frames   run_model_batch + render_batch (the ResNet-50 network, seeded weights, fp32) in frames per second, against the same
           network and renderer fed and blended by the host path above, one frame at a time.

Prints one JSON line and writes it to <profile-dir>/demo_bench.json (the same line and the windows to .log).
    python tools/demo_bench.py [--profile-dir profiles/demo]
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
    windows, reps = {k: [] for k in calls}, {}
    for k, fn in calls.items():
        fn()
        reps[k] = max(3, int(window_ms * 1e3 / device_window(fn, 3)) + 1)
    for _ in range(rounds):
        for k, fn in calls.items():
            windows[k].append(device_window(fn, reps[k]))
    return {k: float(np.median(v)) for k, v in windows.items()}, {k: float(max(v) - min(v)) for k, v in windows.items()}


def host_resize(img, Sy, Sx):
    """The contract's resize in numpy (what cv.resize does on the host in the reference)."""
    from renderih_amd import demo
    P = img.astype(np.int64)
    if P.shape[:2] == (Sy, Sx):
        return img
    if P.shape[:2] == (2 * Sy, 2 * Sx):
        return ((P[0::2, 0::2] + P[0::2, 1::2] + P[1::2, 0::2] + P[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    ty, tx = demo.axis_table(P.shape[0], Sy).astype(np.int64), demo.axis_table(P.shape[1], Sx).astype(np.int64)
    T = P[ty[:, 0]][:, tx[:, 0]] * tx[:, 2][None, :, None] + P[ty[:, 0]][:, tx[:, 1]] * tx[:, 3][None, :, None]
    U = P[ty[:, 1]][:, tx[:, 0]] * tx[:, 2][None, :, None] + P[ty[:, 1]][:, tx[:, 1]] * tx[:, 3][None, :, None]
    v = (((ty[:, 2][:, None, None] * (T >> 4)) >> 16) + ((ty[:, 3][:, None, None] * (U >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8)


def host_process(img, S, dev):
    """InterRender.process_img as the reference runs it: pad, resize, swap, / 255, normalise on the host, then upload."""
    from renderih_amd import demo
    H, W = img.shape[:2]
    pt, pl, side = demo.pad_to_square(H, W)
    P = np.zeros((side, side, 3), np.uint8)
    P[pt:pt + H, pl:pl + W] = img
    x = torch.tensor(np.ascontiguousarray(host_resize(P, S, S)[..., ::-1]), dtype=torch.float32) / 255
    x = x.permute(2, 0, 1)
    x = (x - torch.tensor(demo.MEAN).view(3, 1, 1)) / torch.tensor(demo.STD).view(3, 1, 1)
    return x.to(dev).unsqueeze(0)


def host_blend(img_out, mask_out, bg, R):
    """InterRender.render lines 89-98 as the reference runs them: download, resize the frame, blend in numpy."""
    img_out = img_out[0].detach().cpu().numpy() * 255
    mask_out = mask_out[0].detach().cpu().numpy()[..., np.newaxis]
    bg = host_resize(bg, R, R)
    return (img_out * mask_out + bg * (1 - mask_out)).astype(np.uint8)


def host_loop(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--profile-dir', default=os.path.join(ROOT, 'profiles', 'demo'))
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 32])
    ap.add_argument('--render-sizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--frame', type=int, nargs=2, default=[480, 640], metavar=('H', 'W'))
    ap.add_argument('--window-ms', type=float, default=200.0)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--host-reps', type=int, default=10)
    ap.add_argument('--no-network', action='store_true', help='skip the frames-per-second section')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'demo_bench needs a GPU'
    from renderih_amd import demo, testing
    from renderih_amd.render import mano_two_hands_renderer
    os.makedirs(args.profile_dir, exist_ok=True)
    dev = torch.device('cuda:0')
    H, W = args.frame
    S, L = 256, max(H, W)
    lines, result = [], {'frame': [H, W], 'input_size': S, 'stages': {}, 'host': {}, 'frames': {}}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def stage(name, calls, nbytes=None):
        us, sp = alternate(calls, args.window_ms, args.rounds)
        row = {'us': us, 'spread': sp, 'launches': {k: launches(fn) for k, fn in calls.items()},
               'mirror_over_fused': us['mirror'] / us['fused']}
        extra = ''
        if nbytes is not None:
            row['bytes'], row['fused_GBps'] = nbytes, nbytes / us['fused'] / 1e3
            extra = '; %.2f MB model = %.0f GB/s' % (nbytes / 1e6, row['fused_GBps'])
        result['stages'][name] = row
        say('%-28s fused %9.1f us (spread %.1f, %d launches%s), mirror %9.1f us (spread %.1f, %d launches), ratio %.1f'
            % (name, us['fused'], sp['fused'], row['launches']['fused'], extra, us['mirror'], sp['mirror'],
               row['launches']['mirror'], row['mirror_over_fused']))

    rs = np.random.RandomState(0)
    for B in args.batches:
        frames_np = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
        frames = torch.from_numpy(frames_np).to(dev)
        n, h, _ = demo.prepare(frames, S, dev, h8=True)
        mn, mh, _ = demo.prepare_mirror(frames, S, dev)
        assert torch.equal(n, mn) and torch.equal(h, mh)
        px = B * S * S
        stage('prepare fp32 B=%d' % B, {'fused': lambda: demo.prepare(frames, S, dev),
                                       'mirror': lambda: demo.prepare_mirror(frames, S, dev)}, px * (3 * (L / S) ** 2 + 12))
        stage('prepare fp16 B=%d' % B, {'fused': lambda: demo.prepare(frames, S, dev, norm=False, h8=True),
                                       'mirror': lambda: demo.prepare_mirror(frames, S, dev)}, px * (3 * (L / S) ** 2 + 16))
        for R in args.render_sizes:
            rgba = torch.rand((B, R, R, 4), generator=torch.Generator().manual_seed(R)).to(dev)
            rgb, mask = rgba[..., :3], rgba[..., 3]
            assert torch.equal(demo.compose(rgb, mask, frames), demo.compose_mirror(rgb, mask, frames))
            stage('compose R=%d B=%d' % (R, B), {'fused': lambda: demo.compose(rgb, mask, frames),
                                                  'mirror': lambda: demo.compose_mirror(rgb, mask, frames)},
                  B * R * R * (16 + 3 * H * W / R ** 2 + 3))
        vl, vr = torch.randn(B, 778, 3, device=dev) * 0.05, torch.randn(B, 778, 3, device=dev) * 0.05
        stage('other view B=%d' % B, {'fused': lambda: demo.other_view(vl, vr, 60), 'mirror': lambda: demo.other_view_mirror(vl, vr, 60)},
              B * 778 * 2 * 3 * 4 * 2)
        params = {'scale_left': torch.rand(B, device=dev), 'trans2d_left': torch.rand(B, 2, device=dev),
                  'scale_right': torch.rand(B, device=dev), 'trans2d_right': torch.rand(B, 2, device=dev),
                  'v3d_left': vl, 'v3d_right': vr, 'otherInfo': {}}
        sm, smm = demo.ParamSmoother(), demo.ParamSmootherMirror()
        for _ in range(4):                                            # past the first three frames: the prediction runs
            sm(params), smm(params)
        stage('smoother B=%d' % B, {'fused': lambda: sm(params), 'mirror': lambda: smm(params)})

    # ---- the reference's host path, one frame
    frame = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    for R in args.render_sizes:
        rgba = torch.rand((1, R, R, 4), generator=torch.Generator().manual_seed(R)).to(dev)
        rgb, mask = (rgba[..., :3] / 1).contiguous(), rgba[..., 3].contiguous()
        result['host']['blend R=%d' % R] = host_loop(lambda: host_blend(rgb, mask, frame, R), args.host_reps)
        say('host blend R=%d (download %.1f MB fp32 + numpy resize + blend): %.0f us per frame'
            % (R, R * R * 16 / 1e6, result['host']['blend R=%d' % R]))
    result['host']['process'] = host_loop(lambda: host_process(frame, S, dev), args.host_reps)
    say('host process_img (numpy pad + resize + normalise + upload): %.0f us per frame' % result['host']['process'])

    # ---- frames per second with the network
    if not args.no_network:
        from renderih_amd.model import build_model
        net = build_model(dropout=0.0)
        net.load_state_dict(testing.deterministic_state(net.state_dict(), seed=1))
        for R in args.render_sizes:
            ir = demo.InterRender(input_size=S, render_size=R, model=net, device=dev,
                                  renderer=mano_two_hands_renderer(mano_path={'left': None, 'right': None}, img_size=R, device=dev))
            for B in args.batches:
                frames_np = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)

                def fused():
                    return ir.render_batch(ir.run_model_batch(frames_np), bg_imgs=frames_np)

                def host():
                    with torch.no_grad():
                        for b in range(B):
                            result_, pd, _, _ = ir.model(host_process(frames_np[b], S, dev))
                            img_out, mask_out = ir.renderer.render_rgb_orth(
                                scale_left=pd['scale']['left'], trans2d_left=pd['trans2d']['left'], scale_right=pd['scale']['right'],
                                trans2d_right=pd['trans2d']['right'], v3d_left=result_['verts3d']['left'],
                                v3d_right=result_['verts3d']['right'])
                            host_blend(img_out, mask_out, frames_np[b], R)
                reps = max(2, 64 // B)
                fused(), host()
                t_f = [host_loop(fused, reps) for _ in range(args.rounds)]
                t_h = [host_loop(host, max(1, reps // 4)) for _ in range(args.rounds)]
                row = {'fused_fps': B * 1e6 / float(np.median(t_f)), 'host_fps': B * 1e6 / float(np.median(t_h)),
                       'fused_us': t_f, 'host_us': t_h}
                result['frames']['R=%d B=%d' % (R, B)] = row
                say('frames R=%d B=%d (upload included): batched %.1f frames/s (%.0f us per call, %s), host path one frame at a '
                    'time %.1f frames/s (%s)' % (R, B, row['fused_fps'], float(np.median(t_f)), ' '.join('%.0f' % t for t in t_f),
                                                 row['host_fps'], ' '.join('%.0f' % t for t in t_h)))
    line = json.dumps(result)
    print(line)
    with open(os.path.join(args.profile_dir, 'demo_bench.json'), 'w') as fh:
        fh.write(line + '\n')
    with open(os.path.join(args.profile_dir, 'demo_bench.log'), 'w') as fh:
        fh.write('\n'.join(lines + [line]) + '\n')


if __name__ == '__main__':
    main()
