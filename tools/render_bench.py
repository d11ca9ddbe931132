#!/usr/bin/env python
"""Two-hand renderer micro-benchmark (csrc/rih_render.hip): microseconds per call of rih_render_setup, rih_render_raster,
rih_render_shade and of the whole mano_two_hands_renderer.render_rgb_orth (camera build, right-hand mapping, colour
expansion, the three launches, the /255), for B in {1, 64, 256}, 256^2 and 512^2, Phong and ambient lighting.  HIP events on
the current stream after a warm-up, median of 5 windows of --iters calls.  Prints one JSON line.

Algorithmic bytes per call (for the roofline): setup reads B V 12 + F 12 (+ the CSR) and writes B F 64 (+ B V 12 normals);
raster reads the B F 64 face records once per 32 x 32 tile and writes B S^2 20 bytes of fragments; shade reads those 20
bytes (+ the gathered vertex data) and writes B S^2 16 bytes of RGBA.
    python tools/render_bench.py [--iters 20] [--batches 1 64 256] [--sizes 256 512] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
from renderih_amd import render          # noqa: E402
import render_cases as rc                # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    res = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res.append(e0.elapsed_time(e1) * 1e3 / iters)
    res.sort()
    return round(res[2], 2)


def measure(B, S, light, iters):
    dev = 'cuda'
    r = render.mano_two_hands_renderer(img_size=S, device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    vl, vr, sl, tl, sr, tr = (t(a) for a in rc.ortho_scene(B, seed=11, overlap=True))
    vr_cam = t(rc.right_in_left_camera(*(a.cpu().numpy() for a in (vr, sl, tl, sr, tr))))
    verts = torch.cat([vl, vr_cam], 1).contiguous()
    cam = render.orthographic_camera(sl, tl)
    verts, topo, B_, V = render._prepare(verts, r._faces, cam)
    F = topo[0].shape[0]
    point = light == 'point'
    colors = r._default_colors().to(dev).expand(B, V, 3).contiguous()
    rec, vn = render._setup(verts, topo, cam, B, V, normals=point)
    frags = render._raster(rec, B, F, S, cam.kind, dev)
    out = {'B': B, 'S': S, 'light': light}
    out['setup_us'] = timed(lambda: render._setup(verts, topo, cam, B, V, normals=point), iters)
    out['raster_us'] = timed(lambda: render._raster(rec, B, F, S, cam.kind, dev), iters)
    out['shade_us'] = timed(lambda: render._shade(frags, verts, topo, vn, colors, light, cam, B, V), iters)
    out['render_rgb_orth_us'] = timed(lambda: r.render_rgb_orth(sl, tl, sr, tr, vl, vr, amblights=not point), iters)
    out['covered'] = round((frags.pix_to_face >= 0).float().mean().item(), 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 64, 256])
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--json', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'render_bench needs the GPU'
    rows = []
    with torch.no_grad():
        for S in a.sizes:
            for B in a.batches:
                for light in ('point', 'ambient'):
                    rows.append(measure(B, S, light, a.iters))
                    print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    line = json.dumps({'tool': 'render_bench', 'device': torch.cuda.get_device_name(0), 'iters': a.iters, 'rows': rows})
    print(line)
    if a.json:
        with open(a.json, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
