#!/usr/bin/env python
"""Fused MANO-head loss (csrc/rih_mano_loss.hip, renderih_amd.loss.FusedManoLoss) against the torch mirror of
core/Loss_mano.py, and what it does to a training step.  Prints one JSON line.

  loss_us          microseconds per evaluation, forward + backward of the loss alone, at --batch (default 64): the fused
                   kernels against the torch mirror.  HIP events on the current stream after a warm-up, median of 5 windows
                   of --iters evaluations.
  train_step       images/s of the `load_new_model` TrainStep (one captured hipGraph, renderih_amd Adam) with FusedManoLoss
                   (the reference's recipe for this model) next to the same step with FusedMeshLoss (the family-(a)
                   GraphLoss recipe that `bench.py --family b-mano` times).  The two steps alternate, --rounds windows of
                   --steps steps each, on one box; medians.

    python tools/mano_loss_bench.py [--batch 64] [--iters 20] [--steps 10] [--rounds 5] [--no-train] [--json out.json]
Under `rocprofv3 --kernel-trace --stats -- python tools/mano_loss_bench.py --count-launches mirror|fused` it runs ten
evaluations of one loss only (after the set-up of inputs and topology, whose few launches the trace also holds)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from renderih_amd import assets  # noqa: E402


def hand_losses(device):
    from renderih_amd.loss import ManoLoss
    from renderih_amd.manolayer import ManoLayer
    out = {}
    for s in ('left', 'right'):
        m = ManoLayer(assets.synthetic_mano_dict(s))
        out[s] = ManoLoss(m.J_regressor, m.get_faces(), level=4, device=device)
    return out


def labels(B, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    lab = {'v3d_l': 0.05 * torch.randn(B, 778, 3, generator=g), 'v3d_r': 0.05 * torch.randn(B, 778, 3, generator=g),
           'v2d_l': 256 * torch.rand(B, 778, 2, generator=g), 'v2d_r': 256 * torch.rand(B, 778, 2, generator=g),
           'root_rel': 0.05 * torch.randn(B, 3, generator=g), 'lp': 0.5 * torch.randn(B, 48, generator=g),
           'ls': torch.randn(B, 10, generator=g), 'rp': 0.5 * torch.randn(B, 48, generator=g),
           'rs': torch.randn(B, 10, generator=g)}
    return {k: v.to(device) for k, v in lab.items()}


def predictions(B, device, seed=1):
    g = torch.Generator().manual_seed(seed)
    p = {}
    for s in ('left', 'right'):
        p['v3d_' + s] = 0.05 * torch.randn(B, 778, 3, generator=g)
        p['v2d_' + s] = 256 * torch.rand(B, 778, 2, generator=g)
        p['pose_' + s] = 0.5 * torch.randn(B, 48, generator=g)
        p['shape_' + s] = torch.randn(B, 10, generator=g)
    p['root_rel'] = 0.05 * torch.randn(B, 3, generator=g)
    return {k: v.to(device).requires_grad_(True) for k, v in p.items()}


def model_outputs(p):
    result = {'verts3d': {s: p['v3d_' + s] for s in ('left', 'right')}, 'verts2d': {s: p['v2d_' + s] for s in ('left', 'right')}}
    other = {'root_rel': p['root_rel'],
             'verts3d_MANO_list': {s: {'mano_pose': p['pose_' + s], 'mano_shape': p['shape_' + s]} for s in ('left', 'right')}}
    return result, None, [], other


def loss_args(out, lab):
    result, paramsDict, handDictList, otherInfo = out
    return (None, None, result, paramsDict, handDictList, otherInfo, None, None, None, lab['v2d_l'], None, lab['v2d_r'], None,
            lab['v3d_l'], None, lab['v3d_r'], None, lab['root_rel'], 256, lab['lp'], lab['ls'], lab['rp'], lab['rs'])


def loss_step(kind, losses, fused, out, lab, epoch=60):
    from renderih_amd.loss import mano_loss_GCN, mano_loss_GCN_fused
    if kind == 'fused':
        total = mano_loss_GCN_fused(fused, epoch, losses['left'], losses['right'], *loss_args(out, lab))[0]
    else:
        total = mano_loss_GCN(None, epoch, losses['left'], losses['right'], *loss_args(out, lab))[0]
    total.backward()


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
    return round(res[len(res) // 2], 1)


def train_steps(B, steps, rounds, warmup=3):
    """The load_new_model TrainStep with each loss, alternating windows; images/s medians."""
    from renderih_amd import optim as rih_optim
    from renderih_amd.lijun import build_new_model
    from renderih_amd.loss import FusedManoLoss, FusedMeshLoss, calc_loss_GCN_fused, mano_loss_GCN_fused
    from renderih_amd.train import TrainStep
    dev = torch.device('cuda', 0)
    losses = hand_losses(dev)
    g = torch.Generator().manual_seed(0)
    img = torch.randn(B, 3, 256, 256, generator=g).to(dev)
    lab = labels(B, dev)
    trainers = {}
    for kind in ('mano', 'mesh'):
        torch.manual_seed(0)
        model = build_new_model(dropout=0.05).to(dev).train()
        model.decoder.unsample_layer.weight.requires_grad_(False)
        opt = rih_optim.Adam([p for p in model.parameters() if p.requires_grad], lr=3e-4, weight_decay=1e-2)
        if kind == 'mano':
            fused = FusedManoLoss(losses['left'], losses['right'])

            def loss_fn(out, labels, fused=fused):
                return mano_loss_GCN_fused(fused, None, losses['left'], losses['right'], *loss_args(out, labels))[0]
        else:
            conv = model.decoder.converter
            fm = FusedMeshLoss(losses['left'], losses['right'], conv['left'], conv['right'])     # ManoLoss is a GraphLoss

            def loss_fn(out, labels, fm=fm):
                return calc_loss_GCN_fused(fm, None, *out, labels['v2d_l'], labels['v2d_r'], labels['v3d_l'],
                                           labels['v3d_r'], labels['root_rel'])[0]
        trainers[kind] = TrainStep(model, opt, loss_fn, (img, lab))
        for _ in range(warmup):
            trainers[kind]()
    torch.cuda.synchronize()
    ips = {k: [] for k in trainers}
    for _ in range(rounds):
        for kind, st in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                st()
            torch.cuda.synchronize()
            ips[kind].append(B * steps / (time.perf_counter() - t0))
    med = {k: round(float(np.median(v)), 1) for k, v in ips.items()}
    return {'batch': B, 'graph': all(t.use_graph for t in trainers.values()),
            'images_per_sec_fused_mano_loss': med['mano'], 'images_per_sec_fused_mesh_loss': med['mesh'],
            'windows': {k: [round(x, 1) for x in v] for k, v in ips.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-train', action='store_true')
    ap.add_argument('--count-launches', choices=['mirror', 'fused'])
    ap.add_argument('--json')
    args = ap.parse_args()
    from renderih_amd import _lib
    from renderih_amd.loss import FusedManoLoss
    _lib.load()
    dev = torch.device('cuda', 0)
    B = args.batch
    losses = hand_losses(dev)
    fused = FusedManoLoss(losses['left'], losses['right'])
    p = predictions(B, dev)
    lab = labels(B, dev)
    out = model_outputs(p)
    if args.count_launches:
        for _ in range(10):
            loss_step(args.count_launches, losses, fused, out, lab)
        torch.cuda.synchronize()
        print(json.dumps({'count_launches': args.count_launches, 'evaluations': 10, 'batch': B}))
        return
    res = {'tool': 'mano_loss_bench', 'batch': B,
           'loss_us': {'fused': timed(lambda: loss_step('fused', losses, fused, out, lab), args.iters),
                       'mirror': timed(lambda: loss_step('mirror', losses, fused, out, lab), args.iters)},
           'what': 'forward + backward of mano_loss_GCN at epoch 60; fused = rih_mano_loss x 2 + rih_mano_loss_final + '
                   'the _foreach_mul of the backward'}
    res['loss_speedup'] = round(res['loss_us']['mirror'] / res['loss_us']['fused'], 1)
    if not args.no_train:
        res['train_step'] = train_steps(B, args.steps, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
