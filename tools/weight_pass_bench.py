#!/usr/bin/env python
"""Microbenchmark of the three weight passes of a training step -- the split-K slab reduction (rih_splitk_reduce_multi), the weight
repack (rih_pack_conv_weight_multi) and the H2 weight planes (rih_h2_multi) -- reference kernel against wide kernel.

The descriptor lists are those of one eager `TrainStep` of bench.py's default workload (ResNet50 + decoder, batch 64, 256 x 256):
the three entry points are wrapped while the step runs and every call's descriptors are copied.  The replay runs on buffers of its
own, of the recorded sizes (the recorded pointers are not used), timed with HIP events, rounds of the reference path
(descriptor field `reserved` = 1) and of the wide path interleaved in one process.  Bytes = what the pass must move (slabs + result,
weights + operand), not what a kernel happens to fetch.

    python tools/weight_pass_bench.py [--batch 64] [--rounds 20] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29         # float4 copy on this part, for scale


class Recorder:
    """stands in for the loaded library: the three entry points copy their descriptor lists, everything else passes through"""
    NAMES = ('rih_splitk_reduce_multi', 'rih_pack_conv_weight_multi', 'rih_h2_multi')

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self.NAMES:
            return fn

        def wrapped(descs, n, stream):
            self.calls.append((name, [{f: getattr(descs[i], f) for f, _ in descs[i]._fields_} for i in range(n)]))
            return fn(descs, n, stream)
        return wrapped


def record(batch):
    import bench
    from renderih_amd import _lib, assets, ops, optim
    from renderih_amd.loss import FusedMeshLoss, GraphLoss, calc_loss_GCN_fused
    from renderih_amd.manolayer import ManoLayer
    from renderih_amd.model import build_model
    from renderih_amd.train import TrainStep
    device = torch.device('cuda', 0)
    torch.manual_seed(0)
    model = build_model(dropout=0.05, encoder_type='resnet50').to(device).train()
    model.decoder.unsample_layer.weight.requires_grad_(False)
    opt = optim.Adam([p for p in model.parameters() if p.requires_grad], lr=3e-4, weight_decay=1e-2)
    mano = {s: ManoLayer(assets.synthetic_mano_dict(s)) for s in ('left', 'right')}
    gl = {s: GraphLoss(mano[s].J_regressor, mano[s].get_faces(), level=4, device=device) for s in ('left', 'right')}
    conv = model.decoder.converter
    fused = FusedMeshLoss(gl['left'], gl['right'], conv['left'], conv['right'])
    img, lab = bench.synth_batch(batch, device, seed=0)

    def loss_fn(out, labels):
        return calc_loss_GCN_fused(fused, None, *out, labels['v2d_l'], labels['v2d_r'], labels['v3d_l'], labels['v3d_r'],
                                   labels['root_rel'])[0]
    step = TrainStep(model, opt, loss_fn, (img, lab), use_graph=False, stages=False, process_group=False)
    step()                      # the first eager step walks the autograd graph once and records the pack cache: list the second
    torch.cuda.synchronize()
    ops._L()                    # make sure the library is loaded before it is wrapped
    real = _lib._lib
    rec = Recorder(real)
    _lib._lib = rec
    try:
        step()
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    return real, rec.calls


def materialise(name, descs, device):
    """(ctypes array on buffers of our own, bytes the pass must move, tensors to keep alive)"""
    from renderih_amd._lib import BOUND_FLOATS, H2Desc, PackDesc, ReduceDesc
    keep, nbytes = [], 0

    def buf(n, fill=None):
        t = torch.randn(n, device=device) if fill is None else torch.full((n,), fill, device=device)
        keep.append(t)
        return t.data_ptr()
    cls = {'rih_splitk_reduce_multi': ReduceDesc, 'rih_pack_conv_weight_multi': PackDesc, 'rih_h2_multi': H2Desc}[name]
    arr = (cls * len(descs))()
    for a, d in zip(arr, descs):
        for f, v in d.items():
            if not isinstance(v, int) or f in ('P', 'dst', 'db', 'w', 'amax'):
                continue
            setattr(a, f, v)
        if name == 'rih_splitk_reduce_multi':
            pitch = d['CinPitch'] or d['CinValid']
            slab, out = d['S'] * d['Mp'] * d['N'], d['N'] * pitch * d['taps']
            a.P, a.dst, a.db = buf(slab), buf(out), (buf(d['N']) if d['db'] else 0)
            rows = d['taps'] * d['CinValid'] + (1 if d['db'] else 0)
            nbytes += 4 * (d['S'] * rows * d['N'] + rows * d['N'] * (2 if d['accumulate'] else 1))
        elif name == 'rih_pack_conv_weight_multi':
            taps = d['KH'] * d['KW'] if d['mode'] == 0 else d['Th'] * d['Tw']
            wn, out = d['Cout'] * d['Cin'] * d['KH'] * d['KW'], taps * d['CinPad'] * d['Cout']
            a.w, a.dst = buf(wn), buf(out)
            nbytes += 4 * (d['Cout'] * d['Cin'] * taps + out)
        else:
            rows = d['CinPad'] if d['for_dgrad'] else d['Cout']
            wn = d['Cout'] * d['Cin'] * d['KH'] * d['KW']
            a.w, a.dst, a.amax = buf(wn), buf(rows * d['Kpad']), buf(BOUND_FLOATS, 1.0)
            nbytes += 4 * (wn + rows * d['Kpad'])
    return arr, nbytes, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('weight_pass_bench.py needs a GPU')
    device = torch.device('cuda', 0)
    lib, calls = record(args.batch)
    torch.cuda.empty_cache()
    stream = torch.cuda.current_stream().cuda_stream
    launches = []
    for name, descs in calls:
        # one call of more than a pack of descriptors is several kernel launches: time each launch (56 descriptors; 48 for H2)
        pack = 48 if name == 'rih_h2_multi' else 56
        for i in range(0, len(descs), pack):
            part = descs[i:i + pack]
            arr, nbytes, keep = materialise(name, part, device)
            note = 'S %d..%d' % (min(d['S'] for d in part), max(d['S'] for d in part)) if 'S' in part[0] else ''
            launches.append({'entry': name, 'n': len(part), 'bytes': nbytes, 'arr': arr, 'keep': keep, 'note': note,
                             'us': {0: [], 1: []}})
    fn = {n: getattr(lib, n) for n in Recorder.NAMES}

    def run(L, reference):
        for a in L['arr']:
            a.reserved = reference
        rc = fn[L['entry']](L['arr'], L['n'], stream)
        assert rc == 0, (L['entry'], rc)
    for L in launches:                  # warm both kernels of every launch
        for reference in (1, 0):
            run(L, reference)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for reference in (1, 0):        # one round of the reference path, one of the wide path, in turn
            marks = []
            for L in launches:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(L, reference)
                e1.record()
                marks.append((e0, e1))
            torch.cuda.synchronize()
            for L, (e0, e1) in zip(launches, marks):
                L['us'][reference].append(1e3 * e0.elapsed_time(e1))
    rows = []

    def med(v):
        return sorted(v)[len(v) // 2]
    print('%-28s %5s %10s %10s %9s %10s %9s' % ('entry point', 'descs', 'MB', 'ref us', 'GB/s', 'wide us', 'GB/s'))
    for L in launches:
        r, w = med(L['us'][1]), med(L['us'][0])
        rows.append({'entry': L['entry'], 'descs': L['n'], 'note': L['note'], 'bytes': L['bytes'], 'reference_us': round(r, 1), 'wide_us': round(w, 1),
                     'reference_GBps': round(L['bytes'] / r / 1e3, 1), 'wide_GBps': round(L['bytes'] / w / 1e3, 1)})
        print('%-28s %5d %10.1f %10.1f %9.0f %10.1f %9.0f   %s' % (L['entry'], L['n'], L['bytes'] / 1e6, r, L['bytes'] / r / 1e3, w,
                                                                   L['bytes'] / w / 1e3, L['note']))
    totals = {}
    for name in Recorder.NAMES:
        sel = [x for x in rows if x['entry'] == name]
        if not sel:
            continue
        b, r, w = sum(x['bytes'] for x in sel), sum(x['reference_us'] for x in sel), sum(x['wide_us'] for x in sel)
        totals[name] = {'launches': len(sel), 'bytes': b, 'reference_us': round(r, 1), 'wide_us': round(w, 1),
                        'reference_GBps': round(b / r / 1e3, 1), 'wide_GBps': round(b / w / 1e3, 1)}
        print('%-28s %5s %10.1f %10.1f %9.0f %10.1f %9.0f   (per step, %d launches)' % (name, '', b / 1e6, r, b / r / 1e3, w,
                                                                                      b / w / 1e3, len(sel)))
    print('for scale: a float4 copy runs at %.2f TB/s on this part; event pairs add 2-4 us per launch' % COPY_TBS)
    result = {'batch': args.batch, 'rounds': args.rounds, 'copy_TBps': COPY_TBS, 'launches': rows, 'per_step': totals}
    if args.json:
        with open(args.json, 'w') as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps({'weight_pass_bench': totals}))


if __name__ == '__main__':
    main()
