"""The pose optimiser's NatureLoss on the GPU (renderih_amd.nature.FusedTwoHandNatureLoss, csrc/rih_nature.hip) at the
reference's hidden width 512: the fused launches against the reference's golden and against the fp64 mirror at B = 1, 3 and 32,
and forward plus backward captured in a graph and replayed on another batch.  Helpers, cases and bars: tests/nature_cases.py.

Measured for the loss / terms bar on an MI355X (profiles/nature_loss/deviation_gpu.log): the fp32 torch mirror deviates from the
fp64 mirror by at most 1.04e-7 over the GPU cases (golden case c); the fused kernels were then found at most 2.2e-7 from the
golden and 2.4e-7 from the fp64 mirror (B = 1).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import nature_cases as nc  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', nc.GOLDEN_CASES)
def test_fused_kernels_match_reference_golden(name):
    case = nc.golden_case(name)
    got = nc.fused_vs(case, dev(), 'fused vs golden ' + name)
    want64 = nc.evaluate(nc.module(nc.mirror_cls(), case['H'], case['pred_scale'], case['seed']), case, 'cpu', torch.float64)
    nc.compare(got, want64, 'fused vs fp64 mirror, golden ' + name)
    if name == 'b':                                                     # the empty side: exactly 0, value and gradient
        assert got['terms'][0] == 0 and got['terms'][2] == 0 and not got['grad_q_r'].any() and got['loss'] == got['terms'][1]


@pytest.mark.parametrize('B,H,scale', nc.GPU_CASES)
def test_fused_kernels_match_fp64_mirror(B, H, scale):
    case = nc.seeded_case(B, H, scale)
    got = nc.fused_vs(case, dev(), 'fused vs fp64 mirror B=%d H=%d scale %g' % (B, H, scale))
    if scale != 1.0:
        assert 0 < got['terms'][2] + got['terms'][3] < 2 * B           # rows on both sides of the mask


def test_both_masks_empty_give_exact_zeros():
    case = nc.seeded_case(3, 512, 8.0)
    got = nc.evaluate(nc.module(nc.fused_cls(), 512, 8.0, case['seed'], bias1=20.0), case, dev())
    assert got['loss'] == 0 and not got['terms'].any() and not got['grad_q_r'].any() and not got['grad_q_l'].any()


def test_captured_graph_replays_on_another_batch_bit_for_bit():
    """Forward and backward in one torch.cuda.graph; the second batch has other masks and counts, which live on the device."""
    first = nc.seeded_case(32, 512, 8.0)
    B = 32
    # the second batch, from rows of the first (so every row stays decided): the left hands as right hands, and one judged
    # right hand as every left hand -- other masks, and a left count of B
    judged = int(np.flatnonzero(first['want']['outputs'][0, :, 1] < 0.6)[0])
    second = {'q_r': first['q_l'], 'q_l': np.tile(first['q_r'][judged:judged + 1], (B, 1, 1))}
    mod = nc.module(nc.fused_cls(), 512, 8.0, first['seed']).to(dev())
    static = [torch.from_numpy(first[k]).to(dev()).requires_grad_(True) for k in ('q_r', 'q_l')]

    def run():
        loss, terms = mod(*static)
        grads = torch.autograd.grad(loss * nc.UPSTREAM, static)
        return loss, terms, grads[0], grads[1]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                           # packs the weights, warms the allocator
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    results = {}
    for name, case in (('first', first), ('second', second)):
        with torch.no_grad():
            for t, k in zip(static, ('q_r', 'q_l')):
                t.copy_(torch.from_numpy(case[k]))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.detach().cpu().numpy().copy() for o in outs]
        eager = nc.evaluate(nc.module(nc.fused_cls(), 512, 8.0, first['seed']), case, dev())
        for got, k in zip(replayed, ('loss', 'terms', 'grad_q_r', 'grad_q_l')):
            assert np.array_equal(got, eager[k]), (name, k)
        results[name] = eager
    a, b = results['first']['terms'], results['second']['terms']
    assert 0 < a[3] < B and b[2] == a[3] and b[3] == B and results['second']['grad_q_r'].any()
