"""Fused two-hand penetration loss (renderih_amd.sdf.FusedTwoHandSDFLoss: csrc/rih_sdf_loss.hip and the sparse voxeliser of
csrc/rih_sdf.hip) on the GPU: both golden cases of the reference's own `NewLoss` end to end, small meshes against the torch
mirror (sparse == dense bitwise, bit-identical repeats, exact zeros), the RIH_SDF_SPARSE=0 switch in a fresh process, and a
captured graph replayed on new vertices.  Helpers and tolerances: tests/test_two_hand_sdf.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_two_hand_sdf import (FIELDS, GRADS, PART_VERT, SMALL_CASES, compare, evaluate, fused_vs_golden,  # noqa: F401
                               fused_vs_mirror, golden_case, seeded_weights, small_case)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.mark.parametrize('name', ['g32', 'g16'])
def test_fused_matches_reference_golden(name):
    fused_vs_golden(name, dev())


def test_mirror_matches_reference_golden_g32():
    """The torch mirror on the dense HIP voxeliser at the reference's own grid size (too slow for the CPU suite)."""
    from renderih_amd.sdf import TwoHandSDFLoss, sdf
    from test_two_hand_sdf import excused
    verts, G, wts, want, inside = golden_case('g32')
    crit = TwoHandSDFLoss(PART_VERT, grid_size=G).to(dev())
    got = evaluate(crit, verts, wts, dev())
    v = torch.from_numpy(verts).to(dev())
    lo, hi = v.min(2)[0], v.max(2)[0]
    box = torch.cat([(lo + hi) / 2, ((1 + 0.1) * 0.5 * (hi - lo).max(-1)[0])[..., None]], -1)
    phi = sdf(crit.faces, ((v - box[:, :, None, :3]) / box[:, :, None, 3:]).reshape(4, -1, 3), G).view(2, 2, G, G, G)
    compare(got, want, G, excused(verts, {'phi': phi, 'box': box}, inside, G))


@pytest.mark.parametrize('bs,G,sub', SMALL_CASES)
def test_fused_matches_mirror(bs, G, sub):
    fused_vs_mirror(bs, G, sub, dev())


CHILD = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')
from renderih_amd import sdf
from test_two_hand_sdf import PART_VERT, evaluate, golden_case
assert sdf.SPARSE is False
verts, G, wts, want, inside = golden_case('g16')
crit = sdf.FusedTwoHandSDFLoss(PART_VERT, grid_size=G).to('cuda:0')
assert crit.sparse is False
np.savez(sys.argv[2], **evaluate(crit, verts, wts, 'cuda:0'))
'''


def test_dense_switch_is_bit_identical(tmp_path):
    """RIH_SDF_SPARSE is read at import: a fresh child with RIH_SDF_SPARSE=0 against this process's default."""
    from renderih_amd import sdf
    verts, G, wts, want, inside = golden_case('g16')
    crit = sdf.FusedTwoHandSDFLoss(PART_VERT, grid_size=G).to(dev())
    assert crit.sparse is sdf.SPARSE
    mine = evaluate(sdf.FusedTwoHandSDFLoss(PART_VERT, grid_size=G, sparse=True).to(dev()), verts, wts, dev())
    out = str(tmp_path / 'dense.npz')
    r = subprocess.run([sys.executable, '-c', CHILD, ROOT, out], env=dict(os.environ, RIH_SDF_SPARSE='0'),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert set(z.files) == set(mine)
    for k in mine:
        assert np.array_equal(mine[k], z[k]), k
    assert mine['loss'][0] > 1e-3


def test_forward_and_backward_inside_a_captured_graph():
    """No host sync anywhere: forward + backward are captured once and replayed on NEW vertices (other boxes, another number
    of sampled voxels: the device-side count), bit-identical to the eager evaluation of those vertices."""
    from renderih_amd.sdf import FusedTwoHandSDFLoss
    bs, G, sub = 3, 12, 2
    verts, faces, weight = small_case(bs, G, sub)
    crit = FusedTwoHandSDFLoss(weight, faces, grid_size=G).to(dev())
    v2 = verts.copy()
    v2[:, 1] += np.float32([0.07, -0.05, 0.03])
    v2[1, 1] = verts[0, 1]                                      # the disjoint sample now penetrates
    static = torch.from_numpy(verts).to(dev()).requires_grad_(True)

    def run():
        loss, left, right = crit(static, return_per_vert_loss=True)
        g, = torch.autograd.grad(loss.sum() + (left * left).sum(), static)
        return loss, left, right, g
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = run()
    with torch.no_grad():
        static.copy_(torch.from_numpy(v2))
    graph.replay()
    replayed = [o.clone() for o in outs]
    eager = run()
    assert float(eager[0][1]) > 1e-3
    for a, b in zip(replayed, eager):
        assert torch.equal(a, b)
