"""Two-hand silhouette IoU on the MI355X (rih_mask_iou of csrc/rih_render.hip, renderih_amd/mask_iou.py): the checks of
tests/test_mask_iou.py on the device -- exact against the rasteriser, the numpy oracle, the three bins, closed forms, chunk and
split edges, degenerate images, the mirror, the annotation scan -- and what only the device shows: 256 x 256 images, a
non-default stream, a captured graph replayed on new vertices."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import mask_iou_cases as mc              # noqa: E402
import test_mask_iou as cpu              # noqa: E402
from renderih_amd import mask_iou        # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('S', [32, 48, 80])
@pytest.mark.parametrize('name', mc.SCENES)
def test_exact_against_rasteriser_and_oracle(name, S):
    vl, vr, cam = mc.scene(name, S)
    iou, counts, mask = mc.check_exact(S, DEV, vl, vr, cam)
    mc.check_oracle(name, S, counts, mask)
    assert (counts[:, :2] >= 55).all()
    assert (counts[:, 2] > 0).all() or not name.endswith('overlap')


@pytest.mark.parametrize('name', ['orth_overlap', 'persp_overlap', 'persp_high'])
def test_exact_against_rasteriser_at_256(name):
    """The reference's IMG_SIZE, 8 x 8 tiles, against the device's own rasteriser only."""
    vl, vr, cam = mc.scene(name, 256, 2)
    iou, counts, _ = mc.check_exact(256, DEV, vl, vr, cam)
    assert (counts[:, :2] > 1000).all() and (counts[:, 2] > 0).all()      # both hands on screen (>= 55 px at 32 x 32), touching
    assert ((iou > 0) & (iou < 1)).all()


@pytest.mark.parametrize('name,lo,hi', [('persp_high', 0.67, 1.0), ('persp_mid', 0.33, 0.67), ('persp_overlap', 0.0, 0.33)])
def test_three_bins_from_real_geometry(name, lo, hi):
    S = 48
    vl, vr, cam = mc.scene(name, S)
    iou, counts, mask = mc.check_exact(S, DEV, vl, vr, cam)
    mc.check_oracle(name, S, counts, mask)
    assert ((iou > 0) & (iou >= lo) & (iou < hi)).all(), iou.tolist()
    assert mask_iou.iou_bins(iou)[{0.0: 0, 0.33: 1, 0.67: 2}[lo]].all()


@pytest.mark.parametrize('flip', [False, True])
def test_rectangles_closed_form(flip):
    vl, vr, faces, want = mc.rectangles(flip)
    iou, counts, mask = mc.check_exact(16, DEV, vl, vr, mc.ORTHO_UNIT, faces, faces, faces)
    assert counts.tolist() == [[64, 36, 16]] and iou[0] == np.float32(16) / np.float32(84)
    assert ((mask[0] & 1 > 0) == want[0]).all() and ((mask[0] & 2 > 0) == want[1]).all()


@pytest.mark.parametrize('F_left,F_right', [(2, 2), (256, 1), (255, 257), (257, 255)])
def test_chunk_and_split_edges(F_left, F_right):
    S = 48
    vl, vr, faces, want_counts, want_mask = mc.split_case(S, F_left, F_right)
    iou, counts, mask = mc.check_exact(S, DEV, vl, vr, mc.ORTHO_UNIT, faces, *faces)
    assert (counts == want_counts).all(), (counts.tolist(), want_counts.tolist())
    assert (mask[0] == want_mask).all()


def test_degenerate_images():
    cpu.check_degenerate_perspective(DEV)
    cpu.check_degenerate_orthographic(DEV)


def test_two_runs_and_reused_buffers():
    cpu.check_two_runs_and_reused_buffers(DEV)


def test_non_default_stream():
    S = 48
    vl, vr, cam = mc.scene('persp_overlap', S)
    want = mc.run_fused(S, DEV, vl, vr, cam)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        got = mc.run_fused(S, DEV, vl, vr, cam)
    stream.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_captured_graph_replays_on_new_vertices():
    S = 48
    vl, vr, cam = mc.scene('persp_overlap', S)
    wl, wr, wcam = mc.scene('persp_mid', S)
    fused = mask_iou.FusedTwoHandMaskIoU(S, DEV)
    s_l, s_r = mc.t(vl, DEV), mc.t(vr, DEV)
    camera = fused.build_camera(cameras=mc.t(cam['cameras'], DEV))     # static: its params are rewritten below
    out = (torch.empty(3, device=DEV), torch.empty((3, 3), dtype=torch.int32, device=DEV),
           torch.empty((3, S, S), dtype=torch.uint8, device=DEV))
    fused(s_l, s_r, cameras=camera, return_masks=True, out=out)          # warm-up: the topology is built outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused(s_l, s_r, cameras=camera, return_masks=True, out=out)
    for a, b, c in ((wl, wr, wcam), (vl, vr, cam)):
        s_l.copy_(mc.t(a, DEV))
        s_r.copy_(mc.t(b, DEV))
        camera.params.copy_(fused.build_camera(cameras=mc.t(c['cameras'], DEV)).params)
        graph.replay()
        torch.cuda.synchronize()
        want = mc.run_fused(S, DEV, a, b, c)
        assert all(torch.equal(g, w) for g, w in zip(out, want))
    assert out[1][:, 2].min() > 0


def test_refusals_on_the_device():
    fused = mask_iou.FusedTwoHandMaskIoU(32, DEV)
    vl, vr, cam = mc.scene('persp', 32)
    a, b, kw = mc.t(vl, DEV), mc.t(vr, DEV), mc.cam_kw(cam, DEV)
    with pytest.raises(ValueError, match='out must be'):
        fused(a, b, out=(torch.zeros(3, device=DEV), torch.zeros((2, 3), dtype=torch.int32, device=DEV)), **kw)
    with pytest.raises(RuntimeError, match='GPU tensors'):
        fused(a, b, out=(torch.zeros(3), torch.zeros((3, 3), dtype=torch.int32)), **kw)
    with pytest.raises(ValueError, match='out of range for'):
        fused(a[:, :700], b, **kw)
    with pytest.raises(ValueError, match='fp32 only'):
        fused(a.double(), b.double(), **kw)
    with pytest.raises(ValueError, match='square'):
        mask_iou.FusedTwoHandMaskIoU((480, 640), DEV)


@pytest.mark.parametrize('name,S', [('orth', 48), ('orth_overlap', 32), ('persp', 48), ('persp_overlap', 80),
                                    ('persp_high', 48), ('persp_mid', 32)])
def test_mirror_equals_fused(name, S):
    cpu.check_mirror(name, S, DEV)


def test_reference_lines_by_hand():
    cpu.check_reference_lines_by_hand(DEV)


def test_scan_annotations(tmp_path):
    cpu.check_scan_annotations(DEV, tmp_path, 5)
