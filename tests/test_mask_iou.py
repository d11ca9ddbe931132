"""Two-hand silhouette IoU (rih_mask_iou of csrc/rih_render.hip, renderih_amd/mask_iou.py, evaluate.summarize_by_iou;
reference utils/compute_maskiou.py:219-275 and apps/eval_interhand.py:230-234, 471-536) on the CPU: the real kernel through the
host-compiled library against the project's rasteriser (exact), the numpy oracle, closed forms and crafted chunk / split
cases; degenerate images, buffer reuse, refusals; the mirror, the annotation scan, the bins and the breakdown."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import mask_iou_cases as mc                     # noqa: E402
from renderih_amd import assets, evaluate, mask_iou   # noqa: E402
from renderih_amd.manolayer import ManoLayer    # noqa: E402

DEV = 'cpu'


@pytest.fixture
def host():
    from hipcpu.host_kernels import host_kernels_abi
    with host_kernels_abi():
        yield


# ------------------------------------------------------------------------------------------------------ 1, 2. the kernel

@pytest.mark.parametrize('S', [32, 48, 80])        # one tile, 2 x 2 tiles with partial ones, 3 x 3 tiles
@pytest.mark.parametrize('name', mc.SCENES)
def test_exact_against_rasteriser_and_oracle(host, name, S):
    vl, vr, cam = mc.scene(name, S)
    iou, counts, mask = mc.check_exact(S, DEV, vl, vr, cam)
    mc.check_oracle(name, S, counts, mask)
    assert (counts[:, :2] >= 55).all()                          # both hands are on screen
    assert (counts[:, 2] > 0).all() or not name.endswith('overlap')


# ------------------------------------------------------------------------------------------- 3. the bins, real geometry

@pytest.mark.parametrize('name,lo,hi', [('persp_high', 0.67, 1.0), ('persp_mid', 0.33, 0.67)])
def test_upper_bins_from_real_geometry(host, name, lo, hi):
    S = 48
    vl, vr, cam = mc.scene(name, S)
    iou, counts, mask = mc.check_exact(S, DEV, vl, vr, cam)     # the fp32 quotient and the fp64 one within a rounding
    mc.check_oracle(name, S, counts, mask)
    assert ((iou >= lo) & (iou < hi)).all(), iou.tolist()
    bins = mask_iou.iou_bins(iou)
    assert bins[2 if name == 'persp_high' else 1].all()


def test_lower_bin_from_real_geometry(host):
    iou, _, _ = mc.check_exact(48, DEV, *mc.scene('persp_overlap', 48))
    assert ((iou > 0) & (iou < 0.33)).all() and mask_iou.iou_bins(iou)[0].all()


# ----------------------------------------------------------------------------------------------------- 4. closed form

@pytest.mark.parametrize('flip', [False, True])
def test_rectangles_closed_form(host, flip):
    vl, vr, faces, want = mc.rectangles(flip)
    assert want[0].sum() == 64 and want[1].sum() == 36 and (want[0] & want[1]).sum() == 16
    iou, counts, mask = mc.check_exact(16, DEV, vl, vr, mc.ORTHO_UNIT, faces, faces, faces)
    assert counts.tolist() == [[64, 36, 16]]
    assert iou[0] == np.float32(16) / np.float32(84)
    assert ((mask[0] & 1 > 0) == want[0]).all() and ((mask[0] & 2 > 0) == want[1]).all()


# ----------------------------------------------------------------------------------------- 5. chunk and split edges

@pytest.mark.parametrize('F_left,F_right', [(2, 2), (256, 1), (255, 257), (257, 255)])
def test_chunk_and_split_edges(host, F_left, F_right):
    """A partial last chunk, the hands' split on a chunk boundary and inside a chunk; hands of different vertex counts."""
    S = 48
    vl, vr, faces, want_counts, want_mask = mc.split_case(S, F_left, F_right)
    iou, counts, mask = mc.check_exact(S, DEV, vl, vr, mc.ORTHO_UNIT, faces, *faces)
    assert (counts == want_counts).all(), (counts.tolist(), want_counts.tolist())
    assert (mask[0] == want_mask).all()


# ----------------------------------------------------------------------------------------------- 6. degenerate images

def check_degenerate_perspective(DEV):
    S = 48
    vl, vr, cam = mc.scene('persp_overlap', S)
    _, base, _ = mc.check_exact(S, DEV, vl, vr, cam)
    far = np.array([5.0, 0.0, 0.0], np.float32)
    # image 1: the right hand off screen; image 2: both
    a_l, a_r = vl.copy(), vr.copy()
    a_r[1] += far
    a_l[2] += far
    a_r[2] += far
    iou, counts, _ = mc.check_exact(S, DEV, a_l, a_r, cam)
    assert (counts[0] == base[0]).all()
    assert counts[1].tolist() == [base[1, 0], 0, 0] and iou[1] == 0
    assert counts[2].tolist() == [0, 0, 0] and iou[2] == 0.0 and not np.signbit(iou[2])
    # image 1: the left hand behind the camera (every face skipped); image 2: a NaN vertex in the right hand
    b_l, b_r = vl.copy(), vr.copy()
    b_l[1, :, 2] -= 1.0
    assert (b_l[1, :, 2] < 0).all()
    b_r[2, 100] = np.nan
    iou, counts, _ = mc.check_exact(S, DEV, b_l, b_r, cam)
    assert (counts[0] == base[0]).all()
    assert counts[1].tolist() == [0, base[1, 1], 0] and iou[1] == 0
    assert counts[2, 0] == base[2, 0] and 0 < counts[2, 1] <= base[2, 1] and np.isfinite(iou[2])


def check_degenerate_orthographic(DEV):
    S = 48
    vl, vr, cam = mc.scene('orth_overlap', S)
    _, base, _ = mc.check_exact(S, DEV, vl, vr, cam)
    c_l = vl.copy()
    c_l[1, :, 2] -= 20.0                                          # view z = z + 10 < 0: behind the image plane
    iou, counts, _ = mc.check_exact(S, DEV, c_l, vr, cam)
    assert (counts[[0, 2]] == base[[0, 2]]).all()
    assert counts[1].tolist() == [0, base[1, 1], 0] and iou[1] == 0


def test_degenerate_images(host):
    check_degenerate_perspective(DEV)
    check_degenerate_orthographic(DEV)


# --------------------------------------------------------------------------------------------- 7. runtime properties

def check_two_runs_and_reused_buffers(DEV):
    S = 48
    vl, vr, cam = mc.scene('persp_overlap', S)
    first = [x.clone() for x in mc.run_fused(S, DEV, vl, vr, cam)]
    out = (torch.full((3,), 7.0, device=DEV), torch.full((3, 3), 12345, dtype=torch.int32, device=DEV),
           torch.full((3, S, S), 255, dtype=torch.uint8, device=DEV))
    for _ in range(2):                                            # the second call finds the first call's counts there
        again = mc.run_fused(S, DEV, vl, vr, cam, out=out)
        assert all(a is o for a, o in zip(again, out))
        assert all(torch.equal(a, f) for a, f in zip(again, first))
    # other hands into the same buffers: nothing is left over
    wl, wr, wcam = mc.scene('persp', S)
    want = [x.clone() for x in mc.run_fused(S, DEV, wl, wr, wcam)]
    assert all(torch.equal(a, w) for a, w in zip(mc.run_fused(S, DEV, wl, wr, wcam, out=out), want))


def test_two_runs_and_reused_buffers(host):
    check_two_runs_and_reused_buffers(DEV)


def test_refusals():
    with pytest.raises(ValueError, match='square'):
        mask_iou.FusedTwoHandMaskIoU((480, 640), DEV)
    with pytest.raises(ValueError, match='square'):
        mask_iou.TwoHandMaskIoU((480, 640), DEV)
    with pytest.raises(ValueError, match=r'faces must be \[F, 3\]'):
        mask_iou.FusedTwoHandMaskIoU(32, DEV, faces=np.zeros((4, 4), np.int64))
    fused = mask_iou.FusedTwoHandMaskIoU(32, DEV)
    v = torch.zeros(2, 778, 3)
    K = torch.eye(3).expand(2, 3, 3)
    with pytest.raises(ValueError, match=r'\[B, V, 3\]'):
        fused(v[..., :2], v, cameras=K)
    with pytest.raises(ValueError, match='one B'):
        fused(v, v[:1], cameras=K)
    with pytest.raises(ValueError, match='scale and trans2d'):
        fused(v, v)
    with pytest.raises(ValueError, match='fp32 only'):
        fused(v.double(), v.double(), cameras=K)
    with pytest.raises(RuntimeError, match='GPU tensors'):       # CPU tensors outside the host-kernel harness
        fused(v, v, cameras=K)
    with pytest.raises(ValueError, match='ascending'):
        mask_iou.iou_bins([0.1], edges=(0.67, 0.33))


def test_refusals_behind_the_device_check(host):
    fused = mask_iou.FusedTwoHandMaskIoU(32, DEV)
    vl, vr, cam = mc.scene('persp', 32)
    with pytest.raises(ValueError, match='out must be'):
        fused(mc.t(vl, DEV), mc.t(vr, DEV), out=(torch.zeros(3), torch.zeros(2, 3, dtype=torch.int32)), **mc.cam_kw(cam, DEV))
    with pytest.raises(ValueError, match='out of range for'):
        fused(mc.t(vl[:, :700], DEV), mc.t(vr, DEV), **mc.cam_kw(cam, DEV))
    with pytest.raises(ValueError, match='camera batch'):
        fused(mc.t(vl, DEV), mc.t(vr, DEV), cameras=mc.t(cam['cameras'][:1], DEV))


# --------------------------------------------------------------------------------------------------------- 8. the mirror

@pytest.mark.parametrize('name,S', [('orth_overlap', 32), ('persp', 48), ('persp_overlap', 48), ('persp_high', 48),
                                    ('persp_mid', 32)])
def test_mirror_equals_fused(host, name, S):
    check_mirror(name, S, DEV)


def check_mirror(name, S, DEV):
    vl, vr, cam = mc.scene(name, S)
    iou, counts, _ = mc.run_fused(S, DEV, vl, vr, cam)
    m_iou, m_counts = mask_iou.TwoHandMaskIoU(S, DEV)(mc.t(vl, DEV), mc.t(vr, DEV), **mc.cam_kw(cam, DEV))
    assert m_counts.dtype == torch.int32 and m_iou.dtype == torch.float32
    assert torch.equal(m_counts, counts) and torch.equal(m_iou, iou)


def check_reference_lines_by_hand(DEV):
    """compute_maskiou.py:263-270 and bm0 (:59-64) written out on `render_single_mask`, one sample at a time."""
    S = 48
    vl, vr, cam = mc.scene('persp_overlap', S)
    mirror = mask_iou.TwoHandMaskIoU(S, DEV)
    iou, counts, _ = mc.run_fused(S, DEV, vl, vr, cam)
    for b in range(vl.shape[0]):
        camera = torch.from_numpy(cam['cameras'][b]).float().unsqueeze(0).to(DEV)
        left_mask = mirror.renderer.render_single_mask(cameras=camera, v3d=torch.from_numpy(vl[b]).unsqueeze(0).to(DEV))
        right_mask = mirror.renderer.render_single_mask(cameras=camera, v3d=torch.from_numpy(vr[b]).unsqueeze(0).to(DEV))
        left_mask[left_mask < 0.2] = 0
        right_mask[right_mask < 0.2] = 0
        mask1, mask2 = left_mask.cpu().numpy()[0, :, :, 0], right_mask.cpu().numpy()[0, :, :, 0]
        mask1_area = np.count_nonzero(mask1 == 1)
        mask2_area = np.count_nonzero(mask2 == 1)
        intersection = np.count_nonzero(np.logical_and(mask1, mask2))
        assert counts[b].tolist() == [mask1_area, mask2_area, intersection]
        assert np.isclose(float(iou[b]), intersection / (mask1_area + mask2_area - intersection), rtol=1.2e-7, atol=0)


def test_reference_lines_by_hand(host):
    check_reference_lines_by_hand(DEV)


# --------------------------------------------------------------------------------------------------- 9. the annotation scan

def check_scan_annotations(DEV, tmp_path, N):
    S = 32
    layers = {side: ManoLayer(assets.write_synthetic_mano_pkl(str(tmp_path / ('%s.pkl' % side)), side), center_idx=None).to(DEV)
              for side in ('left', 'right')}
    annos = mc.synthetic_annotations(N, S)
    got = mask_iou.scan_annotations(iter(annos), layers['left'], layers['right'], img_size=S, batch_size=2, device=DEV)
    assert got.dtype == np.float64 and got.shape == (N,)
    want = mc.scan_by_hand(annos, layers, S, DEV)
    assert (got == want).all(), (got.tolist(), want.tolist())
    assert len(set(want.tolist())) == N and (want > 0).all()      # the order shows
    with pytest.raises(ValueError, match='batch_size'):
        mask_iou.scan_annotations(annos, layers['left'], layers['right'], batch_size=0, device=DEV)


def test_scan_annotations(host, tmp_path):
    check_scan_annotations(DEV, tmp_path, 3)            # the host-compiled MANO kernels take about a second per call


# ------------------------------------------------------------------------------------------ 10. bins and the breakdown

IOU = [0.0, 0.32999, 0.33, 0.5, 0.67, 1.0]


def hand_made_per_sample(N, seed=0):
    rs = np.random.RandomState(seed)
    per = {k: {s: rs.rand(N, 21) * 0.02 for s in ('left', 'right')} for k in ('j_err_ori', 'j_err', 'pa_mpjpe')}
    per['mrrpe_ref_script'] = rs.rand(N, 3) * 0.05
    per['mrrpe'] = np.sqrt((per['mrrpe_ref_script'] ** 2).sum(1))
    per['cdev'] = np.where(rs.rand(N) < 0.5, np.nan, rs.rand(N))
    return per


def test_iou_bins():
    bins = mask_iou.iou_bins(np.array(IOU))
    assert [b.tolist() for b in bins] == [[True, True, False, False, False, False], [False, False, True, True, False, False],
                                          [False, False, False, False, True, True]]
    assert all(b.dtype == np.bool_ for b in bins)
    again = mask_iou.iou_bins(torch.tensor(IOU, dtype=torch.float64))
    assert all((a == b).all() for a, b in zip(again, bins))
    wide = mask_iou.iou_bins(IOU, edges=(0.5, 0.5))
    assert [int(b.sum()) for b in wide] == [3, 0, 3]


def test_summarize_by_iou_is_the_scripts_arithmetic():
    per = hand_made_per_sample(6)
    per['cdev'][:2] = [np.nan, 0.25]
    theiou = np.array(IOU)
    got = evaluate.summarize_by_iou(per, theiou)
    sels = (theiou < 0.33, np.logical_and(theiou < 0.67, theiou >= 0.33), theiou >= 0.67)      # eval_interhand.py:232-234
    assert [g['n'] for g in got] == [2, 2, 2]
    for g, sel in zip(got, sels):
        assert g['mrrpe'] == per['mrrpe'][sel].mean()
        assert g['mrrpe_ref_script'] == per['mrrpe_ref_script'][sel].mean()
        for name, key in (('ori joint mpjpe', 'j_err_ori'), ('joint mean error', 'j_err')):
            loss = per[key]
            assert g[name]['mean'] == (loss['left'][sel].mean() * 1000 + loss['right'][sel].mean() * 1000) / 2
            assert g[name]['std'] == (loss['left'][sel].std() * 1000 + loss['right'][sel].std() * 1000) / 2
        loss = per['pa_mpjpe']
        assert g['pa joint mean error'] == (loss['left'][sel].mean() * 1000 + loss['right'][sel].mean() * 1000) / 2
    assert got[0]['cdev'] == 0.25                                                              # nanmean of (NaN, 0.25)
    err = per['cdev'][sels[2]]
    assert np.isnan(err).all() and np.isnan(got[2]['cdev']) or got[2]['cdev'] == err[~np.isnan(err)].mean()


def test_summarize_by_iou_empty_bin_and_mismatch():
    per = hand_made_per_sample(4)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        got = evaluate.summarize_by_iou(per, [0.1, 0.2, 0.9, 0.95])
    assert [g['n'] for g in got] == [2, 0, 2]
    empty = got[1]
    assert all(np.isnan(empty[k]) for k in ('mrrpe', 'mrrpe_ref_script', 'cdev', 'pa joint mean error'))
    assert all(np.isnan(empty[k][s]) for k in ('ori joint mpjpe', 'joint mean error') for s in ('mean', 'std'))
    assert np.isfinite(got[0]['mrrpe']) and np.isfinite(got[2]['joint mean error']['std'])
    with pytest.raises(ValueError, match='samples'):
        evaluate.summarize_by_iou(per, [0.1, 0.2, 0.9])
    per['j_err']['right'] = per['j_err']['right'][:3]
    with pytest.raises(ValueError, match='samples'):
        evaluate.summarize_by_iou(per, [0.1, 0.2, 0.9, 0.95])
