"""The fused MANO kernels (csrc/rih_mano.hip) where tests/test_gpu_mano.py and tests/test_gpu_quat_mano.py do not reach, values and
all input gradients against oracle/mano_oracle.mano_forward in fp64:
  A. the forward's chunk loop past its first iteration, in both forms (tile-major from 641 hands, hand-chunk-major from 4097), with
     the training workspace that later iterations write and the backward reads; bit-identity of the forms, and of the training and
     the no-grad forward, at those sizes; the quaternion front end at 641 hands;
  B. a covering table of configurations (side, centre joint incl. the five finger tips, PCA size / rotation input, new_skel,
     trans / scale) across a chunk edge, and one tip-centre row inside the chunk loop;
  C. Rodrigues' formula and its gradient at tiny angles, around pi and 2 pi, and beyond.
Builders, the compared hands, the table and the tolerances: tests/mano_cases.py."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import mano_cases as MC  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    """cuda:0 (tests/test_kernels_on_cpu.py re-runs these checks on the host-compiled kernels with this patched)"""
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


DEFAULT_ROW = ('right', 9, 45, False, True, True)
# forms whose outputs and gradients must equal, bit for bit, those of the form under test at that batch (0 = the layer's own
# choice: tile-major below 4096 hands, hand-chunk-major from there)
SAME_BITS_AS = {(MC.TILE_MAJOR, 641): (MC.HAND_MAJOR, 0), (MC.HAND_MAJOR, 4097): (0,)}


# ------------------------------------------------------------------------------------------------ A. chunk loops
def check_chunk_loop(variant, B, same_bits_as=()):
    layer = MC.layer_for(DEFAULT_ROW, dev())
    ins = MC.random_inputs(B, seed=B)
    what = 'variant %d B=%d' % (variant, B)
    got = MC.run_layer(layer, ins, dev(), variant)
    hands = MC.compared_hands(B, variant)
    MC.compare(got, MC.run_oracle(DEFAULT_ROW, ins, hands), hands, what)
    MC.assert_bit_identical(MC.run_layer(layer, ins, dev(), variant, grad=False), got, what + ': no-grad forward vs training forward')
    for other in same_bits_as:
        MC.assert_bit_identical(got, MC.run_layer(layer, ins, dev(), other), '%s vs variant %d' % (what, other))


@pytest.mark.parametrize('variant,B', MC.CHUNK_LOOP_CASES)
def test_chunk_loop_vs_fp64(variant, B):
    """mano_fused_kernel walks 16-hand chunks with `chunk += grid` and reuses s_pf, s_G and s_scr between iterations.
    Tile-major (40 groups): 641 hands = 41 chunks, group 0 runs twice and its second chunk holds one live hand; 1285 = 81 chunks,
    every group runs twice, group 0 a third time on five hands.  Hand-chunk-major (256 workgroups): 4097 and 8197 likewise.
    Forward with gradients (every iteration fills the workspace), backward of (v * wv).sum() + (j * wj).sum(); v, j and the
    gradients of root, pose, shape, trans and scale at 1e-4 / 1e-5 against fp64 -- on the whole batch at 641 and 1285, on
    mano_cases.chunk_loop_hands beyond (the hands at both ends of every chunk group / workgroup 0 takes, their neighbours across
    the 16-hand edges, B - 1, and 48 seeded others); every element of the full batch finite.  Bitwise: the no-grad forward (no
    workspace) equals the training forward; at 641 hands variants 2 and 0 equal variant 3, at 4097 variant 0 equals variant 2,
    in v, j and every gradient.
    GPU only: the group count is fixed in the launch code, so the host build cannot iterate below 641 hands, and there the
    tile-major check (533 workgroups of 256 fibers, forward, backward and no-grad forward) took 82 s, above the minute allowed
    for the host rerun (tests/test_kernels_on_cpu.py)."""
    check_chunk_loop(variant, B, SAME_BITS_AS.get((variant, B), ()))


@pytest.mark.parametrize('per_hand_betas', [False, True], ids=['shared_betas', 'per_hand_betas'])
def test_quat_front_end_chunk_loop(per_hand_betas):
    """rih_mano_quat_fwd is always tile-major: 641 left hands, group 0 iterates.  v, j, transf and the gradients of quat and trans
    with all three upstream gradients present, once with the shape vector shared by the batch (shape_stride 0), once with per-hand
    betas (and their gradient), at the tolerance of tests/quat_mano_cases.py."""
    MC.quat_fused_vs_fp64_mirror('left', 641, per_hand_betas, dev())


# ------------------------------------------------------------------------------------------------ B. configurations
def check_config(row, B, variant=None):
    layer = MC.layer_for(row, dev())
    ins = MC.random_inputs(B, seed=100 + B, pose=row[2], trans=row[4], scale=row[5])
    got = MC.run_layer(layer, ins, dev(), variant)
    MC.compare(got, MC.run_oracle(row, ins), None, '%s B=%d' % (MC.row_id(row), B))
    if row[2] == 'rot':
        assert got['grad_pose'].shape == (B, 15, 3, 3)          # gradient with respect to the 135 matrix entries


@pytest.mark.parametrize('B', MC.CONFIG_BATCHES)
@pytest.mark.parametrize('row', MC.CONFIG_ROWS, ids=MC.row_id)
def test_config_across_chunk_edge(row, B):
    """mano_cases.CONFIG_ROWS at 17 and 33 hands (one / two full chunks plus one hand): values and every input gradient at
    1e-4 / 1e-5 against fp64.  A tip centre (4, 8, 12, 16, 20) puts every vertex tile on the special-vertex path."""
    check_config(row, B)


def test_tip_centre_inside_the_chunk_loop():
    """A tip-centre row at 641 hands, tile-major: every tile requests bv_sp again in every iteration of the chunk loop."""
    check_config(MC.TIP_ROW_IN_CHUNK_LOOP, 641, MC.TILE_MAJOR)


# ------------------------------------------------------------------------------------------------ C. pose extremes
EXTREMES = {'one_joint': (MC.extreme_axis, 11), 'all_joints_2.5_to_3.6': (MC.large_angle_axis, 12), 'exact_zero': (None, 13)}
# outputs that were measured to meet the project's bar as well (figures in the docstring below)
TIGHT = {'one_joint': MC.EXTREME_OUTS, 'all_joints_2.5_to_3.6': MC.EXTREME_OUTS, 'exact_zero': MC.EXTREME_OUTS}


def check_extremes(kind):
    row = ('right', 9, 45, False, False, False)
    layer = MC.layer_for(row, dev())
    make_axis, seed = EXTREMES[kind]
    flat = make_axis is None
    if flat:
        layer.hands_mean.zero_()
        ins = MC.exact_zero_inputs(seed)
    else:
        ins = MC.extreme_inputs(layer, make_axis(), seed)
    got = MC.run_layer(layer, ins, dev())
    return MC.compare_extremes(got, MC.run_oracle(row, ins, dtype=torch.float32, flat_mean=flat),
                               MC.run_oracle(row, ins, flat_mean=flat), TIGHT[kind], kind)


@pytest.mark.parametrize('kind', sorted(EXTREMES))
def test_pose_extremes(kind):
    """The kernel's own PCA -> axis-angle -> Rodrigues path (45 components, pose = axis2pca(prescribed axis), 17 hands).
    one_joint: hand h turns joint h % 15 by 0, 1e-7, 1e-5, 1e-3, 3e-2, pi - 1e-3, pi, pi + 1e-3, 2 pi - 1e-3, 2 pi, 5, 9 (hand 0 is
    the whole zero pose); all_joints: every joint by an angle from [2.5, 3.6]; exact_zero: hands_mean zeroed and pose = 0 in one hand
    of each chunk, so those axes are exactly 0 in the kernel (axis2pca(0) on a non-zero mean is realised at 2e-7 .. 7e-7: it only
    comes near the n > 0 ? ... : 0 branch of rodrigues_bwd).  v, j and the gradients of pose, shape and root:
    finite, at most 4 x as far from the fp64 oracle as the same oracle in fp32 on the CPU plus 2e-5 of max |fp64|
    (assert_fp32_equivalent, defaults), and at 1e-4 / 1e-5 where that was measured to hold (TIGHT: everywhere).
    Measured on the MI355X, max error / max |fp64|: kernel vs fp64 | fp32 oracle vs fp64 | largest share of the 1e-4 / 1e-5 bar
      one_joint   v           4.1e-07 | 3.6e-07 | 0.03        all_joints  v           6.0e-07 | 6.7e-07 | 0.06
                  j           3.4e-07 | 3.6e-07 | 0.02                    j           6.6e-07 | 7.7e-07 | 0.06
                  grad_pose   4.9e-06 | 4.9e-06 | 0.20                    grad_pose   4.9e-07 | 5.1e-07 | 0.03
                  grad_shape  4.2e-07 | 1.6e-06 | 0.02                    grad_shape  4.9e-07 | 1.0e-06 | 0.03
                  grad_root   2.8e-07 | 3.0e-07 | 0.02                    grad_root   3.9e-07 | 4.9e-07 | 0.03
    (the one_joint pose gradient's largest error sits in the hand turned by 1e-3, where 1 - cos cancels, for the fp32 oracle as
    for the kernel: 4.8e-06 and 4.9e-06 of that hand on the host build; the joints prescribed as 0 and 1e-7 are realised at
    2e-7 .. 7e-7 after the fp32 inverse of axis2pca and stay at 2e-07)"""
    check_extremes(kind)
