"""Shared by tests/test_gpu_mano_chunks.py (GPU) and its host rerun in tests/test_kernels_on_cpu.py: input builders, the fp64 /
fp32 oracle (oracle/mano_oracle.mano_forward with its constants promoted), one `run_layer` that evaluates
renderih_amd.manolayer.ManoLayer under a forced form of the fused forward, the hands a chunk-loop test compares, the literal
table of configurations that cross a chunk edge, and the prescribed axis-angle poses at the extremes of Rodrigues' formula.

Tolerance: renderih_amd.testing.assert_close(got, want, 1e-4, 1e-5), the project's bar for an fp32 kernel against fp64, for values
and gradients alike -- except at the pose extremes, where the bar is derived from the fp32 evaluation of the same oracle
(renderih_amd.testing.assert_fp32_equivalent, defaults) and the project's bar is asserted in addition where it was measured to hold.

Geometry of the launches the chunk-loop tests are built around (csrc/rih_mano.hip, rih_mano_fwd): a chunk is HC = 16 hands; the
tile-major form runs min(40, chunks) groups of chunks per vertex tile, the hand-chunk-major form min(256, chunks) workgroups, and
group / workgroup g takes chunks g, g + grid, g + 2 grid, ..."""
import math

import torch

from renderih_amd.testing import assert_close, assert_fp32_equivalent

RTOL, ATOL = 1e-4, 1e-5
HC = 16
TILE_MAJOR, HAND_MAJOR = 3, 2               # manolayer.VARIANT values that force a form of the fused forward
GRID = {TILE_MAJOR: 40, HAND_MAJOR: 256}    # groups of chunks (tile-major) / workgroups (hand-chunk-major) of a full launch
LEAVES = ('root', 'pose', 'shape', 'trans', 'scale')

# (variant, B): the smallest batch at which group / workgroup 0 iterates, and one at which every one of them runs twice and
# group / workgroup 0 a third time on a partial chunk of five hands
CHUNK_LOOP_CASES = [(TILE_MAJOR, 641), (TILE_MAJOR, 1285), (HAND_MAJOR, 4097), (HAND_MAJOR, 8197)]
WHOLE_BATCH_UP_TO = 1285                    # the oracle on every hand is cheap up to here; beyond, chunk_loop_hands()

# ---- configurations across a chunk edge: (side, center_idx, pose, new_skel, trans, scale); pose = PCA components or 'rot'
# (use_pca=False, [B, 15, 3, 3] rotations).  Centres 4, 8, 12, 16, 20 are finger tips: every vertex tile then skins the special
# vertices itself.  Every value of every factor at least twice; every tip centre with new_skel on and off; 'rot' with a tip
# centre and with None; 6 components with a tip centre (tests/test_kernels_on_cpu.py checks these properties of the table).
CONFIG_ROWS = [
    ('right', None, 45, False, True, True),
    ('left', None, 'rot', True, False, False),
    ('right', 0, 30, True, True, False),
    ('left', 0, 6, False, False, True),
    ('left', 9, 45, True, False, True),
    ('right', 9, 'rot', False, True, False),
    ('right', 4, 45, True, True, True),
    ('left', 4, 6, False, False, False),
    ('left', 8, 'rot', True, True, False),
    ('right', 8, 30, False, False, True),
    ('right', 12, 6, True, False, False),
    ('left', 12, 45, False, True, True),
    ('left', 16, 30, True, False, True),
    ('right', 16, 'rot', False, True, True),
    ('right', 20, 45, True, True, False),
    ('left', 20, 30, False, False, False),
    ('right', None, 6, False, False, True),
    ('left', 9, 30, False, True, True),
    ('right', 0, 'rot', True, False, False),
    ('left', 4, 45, False, True, False),
    ('right', 20, 6, True, False, True),
    ('left', 16, 45, True, False, False),
    ('right', 8, 'rot', True, True, True),
    ('left', 12, 30, True, True, False),
]
CONFIG_BATCHES = (17, 33)                   # one and two full chunks plus one hand
TIP_ROW_IN_CHUNK_LOOP = CONFIG_ROWS[6]      # also at B = 641, tile-major: the tip path inside the chunk loop
HOST_CONFIG_ROWS = [CONFIG_ROWS[i] for i in (0, 1, 6, 8, 12, 16)]      # the host rerun: tips 4, 8, 16; 'rot'; 6 and 30 components

# ---- pose extremes
EXTREME_ANGLES = (0.0, 1e-7, 1e-5, 1e-3, 3e-2, math.pi - 1e-3, math.pi, math.pi + 1e-3, 2 * math.pi - 1e-3, 2 * math.pi, 5.0, 9.0)
EXTREME_B = 17
EXTREME_OUTS = ('v', 'j', 'grad_pose', 'grad_shape', 'grad_root')


def row_id(row):
    side, center, pose, new_skel, trans, scale = row
    return '%s-c%s-%s-%s-%s%s' % (side, center, pose, 'newskel' if new_skel else 'skel', 't' if trans else '', 's' if scale else '')


def layer_for(row, device):
    from renderih_amd import assets
    from renderih_amd.manolayer import ManoLayer
    side, center, pose, new_skel = row[:4]
    return ManoLayer(assets.synthetic_mano_dict(side, seed=0), center_idx=center, use_pca=(pose != 'rot'),
                     new_skel=new_skel).to(device)


_CONSTANTS = {}


def oracle_constants(side, dtype, flat_mean=False):
    """flat_mean: hands_mean = 0, the counterpart of `layer.hands_mean.zero_()` (the layer reads its buffers at call time)."""
    from oracle import mano_oracle
    from renderih_amd import assets
    if (side, dtype, flat_mean) not in _CONSTANTS:
        c = mano_oracle.constants_from_dict(assets.synthetic_mano_dict(side, seed=0))
        if flat_mean:
            c['hands_mean'] = torch.zeros_like(c['hands_mean'])
        _CONSTANTS[(side, dtype, flat_mean)] = {k: (v.to(dtype) if torch.is_tensor(v) else v) for k, v in c.items()}
    return _CONSTANTS[(side, dtype, flat_mean)]


def random_inputs(B, seed, pose=45, trans=True, scale=True):
    """fp32 CPU inputs at the scales of test_mano_matches_oracle, and the weights wv, wj of the scalar that is differentiated."""
    from renderih_amd.manolayer import rodrigues_batch
    g = torch.Generator().manual_seed(seed)
    ins = {'root': rodrigues_batch(torch.randn(B, 3, generator=g))}
    if pose == 'rot':
        ins['pose'] = rodrigues_batch(torch.randn(B * 15, 3, generator=g) * 0.7).view(B, 15, 3, 3)
    else:
        ins['pose'] = torch.randn(B, pose, generator=g) * 0.7
    ins['shape'] = torch.randn(B, 10, generator=g)
    t, s = torch.randn(B, 3, generator=g) * 0.1, torch.rand(B, generator=g) + 0.5
    ins['trans'], ins['scale'] = (t if trans else None), (s if scale else None)
    ins['wv'], ins['wj'] = torch.randn(B, 778, 3, generator=g), torch.randn(B, 21, 3, generator=g)
    return ins


def run_oracle(row, ins, hands=None, dtype=torch.float64, flat_mean=False):
    """The oracle on the CPU in `dtype`, on the hands `hands` of the batch (all when None) -> v, j, grad_<input>."""
    from oracle import mano_oracle
    side, center, pose, new_skel = row[:4]
    pick = (lambda t: t) if hands is None else (lambda t: t[hands])
    leaves = {n: pick(ins[n]).to(dtype).clone().requires_grad_(True) for n in LEAVES if ins[n] is not None}
    v, j = mano_oracle.mano_forward(oracle_constants(side, dtype, flat_mean), leaves['root'], leaves['pose'], leaves['shape'],
                                    trans=leaves.get('trans'), scale=leaves.get('scale'), center_idx=center,
                                    use_pca=(pose != 'rot'), new_skel=new_skel)
    ((v * pick(ins['wv']).to(dtype)).sum() + (j * pick(ins['wj']).to(dtype)).sum()).backward()
    out = {'v': v.detach(), 'j': j.detach()}
    out.update({'grad_' + n: t.grad for n, t in leaves.items()})
    return out


def run_layer(layer, ins, device, variant=None, grad=True):
    """The layer on `device` with manolayer.VARIANT forced to `variant` for the forward (restored afterwards) -> v, j and, with
    `grad`, grad_<input> of (v * wv).sum() + (j * wj).sum().  Without `grad` the forward runs under no_grad: no workspace."""
    from renderih_amd import manolayer
    leaves = {n: ins[n].clone().to(device).requires_grad_(grad) for n in LEAVES if ins[n] is not None}
    old = manolayer.VARIANT
    try:
        if variant is not None:
            manolayer.VARIANT = variant
        with torch.enable_grad() if grad else torch.no_grad():
            v, j = layer(leaves['root'], leaves['pose'], leaves['shape'], trans=leaves.get('trans'), scale=leaves.get('scale'))
    finally:
        manolayer.VARIANT = old
    out = {'v': v.detach(), 'j': j.detach()}
    if grad:
        ((v * ins['wv'].to(device)).sum() + (j * ins['wj'].to(device)).sum()).backward()
        out.update({'grad_' + n: t.grad for n, t in leaves.items()})
    return out


def compare(got, want, hands, what):
    """Every element of the full batch finite; the hands `hands` (all when None) at the project's bar against `want`."""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in sorted(want):
        assert torch.isfinite(got[k]).all(), '%s %s: non-finite element' % (what, k)
        a = got[k] if hands is None else got[k][hands.to(got[k].device)]
        assert_close(a, want[k], RTOL, ATOL, '%s %s' % (what, k))


def assert_bit_identical(a, b, what):
    assert set(a) <= set(b), (sorted(a), sorted(b))
    for k in sorted(a):
        assert torch.equal(a[k], b[k]), '%s: %s differs in %d elements' % (what, k, int((a[k] != b[k]).sum()))


def chunk_loop_hands(B, grid, seed=0):
    """The hands a chunk-loop test compares with fp64 when the batch is too large for all of them: hand 0, the last hand of the
    first iteration's range (hands 0 .. 16 grid - 1), the first and last hand of every later chunk of group / workgroup 0
    (chunks grid, 2 grid, ...), both neighbours of every 16-hand edge among those, B - 1, and 48 further hands from a seeded
    generator.  Sorted LongTensor."""
    nchunks = -(-B // HC)
    picks = {0, min(HC, B) - 1, min(grid * HC, B) - 1, B - 1}
    for c in range(grid, nchunks, grid):
        picks |= {c * HC, min(c * HC + HC, B) - 1}
    for h in sorted(picks):
        if h % HC == 0:
            picks.add(h - 1)
        if h % HC == HC - 1:
            picks.add(h + 1)
    picks = {h for h in picks if 0 <= h < B}
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(seed)).tolist()
    picks |= set([h for h in perm if h not in picks][:48])
    return torch.tensor(sorted(picks))


def compared_hands(B, variant):
    return None if B <= WHOLE_BATCH_UP_TO else chunk_loop_hands(B, GRID[variant], seed=B)


# ------------------------------------------------------------------------------------------------ pose extremes
def pca_of_axis(layer, axis):
    """layer.axis2pca on the CPU (an fp32 inverse: the realised axis differs from the prescribed one in the last bits, so the
    oracle is fed this fp32 pose, not the axis)."""
    return (axis.reshape(-1, 45) - layer.hands_mean.cpu()).mm(layer.hands_components_inv.cpu())


def extreme_axis(seed=0):
    """[17, 45]: hand h turns joint h % 15 by EXTREME_ANGLES[h % 12] about a random direction, the other joints keep randn * 0.5.
    The first angle-0 hand (hand 0) is the whole zero pose -- exactly axis2pca(0), as the zero_pose golden; the second
    (hand 12) has the one joint at zero inside a random pose."""
    g = torch.Generator().manual_seed(seed)
    axis = torch.randn(EXTREME_B, 15, 3, generator=g) * 0.5
    for h in range(EXTREME_B):
        d = torch.randn(3, generator=g)
        axis[h, h % 15] = d / d.norm() * EXTREME_ANGLES[h % len(EXTREME_ANGLES)]
    axis[0] = 0.0
    return axis.reshape(EXTREME_B, 45)


def large_angle_axis(seed=1):
    """[17, 45]: every joint of every hand turned by an angle drawn uniformly from [2.5, 3.6] about a random direction."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn(EXTREME_B, 15, 3, generator=g)
    ang = 2.5 + 1.1 * torch.rand(EXTREME_B, 15, 1, generator=g)
    return (d / d.norm(dim=-1, keepdim=True) * ang).reshape(EXTREME_B, 45)


def extreme_inputs(layer, axis, seed):
    ins = random_inputs(axis.shape[0], seed, 45, trans=False, scale=False)
    ins['pose'] = pca_of_axis(layer, axis)
    return ins


def exact_zero_inputs(seed):
    """For a layer whose hands_mean is zeroed: hands 0 and 16 (one in each chunk) get pose = 0, so all their 15 axes are EXACTLY
    zero in the kernel -- the n > 0 ? ... : 0 branch of rodrigues_bwd, which axis2pca(0) on a non-zero mean only comes near."""
    ins = random_inputs(EXTREME_B, seed, 45, trans=False, scale=False)
    ins['pose'][0] = 0.0
    ins['pose'][EXTREME_B - 1] = 0.0
    return ins


def compare_extremes(got, ref32, ref64, tight, what):
    """Every output in EXTREME_OUTS: finite, and at most 4 x as far from fp64 as the fp32 oracle plus 2e-5 (of max |fp64|); those
    named in `tight` also at the project's bar.  Prints and returns {name: (kernel error, fp32-oracle error)}."""
    figures = {}
    for k in EXTREME_OUTS:
        assert torch.isfinite(got[k]).all(), '%s %s: non-finite element' % (what, k)
        a, b = got[k].detach().double().cpu(), ref64[k]
        used = float(((a - b).abs() / (RTOL * b.abs() + ATOL * b.abs().max())).max())      # share of the project's bar used
        print('%s %-10s kernel vs fp64 %.3g   fp32 oracle vs fp64 %.3g   (of max |fp64|)   kernel error / project bar %.3g'
              % ((what, k) + assert_fp32_equivalent(got[k], ref32[k], ref64[k], k=float('inf')) + (used,)))
        figures[k] = assert_fp32_equivalent(got[k], ref32[k], ref64[k], what='%s %s' % (what, k))
    for k in tight:
        assert_close(got[k], ref64[k], RTOL, ATOL, '%s %s' % (what, k))
    return figures


# ------------------------------------------------------------------------------------------------ quaternion front end
def quat_fused_vs_fp64_mirror(side, B, per_hand_betas, device, seed=0):
    """FusedQuatManoLayer (rih_mano_quat_fwd: always tile-major) against QuatManoLayer in fp64 on the CPU with every upstream
    gradient present and a translation.  Without per-hand betas the batch shares the layer's th_betas buffer (shape_stride 0), set
    to a non-zero vector on both layers; the layer defines no gradient for that buffer, so the shape gradient is compared in
    the run with per-hand betas.  Builders, `evaluate`, `compare` and the tolerance: tests/quat_mano_cases.py."""
    import numpy as np
    import quat_mano_cases as QC
    from renderih_amd.quat_mano import FusedQuatManoLayer, QuatManoLayer
    case = QC.seeded_case(B, 9000 + B + seed, betas=per_hand_betas, trans=True)
    case['center_idx'] = None
    mirror = QC.layer_for(QuatManoLayer, side, case, 'cpu', torch.float64)
    fused = QC.layer_for(FusedQuatManoLayer, side, case, device)
    if not per_hand_betas:
        shared = torch.from_numpy((np.random.RandomState(seed + 5).randn(1, 10) * 0.8).astype(np.float32))
        with torch.no_grad():
            mirror.th_betas.copy_(shared)
            fused.th_betas.copy_(shared)
    want = QC.evaluate(mirror, case, 'cpu', torch.float64)
    got = QC.evaluate(fused, case, device)
    expected = set(QC.OUTS) | {'grad_pose', 'grad_trans'} | ({'grad_betas'} if per_hand_betas else set())
    assert expected <= set(got) and expected <= set(want), (sorted(got), sorted(want))
    for k in expected:
        assert np.isfinite(got[k]).all(), k
    QC.compare(got, want, 'fused quaternion layer vs fp64 mirror %s B=%d' % (side, B))
    assert (got['transf'][:, :, 3] == np.float32([0, 0, 0, 1])).all()
    return got
