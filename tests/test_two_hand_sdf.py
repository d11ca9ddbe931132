"""Two-hand penetration loss of the pose optimiser (renderih_amd.sdf.TwoHandSDFLoss / FusedTwoHandSDFLoss, csrc/rih_sdf_loss.hip
and the sparse voxeliser of csrc/rih_sdf.hip; reference pose_data_optimize/code_sdf/sdf_template.py `NewLoss`), on the CPU: the
torch mirror against values and gradients of the reference's own program (tests/golden/make_two_hand_sdf_golden.py), the real
kernels through the host-compiled library against the mirror and against an fp64 `grid_sample` on the same phi, sparse
against dense bit for bit, the three return forms, the argument checks.  tests/test_gpu_two_hand_sdf.py shares the helpers.

Tolerances (worked out from the formats, not from the code under test):
  per-vertex values  |err| <= 1e-5: the voxeliser's bar is 2e-6 per voxel (tests/test_sdf.py), carried through a convex
                     combination of 8 corners and multiplied by a weight <= 3 and 1/4 (or a scale < 1); fp32 rounding of an
                     index <= 31 moves a trilinear weight by ~2e-6 and phi <= 2, which stays below the rest of the bar.
  gradients          max |err| <= 2 * (2 * 2e-6) / (2 / (G - 1)) of max |want|: the phi bar on a corner difference over the
                     voxel pitch, times 2 for the fp32 trilinear arithmetic.
  loss               |err| <= sum of the per-vertex errors actually found + the fp32 summation bound 2V eps sum |terms|.
  flipped voxels     end-to-end against the golden a vertex is excused when one of its 8 corner voxels lies on the other side
                     of the surface for the kernel than for the CPU oracle (a parity ray grazing an edge flips with one
                     rounding); at most 0.5 % of a case's sampled vertices.
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, 'hipcpu'))

from test_sdf import icosphere  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'two_hand_sdf.npz')
PART_VERT = os.path.join(HERE, 'golden', 'part_vert.npy')
GOLDEN_CASES = ('g32', 'g16')
FIELDS = ('left', 'right', 'per_vert', 'left_oriscale', 'right_oriscale')
GRADS = ('grad_loss', 'grad_form2', 'grad_form3')
VALUE_TOL = 1e-5


def grad_tol(G):
    return 2 * (2 * 2e-6) / (2.0 / (G - 1))


# (bs, G, subdivision): 42 vertices / 80 faces and 162 / 320 -- F neither a multiple of the 128-face LDS tile nor of 64
SMALL_CASES = [(1, 8, 1), (3, 12, 2), (1, 12, 2), (3, 8, 1)]


def small_case(bs, G, sub):
    """vertices [bs,2,V,3], faces, integer weights 1..3.  Sample 0: two overlapping spheres of different size, so the big
    one lies partly outside the small one's cube (zero padding) and cells straddle the grid's faces.  Sample 1: disjoint
    (loss and gradient exactly 0).  Sample 2: nearly concentric, a deep penetration."""
    rs = np.random.RandomState(100 * bs + G + sub)
    pairs = [((0.50, (0.05, -0.02, 0.03)), (0.32, (0.42, 0.18, -0.11))),
             ((0.40, (0.0, 0.0, 0.0)), (0.35, (2.5, 0.3, -0.2))),
             ((0.45, (-0.2, 0.1, 0.0)), (0.38, (-0.12, 0.16, 0.07)))]
    verts = []
    for ra, rb in pairs[:bs]:
        va, faces = icosphere(ra[0], sub, ra[1])
        vb, _ = icosphere(rb[0], sub, rb[1])
        bump = 1 + 0.05 * rs.randn(va.shape[0], 1)
        verts.append(np.stack([(va - ra[1]) * bump + ra[1], vb]))
    verts = np.stack(verts).astype(np.float32)
    weight = rs.randint(1, 4, size=verts.shape[2]).astype(np.int32)
    return verts, faces, weight


def seeded_weights(bs, V, seed):
    rs = np.random.RandomState(seed)
    w = {k: rs.rand(bs, V).astype(np.float32) for k in ('w_left', 'w_right', 'w_ori_left', 'w_ori_right')}
    w['w_pv'] = rs.rand(bs, 2 * V).astype(np.float32)
    return w


def evaluate(crit, verts, wts, device, scale_factor=0.1):
    """All three return forms and the gradients the golden stores -> dict of numpy arrays."""
    t = lambda a: torch.as_tensor(a).to(device)
    out = {}
    v = t(verts).requires_grad_(True)
    loss = crit(v, scale_factor)
    assert loss.shape == (verts.shape[0],)
    out['loss'], out['grad_loss'] = loss, torch.autograd.grad(loss.sum(), v)[0]
    v = t(verts).requires_grad_(True)
    loss2, left, right = crit(v, scale_factor, return_per_vert_loss=True)
    out['left'], out['right'] = left, right
    out['grad_form2'] = torch.autograd.grad((t(wts['w_left']) * left).sum() + (t(wts['w_right']) * right).sum(), v)[0]
    v = t(verts).requires_grad_(True)
    loss3, pv, ori = crit(v, scale_factor, return_per_vert_loss=True, return_origin_scale_loss=True)
    assert isinstance(ori, list) and len(ori) == 2 and pv.shape == (verts.shape[0], 2 * verts.shape[2])
    out['per_vert'], out['left_oriscale'], out['right_oriscale'] = pv, ori[0], ori[1]
    out['grad_form3'] = torch.autograd.grad((t(wts['w_pv']) * pv).sum() + (t(wts['w_ori_left']) * ori[0]).sum() +
                                            (t(wts['w_ori_right']) * ori[1]).sum(), v)[0]
    out['loss2'], out['loss3'] = loss2, loss3
    return {k: x.detach().cpu().numpy() for k, x in out.items()}


def corner_voxels(verts, box, G):
    """For vertices [n,3] sampling the cube box = (cx, cy, cz, scale): voxel indices [n,8,3] (x, y, z) and their validity."""
    f = ((verts.astype(np.float32) - box[:3]) / box[3] + np.float32(1)) / np.float32(2) * np.float32(G - 1)
    i0 = np.floor(f).astype(np.int64)
    d = np.array([[(c >> a) & 1 for a in range(3)] for c in range(8)])
    idx = i0[:, None, :] + d[None]
    return idx, ((idx >= 0) & (idx < G)).all(-1)


def expected_flags(verts, box, G):
    """flags [bs,2,G,G,G] as rih_two_hand_prep defines them, restated in numpy from the kernel's own boxes."""
    bs = verts.shape[0]
    fl = np.zeros((bs, 2, G, G, G), np.uint8)
    for b in range(bs):
        for h in (0, 1):
            idx, ok = corner_voxels(verts[b, 1 - h], box[b, h], G)
            ii = idx[ok]
            fl[b, h][ii[:, 2], ii[:, 1], ii[:, 0]] = 1
    return fl


def excused(verts, debug, oracle_inside, G):
    """[bs,2,V] bool in the output order (left, right): vertices with a corner voxel on which kernel and oracle disagree."""
    phi, box = debug['phi'].cpu().numpy(), debug['box'].cpu().numpy()
    bs, _, V, _ = verts.shape
    ex = np.zeros((bs, 2, V), bool)
    for b in range(bs):
        for h in (0, 1):
            idx, ok = corner_voxels(verts[b, 1 - h], box[b, h], G)
            ii = np.clip(idx, 0, G - 1)
            mine = phi[b, h][ii[..., 2], ii[..., 1], ii[..., 0]] > 0
            theirs = oracle_inside[b, h][ii[..., 2], ii[..., 1], ii[..., 0]]
            ex[b, h] = ((mine != theirs) & ok).any(1)
    return ex


def compare(got, want, G, ex=None, report=None):
    """`got` against `want` (dicts of `evaluate`) at the module's tolerances; ex [bs,2,V]: excused vertices."""
    bs, V = got['left'].shape
    ex = np.zeros((bs, 2, V), bool) if ex is None else ex
    assert ex.sum() <= 0.005 * ex.size, 'excused %d of %d sampled vertices' % (ex.sum(), ex.size)
    keep = {'left': ~ex[:, 0], 'right': ~ex[:, 1], 'per_vert': ~ex.reshape(bs, 2 * V), 'left_oriscale': ~ex[:, 0],
            'right_oriscale': ~ex[:, 1]}
    worst = {}
    for k in FIELDS:
        worst[k] = float(np.abs(got[k] - want[k])[keep[k]].max(initial=0))
    # vertices[:, 0] (right) are the sampled ones of output index 1 and the other way round
    gkeep = np.stack([~ex[:, 1], ~ex[:, 0]], 1)
    for k in GRADS:
        scale = float(np.abs(want[k]).max())
        worst[k] = float(np.abs(got[k] - want[k])[gkeep].max(initial=0)) / scale if scale > 0 else float(np.abs(got[k]).max())
    pv_err = np.abs(got['per_vert'].astype(np.float64) - want['per_vert']).sum(1)
    sum_bound = 2 * V * np.finfo(np.float32).eps * np.abs(want['per_vert']).astype(np.float64).sum(1)
    loss_err = np.abs(got['loss'].astype(np.float64) - want['loss'])
    worst['loss_over_bound'] = float((loss_err / np.maximum(pv_err + sum_bound, 1e-30))[~ex.any((1, 2))].max(initial=0))
    if report is not None:
        report.update(worst, excused=int(ex.sum()))
    print('two_hand_sdf figures:', worst, 'excused', int(ex.sum()))
    for k in FIELDS:
        assert worst[k] <= VALUE_TOL, (k, worst[k])
    for k in GRADS:
        assert worst[k] <= grad_tol(G), (k, worst[k], grad_tol(G))
    assert (loss_err <= pv_err + sum_bound)[~ex.any((1, 2))].all(), (loss_err, pv_err + sum_bound)
    assert np.array_equal(got['loss'], got['loss2']) and np.array_equal(got['loss'], got['loss3'])
    assert np.array_equal(got['per_vert'], np.concatenate([got['left'], got['right']], 1))


def golden_case(name):
    z = np.load(GOLDEN)
    want = {k: z[name + '/' + k] for k in FIELDS + GRADS + ('loss',)}
    wts = {k: z[name + '/' + k] for k in ('w_left', 'w_right', 'w_ori_left', 'w_ori_right', 'w_pv')}
    G = int(z[name + '/grid'])
    verts = z[name + '/vertices']
    inside = np.unpackbits(z[name + '/oracle_inside'])[:verts.shape[0] * 2 * G ** 3].reshape(verts.shape[0], 2, G, G, G) > 0
    return verts, G, wts, want, inside


def fused_vs_golden(name, device, report=None):
    from renderih_amd.sdf import FusedTwoHandSDFLoss
    verts, G, wts, want, inside = golden_case(name)
    crit = FusedTwoHandSDFLoss(PART_VERT, grid_size=G).to(device)
    crit.keep_debug = True
    got = evaluate(crit, verts, wts, device)
    compare(got, want, G, excused(verts, crit.debug, inside, G), report)
    if name == 'g16':                                   # the far-apart sample: exactly nothing
        assert want['loss'][1] == 0 and got['loss'][1] == 0
        assert not any(got[k][1].any() for k in FIELDS + GRADS)


def fused_vs_mirror(bs, G, sub, device):
    """Small closed meshes: fused (sparse and dense) against the mirror, bit-identical repeats, sparse == dense bitwise,
    the flag array against its numpy restatement, exact zeros for the disjoint pair."""
    from renderih_amd.sdf import FusedTwoHandSDFLoss, TwoHandSDFLoss
    verts, faces, weight = small_case(bs, G, sub)
    wts = seeded_weights(bs, verts.shape[2], 5)
    mirror = TwoHandSDFLoss(weight, faces, grid_size=G).to(device)
    want = evaluate(mirror, verts, wts, device, 0.2)
    got = {}
    for sparse in (True, False):
        crit = FusedTwoHandSDFLoss(torch.from_numpy(weight), faces, grid_size=G, sparse=sparse).to(device)
        crit.keep_debug = True
        got[sparse] = evaluate(crit, verts, wts, device, 0.2)
        dbg = {k: v.cpu().numpy() for k, v in crit.debug.items()}
        again = evaluate(crit, verts, wts, device, 0.2)
        assert all(np.array_equal(got[sparse][k], again[k]) for k in got[sparse]), 'repeat is not bit-identical'
        fl = expected_flags(verts, dbg['box'], G)
        assert np.array_equal(dbg['flags'], fl)
        assert np.array_equal(dbg['count'], fl.reshape(bs * 2, -1).sum(1))
        assert (dbg['count'] <= min(G ** 3, 8 * verts.shape[2])).all()
        for m in range(2 * bs):
            assert np.array_equal(dbg['list'][m, :dbg['count'][m]], np.flatnonzero(fl.reshape(bs * 2, -1)[m]))
        lo, hi = verts.min(2), verts.max(2)
        assert np.array_equal(dbg['box'][..., :3], (lo + hi) / np.float32(2))
        assert np.array_equal(dbg['box'][..., 3], np.float32((1 + 0.2) * 0.5) * (hi - lo).max(-1))
        compare(got[sparse], want, G)
        if sparse:
            phi_sparse = dbg['phi']
        else:
            assert np.array_equal(phi_sparse[fl > 0], dbg['phi'][fl > 0])
    assert all(np.array_equal(got[True][k], got[False][k]) for k in got[True]), 'sparse and dense differ'
    assert (want['loss'][0] > 1e-3) and np.abs(want['grad_loss'][0]).max() > 1e-2
    if bs > 1:
        assert got[True]['loss'][1] == 0 and not any(got[True][k][1].any() for k in FIELDS + GRADS)
        assert dbg['count'][2:4].sum() == 0
    # zero padding is exercised: some sampled vertex of sample 0 has corners on both sides of the grid's boundary
    idx, ok = corner_voxels(verts[0, 0], dbg['box'][0, 1], G)
    assert (ok.any(1) & ~ok.all(1)).any() and (~ok.any(1)).any()
    return got[True], dbg


# ------------------------------------------------------------------------------------------------ tests
def test_part_weights_from_dict_file_and_vector(tmp_path):
    from renderih_amd.sdf import TwoHandSDFLoss, part_weights
    table = {0: {0, 1, 2}, 1: [2, 3, 3], 2: (1, 2)}
    w = part_weights(table, 5)
    assert w.dtype == torch.int32 and w.tolist() == [1, 2, 3, 1, 0]     # within a part an index counts once (indexed +=)
    np.save(tmp_path / 'pv.npy', table, allow_pickle=True)
    assert part_weights(str(tmp_path / 'pv.npy'), 5).tolist() == [1, 2, 3, 1, 0]
    assert part_weights(np.array([1, 2, 3, 1, 0]), 5).tolist() == [1, 2, 3, 1, 0]
    with pytest.raises(ValueError):
        part_weights({0: [7]}, 5)
    with pytest.raises(ValueError):
        part_weights(np.array([1.5, 1, 1, 1, 1]), 5)
    ref = part_weights(PART_VERT, 778)                                   # the reference's table: 934 entries, 778 vertices
    assert int(ref.sum()) == 934 and int(ref.min()) >= 1 and np.bincount(ref.numpy()).tolist() == [0, 627, 146, 5]
    crit = TwoHandSDFLoss(PART_VERT)                                     # faces default to the package's right hand
    assert crit.faces.shape == (1538, 3) and crit.weight.shape == (778,) and crit.robustifier is None
    with pytest.raises(ValueError):
        crit(torch.zeros(2, 778, 3))
    with pytest.raises(ValueError):
        crit(torch.zeros(1, 2, 777, 3))


def test_mirror_matches_reference_golden_g16():
    """The torch mirror, its voxeliser served by the CPU oracle (ABI emulator), against the reference's own forward and
    autograd.  The generator asserted that oracle and reference agree on the side of every sampled voxel: nothing excused."""
    from abi_emulator import emulated_abi
    from renderih_amd.sdf import TwoHandSDFLoss
    verts, G, wts, want, _ = golden_case('g16')
    crit = TwoHandSDFLoss(PART_VERT, grid_size=G)
    voxeliser, cache = crit.sdf, {}

    class Once(torch.nn.Module):                  # the three return forms voxelise the same meshes: ask the oracle once
        def forward(self, faces, vertices, grid_size):
            key = vertices.numpy().tobytes()
            if key not in cache:
                cache[key] = voxeliser(faces, vertices, grid_size)
            return cache[key]
    crit.sdf = Once()
    with emulated_abi():
        got = evaluate(crit, verts, wts, 'cpu')
    compare(got, want, G)
    assert got['loss'][1] == 0 and not got['grad_loss'][1].any() and not got['grad_form3'][1].any()


def test_fused_kernels_match_reference_golden_g16_on_cpu():
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        fused_vs_golden('g16', 'cpu')


@pytest.mark.parametrize('bs,G,sub', SMALL_CASES)
def test_fused_kernels_match_mirror_on_cpu(bs, G, sub):
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        fused_vs_mirror(bs, G, sub, 'cpu')


def test_fused_gradient_against_fp64_grid_sample_on_cpu():
    """Values and gradients of the sampling kernels against torch's grid_sample in fp64 on the kernels' own phi and boxes."""
    from host_kernels import host_kernels_abi
    from renderih_amd.sdf import FusedTwoHandSDFLoss
    bs, G, sub = 3, 12, 2
    verts, faces, weight = small_case(bs, G, sub)
    wts = seeded_weights(bs, verts.shape[2], 9)
    with host_kernels_abi():
        crit = FusedTwoHandSDFLoss(weight, faces, grid_size=G)
        crit.keep_debug = True
        got = evaluate(crit, verts, wts, 'cpu')
    phi, box = crit.debug['phi'].double(), crit.debug['box'].double()
    phi = phi * crit.debug['flags'].double()                      # the voxels that were not voxelised are never read

    class Restated(torch.nn.Module):
        def forward(self, v, scale_factor=0.1, return_per_vert_loss=False, return_origin_scale_loss=False):
            v = v.double()
            pv, ori = [], []
            for h in (0, 1):
                local = ((v[:, 1 - h] - box[:, h, None, :3]) / box[:, h, None, 3:]).view(bs, -1, 1, 1, 3)
                val = torch.nn.functional.grid_sample(phi[:, h].unsqueeze(1), local, align_corners=True).view(bs, -1)
                val = val * torch.from_numpy(weight).double()
                pv.append(val / 4)
                ori.append(val * box[:, h, 3:])
            pv, ori = torch.stack(pv, 1), torch.stack(ori, 1)
            return crit._returns((pv[:, 0] + pv[:, 1]).sum(1), pv, ori, return_per_vert_loss, return_origin_scale_loss)
    want = evaluate(Restated(), verts, wts, 'cpu')
    compare(got, want, G)


def test_argument_checks():
    """RIH_EINVAL (-1 is not assumed: whatever rih_sdf returns for a null pointer) for null pointers and sizes out of range."""
    from host_kernels import load
    lib = load()
    a = np.zeros(4096, np.float32)
    p = a.ctypes.data
    einval = lib.rih_sdf(None, p, p, 1, 1, 3, 8, None)
    assert einval != 0
    cap = min(8 ** 3, 8 * 4)
    assert lib.rih_two_hand_prep(None, 0.55, p, p, p, p, p, 1, 4, 8, cap, None) == einval
    assert lib.rih_two_hand_prep(p, 0.55, p, p, p, p, p, 0, 4, 8, cap, None) == einval
    assert lib.rih_two_hand_prep(p, 0.55, p, p, p, p, p, 1, 2, 8, cap, None) == einval          # V < 3
    assert lib.rih_two_hand_prep(p, 0.55, p, p, p, p, p, 1, 4, 1, cap, None) == einval          # G < 2
    assert lib.rih_two_hand_prep(p, 0.55, p, p, p, p, p, 1, 4, 257, cap, None) == einval
    assert lib.rih_two_hand_prep(p, 0.55, p, p, p, p, p, 1, 4, 8, cap - 1, None) == einval      # list too short for the worst case
    assert lib.rih_sdf_sparse(p, p, p, None, p, cap, 1, 1, 3, 8, None) == einval
    assert lib.rih_sdf_sparse(p, p, p, p, p, 0, 1, 1, 3, 8, None) == einval
    assert lib.rih_sdf_sparse(p, p, p, p, p, 8 ** 3 + 1, 1, 1, 3, 8, None) == einval
    assert lib.rih_sdf_sparse(p, p, p, p, p, cap, 0, 1, 3, 8, None) == einval
    assert lib.rih_two_hand_sample(p, p, p, None, p, p, p, p, 1, 4, 8, None) == einval
    assert lib.rih_two_hand_sample(p, p, p, p, p, p, p, p, 1, 4, 1, None) == einval
    assert lib.rih_two_hand_bwd(None, p, p, p, p, p, 1, 4, None) == einval
    assert lib.rih_two_hand_bwd(p, p, None, None, None, p, 0, 4, None) == einval
    assert lib.rih_two_hand_bwd(p, p, None, None, None, p, 1, 4, None) == 0                      # no upstream gradient: zeros
