"""The pose optimiser's contact search (renderih_amd.contact_search; reference `search_anchors` / `update_scene` of
pose_data_optimize/batch_optimize_mocap_origin.py) on the CPU: the plain-torch mirror in fp64 and fp32 and the kernel
(csrc/rih_contact.hip) through the host-compiled library.  tests/test_gpu_contact_search.py runs the same checks on the GPU.

Bars (none of them taken from the code under test):
  golden    tests/golden/contact_search.npz holds the reference's own outputs on B = 4 frames at A = 108, V = 778 and a mask of
            DECIDED rows: those on which no discrete decision is within an fp32 rounding of flipping (a cosine 1e-4 from -0.6,
            two of the five smallest distances 1e-6 apart, a selected distance 1e-5 from the radius; make_contact_search_golden.py
            asserts that at most 5 % of a scene set and 10 % of a frame are undecided, and so does this file).  On decided rows
            ids, mask and vertex_contact are EQUAL; elastic meets the project's bar, rtol 1e-4 and atol 1e-5.
  crafted   8 anchors, each on its own triangle, with normals at chosen angles so that the rows have 0, 1, 2, 3, 4 and 5
            candidates that the against rule leaves (asserted): the rest of a row is filled from the against pairs, all at
            distance 1000, where the reference's order is unspecified and this project's is ascending j.  Every gap between
            two distances of a row, and of a distance to a radius, is above 1e-6 -- a hundred fp32 roundings of a 0.01
            distance -- and every cosine 0.04 from -0.6 (asserted in fp64), so the kernel equals the fp64 mirror in EVERY id,
            mask and contact.
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

from quat_mano_cases import ANCHOR_DIR  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'contact_search.npz')
RTOL, ATOL = 1e-4, 1e-5
KEYS = ('vertex_contact', 'anchor_id', 'anchor_elasti', 'anchor_padding_mask')
DTYPES = {'vertex_contact': torch.int64, 'anchor_id': torch.int64, 'anchor_elasti': torch.float32, 'anchor_padding_mask': torch.int64,
          'optimize_it': torch.bool}
SETS = (('fresh0', 'fresh', None, ''), ('fresh4', 'fresh', 'class4', ''), ('refresh', 'refresh', 'class4', '2'))
_CACHE = {}


def golden():
    if 'golden' not in _CACHE:
        z = np.load(GOLDEN)
        _CACHE['golden'] = {k: z[k] for k in z.files}
    return _CACHE['golden']


def check_result(res, B, A, D, device):
    assert tuple(res) == KEYS + ('optimize_it',)
    for k, shape in zip(res, ((B, A), (B, A, D), (B, A, D), (B, A, D), (B,))):
        assert tuple(res[k].shape) == shape and res[k].dtype == DTYPES[k] and res[k].device.type == torch.device(device).type, k
    assert torch.equal(res['optimize_it'], res['vertex_contact'].any(1))
    assert torch.equal(res['anchor_padding_mask'], (res['anchor_elasti'] > 0).long())


def compare(res, want, decided, what):
    """ids, mask, contact equal and elastic close on the rows of `decided` [B,A] (numpy bool)."""
    got = {k: res[k].cpu().numpy() for k in KEYS}
    for k in ('vertex_contact', 'anchor_id', 'anchor_padding_mask'):
        assert np.array_equal(got[k][decided], np.asarray(want[k])[decided]), '%s: %s' % (what, k)
    torch.testing.assert_close(torch.from_numpy(got['anchor_elasti'][decided]).double(),
                               torch.from_numpy(np.asarray(want['anchor_elasti'])[decided]).double(), rtol=RTOL, atol=ATOL,
                               msg=lambda m: '%s: elastic: %s' % (what, m))


def run_golden(cls, device, dtype=torch.float32, log=print):
    g = golden()
    for name, decided_key, table, suffix in SETS:
        decided = g[decided_key + '/decided']
        assert decided.shape == (4, 108) and 1 - decided.mean() <= 0.05 and (1 - decided.mean(1)).max() <= 0.10
        search = cls(ANCHOR_DIR, class_type=None if table is None else g[table]).to(device)
        vm, vs = (torch.from_numpy(g[k + suffix]).to(device=device, dtype=dtype) for k in ('verts_main', 'verts_sub'))
        assert vm.shape == (4, 778, 3)
        prev = torch.from_numpy(g['fresh4/anchor_id']).to(device) if name == 'refresh' else None
        res = search(vm, vs, prev)
        check_result(res, 4, 108, 4, device)
        want = {k: g['%s/%s' % (name, k)] for k in KEYS}
        compare(res, want, decided, '%s %s %s' % (cls.__name__, dtype, name))
        el = res['anchor_elasti'].cpu().numpy()
        log('%s %s on %s, %s: %d of %d rows decided; elastic within %.3g of the reference on them; %d rows in contact'
            % (cls.__name__, dtype, device, name, decided.sum(), decided.size,
               np.abs(el[decided] - want['anchor_elasti'][decided]).max(), int(want['vertex_contact'].sum())))
        if name == 'refresh':
            assert torch.equal(res['anchor_id'], prev)
    assert g['fresh0/vertex_contact'][3].sum() == 0 and g['fresh0/vertex_contact'][:3].sum() > 0       # the far frame, the near ones
    assert not np.array_equal(g['fresh0/anchor_elasti'], g['fresh4/anchor_elasti'])                    # the class table matters


# ------------------------------------------------------------------------------------------------ the crafted table
MAIN_ANGLES = (0.0, 10.0, 20.0, 30.0, 40.0, 180.0, 180.0, 180.0)
SUB_ANGLES = (-50.0, -40.0, -30.0, -20.0, -10.0, 100.0, 180.0, 5.0)          # -> 1, 2, 3, 4, 5, 0, 3, 5 facing main anchors
CRAFTED_CLASS = (0, 4, 1, 0, 4, 2, 0, 0)


def crafted(B=2, seed=0):
    """-> (face_vert_idx [8,3], weights [8,2]), verts_main, verts_sub [B,24,3] float64: anchor a sits on the triangle of the
    vertices 3a .. 3a+2, whose normal lies in the xy-plane at MAIN_ANGLES[a] / SUB_ANGLES[a] degrees; centres within 0.01."""
    rs = np.random.RandomState(900 + seed)
    fvi = np.arange(24).reshape(8, 3)
    w = rs.uniform(0.2, 0.4, size=(8, 2))
    verts = []
    for angles in (MAIN_ANGLES, SUB_ANGLES):
        th = np.radians(np.asarray(angles))
        t1, t2 = np.stack([-np.sin(th), np.cos(th), 0 * th], -1), np.tile([0.0, 0.0, 1.0], (8, 1))       # t1 x t2 = the normal
        c = rs.uniform(-0.006, 0.006, size=(B, 8, 3))
        s = rs.uniform(5e-4, 2e-3, size=(B, 8, 2, 1))
        verts.append(np.stack([c, c + s[:, :, 0] * t1, c + s[:, :, 1] * t2], 2).reshape(B, 24, 3))
    return (fvi, w), verts[0], verts[1]


def crafted_facts(search64, vm, vs):
    """In fp64: the number of main anchors the against rule leaves per row, the smallest gap between two distances of a row
    (and to the radii), the smallest distance of a cosine from the threshold."""
    main, n_main = search64._geometry(vm)
    sub, n_sub = search64._geometry(vs)
    cos = torch.einsum('bic,bjc->bij', -n_sub, n_main)
    dis = (sub[:, :, None] - main[:, None]).norm(dim=-1)
    srt = torch.sort(dis, dim=-1)[0]
    gap = min(float((srt[..., 1:] - srt[..., :-1]).min()), float((dis - search64.fresh_radius).abs().min()),
              float((dis - search64.refresh_radius).abs().min()))
    return (cos <= search64.against_cos).sum(-1), gap, float((cos - search64.against_cos).abs().min()), dis


def run_crafted(fused_cls, device, log=print):
    from renderih_amd.contact_search import TwoHandContactSearch
    anchor, vm64, vs64 = crafted()
    vm64, vs64 = torch.from_numpy(vm64), torch.from_numpy(vs64)
    for D in (4, 1):
        mirror = TwoHandContactSearch(anchor, class_type=CRAFTED_CLASS, dim=D)
        fused = fused_cls(anchor, class_type=CRAFTED_CLASS, dim=D).to(device)
        left, gap, cos_gap, dis = crafted_facts(mirror, vm64, vs64)
        assert gap > 1e-6 and cos_gap > 0.04
        for b in range(2):
            assert left[b].tolist() == [1, 2, 3, 4, 5, 0, 3, 5]
        want = mirror(vm64, vs64)
        if D == 4:                # rows with fewer than D candidates are filled from the against pairs in ascending j
            ids = want['anchor_id']
            assert ids[0, 5].tolist() == [0, 1, 2, 3] and ids[0, 0].tolist() == [0, 1, 2, 3] and ids[0, 1, 2:].tolist() == [2, 3]
            assert ids[0, 6, :3].sort()[0].tolist() == [5, 6, 7] and ids[0, 6, 3] == 0
            assert 0 < want['vertex_contact'].sum() and want['anchor_padding_mask'].sum() < want['anchor_padding_mask'].numel()
            assert (want['anchor_padding_mask'][:, 5] == 0).all()              # only against pairs: distance 1000, no contact
        for B in (2, 1):
            res = fused(vm64[:B].float().to(device), vs64[:B].float().to(device))
            check_result(res, B, 8, D, device)
            everything = np.ones((B, 8), bool)
            compare(res, {k: want[k][:B].numpy() for k in KEYS}, everything, 'crafted D=%d B=%d' % (D, B))
        # refresh on the other seed's positions with these ids, one of each kind of out-of-range id among them
        _, vm2, vs2 = crafted(seed=1)
        vm2, vs2 = torch.from_numpy(vm2), torch.from_numpy(vs2)
        assert crafted_facts(mirror, vm2, vs2)[1] > 1e-6
        prev = want['anchor_id'].clone()
        bad = [((0, 2, 0), -1), ((1, 7, D - 1), 8), ((1, 0, 0), 1 << 40), ((0, 4, D - 1), -(1 << 62))]
        for idx, v in bad:
            prev[idx] = v
        want_r = mirror(vm2, vs2, prev)
        res = fused(vm2.float().to(device), vs2.float().to(device), prev.to(device))
        check_result(res, 2, 8, D, device)
        compare(res, {k: want_r[k].numpy() for k in KEYS}, np.ones((2, 8), bool), 'crafted refresh D=%d' % D)
        assert torch.equal(res['anchor_id'].cpu(), prev)
        for idx, _ in bad:
            assert res['anchor_elasti'][idx] == 0 and res['anchor_padding_mask'][idx] == 0
        if D == 4:
            el = want_r['anchor_elasti']
            assert (el > 0).sum() > 4 and want_r['vertex_contact'].sum() > 0
    log('crafted table on %s: smallest distance gap %.3g, cosines at least %.3g from the threshold' % (device, gap, cos_gap))


def run_wide(fused_cls, device, A=136, log=print):
    """A table above 128 anchors, where the kernel takes its larger LDS array and every thread owns two rows: random triangles,
    against the fp64 mirror on the rows that are decided in fp64 by the golden's margins (every cosine 1e-4 from the threshold,
    the five smallest distances 1e-6 apart, the selected ones 1e-5 from the radii)."""
    from renderih_amd.contact_search import TwoHandContactSearch
    rs = np.random.RandomState(77)
    anchor = (np.arange(3 * A).reshape(A, 3), rs.uniform(0.2, 0.4, size=(A, 2)))
    cls = rs.randint(3, 6, size=A)
    c = rs.uniform(-0.025, 0.025, size=(2, 2, A, 1, 3))
    verts = torch.from_numpy((c + rs.uniform(-2e-3, 2e-3, size=(2, 2, A, 3, 3))).reshape(2, 2, 3 * A, 3))
    mirror, fused = TwoHandContactSearch(anchor, class_type=cls), fused_cls(anchor, class_type=cls).to(device)
    main, n_main = mirror._geometry(verts[0])
    sub, n_sub = mirror._geometry(verts[1])
    cos = torch.einsum('bic,bjc->bij', -n_sub, n_main)
    dis = (sub[:, :, None] - main[:, None]).norm(dim=-1)
    want = mirror(verts[0], verts[1])
    five = torch.sort(torch.where(cos > mirror.against_cos, torch.full_like(dis, float('inf')), dis), dim=-1)[0][..., :5]
    gaps = torch.where(torch.isfinite(five[..., 1:]), five[..., 1:] - five[..., :-1], torch.full_like(five[..., 1:], float('inf')))
    kept = dis.gather(2, want['anchor_id'])                                          # the true distances the refresh weighs
    decided = ((cos - mirror.against_cos).abs() > 1e-4).all(-1) & (gaps > 1e-6).all(-1) & \
        ((five[..., :4] - mirror.fresh_radius).abs() > 1e-5).all(-1) & ((kept - mirror.refresh_radius).abs() > 1e-5).all(-1)
    assert decided.float().mean() > 0.9 and decided[:, 128:].any()
    res = fused(verts[0].float().to(device), verts[1].float().to(device))
    check_result(res, 2, A, 4, device)
    compare(res, {k: want[k].numpy() for k in KEYS}, decided.numpy(), 'wide table fresh')
    want_r = mirror(verts[0], verts[1], want['anchor_id'])
    res_r = fused(verts[0].float().to(device), verts[1].float().to(device), want['anchor_id'].to(device))
    compare(res_r, {k: want_r[k].numpy() for k in KEYS}, decided.numpy(), 'wide table refresh')
    assert 0 < want['vertex_contact'].sum() < want['vertex_contact'].numel()
    log('wide table (A = %d) on %s: %d of %d rows decided' % (A, device, int(decided.sum()), decided.numel()))


def run_einval(lib, p, stream=None):
    """Every refusal of rih_contact_search (`p`: any valid pointer of the library's memory space; nothing is launched)."""
    einval = lib.rih_anchor_fwd(None, p, p, p, 1, 4, 1, None)
    ok = [p, p, p, p, p, None, 0.015, -0.6, 0.3, 4, p, p, p, p, 1, 24, 8, 4, stream]
    cases = [(i, None) for i in (0, 1, 2, 3, 4, 10, 11, 12, 13)] + [(14, 0), (15, 0), (16, 0), (17, 0), (16, 1025), (17, 9), (16, 3),
                                                                  (6, 0.0), (6, -1.0), (6, float('nan'))]
    for i, bad in cases:
        assert lib.rih_contact_search(*(ok[:i] + [bad] + ok[i + 1:])) == einval, (i, bad)


def run_refresh(fused_cls, device):
    """Fresh search on the golden's first meshes, refresh on its moved ones: against the fp64 mirror on the rows where no
    distance is within 1e-5 of the radius; two runs of either mode are bit-identical."""
    from renderih_amd.contact_search import TwoHandContactSearch
    g = golden()
    mirror, fused = TwoHandContactSearch(ANCHOR_DIR, class_type=g['class4']), fused_cls(ANCHOR_DIR, class_type=g['class4']).to(device)
    v = [torch.from_numpy(g[k]) for k in ('verts_main', 'verts_sub', 'verts_main2', 'verts_sub2')]
    vd = [x.to(device) for x in v]
    fresh = fused(vd[0], vd[1])
    res = fused(vd[2], vd[3], fresh['anchor_id'])
    prev = fresh['anchor_id'].cpu()
    want = mirror(v[2].double(), v[3].double(), prev)
    main, sub = mirror._geometry(v[2].double())[0], mirror._geometry(v[3].double())[0]
    dis = (sub[:, :, None] - main[:, None]).norm(dim=-1).gather(2, prev)
    decided = ((dis - mirror.refresh_radius).abs() > 1e-5).all(-1).numpy()
    assert decided.mean() > 0.95
    compare(res, {k: want[k].numpy() for k in KEYS}, decided, 'refresh after fresh')
    assert torch.equal(res['anchor_id'], fresh['anchor_id']) and not torch.equal(res['anchor_elasti'], fresh['anchor_elasti'])
    assert res['anchor_padding_mask'][:3].sum() > 0 and res['anchor_padding_mask'][3].sum() == 0
    for a, b in ((fresh, fused(vd[0], vd[1])), (res, fused(vd[2], vd[3], fresh['anchor_id']))):
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------ the CPU tests
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_mirror_matches_reference_on_decided_rows(dtype):
    from renderih_amd.contact_search import TwoHandContactSearch
    run_golden(TwoHandContactSearch, 'cpu', dtype)


def test_kernel_matches_reference_on_decided_rows_on_cpu():
    from host_kernels import host_kernels_abi
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    with host_kernels_abi():
        run_golden(FusedTwoHandContactSearch, 'cpu')


def test_kernel_orders_ties_by_ascending_index_on_cpu():
    from host_kernels import host_kernels_abi
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    with host_kernels_abi():
        run_crafted(FusedTwoHandContactSearch, 'cpu')


def test_kernel_above_128_anchors_on_cpu():
    from host_kernels import host_kernels_abi
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    with host_kernels_abi():
        run_wide(FusedTwoHandContactSearch, 'cpu')


def test_kernel_refresh_and_bit_identical_runs_on_cpu():
    from host_kernels import host_kernels_abi
    from renderih_amd.contact_search import FusedTwoHandContactSearch
    with host_kernels_abi():
        run_refresh(FusedTwoHandContactSearch, 'cpu')


def test_kernel_refuses_bad_arguments():
    from host_kernels import load
    buf = np.zeros(64, np.float64)
    run_einval(load(), buf.ctypes.data)


def test_surface_refuses_what_it_cannot_run():
    from renderih_amd.contact_search import FusedTwoHandContactSearch, TwoHandContactSearch
    anchor, vm, vs = crafted()
    vm, vs = torch.from_numpy(vm), torch.from_numpy(vs)
    with pytest.raises(ValueError):
        TwoHandContactSearch(anchor)                                              # no directory to read the class table from
    with pytest.raises(ValueError):
        TwoHandContactSearch(anchor, class_type=CRAFTED_CLASS[:7])
    for dim in (0, 9):
        with pytest.raises(ValueError):
            TwoHandContactSearch(anchor, class_type=CRAFTED_CLASS, dim=dim)
    with pytest.raises(ValueError):
        FusedTwoHandContactSearch((np.zeros((1025, 3), np.int64), np.zeros((1025, 2))), class_type=np.zeros(1025))
    mirror = TwoHandContactSearch(anchor, class_type=CRAFTED_CLASS)
    mirror.face_vert_idx[0, 0] = -1                                                 # a table that went bad after construction
    with pytest.raises(ValueError):
        mirror(vm, vs)
    mirror = TwoHandContactSearch(anchor, class_type=CRAFTED_CLASS)
    assert TwoHandContactSearch(ANCHOR_DIR).class_type.shape == (108,)             # merged_vertex_assignment.txt
    for bad in ((vm[:, :23], vs[:, :23]), (vm, vs[:1]), (vm, vs.float()), (vm[0], vs[0]), (vm.long(), vs.long())):
        with pytest.raises(ValueError):                                             # vertex 23 missing, shapes, dtypes
            mirror(*bad)
    with pytest.raises(ValueError):
        mirror(vm, vs, torch.zeros(2, 8, 3, dtype=torch.int64))
    with pytest.raises(ValueError):
        mirror(vm, vs, torch.zeros(2, 8, 4, dtype=torch.int32))
    fused = FusedTwoHandContactSearch(anchor, class_type=CRAFTED_CLASS)
    with pytest.raises(ValueError):
        fused(vm, vs)                                                               # fp32 only
    with pytest.raises(RuntimeError):
        fused(vm.float(), vs.float())                                               # GPU only: no CPU fallback
