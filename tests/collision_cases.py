"""Helpers of tests/test_collision.py (CPU) and tests/test_gpu_collision.py (GPU): the oracle, the cases and the checks of the
two-hand collision count (renderih_amd.collision, csrc/rih_collision.hip).

ORACLE.  `oracle_frame` is numpy fp64, written from the predicate and independent of renderih_amd:
    orient(a,b,c,d) = dot(cross(b - a, c - a), d - a); an edge (p,q) pierces a triangle (a,b,c) when orient(a,b,c,p) and
    orient(a,b,c,q) have strictly opposite signs and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all > 0 or all < 0; a
    pair intersects when one of its six edge-against-triangle tests pierces; a void face (a vertex that is not finite, or a
    normal cross(v1 - v0, v2 - v0) that is exactly zero) intersects nothing.
It evaluates every pair of a frame whose fp64 boxes overlap (disjoint boxes cannot intersect), all at once: no tiles, no chunks.
A discrete result cannot be compared with a tolerance, so the oracle also marks pairs as DECIDED (the contact search's
precedent).  With delta = 1e-4 L^3, L the mean |v1 - v0| over the frame's main faces: a piercing test is a robust hit if it hits
with all five determinants beyond delta; a robust miss if the two plane determinants have the same sign, both beyond delta, or
two of the three edge determinants have opposite signs, both beyond delta.  A pair is decided if one test is a robust hit or all
six are robust misses.  An fp32 determinant of such vectors is off by a few 1e-7 L^3, so delta is some hundred roundings.

BARS, with H = the decided intersecting pairs of a frame and U = its undecided pairs:
    H <= count <= H + U, the same per row of pairs_main and per column of pairs_sub;
    pairs_main.sum(1) == pairs_sub.sum(1) == count exactly;
    U <= max(3, 3 % of H) per frame (a property of the cases, asserted so that the bars stay tight).
The crafted pairs have small-integer coordinates, every determinant is exact in fp32, and the expected count is exact.
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

GOLDEN = os.path.join(HERE, 'golden', 'contact_search.npz')
KEYS = ('pairs_main', 'pairs_sub', 'count')
_CACHE = {}


# ------------------------------------------------------------------------------------------------ the oracle
def _det(u, v, w):
    return np.einsum('...c,...c->...', np.cross(u, v), w)


def _edge_test(p, q, a, b, c, delta):
    """-> hit, robust hit, robust miss, each [K] bool."""
    dp, dq = _det(b - a, c - a, p - a), _det(b - a, c - a, q - a)
    s = [_det(q - p, a - p, b - p), _det(q - p, b - p, c - p), _det(q - p, c - p, a - p)]
    hit = (((dp > 0) & (dq < 0)) | ((dp < 0) & (dq > 0))) & \
        (((s[0] > 0) & (s[1] > 0) & (s[2] > 0)) | ((s[0] < 0) & (s[1] < 0) & (s[2] < 0)))
    beyond = (np.abs(dp) > delta) & (np.abs(dq) > delta) & (np.abs(s[0]) > delta) & (np.abs(s[1]) > delta) & (np.abs(s[2]) > delta)
    miss = ((dp > delta) & (dq > delta)) | ((dp < -delta) & (dq < -delta))
    for x, y in ((s[0], s[1]), (s[1], s[2]), (s[0], s[2])):
        miss |= ((x > delta) & (y < -delta)) | ((x < -delta) & (y > delta))
    return hit, hit & beyond, miss


def oracle_frame(vm, vs, fm, fs):
    """vm [Vm,3], vs [Vs,3] (any float, taken to fp64), fm [Fm,3], fs [Fs,3] -> dict: per row / column / frame the decided hits
    ('h_main' [Fm], 'h_sub' [Fs], 'H'), the undecided pairs ('u_main', 'u_sub', 'U'), all hits whether decided or not ('all')."""
    vm, vs = np.asarray(vm, np.float64), np.asarray(vs, np.float64)
    tm, ts = vm[fm], vs[fs]                                                             # [F,3,3]
    L = np.linalg.norm(tm[:, 1] - tm[:, 0], axis=-1)
    delta = 1e-4 * np.mean(L[np.isfinite(L)]) ** 3
    with np.errstate(invalid='ignore'):
        okm = np.isfinite(tm).all((1, 2)) & (np.cross(tm[:, 1] - tm[:, 0], tm[:, 2] - tm[:, 0]) != 0).any(-1)
        oks = np.isfinite(ts).all((1, 2)) & (np.cross(ts[:, 1] - ts[:, 0], ts[:, 2] - ts[:, 0]) != 0).any(-1)
        near = (tm.min(1)[:, None] <= ts.max(1)[None]).all(-1) & (ts.min(1)[None] <= tm.max(1)[:, None]).all(-1)
    near &= okm[:, None] & oks[None]
    i, j = np.nonzero(near)
    m, s = tm[i], ts[j]
    hit = np.zeros(i.shape, bool)
    robust_hit = np.zeros(i.shape, bool)
    all_miss = np.ones(i.shape, bool)
    for k in range(3):
        for p, q, t in ((m[:, k], m[:, (k + 1) % 3], s), (s[:, k], s[:, (k + 1) % 3], m)):
            h, rh, rm = _edge_test(p, q, t[:, 0], t[:, 1], t[:, 2], delta)
            hit |= h
            robust_hit |= rh
            all_miss &= rm
    assert not (robust_hit & all_miss).any()
    decided = robust_hit | all_miss
    Fm, Fs = len(fm), len(fs)
    dh, un = decided & hit, ~decided
    return {'h_main': np.bincount(i[dh], minlength=Fm), 'h_sub': np.bincount(j[dh], minlength=Fs), 'H': int(dh.sum()),
            'u_main': np.bincount(i[un], minlength=Fm), 'u_sub': np.bincount(j[un], minlength=Fs), 'U': int(un.sum()),
            'all': int(hit.sum()), 'near': int(near.sum()), 'delta': delta}


def oracle(name, vm, vs, fm, fs):
    """One oracle per named frame set, computed once and shared by every test of the session."""
    if name not in _CACHE:
        _CACHE[name] = [oracle_frame(vm[b], vs[b], fm, fs) for b in range(vm.shape[0])]
    return _CACHE[name]


# ------------------------------------------------------------------------------------------------ the checks
def check_result(res, B, Fm, Fs, device):
    assert tuple(res) == KEYS
    for k, shape in zip(KEYS, ((B, Fm), (B, Fs), (B,))):
        assert tuple(res[k].shape) == shape and res[k].dtype == torch.int32 and res[k].device.type == torch.device(device).type, k
    assert torch.equal(res['pairs_main'].sum(1), res['count'].long()) and torch.equal(res['pairs_sub'].sum(1), res['count'].long())
    assert int(res['pairs_main'].min()) >= 0 and int(res['pairs_sub'].min()) >= 0


def check_bars(res, want, what, log=print, cap=True):
    got = {k: res[k].cpu().numpy().astype(np.int64) for k in KEYS}
    for b, o in enumerate(want):
        log('%s frame %d: H %d U %d (all fp64 hits %d, %d pairs with overlapping boxes), count %d'
            % (what, b, o['H'], o['U'], o['all'], o['near'], got['count'][b]))
        if cap:
            assert o['U'] <= max(3, 0.03 * o['H']), '%s frame %d: %d undecided pairs beside %d decided hits' % (what, b, o['U'], o['H'])
        assert o['H'] <= got['count'][b] <= o['H'] + o['U'], '%s frame %d: count' % (what, b)
        assert ((o['h_main'] <= got['pairs_main'][b]) & (got['pairs_main'][b] <= o['h_main'] + o['u_main'])).all(), '%s frame %d: rows' % (what, b)
        assert ((o['h_sub'] <= got['pairs_sub'][b]) & (got['pairs_sub'][b] <= o['h_sub'] + o['u_sub'])).all(), '%s frame %d: columns' % (what, b)


def run(counter, vm, vs, device, dtype=torch.float32):
    """numpy fp32 frames -> the counter's result (`counter` already sits on `device`)."""
    res = counter(torch.from_numpy(vm).to(device=device, dtype=dtype), torch.from_numpy(vs).to(device=device, dtype=dtype))
    check_result(res, vm.shape[0], counter.faces_main.shape[0], counter.faces_sub.shape[0], device)
    return res


# ------------------------------------------------------------------------------------------------ 1. the fixture's frames
def fixture(suffix=''):
    if 'golden' not in _CACHE:
        z = np.load(GOLDEN)
        _CACHE['golden'] = {k: z[k] for k in ('verts_main', 'verts_sub', 'verts_main2', 'verts_sub2')}
    g = _CACHE['golden']
    return g['verts_main' + suffix].astype(np.float32), g['verts_sub' + suffix].astype(np.float32)


def run_fixture(cls, device, dtype=torch.float32, log=print):
    """The 8 frames of tests/golden/contact_search.npz (the reference manopth layer's meshes) with the default 1538-face table;
    frame 3 of either set is the far one."""
    counter = cls().to(device)
    faces = counter.faces_main.cpu().numpy()
    assert faces.shape == (1538, 3) and torch.equal(counter.faces_main, counter.faces_sub)
    for suffix in ('', '2'):
        vm, vs = fixture(suffix)
        assert vm.shape == (4, 778, 3)
        want = oracle('fixture' + suffix, vm, vs, faces, faces)
        res = run(counter, vm, vs, device, dtype)
        check_bars(res, want, '%s %s on %s, fixture%s' % (cls.__name__, dtype, device, suffix), log)
        assert all(o['H'] > 400 for o in want[:3]) and want[3]['H'] == 0 and want[3]['near'] == 0 and int(res['count'][3]) == 0


# ------------------------------------------------------------------------------------------------ 2. exact crafted pairs
# (main triangle, sub triangle, intersecting pairs): small integers, so every determinant is exact in fp32
CRAFTED = (
    ('piercing', ((0, 0, 0), (4, 0, 0), (0, 4, 0)), ((1, 1, -1), (1, 1, 1), (5, 5, 1)), 1),
    ('disjoint with overlapping boxes', ((0, 0, 0), (4, 0, 0), (0, 4, 0)), ((3, 3, -1), (3, 3, 1), (4, 4, 1)), 0),
    ('coplanar and overlapping', ((0, 0, 0), (4, 0, 0), (0, 4, 0)), ((1, 1, 0), (5, 1, 0), (1, 5, 0)), 0),
    ('touching at a vertex', ((0, 0, 0), (4, 0, 0), (0, 4, 0)), ((1, 1, 0), (1, 1, 2), (3, 3, 2)), 0),
    ('touching along an edge', ((0, 0, 0), (4, 0, 0), (0, 4, 0)), ((0, 0, 0), (4, 0, 0), (0, 0, 3)), 0),
    ('zero area through the other', ((0, 0, 0), (4, 0, 0), (0, 4, 0)), ((1, 1, -1), (1, 1, 1), (1, 1, 3)), 0),
    # the main triangle is large and its edges pass far outside the small sub triangle, one of whose edges goes through it
    ('only an edge of the sub face pierces', ((-8, -8, 0), (8, -8, 0), (0, 8, 0)), ((0, 0, -1), (0, 0, 1), (1, 0, 1)), 1),
)


def run_crafted(cls, device, dtype=torch.float32, log=print):
    faces = np.array([[0, 1, 2]])                     # V = 6 per hand: three vertices no face names follow the triangle's
    counter = cls(faces, faces).to(device)
    pad = np.full((3, 3), 50.0)
    vm = np.stack([np.concatenate([np.asarray(m, np.float64), pad]) for _, m, _, _ in CRAFTED]).astype(np.float32)
    vs = np.stack([np.concatenate([np.asarray(s, np.float64), -pad]) for _, _, s, _ in CRAFTED]).astype(np.float32)
    assert vm.shape == (len(CRAFTED), 6, 3)
    want = [n for _, _, _, n in CRAFTED]
    ora = oracle('crafted', vm, vs, faces, faces)
    assert [o['all'] for o in ora] == want                                          # the fp64 predicate
    assert [o['near'] for o in ora] == [0 if c[0].startswith('zero area') else 1 for c in CRAFTED]   # every box overlaps; one void face
    long_edge = _edge_test(*[np.asarray(x, np.float64)[None] for x in (CRAFTED[5][2][0], CRAFTED[5][2][2]) + CRAFTED[5][1]], 0.0)
    assert long_edge[0].all()                         # without the void rule the zero-area face's long edge would pierce
    tm, ts = vm[:, :3].astype(np.float64), vs[:, :3].astype(np.float64)
    only_sub = len(CRAFTED) - 1                       # the last pair: none of the main face's edges pierces the sub face
    for k in range(3):
        assert not _edge_test(tm[only_sub:, k], tm[only_sub:, (k + 1) % 3], ts[only_sub:, 0], ts[only_sub:, 1], ts[only_sub:, 2], 0.0)[0].any()
    for cut in (slice(None), slice(0, 1), slice(only_sub, None)):
        res = run(counter, vm[cut], vs[cut], device, dtype)
        for k in KEYS:
            assert res[k].cpu().reshape(-1).tolist() == want[cut], (k, [c[0] for c in CRAFTED])
    swapped = run(counter, vs, vm, device, dtype)      # the roles exchanged: the first three tests alone on the last pair
    assert swapped['count'].cpu().tolist() == want
    log('%s %s on %s: the %d crafted pairs give %s' % (cls.__name__, dtype, device, len(CRAFTED), want))


# ------------------------------------------------------------------------------------------------ 3.-5. triangle soups
def soup(seed, B, Fm, Fs, box, size):
    """Per frame and hand a soup of triangles, each with its own three vertices: centres uniform in a box of half-width `box`,
    corners within +-`size` of the centre; rounded to fp32.  -> vm [B,3Fm,3], vs [B,3Fs,3], faces_main, faces_sub."""
    rs = np.random.RandomState(seed)
    out = []
    for F in (Fm, Fs):
        c = rs.uniform(-box, box, size=(B, F, 1, 3))
        out.append((c + rs.uniform(-size, size, size=(B, F, 3, 3))).reshape(B, 3 * F, 3).astype(np.float32))
    return out[0], out[1], np.arange(3 * Fm).reshape(Fm, 3), np.arange(3 * Fs).reshape(Fs, 3)


# name: (seed, B, Fm, Fs, box, size, least decided hits over the frames together)
SOUPS = {
    'one pair': (11, 3, 1, 1, 0.005, 0.02, 1),
    'below a tile B=1': (1, 1, 63, 65, 0.05, 0.02, 20), 'below a tile B=3': (2, 3, 63, 65, 0.05, 0.02, 60),
    'quarter tile B=1': (3, 1, 64, 64, 0.05, 0.02, 20), 'quarter tile B=3': (4, 3, 64, 64, 0.05, 0.02, 60),
    'past a tile B=1': (5, 1, 257, 130, 0.08, 0.02, 20), 'past a tile B=3': (6, 3, 257, 130, 0.08, 0.02, 60),
    'survivor-list pressure': (7, 1, 300, 300, 0.01, 0.02, 10000),
    'wide tables': (8, 1, 1538, 700, 0.15, 0.01, 20),
    'sub table above 1538 faces': (9, 2, 130, 2000, 0.08, 0.01, 20),
}
EDGE_SOUPS = tuple(k for k in SOUPS if k[-3:-1] == 'B=') + ('one pair',)


def run_soup(cls, device, name, dtype=torch.float32, log=print):
    seed, B, Fm, Fs, box, size, least = SOUPS[name]
    vm, vs, fm, fs = soup(seed, B, Fm, Fs, box, size)
    assert vm.shape[1] != vs.shape[1] or Fm == Fs
    want = oracle(name, vm, vs, fm, fs)
    assert sum(o['H'] for o in want) >= least, (name, [o['H'] for o in want])
    if name == 'survivor-list pressure':              # more than half of all pairs overlap in boxes: every chunk's list fills
        assert want[0]['near'] > 0.5 * Fm * Fs
    counter = cls(fm, fs).to(device)
    res = run(counter, vm, vs, device, dtype)
    check_bars(res, want, '%s %s on %s, %s (Fm %d, Fs %d)' % (cls.__name__, dtype, device, name, Fm, Fs), log)
    return counter, vm, vs, fm, fs, res


# ------------------------------------------------------------------------------------------------ 6. runtime properties
def run_repeat(cls, device):
    """Two runs are bit-identical (the survivor lists' order may vary; the integer sums may not)."""
    counter = cls().to(device)
    vm, vs = fixture()
    a, b = run(counter, vm, vs, device), run(counter, vm, vs, device)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    assert int(a['count'].sum()) > 0


def run_offset(cls, device, log=print):
    """A frame moved by (5, -3, 2): the fp32 inputs are moved, the oracle sees the moved fp32 values, the bars hold as before
    and the decided hits are those of the frame at the origin up to the pairs the move's roundings left undecided."""
    seed, B, Fm, Fs, box, size, _ = SOUPS['past a tile B=1']
    vm, vs, fm, fs = soup(seed, B, Fm, Fs, box, size)
    off = np.array([5.0, -3.0, 2.0], np.float32)
    vmo, vso = vm + off, vs + off
    assert vmo.dtype == np.float32
    home, want = oracle('past a tile B=1', vm, vs, fm, fs), oracle('moved', vmo, vso, fm, fs)
    counter = cls(fm, fs).to(device)
    res = run(counter, vmo, vso, device)
    check_bars(res, want, '%s on %s, moved by (5, -3, 2)' % (cls.__name__, device), log)
    assert abs(want[0]['H'] - home[0]['H']) <= want[0]['U'] + home[0]['U'] + 3 and want[0]['H'] >= 20


def run_nan(cls, device, log=print):
    """A NaN vertex zeroes the pairs of the faces that name it and no others; the call returns normally."""
    counter = cls().to(device)
    faces = counter.faces_main.cpu().numpy()
    vm, vs = fixture()
    home = oracle('fixture', vm, vs, faces, faces)
    v = int(np.argmax(np.bincount(faces[home[2]['h_main'] > 0].reshape(-1), minlength=778)))   # a vertex of many hitting faces
    vm = vm[2:3].copy()
    vm[0, v, 1] = np.nan
    want = oracle('nan', vm, vs[2:3], faces, faces)
    res = run(counter, vm, vs[2:3], device)
    named = (faces == v).any(1)
    assert home[2]['h_main'][named].sum() > 0 and want[0]['h_main'][named].sum() == 0 and want[0]['u_main'][named].sum() == 0
    assert int(res['pairs_main'][0].cpu()[torch.from_numpy(named)].sum()) == 0
    check_bars(res, want, '%s on %s, a NaN vertex' % (cls.__name__, device), log, cap=False)
    assert 1000 < want[0]['H'] < home[2]['H']
    log('NaN in vertex %d: %d faces name it, %d decided hits left of %d' % (v, named.sum(), want[0]['H'], home[2]['H']))


def run_einval(lib, p, stream=None):
    """Every refusal of rih_collision_count (`p`: any valid pointer of the library's memory space; nothing is launched)."""
    einval = lib.rih_anchor_fwd(None, p, p, p, 1, 4, 1, None)
    ok = [p, p, p, p, p, p, p, 1, 6, 6, 1, 1, stream]
    cases = [(i, None) for i in range(7)] + [(i, bad) for i in range(7, 12) for bad in (0, -1)] + [(7, 1 << 30)]
    for i, bad in cases:
        args = ok[:i] + [bad] + ok[i + 1:]
        if bad == 1 << 30:
            args[10] = 1025                            # 2^30 frames x 5 tiles: more workgroups than a grid holds
        assert lib.rih_collision_count(*args) == einval, (i, bad)


def run_bad_table(cls, device):
    vm, vs, fm, fs = soup(1, 1, 4, 5, 0.05, 0.02)
    vm, vs = torch.from_numpy(vm).to(device), torch.from_numpy(vs).to(device)
    for bad_m, bad_s in ((12, None), (-1, None), (None, 15), (None, -1)):
        a, b = fm.copy(), fs.copy()
        if bad_m is not None:
            a[3, 2] = bad_m
        if bad_s is not None:
            b[0, 0] = bad_s
        with pytest.raises(ValueError):
            cls(a, b).to(device)(vm, vs)               # refused on the host, before any launch
    counter = cls(fm, fs).to(device)
    with pytest.raises(ValueError):
        counter(vm[:, :11], vs)                        # vertex 11 of the main hand is missing
    for bad in ((vm, vs[0]), (vm, vs.double()), (vm.long(), vs.long()), (vm, torch.cat([vs, vs]))):
        with pytest.raises(ValueError):
            counter(*bad)
    for table in (np.zeros((0, 3), np.int64), np.zeros((2, 4), np.int64), np.zeros((2, 3))):
        with pytest.raises(ValueError):
            cls(table)


# ------------------------------------------------------------------------------------------------ 7. filter_sequence
def run_filter(opt_cls, counter_cls, device, log=print, **kw):
    """N = 5 in batches of 2 + 2 + 1 against the same composition written out here; `valid` flips exactly at the count."""
    from renderih_amd.collision import filter_sequence
    from renderih_amd.pose_driver import scene_meshes
    from test_pose_driver import real_sequence
    from test_pose_opt import make
    opt = make(opt_cls, device, **kw)
    counter = counter_cls().to(device)
    seq = real_sequence(N=5)
    rows = [torch.from_numpy(x.copy()).to(opt.dtype) for x in seq]
    counts = []
    for cut in (slice(0, 2), slice(2, 4), slice(4, 5)):
        vm, vs = scene_meshes(opt, *[x[cut] for x in rows])
        assert vm.shape == (cut.stop - cut.start, 778, 3)
        counts.append(counter(vm, vs)['count'].cpu())
    want = torch.cat(counts)
    got = filter_sequence(opt, counter, *seq, max_pairs=int(want.max()), batch_size=2)
    assert tuple(got) == ('count', 'valid') and got['count'].dtype == torch.int32 and got['valid'].dtype == torch.bool
    assert got['count'].device.type == 'cpu' and got['valid'].device.type == 'cpu' and got['count'].shape == (5,)
    assert torch.equal(got['count'], want) and got['valid'].all() and int(want.max()) > 0
    for n in (int(want.argmin()), 4):                  # the frame that flips first, and the one of the short last batch
        c = int(want[n])
        at = filter_sequence(opt, counter, *seq, max_pairs=c, batch_size=2)
        assert torch.equal(at['count'], want) and bool(at['valid'][n]) and torch.equal(at['valid'], want <= c)
        if c > 0:
            below = filter_sequence(opt, counter, *seq, max_pairs=c - 1, batch_size=5)
            assert torch.equal(below['count'], want) and not bool(below['valid'][n]) and torch.equal(below['valid'], want <= c - 1)
    # what optimize_sequence returns goes straight in
    out = {'right': {'rot': rows[0], 'loc': rows[1]}, 'left': {'rot': rows[2], 'loc': rows[3]}}
    again = filter_sequence(opt, counter, out['right']['rot'], out['right']['loc'], out['left']['rot'], out['left']['loc'], seq[4],
                            max_pairs=0, batch_size=3)
    assert torch.equal(again['count'], want) and torch.equal(again['valid'], want <= 0)
    with pytest.raises(TypeError):
        filter_sequence(opt, counter, *seq, batch_size=2)                               # max_pairs has no default
    for bad in (dict(batch_size=0), dict(max_pairs=-1), dict(max_pairs=1.5)):
        with pytest.raises(ValueError):
            filter_sequence(opt, counter, *seq, **dict(dict(max_pairs=3, batch_size=2), **bad))
    with pytest.raises(ValueError):
        filter_sequence(opt, counter, seq[0][:4], *seq[1:], max_pairs=3, batch_size=2)
    log('filter_sequence on %s: counts %s' % (device, want.tolist()))
