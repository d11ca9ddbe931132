"""The collision gate behind the pose optimiser -- pose_data_optimize/collision/CollisionFilter.py and CollisionCheck.py, which
rebuild both hand meshes per frame on the CPU, hand them to trimesh / FCL and keep a frame whose number of reported contacts
stays under a threshold (75 in the filter, 100 in the check) -- for a batch of frames on the device.

WHAT IS COUNTED.  FCL reports contact POINTS, up to several per intersecting triangle pair, a number that depends on its
clipping code and cannot be pinned without it.  This module counts INTERSECTING TRIANGLE PAIRS, which is defined exactly: every
intersecting pair gives FCL at least one contact, so pairs <= contacts and a threshold on pairs is the looser of the two.  The
reference's 75 and 100 do not carry over: `max_pairs` has no default.

The predicate (shared by csrc/rih_collision.hip, by the mirror below and by the tests' oracle):
    orient(a,b,c,d) = dot(cross(b - a, c - a), d - a)
    an edge (p,q) pierces a triangle (a,b,c) when orient(a,b,c,p) and orient(a,b,c,q) have strictly opposite signs (decided by
      comparisons) and orient(p,q,a,b), orient(p,q,b,c), orient(p,q,c,a) are all > 0 or all < 0;
    main face i and sub face j intersect when their axis-aligned boxes overlap (<=; disjoint boxes cannot intersect) and one of
      the six edge-against-triangle tests pierces: the three edges of i against j, the three edges of j against i.
Everything is strict: coplanar, touching and zero-area configurations do not intersect, nor does a comparison with a NaN in it.
A VOID face -- a vertex that is not finite, or a normal cross(v1 - v0, v2 - v0) that is exactly zero -- intersects nothing
(otherwise the edge between the two good vertices of a face with a NaN, or the long edge of a zero-area face, could still
pierce).  Differences are taken from a vertex of the pair, so the hands' distance from the origin does not matter.

`TwoHandCollisionCount` is the plain-torch mirror (any floating dtype, any device); `FusedTwoHandCollisionCount` is the same
surface on rih_collision_count (one launch, outputs stay on the device; fp32 GPU tensors only).  Both return
{'pairs_main' [B,Fm] int32, 'pairs_sub' [B,Fs] int32, 'count' [B] int32}.  `filter_sequence` applies a counter to the sequences
that `pose_driver.optimize_sequence` returns.  Out of scope: FCL's contact points, self-collision within one hand, penetration depth.
"""
import numpy as np
import torch

from . import assets, ops
from .ops import check
from .pose_driver import _sequence, scene_meshes

MIRROR_PAIRS = 1 << 22                        # box tests the mirror holds at once (B x chunk of main faces x Fs)


def _faces(table):
    f = np.asarray(table.detach().cpu() if torch.is_tensor(table) else table)
    if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1 or f.dtype.kind not in 'iu':
        raise ValueError('a face table must be integer [F,3] with F >= 1; got %s %s' % (f.dtype, f.shape))
    return torch.from_numpy(f.astype(np.int64))


def _orient_parts(tri):
    return tri[:, 0], tri[:, 1], tri[:, 2]


def _pierces(p, q, a, b, c, n):
    dp, dq = ((p - a) * n).sum(-1), ((q - a) * n).sum(-1)
    d, A, B, C = q - p, a - p, b - p, c - p
    s1 = (torch.cross(d, A, dim=-1) * B).sum(-1)
    s2 = (torch.cross(d, B, dim=-1) * C).sum(-1)
    s3 = (torch.cross(d, C, dim=-1) * A).sum(-1)
    return (((dp > 0) & (dq < 0)) | ((dp < 0) & (dq > 0))) & (((s1 > 0) & (s2 > 0) & (s3 > 0)) | ((s1 < 0) & (s2 < 0) & (s3 < 0)))


def pairs_intersect(tri_m, tri_s):
    """[K,3,3] against [K,3,3] -> [K] bool, the six tests of the predicate (the box rule is the caller's)."""
    m, s = _orient_parts(tri_m), _orient_parts(tri_s)
    ns = torch.cross(s[1] - s[0], s[2] - s[0], dim=-1)
    nm = torch.cross(m[1] - m[0], m[2] - m[0], dim=-1)
    hit = torch.zeros(tri_m.shape[0], dtype=torch.bool, device=tri_m.device)
    for k in range(3):
        hit |= _pierces(m[k], m[(k + 1) % 3], s[0], s[1], s[2], ns)
        hit |= _pierces(s[k], s[(k + 1) % 3], m[0], m[1], m[2], nm)
    return hit


def _boxes(tri):
    """[B,F,3,3] -> low, high [B,F,3]; a void face gets the empty box."""
    normal = torch.cross(tri[:, :, 1] - tri[:, :, 0], tri[:, :, 2] - tri[:, :, 0], dim=-1)
    finite = (torch.isfinite(tri).all(-1).all(-1) & (normal != 0).any(-1))[..., None]
    inf = torch.full_like(tri[:, :, 0], float('inf'))
    return torch.where(finite, tri.amin(2), inf), torch.where(finite, tri.amax(2), -inf)


class TwoHandCollisionCount(torch.nn.Module):
    """The count in plain torch; see the module docstring.  `faces_main` [Fm,3], `faces_sub` [Fs,3]: integer tables (None: the
    1538 faces of `assets.hand_faces('right')` for the main hand, as `FusedTwoHandSDFLoss`; `faces_sub=None`: the main table)."""

    def __init__(self, faces_main=None, faces_sub=None):
        super().__init__()
        fm = _faces(assets.hand_faces('right') if faces_main is None else faces_main)
        self.register_buffer('faces_main', fm)
        self.register_buffer('faces_sub', fm.clone() if faces_sub is None else _faces(faces_sub))
        self._checked = set()                                  # (Vm, Vs) the tables were range-checked against

    def _check(self, verts_main, verts_sub):
        for name, v in (('verts_main', verts_main), ('verts_sub', verts_sub)):
            if not torch.is_tensor(v) or v.dim() != 3 or v.shape[2] != 3 or v.shape[1] < 1:
                raise ValueError('%s must be a tensor [B,V,3]; got %s' % (name, tuple(getattr(v, 'shape', ()))))
        if (verts_main.shape[0] != verts_sub.shape[0] or verts_main.shape[0] < 1 or verts_sub.dtype != verts_main.dtype
                or not verts_main.is_floating_point() or verts_sub.device != verts_main.device):
            raise ValueError('the vertices must be floating point, of one dtype and device, with one B >= 1')
        Vm, Vs = verts_main.shape[1], verts_sub.shape[1]
        if (Vm, Vs) not in self._checked:                      # once per (tables, V), on the host
            for name, f, V in (('faces_main', self.faces_main, Vm), ('faces_sub', self.faces_sub, Vs)):
                low, top = int(f.min()), int(f.max())
                if low < 0 or top >= V:
                    raise ValueError('%s names vertex %d of %d' % (name, low if low < 0 else top, V))
            self._checked.add((Vm, Vs))
        return verts_main.shape[0], Vm, Vs, self.faces_main.shape[0], self.faces_sub.shape[0]

    def forward(self, verts_main, verts_sub):
        B, _, _, Fm, Fs = self._check(verts_main, verts_sub)
        dev = verts_main.device
        with torch.no_grad():
            tm, ts = verts_main[:, self.faces_main], verts_sub[:, self.faces_sub]           # [B,F,3,3]
            (mlo, mhi), (slo, shi) = _boxes(tm), _boxes(ts)
            pairs_main = torch.zeros(B * Fm, dtype=torch.int64, device=dev)
            pairs_sub = torch.zeros(B * Fs, dtype=torch.int64, device=dev)
            step = max(1, MIRROR_PAIRS // (B * Fs))
            for i0 in range(0, Fm, step):
                i1 = min(i0 + step, Fm)
                near = ((mlo[:, i0:i1, None] <= shi[:, None]) & (slo[:, None] <= mhi[:, i0:i1, None])).all(-1)     # [B,c,Fs]
                b, i, j = near.nonzero(as_tuple=True)
                i = i + i0
                hit = pairs_intersect(tm[b, i], ts[b, j])
                pairs_main += torch.bincount((b * Fm + i)[hit], minlength=B * Fm)
                pairs_sub += torch.bincount((b * Fs + j)[hit], minlength=B * Fs)
            pairs_main, pairs_sub = pairs_main.view(B, Fm).to(torch.int32), pairs_sub.view(B, Fs).to(torch.int32)
        return {'pairs_main': pairs_main, 'pairs_sub': pairs_sub, 'count': pairs_main.sum(1, dtype=torch.int32)}


class FusedTwoHandCollisionCount(TwoHandCollisionCount):
    """`TwoHandCollisionCount` on csrc/rih_collision.hip: boxes, the cull of the sub faces against a tile of 256 main faces, the
    six tests and the three integer sums in ONE launch per call, however many frames; nothing comes back to the host, and a
    call can be captured in a `torch.cuda.graph`.  GPU fp32 only; no cap on the tables' sizes."""

    def __init__(self, faces_main=None, faces_sub=None):
        super().__init__(faces_main, faces_sub)
        self.register_buffer('_fm32', self.faces_main.to(torch.int32).contiguous(), persistent=False)
        self.register_buffer('_fs32', self.faces_sub.to(torch.int32).contiguous(), persistent=False)

    def forward(self, verts_main, verts_sub):
        B, Vm, Vs, Fm, Fs = self._check(verts_main, verts_sub)
        if verts_main.dtype != torch.float32:
            raise ValueError('the fused count is fp32 only; got %s' % verts_main.dtype)
        vm, vs = verts_main.detach().contiguous(), verts_sub.detach().contiguous()
        ops._chk(vm, vs)
        ops._chk(self._fm32, self._fs32, dtype=torch.int32)
        pairs_main = torch.empty((B, Fm), device=vm.device, dtype=torch.int32)
        summed = torch.zeros(B * Fs + B, device=vm.device, dtype=torch.int32)      # the kernel ADDS into pairs_sub and count
        pairs_sub, count = summed[:B * Fs].view(B, Fs), summed[B * Fs:]
        check(ops._L().rih_collision_count(vm.data_ptr(), vs.data_ptr(), self._fm32.data_ptr(), self._fs32.data_ptr(),
                                           pairs_main.data_ptr(), pairs_sub.data_ptr(), count.data_ptr(), B, Vm, Vs, Fm, Fs,
                                           ops._stream()), 'rih_collision_count')
        return {'pairs_main': pairs_main, 'pairs_sub': pairs_sub, 'count': count}


def filter_sequence(optimizer, counter, right_quat, right_loc, left_quat, left_loc, hand_shape, max_pairs, batch_size):
    """The gate over a sequence of N frames: both hands' meshes by `pose_driver.scene_meshes` in batches of `batch_size` (the
    last one shorter), counted by `counter` (either class above, on the optimiser's device).  The pose arguments are what
    `optimize_sequence` takes and returns (right_quat = out['right']['rot'], right_loc = out['right']['loc'], ...).
    -> {'count' [N] int32, 'valid' [N] bool = count <= max_pairs} as CPU tensors.  `max_pairs` is required: it bounds intersecting
    triangle pairs, not FCL's contact points, so the reference's 75 and 100 are no defaults for it."""
    dtype = optimizer.dtype
    rq, lq = _sequence(right_quat, (16, 4), dtype, 'right_quat'), _sequence(left_quat, (16, 4), dtype, 'left_quat')
    rl, ll = _sequence(right_loc, (3,), dtype, 'right_loc'), _sequence(left_loc, (3,), dtype, 'left_loc')
    shape = _sequence(hand_shape, (20,), dtype, 'hand_shape')
    N, batch_size = rq.shape[0], int(batch_size)
    if N < 1 or any(x.shape[0] != N for x in (lq, rl, ll, shape)):
        raise ValueError('the five sequences must have one length N >= 1; got %s' % [x.shape[0] for x in (rq, rl, lq, ll, shape)])
    if batch_size < 1:
        raise ValueError('batch_size must be at least 1; got %r' % (batch_size,))
    if isinstance(max_pairs, bool) or int(max_pairs) != max_pairs or max_pairs < 0:
        raise ValueError('max_pairs must be a whole number >= 0; got %r' % (max_pairs,))
    counts = []
    for start in range(0, N, batch_size):
        cut = slice(start, min(start + batch_size, N))
        vm, vs = scene_meshes(optimizer, rq[cut], rl[cut], lq[cut], ll[cut], shape[cut])
        counts.append(counter(vm, vs)['count'])
    count = torch.cat(counts).cpu()
    return {'count': count, 'valid': count <= int(max_pairs)}
