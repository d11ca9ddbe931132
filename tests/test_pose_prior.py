"""Hand-prior and contact terms of the pose optimiser (renderih_amd.pose_prior; reference hocontact/postprocess/geo_loss.py and
scripts/HandPoseConverter.py) on the CPU: the torch mirrors against values and gradients of the reference's own program
(tests/golden/pose_prior.npz, written by tests/golden/make_pose_prior_golden.py), the real kernels (csrc/rih_pose_prior.hip)
through the host-compiled library against the golden and against the mirror evaluated in fp64, bit-identical repeats, the
isolated vertex, the empty mask, the argument checks.  tests/test_gpu_pose_prior.py shares the helpers.

Tolerances (from the issue and from measurements of the REFERENCE computation, not of the code under test):
  mirror vs golden    max |err| <= 1e-6 max |want| per array (both are fp32 torch on the CPU; found: at most 2.2e-7).
  gradients           the project's operator bar |err| <= 1e-4 |want| + 1e-5 max |want| (renderih_amd.testing.assert_close).
  scalar terms, loss  relative error <= TERM_RTOL = 4 x the largest relative deviation of the fp32 torch MIRROR from the fp64
                      mirror over `deviation_cases()` (the golden total and every seeded case the fused tests use), taken on
                      the CPU and on the GPU; the factor 4 covers another summation order over at most 2315 edges.
                      Measured: 5.15e-7 on the CPU and 5.15e-7 on an MI355X (both at B = 1, D = 1 on the 5-vertex mesh; the
                      778-vertex cases stay below 2.2e-7) -> TERM_RTOL = 2.06e-6.  The fused kernels were then found at most
                      5.15e-7 from the fp64 mirror and 1.9e-7 from the golden (profiles/pose_prior/).
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

from renderih_amd import testing  # noqa: E402

GOLDEN = os.path.join(HERE, 'golden', 'pose_prior.npz')
SIDES = ('right', 'left')
INPUTS = ('q_r', 'q_l', 'verts_r', 'verts_l', 'anchors_r', 'anchors_l')
TERMS = ('quat_norm_r', 'quat_norm_l', 'edge_r', 'edge_l', 'contact', 'ergo_r', 'ergo_l')
UPSTREAM = 1.5                            # the scalar the loss is multiplied by before the backward
# largest relative deviation of a term (or the loss) of the fp32 torch mirror from the fp64 mirror over deviation_cases()
MEASURED_CPU = 5.15e-7
MEASURED_GPU = 5.15e-7
TERM_RTOL = 4 * max(MEASURED_CPU, MEASURED_GPU)
SMALL_FACES = np.array([[0, 1, 2], [1, 2, 3]])                  # 5 vertices, vertex 4 in no face
# (B, D, mesh): B = 1 the optimiser's smallest batch, 3 odd, 32 its largest; D = 1 and 4; both meshes
CASES = [(1, 4, 'mano'), (3, 1, 'mano'), (32, 4, 'mano'), (3, 4, 'small'), (1, 1, 'small')]


def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def mano_dict(side):
    from renderih_amd import assets
    return assets.synthetic_mano_dict(side, seed=0)


def close_to_golden(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    assert err <= 1e-6 * np.abs(want).max(), '%s: max err %g of max %g' % (what, err, np.abs(want).max())


def small_rest():
    """Rest positions of the 5-vertex mesh, right and left."""
    rs = np.random.RandomState(5)
    return rs.randn(5, 3).astype(np.float32), rs.randn(5, 3).astype(np.float32)


_MODULES = {}


def module(cls, mesh='mano'):
    """One instance per class and mesh on the CPU (constructing runs the MANO mirror four times); tests move COPIES."""
    key = (cls.__name__, mesh)
    if key not in _MODULES:
        mod = cls(mano_dict('right'), mano_dict('left'))
        if mesh == 'small':
            mod.set_mesh(SMALL_FACES, *small_rest())
        _MODULES[key] = mod
    import copy
    return copy.deepcopy(_MODULES[key])


def seeded_case(B, D, mesh, seed=0):
    """Inputs in the golden's ranges: rotations by up to ~80 degrees with |q| in [0.7, 1.4], vertices near the rest meshes
    (noise of about a third of an edge), anchors 0.02 across, random contact tables with padded entries."""
    rs = np.random.RandomState(9000 + 131 * B + 7 * D + seed + (1000 if mesh == 'small' else 0))
    axis = rs.randn(2, B, 16, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * rs.uniform(0.0, 1.4, size=(2, B, 16, 1))
    q = np.concatenate([np.cos(half), np.sin(half) * axis], -1) * rs.uniform(0.7, 1.4, size=(2, B, 16, 1))
    mod = module(_mirror_cls(), mesh)
    edges, static = mod.edges.numpy(), mod.static_len.numpy()
    V = 5 if mesh == 'small' else 778
    A = 3 if mesh == 'small' else 32
    if mesh == 'small':
        rest, noise = np.stack(small_rest()), 0.2
    else:
        rest = np.stack([_rest_mesh(s) for s in SIDES])
        noise = 3e-4
    verts = rest[:, None] + noise * rs.randn(2, B, V, 3)
    assert edges.max() < V and static.shape == (2, edges.shape[0])
    mask = (rs.rand(B, A, D) < 0.6).astype(np.int64)
    mask[0, 0, 0] = 1
    case = {'q_r': q[0], 'q_l': q[1], 'verts_r': verts[0], 'verts_l': verts[1],
            'anchors_r': 0.02 * rs.randn(B, A, 3), 'anchors_l': 0.02 * rs.randn(B, A, 3)}
    case = {k: v.astype(np.float32) for k, v in case.items()}
    case.update(anchor_id=rs.randint(0, A, size=(B, A, D)), mask=mask, elastic=rs.rand(B, A, D).astype(np.float32), mesh=mesh)
    return case


def _mirror_cls():
    from renderih_amd.pose_prior import TwoHandPriorLoss
    return TwoHandPriorLoss


_REST = {}


def _rest_mesh(side):
    if side not in _REST:
        from renderih_amd.quat_mano import QuatManoLayer
        q = torch.zeros(1, 16, 4)
        q[..., 0] = 1.0
        with torch.no_grad():
            _REST[side] = QuatManoLayer(mano_dict(side), side=side, center_idx=0)(q, torch.zeros(1, 10))[0][0].numpy()
    return _REST[side]


def golden_total_case():
    z = golden()
    case = {'q_r': z['right/q'][:2], 'q_l': z['left/q'][:2], 'verts_r': z['right/verts'], 'verts_l': z['left/verts'],
            'anchors_r': z['contact/anchors_main'], 'anchors_l': z['contact/anchors_sub']}
    case.update(anchor_id=z['contact/anchor_id'], mask=z['contact/mask'], elastic=z['contact/elastic'], mesh='mano')
    return case


def evaluate(mod, case, device, dtype=torch.float32):
    """-> dict of numpy arrays: loss, terms, grad_<input> of UPSTREAM * loss."""
    mod = (mod.to(device) if dtype == torch.float32 else mod.to(device=device, dtype=dtype))
    mod.set_contacts(case['anchor_id'], case['mask'], case['elastic'])
    ins = [torch.as_tensor(case[k]).to(device=device, dtype=dtype).requires_grad_(True) for k in INPUTS]
    loss, terms = mod(*ins)
    assert loss.shape == () and terms.shape == (7,)
    grads = torch.autograd.grad(loss * UPSTREAM, ins)
    out = {'loss': loss.detach().cpu().numpy(), 'terms': terms.detach().cpu().numpy()}
    out.update({'grad_' + k: g.detach().cpu().numpy() for k, g in zip(INPUTS, grads)})
    return out


def relative_deviation(got, want):
    """Largest relative deviation over the seven terms and the loss."""
    g = np.concatenate([np.asarray(got['terms'], np.float64), [float(got['loss'])]])
    w = np.concatenate([np.asarray(want['terms'], np.float64), [float(want['loss'])]])
    return float((np.abs(g - w) / np.abs(w)).max())


def compare(got, want, what):
    dev = relative_deviation(got, want)
    print('%s: scalar relative deviation %.3g (bar %.3g)' % (what, dev, TERM_RTOL))
    for k in INPUTS:
        testing.assert_close(torch.as_tensor(got['grad_' + k]), torch.as_tensor(want['grad_' + k]), 1e-4, 1e-5,
                             '%s grad %s' % (what, k))
    assert dev <= TERM_RTOL, '%s: terms %s want %s' % (what, got['terms'], want['terms'])
    lam = 10.0
    t = np.asarray(got['terms'], np.float64)
    assert abs(t.sum() + (lam - 1) * t[4] - float(got['loss'])) <= 4 * np.finfo(np.float32).eps * 8 * np.abs(t).sum() * lam


def deviation_cases():
    return [('golden', golden_total_case())] + [('B%d D%d %s' % c, seeded_case(*c)) for c in CASES]


def mirror_fp32_deviation(device):
    """What TERM_RTOL is built from: fp32 mirror against fp64 mirror (the latter on the CPU) over every case."""
    worst = 0.0
    for name, case in deviation_cases():
        want = evaluate(module(_mirror_cls(), case['mesh']), case, 'cpu', torch.float64)
        got = evaluate(module(_mirror_cls(), case['mesh']), case, device)
        dev = relative_deviation(got, want)
        print('fp32 mirror vs fp64 mirror on %s, %s: %.3g' % (device, name, dev))
        worst = max(worst, dev)
    return worst


def fused_vs_fp64_mirror(case, device, what):
    from renderih_amd.pose_prior import FusedTwoHandPriorLoss
    want = evaluate(module(_mirror_cls(), case['mesh']), case, 'cpu', torch.float64)
    fused = module(FusedTwoHandPriorLoss, case['mesh'])
    got = evaluate(fused, case, device)
    compare(got, want, what)
    again = evaluate(fused, case, device)
    for k in got:
        assert np.array_equal(got[k], again[k]), k                      # fixed summation order, no atomics
    return got


# ------------------------------------------------------------------------------------------------ mirrors against the golden
@pytest.mark.parametrize('side', SIDES)
def test_axis_tables_and_matrices_match_reference_golden(side):
    from renderih_amd import pose_prior as pp
    from renderih_amd.quat_mano import normalize_quaternion
    z = golden()
    tables = pp.axis_tables(side, mano_dict(side))
    assert tables[0].shape == (16, 3, 3) and tables[0].dtype == torch.float32
    close_to_golden(tables[0], z[side + '/inv_m_u_0'], 'invM_U_n_0')
    close_to_golden(tables[1], z[side + '/inv_u_m_1'], 'invU_M_n_1')
    q = torch.from_numpy(z[side + '/q'])
    keep = q.clone()
    close_to_golden(pp.mano_quat_2_mat(normalize_quaternion(q), tables, side), z[side + '/mat'], 'mano_quat_2_mat')
    assert torch.equal(q, keep)                                         # the left hand's signs go onto a copy
    with pytest.raises(ValueError):
        pp.axis_tables('both', mano_dict(side))
    with pytest.raises(ValueError):
        pp.mano_quat_2_mat(q[:, 1:], tables, side)


@pytest.mark.parametrize('side', SIDES)
def test_mirror_terms_match_reference_golden(side):
    from renderih_amd import pose_prior as pp
    from renderih_amd.quat_mano import normalize_quaternion
    z = golden()
    mod = module(pp.TwoHandPriorLoss)
    q = torch.from_numpy(z[side + '/q']).requires_grad_(True)
    tables = (getattr(mod, 'inv_m_u_0_' + side), getattr(mod, 'inv_u_m_1_' + side))
    ja = pp.mano_quat_2_mat(normalize_quaternion(q), tables, side)[:, 1:]
    ergo = pp.ergonomics_loss(ja, getattr(mod, 'zero_ja_' + side), side[0])
    close_to_golden(ergo.detach(), z[side + '/ergo'], 'ergonomics')
    close_to_golden(torch.autograd.grad(ergo, q)[0], z[side + '/grad_ergo'], 'ergonomics gradient')
    qn = pp.quat_norm_loss(q)
    close_to_golden(qn.detach(), z[side + '/quat_norm'], 'quaternion norm')
    close_to_golden(torch.autograd.grad(qn, q)[0], z[side + '/grad_quat_norm'], 'quaternion norm gradient')
    i = SIDES.index(side)
    assert np.array_equal(mod.edges.numpy(), np.sort(z[side + '/edges'], axis=1))          # same rows in the same order
    assert np.array_equal(z['left/edges'], z['right/edges'])                                # both from the right hand's faces
    close_to_golden(mod.static_len[i], z[side + '/static_len'], 'static lengths')
    v = torch.from_numpy(z[side + '/verts']).requires_grad_(True)
    edge = pp.edge_len_loss(v, mod.edges, mod.static_len[i])
    close_to_golden(edge.detach(), z[side + '/edge'], 'edge')
    close_to_golden(torch.autograd.grad(edge, v)[0], z[side + '/grad_edge'], 'edge gradient')


@pytest.mark.parametrize('name', ['contact', 'contact_d1'])
def test_contact_mirror_matches_reference_golden(name):
    from renderih_amd.pose_prior import batch_contact_loss
    z = golden()
    mask, elastic = z[name + '/mask'], z[name + '/elastic']
    assert ((mask == 0) & (elastic != 0)).sum() == 1 and ((mask == 1) & (elastic == 0)).any()      # the quirk is in the data
    a = torch.from_numpy(z[name + '/anchors_main']).requires_grad_(True)
    s = torch.from_numpy(z[name + '/anchors_sub']).requires_grad_(True)
    loss = batch_contact_loss(a, s, torch.from_numpy(z[name + '/anchor_id']), torch.from_numpy(mask), torch.from_numpy(elastic))
    g = torch.autograd.grad(loss, (a, s))
    close_to_golden(loss.detach(), z[name + '/loss'], 'contact')
    close_to_golden(g[0], z[name + '/grad_main'], 'contact gradient, main hand')
    close_to_golden(g[1], z[name + '/grad_sub'], 'contact gradient, sub hand')
    masked = batch_contact_loss(a, s, torch.from_numpy(z[name + '/anchor_id']), torch.from_numpy(mask),
                                torch.from_numpy(elastic * mask))
    assert float(masked.detach()) < float(loss.detach())                                 # masking the product would change the value


def test_mirror_total_matches_reference_golden():
    z = golden()
    got = evaluate(module(_mirror_cls()), golden_total_case(), 'cpu')
    close_to_golden(got['loss'], z['total/loss'], 'total')
    close_to_golden(got['terms'], z['total/terms'], 'terms')
    for k in INPUTS:
        close_to_golden(got['grad_' + k] / UPSTREAM, z['total/grad_' + k], 'total gradient ' + k)


# ------------------------------------------------------------------------------------------------ the kernels on the host shim
def test_fused_kernels_match_reference_golden_on_cpu():
    from host_kernels import host_kernels_abi
    z = golden()
    case = golden_total_case()
    with host_kernels_abi():
        got = fused_vs_fp64_mirror(case, 'cpu', 'fused vs fp64 mirror, golden case')
    want = {'loss': z['total/loss'], 'terms': z['total/terms']}
    want.update({'grad_' + k: z['total/grad_' + k] * np.float32(UPSTREAM) for k in INPUTS})
    compare(got, want, 'fused vs golden')


@pytest.mark.parametrize('B,D,mesh', [c for c in CASES if c[0] < 32])
def test_fused_kernels_match_fp64_mirror_on_cpu(B, D, mesh):
    from host_kernels import host_kernels_abi
    with host_kernels_abi():
        fused_vs_fp64_mirror(seeded_case(B, D, mesh), 'cpu', 'fused vs fp64 mirror B=%d D=%d %s' % (B, D, mesh))


def test_isolated_vertex_gets_exact_zero_and_csr_checks_the_range():
    from host_kernels import host_kernels_abi
    from renderih_amd.pose_prior import FusedTwoHandPriorLoss, edge_csr, edge_index
    edges = edge_index(SMALL_FACES)
    assert edges.tolist() == [[0, 1], [1, 2], [0, 2], [2, 3], [1, 3]]                       # first-seen order
    vptr, vlist = edge_csr(edges, 5)
    assert vptr.tolist() == [0, 2, 5, 8, 10, 10] and sorted(vlist.tolist()) == list(range(10))
    flat = edges.reshape(-1)
    for v in range(5):
        seg = vlist[vptr[v]:vptr[v + 1]].tolist()
        assert seg == sorted(seg) and all(int(flat[e]) == v for e in seg)
    with pytest.raises(ValueError):
        edge_csr(edges, 3)
    with pytest.raises(ValueError):
        edge_csr(torch.tensor([[0, -1]]), 5)
    with pytest.raises(ValueError):
        module(FusedTwoHandPriorLoss).set_mesh(np.array([[0, 1, 5]]), np.zeros((5, 3)), np.zeros((5, 3)))
    case = seeded_case(3, 4, 'small')
    with host_kernels_abi():
        got = evaluate(module(FusedTwoHandPriorLoss, 'small'), case, 'cpu')
    for k in ('grad_verts_r', 'grad_verts_l'):
        assert not got[k][:, 4].any() and np.abs(got[k][:, :4]).min() > 0


def test_empty_mask_gives_zero_loss_and_zero_gradients():
    from host_kernels import host_kernels_abi
    from renderih_amd.pose_prior import FusedTwoHandPriorLoss
    case = seeded_case(3, 4, 'mano')
    case['mask'] = np.zeros_like(case['mask'])
    mirror = evaluate(module(_mirror_cls()), case, 'cpu')
    with host_kernels_abi():
        fused = evaluate(module(FusedTwoHandPriorLoss), case, 'cpu')
    for got in (mirror, fused):
        assert got['terms'][4] == 0.0 and not got['grad_anchors_r'].any() and not got['grad_anchors_l'].any()
        assert got['terms'][0] > 0 and np.abs(got['grad_q_r']).max() > 0


def test_refused_arguments_raise():
    from host_kernels import host_kernels_abi, load
    from renderih_amd.pose_prior import FusedTwoHandPriorLoss, contact_csr
    case = seeded_case(2, 4, 'mano')
    ins = [torch.from_numpy(case[k]) for k in INPUTS]
    for cls in (_mirror_cls(), FusedTwoHandPriorLoss):
        mod = module(cls)
        with pytest.raises(RuntimeError):
            mod(*ins)                                                   # no contacts set
        for bad in (32, -1):
            ids = case['anchor_id'].copy()
            ids[1, 3, 2] = bad
            with pytest.raises(ValueError):
                mod.set_contacts(ids, case['mask'], case['elastic'])
        with pytest.raises(ValueError):
            mod.set_contacts(case['anchor_id'].astype(np.float32), case['mask'], case['elastic'])
        with pytest.raises(ValueError):
            mod.set_contacts(case['anchor_id'], case['mask'][:, :, :2], case['elastic'])
        mod.set_contacts(case['anchor_id'], case['mask'], case['elastic'])
        with pytest.raises(ValueError):
            mod(ins[0][:1], *ins[1:])
        with pytest.raises(ValueError):
            mod(ins[0], ins[1], ins[2][:, :700], *ins[3:])
        with pytest.raises(ValueError):
            mod(*ins[:5], ins[5][:, :5])
    with pytest.raises(RuntimeError):                                   # GPU fp32 only: no CPU fallback
        mod(*ins)
    with host_kernels_abi():
        strided = [t.transpose(0, 1).contiguous().transpose(0, 1) for t in ins]
        assert not any(t.is_contiguous() for t in strided)
        loss, terms = mod(*strided)                                     # non-contiguous inputs are taken
        want, _ = mod(*ins)
        assert torch.equal(loss, want) and not terms.requires_grad
    with pytest.raises(ValueError):
        contact_csr(np.full((1, 2, 2), 2))
    cptr, clist = contact_csr(case['anchor_id'])
    flat = case['anchor_id'].reshape(2, -1)
    for b in range(2):
        assert sorted(clist[b].tolist()) == list(range(flat.shape[1]))
        for a in range(32):
            assert all(flat[b, e] == a for e in clist[b, cptr[b, a]:cptr[b, a + 1]].tolist())
    lib = load()
    buf = np.zeros(1 << 16, np.float32)
    p = buf.ctypes.data
    einval = lib.rih_anchor_fwd(None, p, p, p, 1, 4, 1, None)
    ok = [p] * 15 + [1.0, 10.0, p, p, 1, 4, 1, 1, 1, None]
    for i in list(range(15)) + [17, 18]:
        assert lib.rih_pose_prior_fwd(*(ok[:i] + [None] + ok[i + 1:])) == einval, i
    for i, bad in ((19, 0), (19, 65536), (20, 0), (21, 0), (22, 0), (23, 0), (15, -1.0), (15, float('nan'))):
        assert lib.rih_pose_prior_fwd(*(ok[:i] + [bad] + ok[i + 1:])) == einval, i
    assert lib.rih_pose_prior_reduce(None, 10.0, p, p, 1, None) == einval
    assert lib.rih_pose_prior_reduce(p, 10.0, None, p, 1, None) == einval
    assert lib.rih_pose_prior_reduce(p, 10.0, p, None, 1, None) == einval
    assert lib.rih_pose_prior_reduce(p, 10.0, p, p, 0, None) == einval
    assert lib.rih_pose_prior_bwd(None, p, p, 4, None) == einval
    assert lib.rih_pose_prior_bwd(p, None, p, 4, None) == einval
    assert lib.rih_pose_prior_bwd(p, p, None, 4, None) == einval
    assert lib.rih_pose_prior_bwd(p, p, p, 0, None) == einval
