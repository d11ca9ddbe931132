"""Shared by tests/test_joint_fit.py (CPU: the mirrors, and the kernels compiled for the host) and tests/test_gpu_joint_fit.py: the
cases of the joints -> MANO fit (renderih_amd.joint_fit, csrc/rih_joint_fit.hip), an fp64 numpy oracle of the inverse kinematics
written independently of the torch mirror, and the checks.  Every check takes the device the fused code runs on.

Golden: tests/golden/joint_fit.npz, written by tests/golden/make_joint_fit_golden.py from the reference's own adaptive_IK, mat2aa
and fitting loop on six synthetic hands (both sides, seeds 1-3; joints in centimetres).

Bars (none taken from the code under test):
  IK            RTOL, ATOL = 1e-4, 1e-5 (the project's bar for fp32 kernels against a reference) against the golden and the oracle.
  mat2aa, loss, one iteration, prefix
                testing.assert_fp32_equivalent, k = 4 with the project's floor 2e-5: the fused result is at most 4 x as far
                from the fp64 mirror as the fp32 mirror is, relative to the largest value of the tensor.
  schedule      the rate after every step EQUALS Python's double expression.
  whole fit     each hand's final loss <= max(fp32 mirror's, fp64 mirror's) x R, R >= 1 the worst ratio between the two mirrors'
                final losses over these hands: the loop's own chaos (Adam divides by sqrt(v), the L1 gradient is a sign).
Figures go to the log given by RIH_JOINT_FIT_LOG (profiles/joint_fit/deviation_{cpu,gpu}.log were written that way)."""
import math
import os

import numpy as np
import torch

from renderih_amd import _lib, assets, ops, testing
from renderih_amd import joint_fit as JF
from renderih_amd.manolayer import ManoLayer

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'joint_fit.npz')
RTOL, ATOL = 1e-4, 1e-5
PREFIX = 8
SIDES = ('right', 'left')
PARENT = [0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19]
CHAIN = [2, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16, 18, 19, 20]
SLOT = {2: 13, 3: 14, 4: 15, 6: 1, 7: 2, 8: 3, 10: 4, 11: 5, 12: 6, 14: 10, 15: 11, 16: 12, 18: 7, 19: 8, 20: 9}


def log(msg):
    path = os.environ.get('RIH_JOINT_FIT_LOG')
    if path:
        with open(path, 'a') as fh:
            fh.write(msg + '\n')
    print(msg)


def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def close(got, want, what):
    torch.testing.assert_close(torch.as_tensor(np.asarray(got), dtype=torch.float64), torch.as_tensor(np.asarray(want), dtype=torch.float64),
                               rtol=RTOL, atol=ATOL, msg=lambda m: '%s: %s' % (what, m))


def layer(side, device):
    L = ManoLayer(assets.synthetic_mano_dict(side, seed=0), center_idx=9, use_pca=True)
    if side == 'left':
        L.shapedirs[:, 0, :] *= -1
    return L.to(device)


def hands(side, B, G=None):
    """B hands of one side: the golden's three, then noisy copies of them (seeded)."""
    G = G or golden()
    own = G['joints'][G['side'] == SIDES.index(side)]
    rs = np.random.RandomState(31 + B)
    out = [own[i % 3] + (0 if i < 3 else rs.randn(21, 3) * 1.5) for i in range(B)]
    return np.stack(out).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the IK oracle
def _norm(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def ik_oracle(T, P, normalize, report=None):
    """adaptive_IK for one hand in numpy / Python doubles with the documented deviations; `report` (a dict) receives the
    unclamped cosine of every bone."""
    T, P = np.asarray(T, np.float64), np.asarray(P, np.float64)
    if normalize:
        P = P * (np.linalg.norm(T[9] - T[0]) / np.linalg.norm(P[9] - P[0]))
        P = P - P[0] + T[0]
    kn = [1, 5, 9, 13, 17]
    H = (T[kn] - T[0]).T @ (P[kn] - P[0])
    U, S, Vt = np.linalg.svd(H)
    V = Vt.T
    R0 = V @ np.diag([1.0, 1.0, np.sign(np.linalg.det(V @ U.T))]) @ U.T
    if np.array_equal(T[kn] - T[0], P[kn] - P[0]):            # the maximiser is the identity; the SVD returns it to 1e-16
        R0 = np.eye(3)
    R, q, out = {0: R0}, {0: T[0]}, np.zeros((16, 3, 3))
    out[0] = R0
    for k in kn:
        R[k] = R0
    for k in CHAIN:
        pa = PARENT[k]
        q[pa] = R[pa] @ (T[pa] - T[PARENT[pa]]) + q[PARENT[pa]]
        w = P[k] - q[pa]
        dp = [R[pa][0][a] * w[0] + R[pa][1][a] * w[1] + R[pa][2][a] * w[2] for a in range(3)]
        dt = [float(x) for x in T[k] - T[pa]]
        ax = [dt[1] * dp[2] - dt[2] * dp[1], dt[2] * dp[0] - dt[0] * dp[2], dt[0] * dp[1] - dt[1] * dp[0]]
        D = np.eye(3)
        if any(a != 0.0 for a in ax):
            n1 = _norm(ax) + 1e-8
            ax = [a / n1 for a in ax]
            n2 = _norm(ax)
            x, y, z = (a / n2 for a in ax)
            cos = (dt[0] * dp[0] + dt[1] * dp[1] + dt[2] * dp[2]) / ((_norm(dt) + 1e-8) * (_norm(dp) + 1e-8))
            if report is not None:
                report[k] = cos
            al = math.acos(min(1.0, max(-1.0, cos)))
            c, s = math.cos(al), math.sin(al)
            C = 1.0 - c
            D = np.array([[x * x * C + c, x * y * C - z * s, z * x * C + y * s],
                          [x * y * C + z * s, y * y * C + c, y * z * C - x * s],
                          [z * x * C - y * s, y * z * C + x * s, z * z * C + c]])
        out[SLOT[k]] = D
        R[k] = R[pa] @ D
    return out


def _ik_all(template, joints, normalize, device):
    """-> fused, fp64 mirror, fp32 mirror, oracle as float64 numpy [B,16,3,3]."""
    T = torch.as_tensor(template, dtype=torch.float32)
    J = torch.as_tensor(joints, dtype=torch.float32)
    fused = JF.fused_adaptive_ik(T.to(device).contiguous(), J.to(device).contiguous(), normalize)
    m64 = JF.adaptive_ik(T, J, normalize, torch.float64)
    m32 = JF.adaptive_ik(T, J, normalize, torch.float32)
    orc = np.stack([ik_oracle(T.numpy(), j, normalize) for j in J.numpy()])
    return fused, m64.numpy(), m32.double().numpy(), orc


def check_ik_parity(device, side, B, normalize):
    G = golden()
    idx = np.nonzero(G['side'] == SIDES.index(side))[0]
    T = G['template/' + side]
    if normalize:
        J, gold = hands(side, B, G), G['aik'][idx]
    else:
        pre = G['pre'][idx]
        rs = np.random.RandomState(77 + B)
        J = np.stack([pre[i % 3] + (0 if i < 3 else rs.randn(21, 3) * 0.004) for i in range(B)]).astype(np.float32)
        gold = G['aik_pre'][idx]
    fused, m64, m32, orc = _ik_all(T, J, normalize, device)
    n = min(B, 3)
    for name, got in (('rih_aik', fused.double().cpu().numpy()), ('fp64 mirror', m64), ('fp32 mirror', m32)):
        close(got[:n], gold[:n], '%s vs the reference, %s B=%d normalize=%s' % (name, side, B, normalize))
        close(got, orc, '%s vs the oracle, %s B=%d normalize=%s' % (name, side, B, normalize))
    close(orc[:n], gold[:n], 'oracle vs the reference')
    Jd = torch.as_tensor(J).to(device)
    Td = torch.as_tensor(T).to(device)
    for b in range(B):
        alone = JF.fused_adaptive_ik(Td, Jd[b:b + 1].contiguous(), normalize)
        assert torch.equal(alone[0], fused[b]), 'hand %d of %d differs from the same hand alone' % (b, B)
    assert torch.equal(JF.fused_adaptive_ik(Td, Jd.contiguous(), normalize), fused), 'two runs differ'


def planar_case():
    """A flat template of huge bones in the z = 0 plane (every coordinate an fp32 value) and a target equal to it but for a unit
    z offset of the five finger tips: the root solve is exactly the identity, twelve bones lie exactly along their template
    bones, and the tips' cosines differ from 1 by 1e-19 -- the first seed for which one of them ROUNDS ABOVE 1 is used."""
    for seed in range(64):
        rs = np.random.RandomState(seed)
        T = np.zeros((21, 3), np.float32)
        for f in range(5):
            d = np.array([math.cos(0.4 * f - 0.8), math.sin(0.4 * f - 0.8)])
            for s in range(4):
                T[1 + 4 * f + s, :2] = (T[PARENT[1 + 4 * f + s], :2] + d * rs.uniform(2e8, 9e8) + rs.randn(2) * 1e8).astype(np.float32)
        P = T.copy()
        P[[4, 8, 12, 16, 20], 2] = 1.0
        rep = {}
        ik_oracle(T, P, False, rep)
        if any(c > 1.0 for c in rep.values()):
            return T, P, rep
    raise AssertionError('no seed gives a cosine above 1')


def check_ik_rules(device):
    G = golden()
    T = G['template/right']
    eye = np.broadcast_to(np.eye(3), (16, 3, 3))
    # a mirrored target (a left hand on the right template): the unconstrained optimum V U^T is a reflection
    J = hands('right', 2, G) * np.float32([-1, 1, 1])
    fused, m64, m32, orc = _ik_all(T, J, True, device)
    for name, got in (('rih_aik', fused.double().cpu().numpy()), ('fp64 mirror', m64)):
        assert np.isfinite(got).all(), name
        close(got, orc, '%s on a mirrored target' % name)
        np.testing.assert_allclose(np.linalg.det(got[:, 0]), 1.0, atol=1e-5)
        np.testing.assert_allclose(got[:, 0] @ got[:, 0].transpose(0, 2, 1), np.broadcast_to(np.eye(3), (2, 3, 3)), atol=1e-5)
    U, S, Vt = np.linalg.svd(np.einsum('ka,bkc->bac', T[[1, 5, 9, 13, 17]].astype(np.float64) - T[0],
                                       np.stack([ik_oracle_pre(T, j) for j in J])))
    assert (np.linalg.det(np.swapaxes(Vt, 1, 2) @ np.swapaxes(U, 1, 2)) < 0).all(), 'not the case this check is about'
    # every bone exactly along its template bone: the identity, bit for bit
    fused = JF.fused_adaptive_ik(torch.as_tensor(T).to(device), torch.as_tensor(T[None]).to(device).contiguous(), False)
    assert np.array_equal(fused.cpu().numpy()[0], eye.astype(np.float32)), 'identity swing'
    m = JF.adaptive_ik(torch.as_tensor(T), torch.as_tensor(T[None]), False).numpy()
    # the mirror's SVD returns the identity to 1e-16, so its cross products are not exactly zero and AIK.py's two 1e-8 terms
    # show: cos = 1 - 2e-8 / |bone|, a swing of sqrt(4e-8 / |bone|) about a noise axis, which the next two bones undo
    bones = np.linalg.norm(T[CHAIN].astype(np.float64) - T[[PARENT[k] for k in CHAIN]], axis=1)
    assert np.isfinite(m).all() and np.abs(m[0] - eye).max() < 3 * math.sqrt(4e-8 / bones.min())
    # a cosine that rounds above 1
    Tp, Pp, rep = planar_case()
    with np.errstate(invalid='ignore'):                                  # without the clamp: NaN
        assert any(math.isnan(np.arccos(np.float64(c))) for c in rep.values() if c > 1.0)
    fused = JF.fused_adaptive_ik(torch.as_tensor(Tp).to(device), torch.as_tensor(Pp[None]).to(device).contiguous(), False).cpu().numpy()[0]
    orc = ik_oracle(Tp, Pp, False)
    assert np.isfinite(fused).all()
    np.testing.assert_allclose(fused, orc, atol=1e-6)
    for k, c in rep.items():
        if c >= 1.0:
            assert np.array_equal(fused[SLOT[k]], np.eye(3, dtype=np.float32)), 'bone %d: cos %r' % (k, c)
    mirror = JF.adaptive_ik(torch.as_tensor(Tp), torch.as_tensor(Pp[None]), False).numpy()
    assert np.isfinite(mirror).all()


def ik_oracle_pre(T, P):
    """convert2mano.py:167-169 on one hand, relative to the wrist."""
    T, P = np.asarray(T, np.float64), np.asarray(P, np.float64)
    P = P * (np.linalg.norm(T[9] - T[0]) / np.linalg.norm(P[9] - P[0]))
    return (P - P[0])[[1, 5, 9, 13, 17]]


# ---------------------------------------------------------------------------------------------------- mat2aa
def mat2aa_matrices(N):
    """N matrices cycling through the golden's crafted ones (each mat2quat branch, cos < 0, non-rotations, IK results)."""
    R = golden()['m2a_R']
    return np.stack([R[(7 * i) % len(R)] for i in range(N)]) if N < len(R) else np.concatenate([R] * (N // len(R) + 1))[:N]


def check_mat2aa_golden():
    """The mirror against the reference's mat2aa and torch's autograd through it (fp64, away from the NaN rules)."""
    G = golden()
    R = torch.tensor(G['m2a_R'], requires_grad=True)
    aa = JF.mat2aa(R)
    grad, = torch.autograd.grad((aa * torch.tensor(G['m2a_w'])).sum(), R)
    close(aa.detach(), G['m2a_aa'], 'mirror mat2aa')
    close(grad, G['m2a_grad'], 'mirror mat2aa gradient')
    branches = JF._mat2aa_parts(R.detach())
    assert set(int(t) for t in branches[1]) == {0, 1, 2, 3} and (branches[4][:, 0] < 0).any()     # every branch, cos < 0 too


def _mat2aa_run(fn, R, w):
    R = R.clone().requires_grad_(True)
    aa = fn(R)
    grad, = torch.autograd.grad((aa * w).sum(), R)
    return aa.detach(), grad


def check_mat2aa_parity(device, N):
    R64 = torch.tensor(mat2aa_matrices(N))
    w64 = torch.tensor(np.random.RandomState(N).randn(N, 3))
    R32 = R64.float()
    want = _mat2aa_run(JF.mat2aa, R32.double(), w64)
    ref = _mat2aa_run(JF.mat2aa, R32, w64.float())
    got = _mat2aa_run(JF.FusedMat2AA.apply, R32.to(device).contiguous(), w64.float().to(device))
    for name, g, r, w in zip(('aa', 'gradient'), got, ref, want):
        e = testing.assert_fp32_equivalent(g, r, w, k=4.0, what='mat2aa %s N=%d' % (name, N))
        log('mat2aa %s N=%d on %s: fused vs fp64 %.3g, fp32 mirror vs fp64 %.3g' % (name, N, device, *e))


def check_mat2aa_rules(device):
    """Exact identity (sin^2 = 0: aa = 0, the gradient that of aa = 2 (x, y, z)) and a forward that is NaN (output 0, gradient
    0).  The term under the square root cannot be negative for a finite matrix -- each branch's mask bounds its own t below by
    1 - eps (branches 0 and 1: r22 < eps and the sign of r00 - r11; 2 and 3: r22 >= eps and the sign of r00 + r11) -- so the
    rule is reached through a NaN or an infinite entry only; far-from-rotation matrices of every branch stay finite."""
    eye = torch.eye(3)
    wild = torch.tensor([[[-1.5, 0.2, 0.1], [0.0, -1.2, 0.3], [0.1, 0.0, 0.4]],       # branch 2
                         [[-0.5, 0.2, 0.1], [0.0, -0.4, 0.3], [0.1, 0.0, -0.3]],      # branch 1
                         [[3.0, 0.2, 0.1], [0.0, 1.0, 0.3], [0.1, 0.0, -0.5]],        # branch 0
                         [[2.0, 0.2, 0.1], [0.0, 3.0, 0.3], [0.1, 0.0, 0.5]]])        # branch 3
    assert [int(x) for x in JF._mat2aa_parts(wild)[1]] == [3, 2, 1, 0] and (JF._mat2aa_parts(wild)[3] > 0).all()
    nan_in, inf_in = eye.clone(), eye.clone()
    nan_in[0, 1], inf_in[1, 1] = float('nan'), float('-inf')
    R = torch.cat([eye[None], wild, nan_in[None], inf_in[None]])
    w = torch.tensor(np.random.RandomState(5).randn(len(R), 3)).float()
    for name, fn, dev in (('mirror', JF.mat2aa, 'cpu'), ('fused', JF.FusedMat2AA.apply, device)):
        aa, grad = _mat2aa_run(fn, R.to(dev).contiguous(), w.to(dev))
        aa, grad = aa.cpu(), grad.cpu()
        assert torch.isfinite(aa).all() and torch.isfinite(grad).all(), name
        assert torch.equal(aa[0], torch.zeros(3)), name
        want = torch.zeros(3, 3)                   # at the identity (x, y, z) = (r21 - r12, r02 - r20, r10 - r01) / 4
        want[2, 1], want[1, 2] = 0.5 * w[0, 0], -0.5 * w[0, 0]
        want[0, 2], want[2, 0] = 0.5 * w[0, 1], -0.5 * w[0, 1]
        want[1, 0], want[0, 1] = 0.5 * w[0, 2], -0.5 * w[0, 2]
        torch.testing.assert_close(grad[0], want, rtol=1e-6, atol=1e-7, msg=name + ': gradient at the identity')
        for i in (5, 6):
            assert not aa[i].any() and not grad[i].any(), name + ': a NaN forward gives 0 and a zero gradient'
    a = _mat2aa_run(JF.mat2aa, R[1:5].double(), w[1:5].double())
    b = _mat2aa_run(JF.FusedMat2AA.apply, R[1:5].to(device).contiguous(), w[1:5].to(device))
    for x, y in zip(a, b):
        torch.testing.assert_close(y.double().cpu(), x, rtol=RTOL, atol=ATOL)


# ---------------------------------------------------------------------------------------------------- loss and schedule
def _state(step, device):
    st = _lib.OptState(best=float('inf'), step=step, ngroups=1)
    return JF._bytes_tensor(st, device)


def check_joint_l1(device, B):
    rs = np.random.RandomState(B)
    j = (rs.randn(B, 21, 3) * 0.05).astype(np.float32)
    t = (rs.randn(B, 21, 3) * 0.05).astype(np.float32)
    t[:, 0] = 0
    t[0, 5] = j[0, 5] - j[0, 0]                                   # an exactly-zero residual (three of them)
    t[B - 1, 20, 1] = j[B - 1, 20, 1] - j[B - 1, 0, 1]
    assert ((j[0, 5] - j[0, 0]) - t[0, 5] == 0).all()
    outs = {}
    for dt in (torch.float64, torch.float32):
        jj = torch.tensor(j, dtype=dt, requires_grad=True)
        per = ((jj - jj[:, :1]) - torch.tensor(t, dtype=dt)).abs().mean((1, 2))
        per.sum().backward()
        outs[dt] = (per.detach(), per.sum().detach().reshape(1), jj.grad)
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=device)
    loss, total, dj, hist = f(B), f(1), f(B, 21, 3), f(4, B)
    jd, td = torch.tensor(j).to(device), torch.tensor(t).to(device)
    L = ops._L()
    for step in (2, 0, 7):                                            # row 7 does not exist: nothing is written
        st = _state(step, device)
        ops.check(L.rih_joint_l1(jd.data_ptr(), td.data_ptr(), st.data_ptr(), loss.data_ptr(), total.data_ptr(), dj.data_ptr(),
                                 hist.data_ptr(), 4, B, ops._stream()), 'rih_joint_l1')
    assert torch.equal(hist[2], loss) and torch.equal(hist[0], loss) and not hist[1].any() and not hist[3].any()
    for name, g, r, w in zip(('loss', 'total', 'dj'), (loss, total, dj), outs[torch.float32], outs[torch.float64]):
        e = testing.assert_fp32_equivalent(g, r, w, k=4.0, what='joint_l1 %s B=%d' % (name, B))
        log('joint_l1 %s B=%d on %s: fused vs fp64 %.3g, fp32 torch vs fp64 %.3g' % (name, B, device, *e))
    d = dj.cpu()
    assert (d[0, 5] == 0).all() and d[B - 1, 20, 1] == 0                                   # sign(0) = 0
    assert set(np.unique(np.abs(d[:, 1:].numpy()))) <= {0.0, float(np.float32(1) / np.float32(63))}
    torch.testing.assert_close(d[:, 0], -d[:, 1:].sum(1), rtol=0, atol=1e-7)
    ops.check(L.rih_joint_l1(jd.data_ptr(), td.data_ptr(), 0, loss.data_ptr(), total.data_ptr(), dj.data_ptr(), 0, 0, B,
                             ops._stream()), 'rih_joint_l1 without a history')


def check_lr_schedule(device):
    """200 steps at lr 0.1, then the same launches on a block rewritten for n_iter = 7 and lr = 0.03: no other change."""
    p = torch.zeros(8, device=device)
    stepper = JF.DeviceAdamLinear([{'p': p, 'group': 0}], 1e-1, 200)
    stepper.set_grads([torch.ones(8, device=device)])
    for lr, n in ((1e-1, 200), (0.03, 7)):
        stepper.reset(lr, n)
        assert stepper.read_state()['lr'] == [lr] and stepper.read_state()['step'] == 0
        for i in range(n):
            stepper.step()
            st = stepper.read_state()
            want = lr * (n - i) / n
            assert st['lr'] == [want] and st['step'] == i + 1, (i, st, want)
            assert np.float32(st['lr'][0]) == np.float32(want)


# ---------------------------------------------------------------------------------------------------- the loop
def fitters(side, device, n_iter=200, select='last', graph=False):
    fused = JF.FusedManoJointFitter(layer(side, device), n_iter=n_iter, select=select, device=device, graph=graph)
    m32 = JF.ManoJointFitter(layer(side, 'cpu'), n_iter=n_iter, select=select, dtype=torch.float32)
    m64 = JF.ManoJointFitter(layer(side, 'cpu'), n_iter=n_iter, select=select, dtype=torch.float64)
    return fused, m32, m64


def _state_of(f):
    return [f.P.detach().clone().cpu(), f.beta.detach().clone().cpu()]


def check_golden_prefix():
    """The mirrors against the reference's own loop: the loss of iteration 0 at the project's bar; the fp32 mirror's
    parameters over the prefix as near the fp64 mirror as the reference's fp32 parameters are (k = 4), and `ori_pose`."""
    G = golden()
    for h in range(6):
        side = SIDES[int(G['side'][h])]
        _, m32, m64 = (None,) + fitters(side, 'cpu')[1:]
        J = torch.tensor(G['joints'][h:h + 1])
        for m in (m32, m64):
            m.start(J)
        close(m64.init_R, G['aik'][h:h + 1], 'init_R')
        for i in range(PREFIX + 1):
            for name, a, b, g in (('P', m32.P, m64.P, G['traj_P'][h, i]), ('beta', m32.beta, m64.beta, G['traj_beta'][h, i])):
                if i:
                    testing.assert_fp32_equivalent(a[0], torch.tensor(g), b[0], k=4.0, what='hand %d %s before iteration %d' % (h, name, i))
            m32.run(1), m64.run(1)
        close(m32.history[:PREFIX + 1, 0], G['hist'][h, :PREFIX + 1], 'loss history of hand %d' % h)
        # lines 226-231 on the reference's final parameters
        m64.P = torch.tensor(G['final_P'][h:h + 1], dtype=torch.float64)
        close(m64._ori_pose(m64.P), G['ori_pose'][h:h + 1], 'ori_pose of hand %d' % h)


def check_one_iteration(device, at=(0, 5, 50)):
    """Teacher-forced: one iteration (fresh moments) from the fp64 mirror's parameters at the given iterations."""
    J = torch.tensor(hands('right', 2))
    fused, m32, m64 = fitters('right', device)
    traj = JF.ManoJointFitter(layer('right', 'cpu'), dtype=torch.float64)
    traj.start(J)
    done = 0
    for it in at:
        traj.run(it - done)
        done = it
        P0, b0 = traj.P.detach().float(), traj.beta.detach().float()
        res = {}
        for name, f in (('fused', fused), ('m32', m32), ('m64', m64)):
            f.start(J.to(f.device).contiguous())
            with torch.no_grad():
                f.P.copy_(P0.to(f.P.dtype)), f.beta.copy_(b0.to(f.beta.dtype))
            f.run(1)
            grads = (f.g_P, f.g_beta) if name == 'fused' else (f.P.grad, f.beta.grad)
            hist = f.history
            res[name] = [hist[0].detach().clone()] + [g.detach().clone() for g in grads] + [f.P.detach().clone(), f.beta.detach().clone()]
        for k, name in enumerate(('loss', 'g_P', 'g_beta', 'P', 'beta')):
            e = testing.assert_fp32_equivalent(res['fused'][k], res['m32'][k], res['m64'][k], k=4.0,
                                               what='one iteration from iteration %d: %s' % (it, name))
            log('one iteration from %2d on %s, %s: fused vs fp64 %.3g, fp32 mirror vs fp64 %.3g' % (it, device, name, *e))


def check_prefix(device, B):
    J = torch.tensor(hands('right' if B == 1 else 'left', B))
    fused, m32, m64 = fitters('right' if B == 1 else 'left', device)
    for f in (fused, m32, m64):
        f.start(J.to(f.device).contiguous())
    for i in range(PREFIX):
        for f in (fused, m32, m64):
            f.run(1)
        for name, get in (('P', lambda f: f.P), ('beta', lambda f: f.beta), ('loss', lambda f: f.history[i])):
            e = testing.assert_fp32_equivalent(get(fused), get(m32), get(m64), k=4.0, what='B=%d after %d iterations: %s' % (B, i + 1, name))
            log('prefix B=%d on %s after %d iterations, %s: fused vs fp64 %.3g, fp32 mirror vs fp64 %.3g' % (B, device, i + 1, name, *e))
        e32 = float((m32.P.detach().double() - m64.P.detach()).abs().max() / m64.P.detach().abs().max())
        assert e32 < 1e-3, 'the fp32 mirror itself left the prefix: %g' % e32


_MIRROR_FITS = {}


def mirror_fits(select='last'):
    """The two mirrors' whole fits of the four hands of check 7 (two per side), computed once."""
    if select not in _MIRROR_FITS:
        out = {}
        for side in SIDES:
            J = torch.tensor(hands(side, 2))
            _, m32, m64 = (None,) + fitters(side, 'cpu', select=select)[1:]
            out[side] = (J, m32.fit(J), m64.fit(J))
        _MIRROR_FITS[select] = out
    return _MIRROR_FITS[select]


def chaos_ratio(fits):
    r = 1.0
    for J, r32, r64 in fits.values():
        a, b = r32['loss'].double(), r64['loss'].double()
        r = max(r, float(torch.maximum(a / b, b / a).max()))
    return r


def check_mirror_whole_fit():
    fits = mirror_fits()
    for side, (J, r32, r64) in fits.items():
        for r in (r32, r64):
            assert all(torch.isfinite(r[k]).all() for k in JF.KEYS)
            assert (r['loss'] < r['loss_history'][0]).all()
    log('whole fit: the mirrors\' own fp32 / fp64 ratio of final losses R = %.3g' % chaos_ratio(fits))


def check_whole_fit(device, graph):
    """200 iterations at B = 4 (two hands per side, one fitter per side: the template is the side's)."""
    fits = mirror_fits()
    R = chaos_ratio(fits)
    for side, (J, r32, r64) in fits.items():
        fused = JF.FusedManoJointFitter(layer(side, device), device=device, graph=graph)
        got = fused.fit(J.to(device).contiguous())
        assert all(torch.isfinite(got[k]).all() for k in JF.KEYS)
        loss, first = got['loss'].double().cpu(), got['loss_history'][0].double().cpu()
        bar = torch.maximum(r32['loss'].double(), r64['loss']) * R
        for b in range(2):
            log('whole fit %s hand %d on %s: final loss fused %.4g, fp32 mirror %.4g, fp64 mirror %.4g (first %.4g, R = %.3g)'
                % (side, b, device, loss[b], r32['loss'][b], r64['loss'][b], first[b], R))
        assert (loss < first).all(), (loss, first)
        assert (loss <= bar).all(), (loss, bar)
        best = JF.FusedManoJointFitter(layer(side, device), device=device, graph=graph, select='best')
        gb = best.fit(J.to(device).contiguous())
        hist = gb['loss_history']
        low = hist.min(0)[0]
        at = np.argmax((hist == low).cpu().numpy(), axis=0)                    # the first iteration that reached it
        assert (gb['loss'] <= low * (1 + 1e-4) + 1e-9).all(), (gb['loss'], low)
        assert torch.equal(hist, got['loss_history']), 'selection changed the trajectory'
        # the parameters of that iteration: rerun up to it
        again = JF.FusedManoJointFitter(layer(side, device), device=device, graph=graph)
        again.start(J.to(device).contiguous())
        done = 0
        for b in np.argsort(at):
            again.run(int(at[b]) - done)
            done = int(at[b])
            assert torch.equal(again.P[b], gb['pose_R'][b]) and torch.equal(again.beta[b], gb['beta'][b]), 'hand %d' % b


def check_surface(device):
    J = torch.tensor(hands('right', 2)).to(device)
    fused, m32, _ = fitters('right', device, n_iter=3)
    got, want = fused.fit(J.contiguous()), m32.fit(J.cpu())
    shapes = dict(pose_R=(2, 16, 3, 3), beta=(2, 10), ori_pose=(2, 48), verts=(2, 778, 3), joints=(2, 21, 3), loss=(2,),
                  loss_history=(3, 2), init_R=(2, 16, 3, 3))
    for r, dev in ((got, torch.device(device)), (want, torch.device('cpu'))):
        assert tuple(r.keys()) == JF.KEYS
        for k, s in shapes.items():
            assert tuple(r[k].shape) == s and r[k].device.type == dev.type and r[k].dtype == torch.float32, k
    assert not got['joints'][:, 0].any() and not want['joints'][:, 0].any()
    for k in JF.KEYS:
        torch.testing.assert_close(got[k].cpu(), want[k], rtol=1e-3, atol=1e-4, msg=k)
    # ori_pose is lines 226-231 on the returned parameters
    aa = JF.mat2aa(want['pose_R'].reshape(-1, 3, 3)).reshape(2, 48)
    L = layer('right', 'cpu')
    torch.testing.assert_close(want['ori_pose'], torch.cat([aa[:, :3], L.pca2axis(aa[:, 3:]) - L.hands_mean], 1), rtol=1e-5, atol=1e-6)


def check_refusals(device):
    import pytest
    J = torch.tensor(hands('right', 2)).to(device)
    fused = JF.FusedManoJointFitter(layer('right', device), device=device, graph=False)
    for bad in (J[:, :20], J[0], J.double(), J.transpose(0, 1).contiguous().transpose(0, 1), J[:0]):
        with pytest.raises(ValueError):
            fused.fit(bad)
    fused.n_iter = 0
    with pytest.raises(ValueError):
        fused.fit(J.contiguous())
    with pytest.raises(ValueError):
        JF.ManoJointFitter(layer('right', 'cpu'), select='first')
    with pytest.raises(RuntimeError):
        JF.ManoJointFitter(layer('right', 'cpu')).run(1)
    T = torch.tensor(golden()['template/right']).to(device)
    for args in ((T[:20], J), (T, J[:, :20]), (T.double(), J), (T, J.double())):
        with pytest.raises(ValueError):
            JF.fused_adaptive_ik(*args)
    with pytest.raises(ValueError):
        JF.FusedMat2AA.apply(torch.zeros(2, 3, 4, device=device))
    with pytest.raises(ValueError):
        JF.mat2aa(torch.zeros(2, 3, 4))
    # the entry points themselves
    L = ops._L()
    buf = torch.zeros(4096, device=device)
    p, einval = buf.data_ptr(), -1                 # RIH_EINVAL
    assert L.rih_aik(0, p, 1, p, 1, 0) == einval and L.rih_aik(p, p, 1, p, 0, 0) == einval and L.rih_aik(p, p, 2, p, 1, 0) == einval
    assert L.rih_mat2aa_fwd(0, p, 0, 1, 0, 0, 0) == einval and L.rih_mat2aa_fwd(p, p, 0, 0, 0, 0, 0) == einval
    assert L.rih_mat2aa_fwd(p, p, 0, 17, 16, 1, 0) == einval and L.rih_mat2aa_fwd(p, p, 0, 16, 16, 16, 0) == einval
    assert L.rih_mat2aa_fwd(p, p, 0, 4, 0, 1, 0) == einval
    assert L.rih_mat2aa_bwd(p, 0, 0, p, 1, 0, 0, 0) == einval and L.rih_mat2aa_bwd(p, p, 0, 0, 1, 0, 0, 0) == einval
    assert L.rih_joint_l1(p, p, 0, p, p, p, p, 4, 1, 0) == einval and L.rih_joint_l1(p, p, p, p, p, p, p, 0, 1, 0) == einval
    assert L.rih_joint_l1(0, p, p, p, p, p, p, 4, 1, 0) == einval and L.rih_joint_l1(p, p, p, p, p, p, p, 4, 0, 0) == einval
    assert L.rih_lr_linear_step(0, p, 0) == einval and L.rih_lr_linear_step(p, 0, 0) == einval
    assert L.rih_fit_select(p, p, p, p, p, 0, 1, 0) == einval and L.rih_fit_select(p, p, p, p, p, p, 0, 0) == einval


def check_graph(device):
    """Replayed graph against eager launches: every returned tensor, the moments and the state block, bit for bit; after a
    second fit on other joints; as 100 + 100 iterations; two runs."""
    L = layer('right', device)
    g = JF.FusedManoJointFitter(L, device=device, graph=True)
    e = JF.FusedManoJointFitter(L, device=device, graph=False)
    Ja, Jb = (torch.tensor(hands('right', 3)).to(device).contiguous(), torch.tensor(hands('right', 3)[::-1].copy() * 0.9).to(device).contiguous())

    def same(ra, rb, what):
        for k in JF.KEYS:
            assert torch.equal(ra[k], rb[k]), '%s: %s' % (what, k)
        for x, y in zip(g._statics()[6:], e._statics()[6:]):
            assert torch.equal(x, y), what + ': state or moments'
    first = g.fit(Ja)
    same(first, e.fit(Ja), 'first fit')
    same(g.fit(Jb), e.fit(Jb), 'second fit on other joints')
    e.start(Ja), e.run(100), e.run(100)
    again = g.fit(Ja)
    same(again, e.result(), '100 + 100 iterations')
    for k in JF.KEYS:
        assert torch.equal(first[k], again[k]), 'two runs: ' + k
    assert g.stepper.read_state()['step'] == 200
    g.n_iter, e.n_iter, g.lr, e.lr = 40, 40, 0.05, 0.05                     # no recapture: the same graph object
    graph = g._graph
    same(g.fit(Ja), e.fit(Ja), 'another n_iter and lr')
    assert g._graph is graph
