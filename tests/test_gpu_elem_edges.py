"""The fp32 kernels of csrc/rih_elem.hip that every forward and backward pass goes through -- LayerNorm (generic and 16-byte
forms), softmax (+ dropout; generic and three 16-byte forms), max and average pooling, the Chebyshev feature build (LDS,
16-byte gather and scalar forms), row gather / scatter -- against torch.float64 at the edges of their shapes, dispatch
thresholds and value ranges.  Case tables, references and the bar: tests/elem_cases.py.

What the early parity tests in test_gpu_ops.py leave open: unit-scale randn at workload-like shapes against torch fp32 with one
fixed tolerance.  Softmax beyond 512 columns or at a pitch above its width, a LayerNorm row whose mean dwarfs its spread, the
generic kernels on misaligned operands, a CSR with empty rows, a pooling window that ties: none of it ran.

The check_* helpers also run on the host-compiled kernels (tests/test_kernels_on_cpu.py), which replaces dev()."""
import pytest
import torch

import elem_cases as EC

pytestmark = pytest.mark.gpu

RIH_EINVAL = -1
SENT = -7.25                # fills guard bands, pitch gaps and outputs before a launch
GUARD = 64                  # floats in front of and behind every buffer


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _lib():
    from renderih_amd import ops
    return ops._L(), ops._stream()


def leaf(t):
    """A fresh leaf on the device under test (the inputs of a case are shared)."""
    return t.detach().clone().to(dev()).requires_grad_(True)


class Buf:
    """n floats starting `off` floats past a 16-byte boundary, between two guard bands of SENT inside one allocation; the payload
    holds `values`, or SENT."""

    def __init__(self, n, off=0, values=None):
        self.flat = torch.full((GUARD + 4 + n + GUARD,), SENT).to(dev())
        base = self.flat.data_ptr()
        assert base % 4 == 0
        self.start = GUARD + (-(base // 4 + GUARD)) % 4 + off
        self.n = n
        self.ptr = base + 4 * self.start
        assert self.ptr % 16 == 4 * off
        if values is not None:
            self.t.copy_(values.reshape(-1).to(dev()))

    @property
    def t(self):
        return self.flat[self.start:self.start + self.n]

    def guards_intact(self):
        f = self.flat.cpu()
        return bool((f[:self.start] == SENT).all()) and bool((f[self.start + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.flat == SENT).all())


def _intact(bufs, what):
    for name, b in bufs.items():
        assert b is None or b.guards_intact(), (what, name, 'a guard band was written')


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
def layernorm_abi(case, off=0):
    """rih_layernorm_fwd / _bwd on guarded buffers, x (and x2, dy, y, dx) `off` floats off a 16-byte boundary: name -> tensor."""
    rows, D, regime, sw = case
    inp = EC.ln_inputs(case)
    relu = 1 if 'relu' in sw else 0
    L, stream = _lib()
    opt = lambda t: None if t is None else Buf(rows * D, off, t)
    nblk = L.rih_ln_nblk(rows)
    b = dict(x=Buf(rows * D, off, inp['x']), x2=opt(inp['x2']), g=Buf(D, 0, inp['g']), b=Buf(D, 0, inp['b']),
             y=Buf(rows * D, off), mean=Buf(rows), rstd=Buf(rows), dy=Buf(rows * D, off, inp['gy']), dres=opt(inp['dres']),
             dx=Buf(rows * D, off), dg=Buf(D), db=Buf(D), ws=Buf(2 * nblk * D))
    p = lambda k: 0 if b[k] is None else b[k].ptr
    rc = L.rih_layernorm_fwd(p('x'), p('x2'), p('g'), p('b'), p('y'), p('mean'), p('rstd'), rows, D, EC.EPS, relu, stream)
    assert rc == 0, rc
    rc = L.rih_layernorm_bwd(p('dy'), p('x'), p('x2'), p('y') if relu else 0, p('g'), p('mean'), p('rstd'), p('dres'), p('dx'),
                             p('dg'), p('db'), rows, D, relu, p('ws'), stream)
    assert rc == 0, rc
    _intact(b, case)
    for k in ('x', 'g', 'b', 'dy'):
        assert torch.equal(b[k].t.cpu(), inp['gy' if k == 'dy' else k].reshape(-1)), (case, k, 'input overwritten')
    return dict(y=b['y'].t.view(rows, D), dx=b['dx'].t.view(rows, D), dg=b['dg'].t, db=b['db'].t)


def check_layernorm_abi(case, off=0):
    got = layernorm_abi(case, off)
    EC.check_bar('layernorm %s%s' % (EC.case_id(case), ' misaligned' if off else ''), got, EC.ln_reference(case))


OPS_SWITCHES = ('x2', 'relu', 'skip', 'pair')        # what the ops layer offers; all three at once only through the C ABI


def check_layernorm_ops(case):
    """The switches through the ops layer: x2 (the residual add in front of the norm), ReLU, the skip gradient
    (ops.layernorm_skip), and both hands in one launch with their own parameters (ops.layernorm_pair)."""
    from renderih_amd import ops
    rows, D, regime, sw = case
    inp = EC.ln_inputs(case)
    d = dev()
    x = leaf(inp['x'])
    if sw == 'pair':
        mods = []
        for h in (0, 1):
            m = torch.nn.LayerNorm(D, eps=EC.EPS).to(d)
            with torch.no_grad():
                m.weight.copy_(inp['g'][h])
                m.bias.copy_(inp['b'][h])
            mods.append(m)
        y = ops.layernorm_pair(x, mods[0], mods[1])
        y.backward(inp['gy'].to(d))
        got = dict(y=y, dx=x.grad, dg=torch.stack([m.weight.grad for m in mods]), db=torch.stack([m.bias.grad for m in mods]))
    else:
        g, b = leaf(inp['g']), leaf(inp['b'])
        if sw == 'skip':
            y, xs = ops.layernorm_skip(x, g, b, EC.EPS)
            ((y * inp['gy'].to(d)).sum() + (xs * inp['dres'].to(d)).sum()).backward()
        else:
            assert 'skip' not in sw
            y = ops.layernorm(x, g, b, EC.EPS, x2=None if inp['x2'] is None else inp['x2'].to(d), relu='relu' in sw)
            y.backward(inp['gy'].to(d))
        got = dict(y=y, dx=x.grad, dg=g.grad, db=b.grad)
    EC.check_bar('layernorm %s ops' % EC.case_id(case), got, EC.ln_reference(case))


# --------------------------------------------------------------------------------------------------------------------- softmax
def softmax_abi(case, ld=None):
    """rih_softmax_fwd in place (P == S, as the ops layer calls it) and rih_softmax_bwd in place on [rows][ld] buffers whose
    columns cols..ld hold SENT, which must survive both passes: name -> [rows, cols] tensor."""
    rows, cols, ld0, scale, p = case
    ld = ld0 if ld is None else ld
    inp = EC.sm_inputs(case)
    L, stream = _lib()

    def pitched(values=None):
        buf = Buf(rows * ld)
        if values is not None:
            buf.t.view(rows, ld)[:, :cols] = values.to(dev())
        return buf
    window = lambda buf: buf.t.view(rows, ld)[:, :cols].clone()
    b = dict(S=pitched(inp['S']), Pd=pitched() if p > 0 else None, dP=pitched(inp['dP']))
    rc = L.rih_softmax_fwd(b['S'].ptr, b['S'].ptr, b['Pd'].ptr if p > 0 else b['S'].ptr, rows, cols, ld, p, EC.DROP_SEED, None, stream)
    assert rc == 0, rc
    got = dict(P=window(b['S']))
    if p > 0:
        got['Pd'] = window(b['Pd'])
    rc = L.rih_softmax_bwd(b['S'].ptr, b['dP'].ptr, rows, cols, ld, p, EC.DROP_SEED, None, EC.ALPHA, stream)
    assert rc == 0, rc
    got['dS'] = window(b['dP'])
    _intact(b, case)
    for name, buf in b.items():
        if buf is not None and ld > cols:
            assert bool((buf.t.view(rows, ld)[:, cols:] == SENT).all()), (case, ld, name, 'columns cols..ld were written')
    assert torch.equal(got['P'], window(b['S'])), (case, 'the backward wrote P')
    return got


def check_softmax(case):
    got = softmax_abi(case)
    EC.check_bar('softmax %s' % EC.case_id(case), got, EC.sm_reference(case))


def _check_mask(case, got, what):
    p = case[4]
    keep = EC.sm_keep(case)
    P, Pd = got['P'].cpu(), got['Pd'].cpu()
    assert float(P.min()) > 0.0                                         # so a zero of Pd is a dropped element
    assert torch.equal(Pd != 0, keep), (what, 'the zero pattern is not the hash mask', int(((Pd != 0) != keep).sum()))
    want = P.double() / (1.0 - p)
    # one rounding of 1 / (1 - p), one of the product
    assert bool(((Pd.double() - want).abs()[keep] <= 2.0 ** -22 * want[keep]).all()), (what, 'kept values are not P / (1 - p)')


def check_softmax_dropout(case):
    got = softmax_abi(case)
    what = 'softmax %s' % EC.case_id(case)
    frac = float(EC.sm_keep(case).float().mean())
    print('ELEM-EDGE %s keep fraction %.4f' % (what, frac))
    assert abs(frac - (1 - case[4])) <= 0.03, frac
    EC.check_bar(what, got, EC.sm_reference(case))
    _check_mask(case, got, what)


def check_softmax_mask_twin():
    """One set of rows through the 16-byte form and, at an odd pitch, through the scalar form: identical masks."""
    case, odd_ld = EC.SM_MASK_TWIN
    assert case[1] % 4 == 0 and case[2] % 4 == 0 and odd_ld % 2 == 1
    vec, scalar = softmax_abi(case), softmax_abi(case, odd_ld)
    ref = EC.sm_reference(case)
    for got, what in ((vec, 'softmax %s 16-byte' % EC.case_id(case)), (scalar, 'softmax %s ld %d scalar' % (EC.case_id(case), odd_ld))):
        EC.check_bar(what, got, ref)
        _check_mask(case, got, what)
    assert torch.equal(vec['Pd'] == 0, scalar['Pd'] == 0)
    assert torch.equal(vec['dS'] == 0, scalar['dS'] == 0)


# ------------------------------------------------------------------------------------------------------------------- Chebyshev
def cheby_abi(inp, off=0):
    """rih_cheby_fwd / _bwd on guarded buffers, x, y, dy and dx `off` floats off a 16-byte boundary."""
    B, V, Fd = inp['x'].shape
    L, stream = _lib()
    d = dev()
    # a graph without an edge (V = 1) has empty index and weight arrays; one unused element keeps their pointers non-null
    up = lambda t: (t if t.numel() else t.new_zeros(1)).to(d)
    csr, csr_t = [up(t) for t in inp['csr']], [up(t) for t in inp['csr_t']]
    b = dict(x=Buf(B * V * Fd, off, inp['x']), y=Buf(B * V * 2 * Fd, off), dy=Buf(B * V * 2 * Fd, off, inp['gy']),
             dx=Buf(B * V * Fd, off))
    rc = L.rih_cheby_fwd(b['x'].ptr, csr[0].data_ptr(), csr[1].data_ptr(), csr[2].data_ptr(), b['y'].ptr, B, V, Fd, stream)
    assert rc == 0, rc
    rc = L.rih_cheby_bwd(b['dy'].ptr, csr_t[0].data_ptr(), csr_t[1].data_ptr(), csr_t[2].data_ptr(), b['dx'].ptr, B, V, Fd, stream)
    assert rc == 0, rc
    got = dict(y=b['y'].t.view(B, V, 2 * Fd).clone(), dx=b['dx'].t.view(B, V, Fd).clone())
    _intact(b, (V, Fd, B))
    return got


def check_cheby(case, off=0):
    got = cheby_abi(EC.ch_inputs(case), off)
    EC.check_bar('cheby %s%s' % (EC.case_id(case), ' misaligned' if off else ''), got, EC.ch_reference(case))


def check_cheby_forms_bit_identical():
    """B = 65536 takes the 16-byte gather form, its halves of 32768 the LDS form: the same bits in y and dx."""
    inp = EC.ch_twin_inputs()
    B = inp['x'].shape[0]
    whole = cheby_abi(inp)
    for h in (0, 1):
        sl = slice(h * B // 2, (h + 1) * B // 2)
        half = cheby_abi(dict(inp, x=inp['x'][sl], gy=inp['gy'][sl]))
        for n in ('y', 'dx'):
            a, b = whole[n][sl].contiguous().view(torch.int32), half[n].contiguous().view(torch.int32)
            assert torch.equal(a, b), (n, h, int((a != b).sum()))
    L64 = torch.from_numpy(inp['M']).double()
    y64 = torch.stack((inp['x'].double(), torch.matmul(L64, inp['x'].double())), -1).flatten(-2)
    assert EC.rel_err(whole['y'].cpu(), y64) <= EC.FACTOR * EC.U23            # and they are the right bits


# -------------------------------------------------------------------------------------------------------------- gather / scatter
def check_gather(case):
    from renderih_amd import ops
    inp = EC.gs_inputs(case)
    d = dev()
    x = leaf(inp['x'])
    y = ops.RowIndex(inp['idx'], EC.GS_VIN, d)(x)
    y.backward(inp['gy'].to(d))
    ref = EC.gs_reference(case)
    what = 'gather %s' % EC.case_id(case)
    assert torch.equal(y.detach().cpu().double(), ref.x64['y']), (what, 'the forward is a copy: bit-exact')
    EC.check_bar(what, dict(y=y, dx=x.grad), ref)
    unread = EC.gs_unread(case)
    assert unread and bool((x.grad[:, unread] == 0).all()), (what, 'a row nothing reads has a gradient')


# --------------------------------------------------------------------------------------------------------------------- pooling
def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def check_maxpool(case):
    from renderih_amd import ops
    inp = EC.mp_inputs(case)
    d = dev()
    x = leaf(_nhwc(inp['x']))
    y = ops.maxpool3x3s2(x)
    y.backward(_nhwc(inp['gy']).to(d))
    ref = EC.mp_reference(case)
    what = 'maxpool %s' % EC.case_id(case)
    got = dict(y=y.detach().permute(0, 3, 1, 2), dx=x.grad.permute(0, 3, 1, 2))
    assert torch.equal(got['y'].cpu().double(), ref.x64['y']), (what, 'a maximum is one of the inputs: bit-exact')
    EC.check_bar(what, got, ref)


def check_avgpool(case):
    from renderih_amd import ops
    inp = EC.ap_inputs(case)
    d = dev()
    x = leaf(_nhwc(inp['x']))
    y = ops.global_avgpool(x)
    y.backward(inp['gy'].to(d))
    EC.check_bar('avgpool %s' % EC.case_id(case), dict(y=y, dx=x.grad.permute(0, 3, 1, 2)), EC.ap_reference(case))


# -------------------------------------------------------------------------------------------------------------------- refusals
def check_refusals():
    """RIH_EINVAL before any launch, outputs left alone.  Operands of a valid call's size wherever the refused argument allows
    it: a refusal that failed would then still run inside them."""
    L, stream = _lib()
    d = dev()
    rows, cols, D = 4, 1024, 1024
    ones = lambda n: Buf(n, 0, torch.ones(n))
    outs = dict(P=Buf(rows * cols), Pd=Buf(rows * cols), y=Buf(rows * D), mean=Buf(rows), rstd=Buf(rows), dx=Buf(rows * D),
                dg=Buf(D), db=Buf(D), ws=Buf(2 * L.rih_ln_nblk(rows) * D), cy=Buf(2 * 4 * 8), cdx=Buf(2 * 4 * 4), gy=Buf(2 * 3 * 4),
                gdx=Buf(2 * 4 * 4), my=Buf(4 * 4), mdx=Buf(4 * 4 * 4), ay=Buf(4), adx=Buf(4 * 4 * 4))
    S, dPd, x, g, b, dy = ones(rows * cols), ones(rows * cols), ones(rows * D), ones(D), ones(D), ones(rows * D)
    arg = torch.zeros(64, dtype=torch.int8).to(d)
    iptr = torch.tensor([0, 1, 2, 3, 4], dtype=torch.int32).to(d)
    iidx = torch.tensor([0, 1, 2, 3], dtype=torch.int32).to(d)
    o = {k: v.ptr for k, v in outs.items()}
    sm_fwd = lambda S_=S.ptr, P=o['P'], Pd=o['Pd'], r=rows, c=cols, ld=cols, p=0.0: L.rih_softmax_fwd(S_, P, Pd, r, c, ld, p, 1, None, stream)
    sm_bwd = lambda P=S.ptr, dP=o['P'], r=rows, c=cols, ld=cols, p=0.0: L.rih_softmax_bwd(P, dP, r, c, ld, p, 1, None, 0.5, stream)
    ln_fwd = lambda x_=x.ptr, g_=g.ptr, y=o['y'], r=rows, D_=D: L.rih_layernorm_fwd(x_, 0, g_, b.ptr, y, o['mean'], o['rstd'], r, D_, 1e-6, 0, stream)
    ln_bwd = lambda dy_=dy.ptr, y=0, dx=o['dx'], r=rows, D_=D, relu=0: L.rih_layernorm_bwd(
        dy_, x.ptr, 0, y, g.ptr, S.ptr, S.ptr, 0, dx, o['dg'], o['db'], r, D_, relu, o['ws'], stream)
    refused = [
        ('softmax cols > 1024', sm_fwd(c=1025, ld=1028)), ('softmax ld < cols', sm_fwd(c=1024, ld=1020)),
        ('softmax drop_p >= 1', sm_fwd(p=1.0)), ('softmax Pd == P with dropout', sm_fwd(Pd=o['P'], p=0.25)),
        ('softmax null S', sm_fwd(S_=0)), ('softmax null P', sm_fwd(P=0)), ('softmax rows < 1', sm_fwd(r=0)),
        ('softmax bwd cols > 1024', sm_bwd(c=1025, ld=1028)), ('softmax bwd ld < cols', sm_bwd(ld=1020)),
        ('softmax bwd drop_p >= 1', sm_bwd(p=1.5)), ('softmax bwd null dPd', sm_bwd(dP=0)),
        ('layernorm D > 1024', ln_fwd(D_=1025)), ('layernorm rows < 1', ln_fwd(r=0)), ('layernorm null x', ln_fwd(x_=0)),
        ('layernorm null y', ln_fwd(y=0)), ('layernorm bwd D > 1024', ln_bwd(D_=1025)), ('layernorm bwd rows < 1', ln_bwd(r=0)),
        ('layernorm bwd ReLU without y', ln_bwd(relu=1)), ('layernorm bwd null dy', ln_bwd(dy_=0)), ('layernorm bwd null dx', ln_bwd(dx=0)),
        ('cheby null x', L.rih_cheby_fwd(0, iptr.data_ptr(), iidx.data_ptr(), x.ptr, o['cy'], 2, 4, 4, stream)),
        ('cheby null indptr', L.rih_cheby_fwd(x.ptr, 0, iidx.data_ptr(), x.ptr, o['cy'], 2, 4, 4, stream)),
        ('cheby V < 1', L.rih_cheby_fwd(x.ptr, iptr.data_ptr(), iidx.data_ptr(), x.ptr, o['cy'], 2, 0, 4, stream)),
        ('cheby bwd null dy', L.rih_cheby_bwd(0, iptr.data_ptr(), iidx.data_ptr(), x.ptr, o['cdx'], 2, 4, 4, stream)),
        ('gather null idx', L.rih_gather_rows(x.ptr, 0, o['gy'], 2, 4, 3, 4, stream)),
        ('scatter null inv_ptr', L.rih_scatter_rows_add(x.ptr, 0, iidx.data_ptr(), o['gdx'], 2, 4, 4, 4, stream)),
        ('maxpool null x', L.rih_maxpool3x3s2_fwd(0, o['my'], arg.data_ptr(), 1, 4, 4, 4, stream)),
        ('maxpool bwd null arg', L.rih_maxpool3x3s2_bwd(x.ptr, 0, o['mdx'], 1, 4, 4, 4, stream)),
        ('avgpool null x', L.rih_avgpool_fwd(0, o['ay'], 1, 16, 4, stream)),
        ('avgpool bwd HW < 1', L.rih_avgpool_bwd(x.ptr, o['adx'], 1, 0, 4, stream)),
    ]
    for what, rc in refused:
        assert rc == RIH_EINVAL, (what, rc)
    if d.type == 'cuda':
        torch.cuda.synchronize()
    for name, buf in outs.items():
        assert buf.untouched(), (name, 'written by a refused call')
    assert bool((arg == 0).all())


# ---------------------------------------------------------------------------------------------------------------- the GPU tests
@pytest.mark.parametrize('case', EC.LN_CASES, ids=EC.case_id)
def test_layernorm_vs_fp64(case):
    check_layernorm_abi(case)


@pytest.mark.parametrize('case', EC.LN_SWITCH_CASES + EC.LN_PAIR_CASES, ids=EC.case_id)
def test_layernorm_switches_vs_fp64(case):
    if case[3] in OPS_SWITCHES:
        check_layernorm_ops(case)
    if case[3] != 'pair':
        check_layernorm_abi(case)


@pytest.mark.parametrize('case', EC.LN_MISALIGNED_CASES, ids=EC.case_id)
def test_layernorm_misaligned_operands_take_the_generic_kernel(case):
    check_layernorm_abi(case, off=1)


def test_layernorm_offset_1e4_is_measured_not_asserted():
    for case in EC.LN_MEASURED_CASES:
        check_layernorm_abi(case)


@pytest.mark.parametrize('case', EC.SM_CASES, ids=EC.case_id)
def test_softmax_vs_fp64(case):
    check_softmax(case)


@pytest.mark.parametrize('case', EC.SM_DROPOUT_CASES, ids=EC.case_id)
def test_softmax_dropout_vs_fp64_and_hash_mask(case):
    check_softmax_dropout(case)


def test_softmax_scalar_and_16_byte_forms_drop_the_same_elements():
    check_softmax_mask_twin()


@pytest.mark.parametrize('case', EC.CH_CASES, ids=EC.case_id)
def test_cheby_vs_fp64(case):
    check_cheby(case)


def test_cheby_misaligned_operands_take_the_scalar_kernels():
    check_cheby(EC.CH_MISALIGNED_CASE, off=1)


def test_cheby_lds_and_gather_forms_are_bit_identical():
    check_cheby_forms_bit_identical()


@pytest.mark.parametrize('case', EC.GS_CASES, ids=EC.case_id)
def test_gather_scatter_vs_fp64(case):
    check_gather(case)


@pytest.mark.parametrize('case', EC.MP_CASES, ids=EC.case_id)
def test_maxpool_ties_and_padding_vs_torch(case):
    check_maxpool(case)


@pytest.mark.parametrize('case', EC.AP_CASES, ids=EC.case_id)
def test_avgpool_vs_fp64(case):
    check_avgpool(case)


def test_elem_refusals():
    check_refusals()
