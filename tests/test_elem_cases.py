"""The tables of tests/elem_cases.py, checked on the references alone (no GPU, no kernel): every asserted case keeps torch
fp32 within CAP of fp64, so the bar 8 max(e32, 2^-23) never exceeds 1e-3; no asserted tensor has an identically zero reference
unless the case announces an exact zero; and the inputs really hold the edges the kernel tests rely on."""
import numpy as np
import pytest
import torch

import elem_cases as EC


@pytest.mark.parametrize('family', sorted(EC.FAMILIES))
def test_every_asserted_case_meets_the_cap(family):
    cases, reference = EC.FAMILIES[family]
    worst = 0.0
    for case in cases:
        ref = reference(case)
        for name in ref.asserted:
            zero = float(ref.x64[name].abs().max()) == 0.0
            assert zero == (name in ref.exact_zero), (family, case, name, 'zero reference')
            assert bool(torch.isfinite(ref.x64[name]).all()), (family, case, name)
        assert ref.e32 <= EC.CAP, (family, case, ref.e32_each)
        assert ref.bar() <= 1e-3
        worst = max(worst, ref.e32)
        print('ELEM-CASES %s %s e32 %.3e %s' % (family, EC.case_id(case), ref.e32,
                                              ' '.join('%s %.2e' % kv for kv in ref.e32_each.items())))
    print('ELEM-CASES %s worst asserted e32 %.3e over %d cases' % (family, worst, len(cases)))


def test_what_is_asserted_and_what_is_only_measured():
    for case in EC.LN_CASES + EC.LN_SWITCH_CASES + EC.LN_PAIR_CASES + EC.LN_MISALIGNED_CASES:
        assert case[2] in EC.LN_REGIMES and set(EC.ln_reference(case).asserted) == {'y', 'dx', 'dg', 'db'}, case
    for case in EC.LN_MEASURED_CASES:
        assert EC.ln_reference(case).asserted == (), case
    for case in EC.SM_CASES + EC.SM_DROPOUT_CASES:
        ref = EC.sm_reference(case)
        assert 'P' in ref.asserted and ('dS' in ref.asserted) == (case[3] <= 8.0), case
        assert ('Pd' in ref.asserted) == (case[4] > 0), case
    assert {c[3] for c in EC.SM_CASES} == {1e-3, 1.0, 8.0, 30.0, 1e3}
    # every switch on a 16-byte and on a generic shape
    for sw in ('x2', 'relu', 'skip'):
        assert {c[1] for c in EC.LN_SWITCH_CASES if sw in c[3]} >= {64, 200}, sw


def test_softmax_shapes_reach_every_form():
    forms = set()
    for rows, cols, ld in EC.SM_SHAPES:
        assert 1 <= cols <= ld <= 1024
        vec = cols % 4 == 0 and ld % 4 == 0
        forms.add(('vec', 1 if cols <= 256 else 2 if cols <= 512 else 4) if vec else ('generic', cols > 512))
    assert forms == {('vec', 1), ('vec', 2), ('vec', 4), ('generic', False), ('generic', True)}
    assert any(c % 4 == 0 and ld % 4 == 0 and ld > c for _, c, ld in EC.SM_SHAPES)          # a 16-byte form with ld > cols
    case, odd = EC.SM_MASK_TWIN
    assert case in EC.SM_DROPOUT_CASES and odd % 4 != 0 and odd >= case[1]
    for case in EC.SM_DROPOUT_CASES:
        keep = EC.sm_keep(case)
        assert 0.7 <= float(keep.float().mean()) <= 0.8 and not bool(keep.all(1).any())     # every row drops something


def test_cheby_graph_has_empty_rows_and_every_tail():
    for V, Fd, B in EC.CH_CASES + [EC.CH_MISALIGNED_CASE]:
        inp = EC.ch_inputs((V, Fd, B))
        indptr, indices, vals = (t.numpy() for t in inp['csr'])
        deg = np.diff(indptr)
        assert list(deg) == [min(v % 10, V) for v in range(V)], (V, 'row v has v % 10 neighbours')
        if V >= 10:
            assert set(deg) == set(range(10))                                               # empty rows, 4 and 5 among them
        assert bool((vals != 0).all()) and indices.min(initial=0) >= 0 and indices.max(initial=0) < V
        dense = np.zeros((V, V), np.float32)
        for v in range(V):
            dense[v, indices[indptr[v]:indptr[v + 1]]] = vals[indptr[v]:indptr[v + 1]]
        assert np.array_equal(dense, inp['M'])
        t_indptr, t_indices, t_vals = (t.numpy() for t in inp['csr_t'])
        dense_t = np.zeros((V, V), np.float32)
        for v in range(V):
            dense_t[v, t_indices[t_indptr[v]:t_indptr[v + 1]]] = t_vals[t_indptr[v]:t_indptr[v + 1]]
        assert np.array_equal(dense_t, inp['M'].T)
    shapes = EC.CH_CASES
    assert (256, 8, 2) in shapes and (257, 8, 2) in shapes                                   # the last LDS size and the first beyond
    assert any(F % 4 for _, F, _ in shapes) and any(F % 4 == 0 and (F // 4) % 4 for _, F, _ in shapes)
    V, Fd, B = EC.CH_TWIN
    assert B > 65535 and B // 2 <= 65535 and V <= 256 and Fd % 4 == 0
    assert EC.CH_MISALIGNED_CASE[1] % 4 == 0


def test_gather_index_is_the_crafted_one():
    idx = EC.GS_INDEX['crafted']
    counts = np.bincount(idx, minlength=EC.GS_VIN)
    assert sorted(counts)[-2:] == [3, 3] and list(counts).count(0) == 2
    assert len(EC.GS_INDEX['one']) == 1
    assert {D for _, D in EC.GS_CASES} == {1, 3, 4, 130}
    for case in EC.GS_CASES:
        dx = EC.gs_reference(case).x64['dx']
        assert bool((dx[:, EC.gs_unread(case)] == 0).all()) and EC.gs_unread(case)


def test_maxpool_inputs_tie_and_go_negative():
    tied = total = 0
    for shape in EC.MP_SHAPES:
        t, n = EC.mp_tied_windows((shape, 'ties'))
        tied, total = tied + t, total + n
        if shape[1] * shape[2] >= 16:                   # the maps with enough windows for a fraction to mean something
            assert 4 * t >= n, (shape, t, n)
        assert float(EC.mp_inputs((shape, 'neg'))['x'].max()) <= -1.0
        assert EC.mp_tied_windows((shape, 'neg')) == (t, n)
        c = EC.mp_inputs((shape, 'const'))['x']
        assert bool((c == EC.MP_CONST).all())
    assert 4 * tied >= total, (tied, total)
    print('ELEM-CASES maxpool tied windows %d of %d' % (tied, total))
    assert any(s[3] % 4 == 0 for s in EC.MP_SHAPES) and any(s[3] % 4 for s in EC.MP_SHAPES)
    assert any(s[1] != s[2] and s[1] % 2 and s[2] % 2 for s in EC.MP_SHAPES)                 # odd and unequal H and W
