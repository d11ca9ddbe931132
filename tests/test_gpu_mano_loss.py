"""Fused HIP loss of the MANO-head model (csrc/rih_mano_loss.hip, renderih_amd.loss.FusedManoLoss) against the reference's
own core/Loss_mano.py (golden values and gradients), against the torch mirror at full batch sizes, and inside a captured
TrainStep of `load_new_model`, where the edge gate must follow set_epoch() without a re-capture."""
import pytest
import torch

from renderih_amd import testing
from test_mano_loss import (CASES, GOLDEN, PREDS, TERMS, check_against, evaluate, golden_inputs, hand_losses,  # noqa: F401
                            random_inputs)

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


@pytest.mark.parametrize('key,epoch,with_up', CASES)
def test_fused_matches_reference_golden(key, epoch, with_up):
    """Both epochs, the value-only up-sampling term, a predicted and a label rotation of exactly zero."""
    from renderih_amd.loss import FusedManoLoss, mano_loss_GCN_fused
    z, t = golden_inputs(dev())
    losses = hand_losses(dev())
    fused = FusedManoLoss(losses['left'], losses['right'])
    total, terms, grads = evaluate(mano_loss_GCN_fused, fused, epoch, losses, t,
                                   upsample_weight=t['upsample_weight'] if with_up else None)
    check_against(total, terms, grads, float(z[key + '/total']), {k: float(z[key + '/' + k]) for k in TERMS},
                  {k: torch.from_numpy(z[key + '/grad_' + k]) for k in PREDS})
    assert torch.isfinite(grads['pose_left'][0, 3:6]).all()


@pytest.mark.parametrize('B', [1, 64, 257])
def test_fused_matches_mirror_and_is_bit_identical(B):
    """Random data against the torch mirror on the GPU (epoch 60, edge term on); the gradients scale with the incoming
    gradient (3 x total); two fused evaluations are bit-identical (no atomics)."""
    from renderih_amd.loss import FusedManoLoss, mano_loss_GCN, mano_loss_GCN_fused
    losses = hand_losses(dev())
    t = random_inputs(B, seed=100 + B, device=dev())
    fused = FusedManoLoss(losses['left'], losses['right'])
    a = evaluate(mano_loss_GCN_fused, fused, 60, losses, dict(t), scale=3.0)
    b = evaluate(mano_loss_GCN_fused, fused, 60, losses, dict(t), scale=3.0)
    want = evaluate(mano_loss_GCN, None, 60, losses, dict(t), scale=3.0)
    assert torch.equal(a[0], b[0])
    assert all(torch.equal(a[1][k], b[1][k]) for k in TERMS) and all(torch.equal(a[2][k], b[2][k]) for k in PREDS)
    check_against(a[0], a[1], a[2], float(want[0]), {k: float(v) for k, v in want[1].items()}, want[2], rel=2e-5)


# ------------------------------------------------------------------------------------------------ inside TrainStep
def _new_model(seed=11):
    from renderih_amd import _lib
    from renderih_amd.lijun import build_new_model
    _lib.load()
    m = build_new_model(0.0)
    m.load_state_dict(testing.deterministic_state(m.state_dict(), seed=seed))
    m = m.to(dev()).train()
    m.decoder.unsample_layer.weight.requires_grad_(False)
    return m


def _labels(B, seed=3):
    g = torch.Generator().manual_seed(seed)
    lab = {'v3d_l': 0.05 * torch.randn(B, 778, 3, generator=g), 'v3d_r': 0.05 * torch.randn(B, 778, 3, generator=g),
           'v2d_l': 256 * torch.rand(B, 778, 2, generator=g), 'v2d_r': 256 * torch.rand(B, 778, 2, generator=g),
           'root_rel': 0.05 * torch.randn(B, 3, generator=g), 'lp': 0.5 * torch.randn(B, 48, generator=g),
           'ls': torch.randn(B, 10, generator=g), 'rp': 0.5 * torch.randn(B, 48, generator=g),
           'rs': torch.randn(B, 10, generator=g)}
    return {k: v.to(dev()) for k, v in lab.items()}


def _loss_args(out, lab):
    result, paramsDict, handDictList, otherInfo = out
    return (None, None, result, paramsDict, handDictList, otherInfo, None, None, None, lab['v2d_l'], None, lab['v2d_r'], None,
            lab['v3d_l'], None, lab['v3d_r'], None, lab['root_rel'], 256, lab['lp'], lab['ls'], lab['rp'], lab['rs'])


def _check_band(got, want, what):
    """The band of test_train_step_staged_graph_replay_matches_plain_backward: 1e-4 max |want| per tensor, plus for a bias
    1e-5 max |weight gradient|.  The key bias of a softmax attention (`w_ks.bias`) has a true gradient of exactly zero (it
    adds the same q.b_k to every score of a row, which the softmax ignores): both sides are round-off of the sum that forms
    the weight gradient, so it is held to 1e-4 of that weight gradient's magnitude."""
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:10]
    bad = []
    for k in want:
        wk = k[:-len('bias')] + 'weight'
        rel = 1e-4 if k.endswith('.w_ks.bias') else 1e-5
        floor = rel * float(want[wk].abs().max()) if (k.endswith('.bias') and wk in want) else 0.0
        err = float((got[k] - want[k]).abs().max())
        if err > 1e-4 * float(want[k].abs().max()) + floor:
            bad.append('%s: max err %.3g (max |want| %.3g)' % (k, err, float(want[k].abs().max())))
    assert not bad, '%s: %d gradients outside the band: %s' % (what, len(bad), '; '.join(bad[:20]))


def test_train_step_with_fused_mano_loss_matches_eager_mirror():
    """build_new_model(0.0), B = 2, TrainStep(stages='auto') (one captured hipGraph) with FusedManoLoss and SGD lr 0,
    against a plain eager `mano_loss_GCN(...).backward()` on an identical copy: every gradient within 1e-4 max (+ bias
    floor), replays bit-identical.  Then set_epoch(NORM_EPOCH, B, device): the REPLAYED graph's gradients equal the eager
    mirror at that epoch (edge term on) without a re-capture -- the gate is not frozen into the graph."""
    from renderih_amd import ops
    from renderih_amd.loss import FusedManoLoss, mano_loss_GCN, mano_loss_GCN_fused
    from renderih_amd.train import TrainStep
    B = 2
    img = testing.seeded_image(B, 31).cuda()
    lab = _labels(B)
    losses = hand_losses(dev())
    m1 = _new_model()

    def eager(epoch):
        m1.zero_grad(set_to_none=True)
        loss = mano_loss_GCN(None, epoch, losses['left'], losses['right'], *_loss_args(m1(img), lab))[0]
        loss.backward()
        return {k: p.grad.clone() for k, p in m1.named_parameters() if p.grad is not None}
    want0 = eager(0)

    m2 = _new_model()
    fused = FusedManoLoss(losses['left'], losses['right'])
    fused.set_epoch(0)
    opt = torch.optim.SGD([p for p in m2.parameters() if p.requires_grad], lr=0.0)      # lr 0: the state stays put

    def loss_fn(out, labels):
        return mano_loss_GCN_fused(fused, None, losses['left'], losses['right'], *_loss_args(out, labels))[0]
    try:
        step = TrainStep(m2, opt, loss_fn, (img.clone(), {k: v.clone() for k, v in lab.items()}), process_group=False,
                         stages='auto')
        assert step.use_graph and step.nstage == 1
        first = None
        for rep in range(3):
            loss = step(img, lab)
            assert bool(torch.isfinite(loss))
            got = {k: p.grad for k, p in m2.named_parameters() if p.grad is not None}
            _check_band(got, want0, 'epoch 0, replay %d' % rep)
            if first is None:
                first = {k: v.clone() for k, v in got.items()}
            else:
                for k in first:
                    assert torch.equal(got[k], first[k]), 'replay %d is not bit-identical to the first (%s)' % (rep, k)
        edge_off_grads = first
        want50 = eager(fused.w['NORM_EPOCH'])
        fused.set_epoch(fused.w['NORM_EPOCH'], B, dev())
        for rep in range(2):
            step(img, lab)
            got = {k: p.grad for k, p in m2.named_parameters() if p.grad is not None}
            _check_band(got, want50, 'epoch 50 after set_epoch, replay %d' % rep)
        # and the edge term did change the gradients (the check above is not vacuous)
        k = 'decoder.param_regressor.fc.0.weight'
        assert not torch.equal(edge_off_grads[k], got[k])
        assert any(float((want50[n] - want0[n]).abs().max()) > 1e-3 * float(want0[n].abs().max()) for n in want0)
    finally:
        ops.DROPOUT_SEED_TENSOR = None
