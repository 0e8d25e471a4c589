"""loss_bounds.xent_w on the CPU: torch's own float32 weighted cross-entropy and its autograd gradient stay inside the bound (the
condition for holding the HIP kernel to it), and the faults the bound is there to catch are flagged.  Mirrors
test_op_bounds_cpu.py::test_xent_float32_passes_and_faults_are_flagged."""
import pytest
import torch
import torch.nn.functional as F

import loss_bounds as lb

CASES = [(7, 5), (256, 100), (300, 1000), (1, 3), (776, 12)]


def _flagged(fn):
    with pytest.raises(AssertionError):
        fn()


def _inputs(N, NC):
    gen = torch.Generator().manual_seed(1000 * N + NC)
    l = torch.randn(N, NC, generator=gen) * 3
    t = torch.randint(0, NC, (N,), generator=gen)
    cw = 10.0 ** (torch.rand(NC, generator=gen) * 4 - 2)             # 1e-2 ... 1e2
    cw[0], cw[-1] = 1e-2, 1e2
    return l, t, cw


def _torch32(l, t, cw, scale, old=None):
    x = l.clone().requires_grad_(True)
    loss = F.cross_entropy(x, t, weight=cw) * scale
    loss.backward()
    loss = loss.detach() if old is None else loss.detach() + old
    return {'dlogits': x.grad, 'loss': loss.reshape(1)}


@pytest.mark.parametrize('N,NC', CASES)
def test_weighted_xent_float32_passes_and_faults_are_flagged(N, NC):
    l, t, cw = _inputs(N, NC)
    want = lb.xent_w(l, t, cw, 1.0)
    got = _torch32(l, t, cw, 1.0)
    print('weighted xent (%d, %d): torch float32 err/bound %.3f' % (N, NC, lb.check('xent_w', got, want, raise_=False)))
    assert lb.check('xent_w', got, want) < 1.0
    # the aux head: 0.4, accumulated onto the main head's loss
    want_aux = lb.xent_w(l, t, cw, 0.4, old_loss=float(got['loss']))
    got_aux = _torch32(l, t, cw, torch.tensor(0.4), old=got['loss'])
    assert lb.check('xent_w aux', got_aux, want_aux) < 1.0
    _flagged(lambda: lb.check('xent_w aux', {'loss': _torch32(l, t, cw, 1.0, old=got['loss'])['loss']}, want_aux))      # the aux term without 0.4
    _flagged(lambda: lb.check('xent_w aux', {'dlogits': got['dlogits']}, want_aux))
    _flagged(lambda: lb.check('xent_w aux', {'loss': got_aux['loss'] - got['loss']}, want_aux))                         # loss overwritten
    if N == 1:
        return                    # (one sample: w_t / W == 1 whatever the weights are -- the faults below change nothing)
    wt = cw[t]
    W, p = wt.sum(), torch.softmax(l, 1)
    oh = F.one_hot(t, NC).float()
    nll = -torch.log_softmax(l, 1)[torch.arange(N), t]
    # normalising by N instead of W
    _flagged(lambda: lb.check('xent_w', {'loss': ((wt * nll).sum() / N).reshape(1)}, want))
    _flagged(lambda: lb.check('xent_w', {'dlogits': wt[:, None] / N * (p - oh)}, want))
    # the gradient without w_t
    _flagged(lambda: lb.check('xent_w', {'dlogits': (p - oh) / W}, want))
    _flagged(lambda: lb.check('xent_w', {'dlogits': (p - oh) / N}, want))
    # one class's weight dropped to 1: of the classes that occur among the targets, the one whose weight is farthest from 1
    c = int((torch.bincount(t, minlength=NC).clamp_max(1) * cw.log().abs()).argmax())
    cw1 = cw.clone()
    cw1[c] = 1.0
    bad = _torch32(l, t, cw1, 1.0)
    _flagged(lambda: lb.check('xent_w', {'loss': bad['loss']}, want))
    _flagged(lambda: lb.check('xent_w', {'dlogits': bad['dlogits']}, want))


@pytest.mark.parametrize('N,NC', CASES)
def test_all_ones_weights_are_the_unweighted_loss(N, NC):
    """the weighted reference with w = 1 is op_bounds.xent's; its bound is no tighter, and wider only by the terms of W and of the
    rounded w_t * l_n (each at most ~gamma_N relative to the value)"""
    import op_bounds as ob
    l, t, _ = _inputs(N, NC)
    a = lb.xent_w(l, t, torch.ones(NC), 0.4, old_loss=5.0)
    b = ob.xent(l, t, 0.4, old_loss=5.0)
    for k in ('loss', 'dlogits'):
        assert torch.allclose(a[k][0], b[k][0], rtol=1e-14, atol=0)
        assert bool((a[k][1] >= b[k][1]).all())
        extra = 2 * (ob.gamma(N) + 4 * ob.U) * (b[k][0].abs() + 5.0 + b[k][1])
        assert bool((a[k][1] <= b[k][1] * (1 + 1e-3) + extra).all())
