"""TRAIN --mixup / --cutmix on the GPU: the two-target loss kernel (ifcbk_softmax_xent_mix, csrc/loss.hip) against tests/mix_cases.py at
every shape of its list, its ABI (guard words, refusals, run-to-run bits), lam == 1 against the smoothed one-target reference, and the
op dispatch on p[5]."""
import pytest
import torch

import loss_smooth_bounds as sb
import mix_cases as mc

pytestmark = pytest.mark.gpu
GUARD = -12345.0
G = 64                           # guard words on either side of dlogits


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def P(t):
    return _lib().ptr(t)


def st():
    return _lib().cur_stream()


def _call(ctx, ld, td, lmd, cwd, N, NC, scale, eps, acc, with_dl, old=5.0):
    """-> (loss [1], dlogits [N, NC] or None); the words around both are checked"""
    lbuf = torch.full((3,), GUARD, device='cuda')
    if acc:
        lbuf[1] = old
    dbuf = torch.full((2 * G + N * NC,), GUARD, device='cuda') if with_dl else None
    ctx.call('ifcbk_softmax_xent_mix', P(ld), P(td), P(lmd), P(cwd), N, NC, scale, eps, P(lbuf[1:]), acc, P(dbuf[G:]) if with_dl else None, st())
    torch.cuda.synchronize()
    assert float(lbuf[0]) == GUARD and float(lbuf[2]) == GUARD
    if with_dl:
        assert bool((dbuf[:G] == GUARD).all()) and bool((dbuf[G + N * NC:] == GUARD).all())
        return lbuf[1:2].clone(), dbuf[G:G + N * NC].reshape(N, NC).clone()
    return lbuf[1:2].clone(), None


def _dev(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


@pytest.mark.parametrize('NC', mc.LOSS_NCS)
@pytest.mark.parametrize('N', mc.LOSS_NS)
def test_softmax_xent_mix(ctx, N, NC):
    worst = 0.0
    fam = 'softmax_xent_mix'
    for wm in mc.WEIGHTS:
        for eps in mc.EPSS:
            for lam in mc.LAMS:
                l, t, lm, cw = mc.loss_inputs(N, NC, wm, lam)
                ld, td, lmd, cwd = _dev(l, t, lm, cw)
                loss, dl = _call(ctx, ld, td, lmd, cwd, N, NC, 0.4, eps, 0, 1)
                if wm == 'zero' and NC == 1:
                    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dl).all())          # the only class weighs nothing: 0 / 0
                    continue
                tag = '%s (%d, %d) %s eps %g lam %s' % (fam, N, NC, wm, eps, lam)
                worst = max(worst, mc.check(tag, {'loss': loss, 'dlogits': dl}, mc.xent_mix(l, t, lm, cw, 0.4, eps), family=fam))
                if lam == 'ones':
                    # lam == 1 everywhere: the smoothed one-target loss, within ITS reference's bound
                    sb.check(tag + ' vs xent_ls', {'loss': loss, 'dlogits': dl}, sb.xent_ls(l, t, cw, 0.4, eps), family=fam + ' lam 1')
    # the other modes: logits spread by 30, weight 1 and 0.4 each with the accumulate flag, no dlogits; run to run
    l, t, lm, cw = mc.loss_inputs(N, NC, 'random', 'rows', spread=30.0)
    ld, td, lmd, cwd = _dev(l, t, lm, cw)
    for acc, with_dl, scale in ((1, 1, 0.4), (0, 0, 0.4), (1, 0, 1.0), (0, 1, 1.0), (1, 1, 1.0), (0, 1, 0.4)):
        loss, dl = _call(ctx, ld, td, lmd, cwd, N, NC, scale, 0.1, acc, with_dl)
        want = mc.xent_mix(l, t, lm, cw, scale, 0.1, old_loss=5.0 if acc else None)
        got = {'loss': loss, 'dlogits': dl} if with_dl else {'loss': loss}
        worst = max(worst, mc.check('%s (%d, %d) spread 30 acc %d dlogits %d' % (fam, N, NC, acc, with_dl), got, want, family=fam))
        loss2, dl2 = _call(ctx, ld, td, lmd, cwd, N, NC, scale, 0.1, acc, with_dl)
        assert torch.equal(loss, loss2) and (not with_dl or torch.equal(dl, dl2))
    print('%s (%d, %d): worst err/bound %.3f' % (fam, N, NC, worst))


def test_rows_whose_two_targets_coincide(ctx):
    """a == b on every row: both one-hot terms land on one element, and the value is the one-target loss whatever lam is"""
    N, NC = 6, 5
    l, t, lm, cw = mc.loss_inputs(N, NC, 'random', 'rows')
    t = torch.cat([t[:3], t[:3].flip(0)])
    assert torch.equal(t, t.flip(0))
    ld, td, lmd, cwd = _dev(l, t, lm, cw)
    loss, dl = _call(ctx, ld, td, lmd, cwd, N, NC, 1.0, 0.1, 0, 1)
    mc.check('a == b', {'loss': loss, 'dlogits': dl}, mc.xent_mix(l, t, lm, cw, 1.0, 0.1))
    one = sb.reference(l, t, cw, 1.0, 0.1)
    assert abs(float(loss) - float(one[0])) <= 1e-5 * abs(float(one[0])) and torch.allclose(dl.cpu().double(), one[1], atol=1e-6)


def test_refusals_launch_nothing(ctx):
    N, NC = 7, 5
    l, t, lm, cw = mc.loss_inputs(N, NC, 'random')
    ld, td, lmd, cwd = _dev(l, t, lm, cw)
    loss = torch.full((1,), GUARD, device='cuda')
    dl = torch.full((N, NC), GUARD, device='cuda')
    ok = (P(ld), P(td), P(lmd), P(cwd), N, NC, 1.0, 0.1, P(loss), 0, P(dl), st())

    def refused(**kw):
        names = ('logits', 'target', 'lam', 'cw', 'N', 'NC', 'weight', 'eps', 'loss', 'acc', 'dl', 'stream')
        args = [kw.get(k, v) for k, v in zip(names, ok)]
        with pytest.raises(RuntimeError, match=r'ifcbk_softmax_xent_mix failed \(-1\)'):
            ctx.call('ifcbk_softmax_xent_mix', *args)
    refused(lam=None)
    for e in (-0.1, 1.5, float('nan'), float('inf')):
        refused(eps=e)
    refused(N=0)
    refused(NC=0)
    refused(N=-1)
    refused(logits=None)
    refused(target=None)
    refused(loss=None)
    torch.cuda.synchronize()
    assert float(loss) == GUARD and bool((dl == GUARD).all())
    ctx.call('ifcbk_softmax_xent_mix', *ok)
    torch.cuda.synchronize()
    mc.check('after the refusals', {'loss': loss, 'dlogits': dl}, mc.xent_mix(l, t, lm, cw, 1.0, 0.1))


@pytest.mark.parametrize('weights', ['none', 'random'])
def test_op_dispatch_on_p5(ctx, weights):
    """a one-op program: p[5] = the factors runs the two-target kernel with the op's operands and f[1] as eps; p[5] and f[2] together are
    refused, nothing written; p[5] NULL is the one-target dispatch"""
    from ifcb_classifier_amd.engine import OpList, Program
    lib = _lib()
    N, NC = 7, 5
    l, t, lm, cw = mc.loss_inputs(N, NC, weights)
    ld, td, lmd, cwd = _dev(l, t, lm, cw)
    loss = torch.full((1,), GUARD, device='cuda')
    dl = torch.full((N, NC), GUARD, device='cuda')
    kind, extra = (lib.OP_SOFTMAX_XENT, (None,)) if cw is None else (lib.OP_SOFTMAX_XENT_W, (P(cwd),))

    def prog(f, lam=True):
        ops = OpList()
        ops.add(kind, 'loss', p=(P(ld), P(td), P(loss), P(dl)) + extra + ((P(lmd),) if lam else ()), i=(N, NC), f=f)
        return Program(ops)
    bad = prog((1.0, 0.0, 2.0))
    with pytest.raises(RuntimeError, match=r'\(-1\).*p\[5\].*f\[2\]'):               # (-1: IFCBK_EINVAL)
        ctx.run_program(bad.arr, bad.n, st())
    torch.cuda.synchronize()
    assert float(loss) == GUARD and bool((dl == GUARD).all())
    for eps in (0.0, 0.1):
        good = prog((1.0, eps))
        ctx.run_program(good.arr, good.n, st())
        torch.cuda.synchronize()
        mc.check('op p[5], eps %g' % eps, {'loss': loss, 'dlogits': dl}, mc.xent_mix(l, t, lm, cw, 1.0, eps))
        a, b = loss.clone(), dl.clone()
        ctx.call('ifcbk_softmax_xent_mix', P(ld), P(td), P(lmd), P(cwd), N, NC, 1.0, eps, P(loss), 0, P(dl), st())
        torch.cuda.synchronize()
        assert torch.equal(a, loss) and torch.equal(b, dl)
    plain = prog((1.0, 0.1), lam=False)
    ctx.run_program(plain.arr, plain.n, st())
    torch.cuda.synchronize()
    sb.check('op without p[5]', {'loss': loss, 'dlogits': dl}, sb.xent_ls(l, t, cw, 1.0, 0.1))
