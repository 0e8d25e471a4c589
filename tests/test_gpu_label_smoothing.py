"""TRAIN --label-smoothing on the GPU: the smoothed loss kernel (ifcbk_softmax_xent_ls, csrc/loss.hip) against
tests/loss_smooth_bounds.py at every shape of its list, its ABI (guard words, refusals, run-to-run bits), and the loss and head
gradients of whole models through the fused step, the validation loss and the reference-style training_step."""
import argparse

import pytest
import torch

import loss_bounds as lb
import loss_smooth_bounds as sb
import op_bounds as ob

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


# ====================================================================================================== the kernel
def _call(ctx, ld, td, cwd, N, NC, scale, eps, acc, with_dl, old=5.0):
    """-> (loss [1], dlogits [N, NC] or None); the words around both are checked"""
    lbuf = torch.full((3,), GUARD, device='cuda')
    if acc:
        lbuf[1] = old
    dbuf = torch.full((2 * G + N * NC,), GUARD, device='cuda') if with_dl else None
    ctx.call('ifcbk_softmax_xent_ls', P(ld), P(td), P(cwd), N, NC, scale, eps, P(lbuf[1:]), acc, P(dbuf[G:]) if with_dl else None, st())
    torch.cuda.synchronize()
    assert float(lbuf[0]) == GUARD and float(lbuf[2]) == GUARD
    if with_dl:
        assert bool((dbuf[:G] == GUARD).all()) and bool((dbuf[G + N * NC:] == GUARD).all())
        return lbuf[1:2].clone(), dbuf[G:G + N * NC].reshape(N, NC).clone()
    return lbuf[1:2].clone(), None


def _dev(l, t, cw):
    return l.cuda(), t.cuda(), None if cw is None else cw.cuda()


@pytest.mark.parametrize('N,NC', sb.SHAPES)
def test_softmax_xent_ls(ctx, N, NC):
    worst = 0.0
    for wm in sb.WEIGHTS:
        l, t, cw = sb.inputs(N, NC, wm)
        ld, td, cwd = _dev(l, t, cw)
        for eps in (0.1, 0.5, 1.0, 0.0):
            loss, dl = _call(ctx, ld, td, cwd, N, NC, 0.4, eps, 0, 1)
            if wm == 'zero' and NC == 1:
                # the only class weighs nothing: W = 0, and the value is 0 / 0 -- NaN in torch as well
                assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dl).all())
                continue
            want = sb.xent_ls(l, t, cw, 0.4, eps)
            name = 'softmax_xent_ls (%d, %d) %s eps %g' % (N, NC, wm, eps)
            worst = max(worst, sb.check(name, {'loss': loss, 'dlogits': dl}, want, family='softmax_xent_ls'))
    # the other modes: accumulate, no dlogits, weight 1; a row 80 above the others; run to run
    l, t, cw = sb.inputs(N, NC, 'random', offset_row=True)
    ld, td, cwd = _dev(l, t, cw)
    for acc, with_dl, scale in ((1, 1, 0.4), (0, 0, 0.4), (1, 0, 1.0), (0, 1, 1.0)):
        loss, dl = _call(ctx, ld, td, cwd, N, NC, scale, 0.1, acc, with_dl)
        want = sb.xent_ls(l, t, cw, scale, 0.1, old_loss=5.0 if acc else None)
        got = {'loss': loss, 'dlogits': dl} if with_dl else {'loss': loss}
        worst = max(worst, sb.check('softmax_xent_ls (%d, %d) +80 acc %d dlogits %d' % (N, NC, acc, with_dl), got, want, family='softmax_xent_ls'))
        loss2, dl2 = _call(ctx, ld, td, cwd, N, NC, scale, 0.1, acc, with_dl)
        assert torch.equal(loss, loss2) and (not with_dl or torch.equal(dl, dl2))
    print('softmax_xent_ls (%d, %d): worst err/bound %.3f' % (N, NC, worst))


def test_softmax_xent_ls_refusals_launch_nothing(ctx):
    N, NC = 7, 5
    l, t, cw = sb.inputs(N, NC, 'random')
    ld, td, cwd = _dev(l, t, cw)
    loss = torch.full((1,), GUARD, device='cuda')
    dl = torch.full((N, NC), GUARD, device='cuda')
    ok = (P(ld), P(td), P(cwd), N, NC, 1.0, 0.1, P(loss), 0, P(dl), st())

    def refused(**kw):
        names = ('logits', 'target', 'cw', 'N', 'NC', 'weight', 'eps', 'loss', 'acc', 'dl', 'stream')
        args = [kw.get(k, v) for k, v in zip(names, ok)]
        with pytest.raises(RuntimeError, match='softmax_xent_ls'):
            ctx.call('ifcbk_softmax_xent_ls', *args)
    for eps in (-0.1, 1.5, float('nan'), float('inf'), -float('inf')):
        refused(eps=eps)
    refused(N=0)
    refused(NC=0)
    refused(N=-1)
    refused(logits=None)
    refused(target=None)
    refused(loss=None)
    torch.cuda.synchronize()
    assert float(loss) == GUARD and bool((dl == GUARD).all())
    ctx.call('ifcbk_softmax_xent_ls', *ok)                       # ... and the same operands, unrefused, run
    torch.cuda.synchronize()
    sb.check('after the refusals', {'loss': loss, 'dlogits': dl}, sb.xent_ls(l, t, cw, 1.0, 0.1))


# ====================================================================================================== whole models
W7 = [0.02, 0.3, 1.0, 2.5, 7.0, 30.0, 90.0]
B = 3


def _hp(model, **kw):
    hp = dict(MODEL=model, classes=list('abcdefg'), pretrained=False, batch_size=B, precision='fp32', model_id='ls', resize=224,
              img_norm=None, seed=3)
    hp.update(kw)
    return argparse.Namespace(**hp)


def _want(heads, t, cw, eps):
    """fp64 reference and bound of the loss and of every head's dlogits, from the logits the engine holds"""
    main, aux = heads[0], (heads[1] if len(heads) > 1 else None)
    wm = sb.xent_ls(main.logits[:B].cpu(), t, cw, 1.0, eps)
    out = {'main': wm, 'loss': wm}
    if aux is not None:
        wa = sb.xent_ls(aux.logits[:B].cpu(), t, cw, 0.4, eps, old_loss=float(wm['loss'][0]))
        out['aux'], out['loss'] = wa, lb.head_sum(wm, wa)
    return out


@pytest.mark.parametrize('weights', [None, W7], ids=['plain', 'class_weights'])
@pytest.mark.parametrize('model', ['resnet18', 'inception_v3'])
def test_model_loss_and_head_gradients(model, weights):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    torch.manual_seed(11)
    m = NeustonModel(_hp(model, label_smoothing=0.1, class_weights=weights))
    eng = m.model.engine
    heads = m.model._train_heads
    assert eng.label_smoothing == 0.1 and m.criterion.label_smoothing == 0.1
    S = eng.net.S
    x = torch.rand(B, 3, S, S).cuda()
    t = torch.randint(0, 7, (B,))
    cw = None if weights is None else eng.class_weight.cpu()
    if model == 'inception_v3':
        m.model.set_dropout_mask((torch.rand(B, 2048) > 0.5).cuda())          # the same keep-mask in both train-mode forwards
    # reference-style step: torch's criterion (on the device) on the HIP logits
    m.train()
    ts = m.training_step((x, t, None), 0)['loss'].detach().reshape(1)
    # fused step: forward + smoothed loss + backward + Adam as one program
    m.fit_batch(x, t.cuda())
    torch.cuda.synchronize()
    want = _want(heads, t, cw, 0.1)
    fused = eng.loss.clone()
    print('%s: fused loss %.6f, training_step loss %.6f' % (model, float(fused), float(ts)))
    sb.check('%s eng.loss' % model, {'loss': fused}, want['loss'], family='label_smoothing model loss')
    sb.check('%s training_step loss' % model, {'loss': ts}, want['loss'], family='label_smoothing model loss')
    w, e = want['loss']['loss']
    bound = float(0.5 * ob.ulp(w.abs() + e, 'f32') + e)
    assert abs(float(fused) - float(ts)) <= 2 * bound                          # the two paths: within the sum of both bounds
    sb.check('%s main dlogits' % model, {'dlogits': heads[0].dlogits[:B]}, want['main'], family='label_smoothing model dlogits')
    if len(heads) > 1:
        sb.check('%s aux dlogits' % model, {'dlogits': heads[1].dlogits[:B]}, want['aux'], family='label_smoothing model dlogits')
    # the hard loss on the same logits is another number: the smoothing is in force
    hard = lb.xent_w(heads[0].logits[:B].cpu(), t, torch.ones(7) if cw is None else cw, 1.0)['loss'][0]
    assert abs(float(hard) - float(want['main']['loss'][0])) > 1e-3
    # validation: eval forward -> smoothed loss
    eng.load_input_nchw(x)
    eng.target[:B].copy_(t)
    probs, vloss = m.eval_current(B, with_loss=True)
    torch.cuda.synchronize()
    lg = heads[0].logits[:B].cpu()
    sb.check('%s eval_current loss' % model, {'loss': vloss.reshape(1)}, sb.xent_ls(lg, t, cw, 1.0, 0.1), family='label_smoothing model loss')
    assert torch.allclose(probs.cpu(), torch.softmax(lg, 1), atol=1e-5)


def _two_steps(**kw):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    torch.manual_seed(11)
    m = NeustonModel(_hp('resnet18', **kw))
    eng = m.model.engine
    g = torch.Generator().manual_seed(2)
    for _ in range(2):
        x = torch.rand(B, 3, 224, 224, generator=g).cuda()
        t = torch.randint(0, 7, (B,), generator=g)
        m.fit_batch(x, t.cuda())
    torch.cuda.synchronize()
    return dict(P=eng.P.clone(), loss=eng.loss.clone(), loss_sum=eng.loss_sum.clone())


def test_eps_0_steps_are_the_default_steps_bit_for_bit():
    a = _two_steps()
    b = _two_steps(label_smoothing=0.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a['P']).all()
    c = _two_steps(label_smoothing=0.1)
    assert not torch.equal(a['P'], c['P'])
