"""TRAIN --focal-gamma on the GPU: the focal loss kernel (ifcbk_softmax_xent_focal, csrc/loss.hip) against tests/loss_focal_bounds.py at
every shape of its list, its ABI (guard words, refusals, run-to-run bits), the op dispatch (f[2]), and the loss and head gradients of
whole models through the fused step, the validation loss and the reference-style training_step."""
import argparse

import pytest
import torch

import loss_bounds as lb
import loss_focal_bounds as fb
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
def _call(ctx, ld, td, cwd, N, NC, scale, g, acc, with_dl, old=5.0):
    """-> (loss [1], dlogits [N, NC] or None); the words around both are checked"""
    lbuf = torch.full((3,), GUARD, device='cuda')
    if acc:
        lbuf[1] = old
    dbuf = torch.full((2 * G + N * NC,), GUARD, device='cuda') if with_dl else None
    ctx.call('ifcbk_softmax_xent_focal', P(ld), P(td), P(cwd), N, NC, scale, g, P(lbuf[1:]), acc, P(dbuf[G:]) if with_dl else None, st())
    torch.cuda.synchronize()
    assert float(lbuf[0]) == GUARD and float(lbuf[2]) == GUARD
    if with_dl:
        assert bool((dbuf[:G] == GUARD).all()) and bool((dbuf[G + N * NC:] == GUARD).all())
        return lbuf[1:2].clone(), dbuf[G:G + N * NC].reshape(N, NC).clone()
    return lbuf[1:2].clone(), None


def _dev(l, t, cw):
    return l.cuda(), t.cuda(), None if cw is None else cw.cuda()


@pytest.mark.parametrize('N,NC', fb.SHAPES)
def test_softmax_xent_focal(ctx, N, NC):
    worst = 0.0
    fam = 'softmax_xent_focal'
    for wm in fb.WEIGHTS:
        l, t, cw = fb.inputs(N, NC, wm)
        ld, td, cwd = _dev(l, t, cw)
        for g in fb.GAMMAS + (0.0,):
            loss, dl = _call(ctx, ld, td, cwd, N, NC, 0.4, g, 0, 1)
            if wm == 'zero' and NC == 1:
                # the only class weighs nothing: W = 0, and the value is 0 / 0
                assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dl).all())
                continue
            if NC == 1 and g > 0:
                assert float(loss) == 0.0 and not dl.any()                    # u = 0 always: both outputs exactly 0
            want = fb.xent_focal(l, t, cw, 0.4, g)
            worst = max(worst, fb.check('%s (%d, %d) %s gamma %g' % (fam, N, NC, wm, g), {'loss': loss, 'dlogits': dl}, want, family=fam))
    # the other modes: accumulate, no dlogits, weight 1; a row 80 above the others; run to run
    l, t, cw = fb.inputs(N, NC, 'random', mode='row80')
    ld, td, cwd = _dev(l, t, cw)
    for acc, with_dl, scale in ((1, 1, 0.4), (0, 0, 0.4), (1, 0, 1.0), (0, 1, 1.0)):
        loss, dl = _call(ctx, ld, td, cwd, N, NC, scale, 2.0, acc, with_dl)
        want = fb.xent_focal(l, t, cw, scale, 2.0, old_loss=5.0 if acc else None)
        got = {'loss': loss, 'dlogits': dl} if with_dl else {'loss': loss}
        worst = max(worst, fb.check('%s (%d, %d) +80 acc %d dlogits %d' % (fam, N, NC, acc, with_dl), got, want, family=fam))
        loss2, dl2 = _call(ctx, ld, td, cwd, N, NC, scale, 2.0, acc, with_dl)
        assert torch.equal(loss, loss2) and (not with_dl or torch.equal(dl, dl2))
    # the rows at the ends of u: the whole row 120 higher; the target 120 above its row (u == 0 exactly); the target 80 below it (u -> 1)
    for mode in ('row120', 'peak120', 'low80'):
        l, t, cw = fb.inputs(N, NC, 'random', mode=mode)
        ld, td, cwd = _dev(l, t, cw)
        for g in (0.5, 2.0):
            loss, dl = _call(ctx, ld, td, cwd, N, NC, 1.0, g, 0, 1)
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all())
            if mode == 'peak120':
                assert not dl[N // 2].any()
            worst = max(worst, fb.check('%s (%d, %d) %s gamma %g' % (fam, N, NC, mode, g), {'loss': loss, 'dlogits': dl},
                                        fb.xent_focal(l, t, cw, 1.0, g), family=fam))
    print('%s (%d, %d): worst err/bound %.3f' % (fam, N, NC, worst))


def test_softmax_xent_focal_refusals_launch_nothing(ctx):
    N, NC = 7, 5
    l, t, cw = fb.inputs(N, NC, 'random')
    ld, td, cwd = _dev(l, t, cw)
    loss = torch.full((1,), GUARD, device='cuda')
    dl = torch.full((N, NC), GUARD, device='cuda')
    ok = (P(ld), P(td), P(cwd), N, NC, 1.0, 2.0, P(loss), 0, P(dl), st())

    def refused(**kw):
        names = ('logits', 'target', 'cw', 'N', 'NC', 'weight', 'gamma', 'loss', 'acc', 'dl', 'stream')
        args = [kw.get(k, v) for k, v in zip(names, ok)]
        with pytest.raises(RuntimeError, match='softmax_xent_focal'):
            ctx.call('ifcbk_softmax_xent_focal', *args)
    for g in (-0.5, float('nan'), float('inf'), -float('inf')):
        refused(gamma=g)
    refused(N=0)
    refused(NC=0)
    refused(N=-1)
    refused(logits=None)
    refused(target=None)
    refused(loss=None)
    torch.cuda.synchronize()
    assert float(loss) == GUARD and bool((dl == GUARD).all())
    ctx.call('ifcbk_softmax_xent_focal', *ok)                    # ... and the same operands, unrefused, run
    torch.cuda.synchronize()
    fb.check('after the refusals', {'loss': loss, 'dlogits': dl}, fb.xent_focal(l, t, cw, 1.0, 2.0))


# ====================================================================================================== dispatch
@pytest.mark.parametrize('weights', ['none', 'random'])
def test_op_dispatch_on_f2(ctx, weights):
    """a one-op program: f[2] = gamma runs the focal kernel with the op's operands; f[1] and f[2] together are refused, nothing written"""
    from ifcb_classifier_amd.engine import OpList, Program
    lib = _lib()
    N, NC = 7, 5
    l, t, cw = fb.inputs(N, NC, weights)
    ld, td, cwd = _dev(l, t, cw)
    loss = torch.full((1,), GUARD, device='cuda')
    dl = torch.full((N, NC), GUARD, device='cuda')
    kind, extra = (lib.OP_SOFTMAX_XENT, ()) if cw is None else (lib.OP_SOFTMAX_XENT_W, (P(cwd),))

    def prog(f):
        ops = OpList()
        ops.add(kind, 'loss', p=(P(ld), P(td), P(loss), P(dl)) + extra, i=(N, NC), f=f)
        return Program(ops)
    bad = prog((1.0, 0.1, 2.0))
    with pytest.raises(RuntimeError, match=r'\(-1\).*f\[1\].*f\[2\]'):               # (-1: IFCBK_EINVAL)
        ctx.run_program(bad.arr, bad.n, st())
    torch.cuda.synchronize()
    assert float(loss) == GUARD and bool((dl == GUARD).all())
    good = prog((1.0, 0.0, 2.0))
    ctx.run_program(good.arr, good.n, st())
    torch.cuda.synchronize()
    fb.check('op f[2] = 2', {'loss': loss, 'dlogits': dl}, fb.xent_focal(l, t, cw, 1.0, 2.0))
    a, b = loss.clone(), dl.clone()
    ctx.call('ifcbk_softmax_xent_focal', P(ld), P(td), P(cwd), N, NC, 1.0, 2.0, P(loss), 0, P(dl), st())
    torch.cuda.synchronize()
    assert torch.equal(a, loss) and torch.equal(b, dl)


# ====================================================================================================== whole models
W7 = [0.02, 0.3, 1.0, 2.5, 7.0, 30.0, 90.0]
B = 3


def _hp(model, **kw):
    hp = dict(MODEL=model, classes=list('abcdefg'), pretrained=False, batch_size=B, precision='fp32', model_id='fg', resize=224,
              img_norm=None, seed=3)
    hp.update(kw)
    return argparse.Namespace(**hp)


def _want(heads, t, cw, g):
    """fp64 reference and bound of the loss and of every head's dlogits, from the logits the engine holds"""
    main, aux = heads[0], (heads[1] if len(heads) > 1 else None)
    wm = fb.xent_focal(main.logits[:B].cpu(), t, cw, 1.0, g)
    out = {'main': wm, 'loss': wm}
    if aux is not None:
        wa = fb.xent_focal(aux.logits[:B].cpu(), t, cw, 0.4, g, old_loss=float(wm['loss'][0]))
        out['aux'], out['loss'] = wa, lb.head_sum(wm, wa)
    return out


def _crit_want(heads, t, cw, g):
    """the same for training_step: criterion(main) + 0.4 * criterion(aux), each within the kernel's bound of a weight-1 call"""
    wm = fb.xent_focal(heads[0].logits[:B].cpu(), t, cw, 1.0, g)['loss']
    if len(heads) == 1:
        return {'loss': wm}
    wa = fb.xent_focal(heads[1].logits[:B].cpu(), t, cw, 1.0, g)['loss']
    k = ob.f32(0.4)
    v = wm[0] + k * wa[0]
    e = wm[1] + k * wa[1] + ob.U * (k * (wa[0].abs() + wa[1])) + ob.U * (v.abs() + wm[1] + k * wa[1])
    return {'loss': (v, e)}


@pytest.mark.parametrize('weights', [None, W7], ids=['plain', 'class_weights'])
@pytest.mark.parametrize('model', ['resnet18', 'inception_v3'])
def test_model_loss_and_head_gradients(model, weights):
    from ifcb_classifier_amd.neuston_models import FocalLoss, NeustonModel
    torch.manual_seed(11)
    m = NeustonModel(_hp(model, focal_gamma=2.0, class_weights=weights))
    eng = m.model.engine
    heads = m.model._train_heads
    assert eng.focal_gamma == 2.0 and isinstance(m.criterion, FocalLoss) and m.criterion.gamma == 2.0
    S = eng.net.S
    x = torch.rand(B, 3, S, S).cuda()
    t = torch.randint(0, 7, (B,))
    cw = None if weights is None else eng.class_weight.cpu()
    if model == 'inception_v3':
        m.model.set_dropout_mask((torch.rand(B, 2048) > 0.5).cuda())          # the same keep-mask in both train-mode forwards
    # reference-style step: the criterion module (on the device) on the HIP logits
    m.train()
    ts = m.training_step((x, t, None), 0)['loss'].detach().reshape(1)
    # fused step: forward + focal loss + backward + Adam as one program
    m.fit_batch(x, t.cuda())
    torch.cuda.synchronize()
    want = _want(heads, t, cw, 2.0)
    fused = eng.loss.clone()
    print('%s: fused loss %.6f, training_step loss %.6f' % (model, float(fused), float(ts)))
    fb.check('%s eng.loss' % model, {'loss': fused}, want['loss'], family='focal model loss')
    cwant = _crit_want(heads, t, cw, 2.0)
    fb.check('%s training_step loss' % model, {'loss': ts}, cwant, family='focal model loss')
    w, e = want['loss']['loss']
    w2, e2 = cwant['loss']
    bound = float(0.5 * ob.ulp(w.abs() + e, 'f32') + e) + float(0.5 * ob.ulp(w2.abs() + e2, 'f32') + e2)
    assert abs(float(fused) - float(ts)) <= bound                              # the two paths: within the sum of both bounds
    fb.check('%s main dlogits' % model, {'dlogits': heads[0].dlogits[:B]}, want['main'], family='focal model dlogits')
    if len(heads) > 1:
        fb.check('%s aux dlogits' % model, {'dlogits': heads[1].dlogits[:B]}, want['aux'], family='focal model dlogits')
    # the hard loss on the same logits is another number: the focusing is in force
    hard = lb.xent_w(heads[0].logits[:B].cpu(), t, torch.ones(7) if cw is None else cw, 1.0)['loss'][0]
    assert abs(float(hard) - float(want['main']['loss'][0])) > 1e-3
    # validation: eval forward -> focal loss
    eng.load_input_nchw(x)
    eng.target[:B].copy_(t)
    probs, vloss = m.eval_current(B, with_loss=True)
    torch.cuda.synchronize()
    lg = heads[0].logits[:B].cpu()
    fb.check('%s eval_current loss' % model, {'loss': vloss.reshape(1)}, fb.xent_focal(lg, t, cw, 1.0, 2.0), family='focal model loss')
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


def test_gamma_0_steps_are_the_default_steps_bit_for_bit():
    a = _two_steps()
    b = _two_steps(focal_gamma=0.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a['P']).all()
    c = _two_steps(focal_gamma=2.0)
    assert not torch.equal(a['P'], c['P'])
