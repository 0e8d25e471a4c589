"""TRAIN --class-norm / --weight-decay on the GPU: the weighted loss kernel (ifcbk_softmax_xent_w, csrc/loss.hip) against
tests/loss_bounds.py, the loss and the head gradients of whole models teacher-forced on their own logits, the fused step with the
two options, and the command line end to end."""
import argparse
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_bounds as lb
import op_bounds as ob

pytestmark = pytest.mark.gpu
NAN = float('nan')


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def P(t):
    return _lib().ptr(t)


def st():
    return _lib().cur_stream()


# ====================================================================================================== the kernel
SHAPES = [(7, 5), (256, 100), (300, 1000), (1, 3), (776, 12)]
MODES = [(0, 1), (1, 1), (0, 0), (1, 0)]                     # (loss_accumulate, dlogits given)


def _inputs(N, NC):
    gen = torch.Generator().manual_seed(1000 * N + NC)
    l = torch.randn(N, NC, generator=gen) * 3
    t = torch.randint(0, NC, (N,), generator=gen)
    cw = 10.0 ** (torch.rand(NC, generator=gen) * 4 - 2)             # 1e-2 ... 1e2
    cw[0], cw[-1] = 1e-2, 1e2
    return l, t, cw


def _call(ctx, entry, ld, td, cwd, N, NC, scale, acc, with_dl):
    loss = torch.full((1,), 5.0 if acc else NAN, device='cuda')
    dl = torch.full((N + 1, NC), NAN, device='cuda') if with_dl else None
    if entry == 'ifcbk_softmax_xent_w':
        ctx.call(entry, P(ld), P(td), P(cwd), N, NC, scale, P(loss), acc, P(dl), st())
    else:
        ctx.call(entry, P(ld), P(td), N, NC, scale, P(loss), acc, P(dl), st())
    torch.cuda.synchronize()
    if with_dl:
        assert torch.isnan(dl[N]).all() and torch.isfinite(dl[:N]).all()           # nothing behind the last sample, everything before it
    return loss, dl


@pytest.mark.parametrize('acc,with_dl', MODES)
@pytest.mark.parametrize('N,NC', SHAPES)
def test_softmax_xent_w(ctx, N, NC, acc, with_dl):
    l, t, cw = _inputs(N, NC)
    ld, td, cwd = l.cuda(), t.cuda(), cw.cuda()
    loss, dl = _call(ctx, 'ifcbk_softmax_xent_w', ld, td, cwd, N, NC, 0.4, acc, with_dl)
    want = lb.xent_w(l, t, cw, 0.4, old_loss=5.0 if acc else None)
    got = {'loss': loss}
    if with_dl:
        got['dlogits'] = dl[:N]
    print('softmax_xent_w (%d, %d) acc %d dlogits %d: err/bound %.3f' % (N, NC, acc, with_dl, lb.check('xent_w', got, want, raise_=False)))
    lb.check('softmax_xent_w (%d, %d, %d, %d)' % (N, NC, acc, with_dl), got, want, family='softmax_xent_w')
    # run to run: bitwise
    loss2, dl2 = _call(ctx, 'ifcbk_softmax_xent_w', ld, td, cwd, N, NC, 0.4, acc, with_dl)
    assert torch.equal(loss, loss2) and (not with_dl or torch.equal(dl[:N], dl2[:N]))
    # all-ones weights: the unweighted kernel, bit for bit
    ones = torch.ones(NC, device='cuda')
    la, da = _call(ctx, 'ifcbk_softmax_xent_w', ld, td, ones, N, NC, 0.4, acc, with_dl)
    lu, du = _call(ctx, 'ifcbk_softmax_xent', ld, td, None, N, NC, 0.4, acc, with_dl)
    assert torch.equal(la, lu) and (not with_dl or torch.equal(da[:N], du[:N]))


def test_softmax_xent_w_refuses_a_missing_weight_vector(ctx):
    l, t, cw = _inputs(7, 5)
    ld, td = l.cuda(), t.cuda()
    loss = torch.zeros(1, device='cuda')
    with pytest.raises(RuntimeError, match='class_weight'):
        ctx.call('ifcbk_softmax_xent_w', P(ld), P(td), None, 7, 5, 1.0, P(loss), 0, None, st())
    with pytest.raises(RuntimeError):
        ctx.call('ifcbk_softmax_xent_w', P(ld), P(td), P(cw.cuda()), 0, 5, 1.0, P(loss), 0, None, st())


# ====================================================================================================== whole models, teacher-forced
W7 = [0.02, 0.3, 1.0, 2.5, 7.0, 30.0, 90.0]


def _hp(model, B, **kw):
    hp = dict(MODEL=model, classes=list('abcdefg'), pretrained=False, batch_size=B, precision='fp32', model_id='cn', resize=224,
              img_norm=None, seed=3)
    hp.update(kw)
    return argparse.Namespace(**hp)


def _want(heads, N, t, cw):
    """fp64 reference and bound of the loss and of every head's dlogits, from the logits the engine holds; torch's own float64
    CrossEntropyLoss(weight=) on those logits is the same number"""
    main, aux = heads[0], (heads[1] if len(heads) > 1 else None)
    lm = main.logits[:N].cpu()
    wm = lb.xent_w(lm, t, cw, 1.0)
    ref = F.cross_entropy(lm.double(), t, weight=cw.double())
    out = {'main': wm, 'loss': wm}
    if aux is not None:
        la = aux.logits[:N].cpu()
        wa = lb.xent_w(la, t, cw, 0.4, old_loss=float(wm['loss'][0]))
        ref = ref + ob.f32(0.4) * F.cross_entropy(la.double(), t, weight=cw.double())      # (0.4 as the float the op carries)
        out['aux'], out['loss'] = wa, lb.head_sum(wm, wa)
    assert abs(float(out['loss']['loss'][0]) - float(ref)) <= 1e-12 * abs(float(ref))
    return out


@pytest.mark.parametrize('model,B', [('resnet18', 16), ('inception_v3', 8)])
def test_model_loss_and_head_gradients_teacher_forced(model, B):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    torch.manual_seed(11)
    m = NeustonModel(_hp(model, B, class_weights=W7, class_norm=1.0))
    eng = m.model.engine
    heads = m.model._train_heads
    S = eng.net.S
    x = torch.rand(B, 3, S, S).cuda()
    t = torch.randint(0, 7, (B,))
    cw = eng.class_weight.cpu()
    assert m.criterion.weight.is_cuda and torch.equal(m.criterion.weight.cpu(), cw)
    if model == 'inception_v3':
        m.model.set_dropout_mask((torch.rand(B, 2048) > 0.5).cuda())          # the same keep-mask in both train-mode forwards
    # reference-style step: torch's criterion (on the device) on the HIP logits
    m.train()
    ts = m.training_step((x, t, None), 0)['loss'].detach().reshape(1)
    # fused step: forward + weighted loss + backward + Adam as one program
    m.fit_batch(x, t.cuda())
    torch.cuda.synchronize()
    want = _want(heads, B, t, cw)
    print('%s: fused loss %.6f, training_step loss %.6f' % (model, float(eng.loss), float(ts)))
    lb.check('%s eng.loss' % model, {'loss': eng.loss}, want['loss'], family='class_norm model loss')
    lb.check('%s training_step loss' % model, {'loss': ts}, want['loss'], family='class_norm model loss')
    lb.check('%s main dlogits' % model, {'dlogits': heads[0].dlogits[:B]}, want['main'], family='class_norm model dlogits')
    if len(heads) > 1:
        lb.check('%s aux dlogits' % model, {'dlogits': heads[1].dlogits[:B]}, want['aux'], family='class_norm model dlogits')
    # ... and torch's float32 autograd on the same logits gives gradients inside the same bound
    for h, key, s in zip(heads, ('main', 'aux'), (1.0, 0.4)):
        lg = h.logits[:B].cpu().clone().requires_grad_(True)
        (F.cross_entropy(lg, t, weight=cw) * s).backward()
        lb.check('%s torch %s dlogits' % (model, key), {'dlogits': lg.grad}, want[key])
    # the unweighted loss on the same logits is another number: the weights are in force
    plain = F.cross_entropy(heads[0].logits[:B].cpu().double(), t)
    assert abs(float(plain) - float(want['main']['loss'][0])) > 1e-3
    # validation: eval forward -> weighted loss
    probs, vloss = m.eval_batch(x, t.cuda())
    torch.cuda.synchronize()
    lg = heads[0].logits[:B].cpu()
    lb.check('%s eval_batch loss' % model, {'loss': vloss.reshape(1)}, lb.xent_w(lg, t, cw, 1.0), family='class_norm model loss')
    assert torch.allclose(probs.cpu(), torch.softmax(lg, 1), atol=1e-5)
    vs = m.validation_step((x, t, None), 0)['val_batch_loss'].reshape(1)
    lb.check('%s validation_step loss' % model, {'loss': vs}, lb.xent_w(lg, t, cw, 1.0))


# ====================================================================================================== the fused step
def _three_steps(model, B, **kw):
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    eng = Engine(graph.build(model, 7), 0, max_batch=B, **kw)
    eng.init_weights(seed=5)
    g = torch.Generator().manual_seed(2)
    S = eng.net.S
    for k in range(3):
        x = torch.rand(B, 3, S, S, generator=g).cuda()
        t = torch.randint(0, 7, (B,), generator=g)
        eng.load_input_nchw(x)
        eng.target[:B].copy_(t)
        eng.train_step(B)
    torch.cuda.synchronize()
    out = dict(P=eng.P.clone(), RB=eng.RB.clone(), nbt=eng.nbt.clone(), loss=eng.loss.clone(), loss_sum=eng.loss_sum.clone())
    eng.close()
    return out


@pytest.mark.parametrize('model,B', [('inception_v3', 4)])
def test_class_norm_0_steps_are_the_default_steps_bit_for_bit(model, B):
    a = _three_steps(model, B)
    b = _three_steps(model, B, class_weights=[1.0] * 7)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a['P']).all() and int(a['nbt'][0]) == 3


def test_weight_decay_step_is_torch_adam_with_weight_decay():
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    B, wd = 8, 1e-2
    eng = Engine(graph.build('resnet18', 7), 0, max_batch=B, weight_decay=wd)
    eng.init_weights(seed=5)
    g = torch.Generator().manual_seed(4)
    eng.load_input_nchw(torch.rand(B, 3, 224, 224, generator=g).cuda())
    eng.target[:B].copy_(torch.randint(0, 7, (B,), generator=g))
    p0 = eng.P.clone()
    assert not eng.M.any() and not eng.V.any()
    eng.train_step(B)
    torch.cuda.synchronize()
    grad = eng.G.clone()                                   # the engine's own gradient of this step
    assert torch.isfinite(grad).all() and grad.abs().max() > 0
    want = ob.adam(p0, grad, torch.zeros_like(p0), torch.zeros_like(p0), eng.lr, eng.betas[0], eng.betas[1], eng.eps, wd, 1, 1.0)
    # the helper's float64 reference IS torch's Adam(weight_decay=) (L2 form, not AdamW), applied to that gradient
    p = p0.double().cpu().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=ob.f32(eng.lr), betas=(ob.f32(eng.betas[0]), ob.f32(eng.betas[1])), eps=ob.f32(eng.eps), weight_decay=ob.f32(wd))
    p.grad = grad.double().cpu()
    opt.step()
    assert torch.allclose(p.detach(), want['p'][0], rtol=1e-12, atol=1e-15)
    ob.check_dict('adam weight_decay step', {'p': eng.P, 'm': eng.M, 'v': eng.V}, want, family='class_norm adam weight_decay')
    # ... and it is not the step without decay
    nod = ob.adam(p0, grad, torch.zeros_like(p0), torch.zeros_like(p0), eng.lr, eng.betas[0], eng.betas[1], eng.eps, 0.0, 1, 1.0)
    with pytest.raises(AssertionError):
        ob.check_dict('adam without decay', {'p': eng.P}, nod)
    eng.close()


# ====================================================================================================== the command line
def _cli(argv):
    from ifcb_classifier_amd import neuston_net as nn_
    args = nn_.argparse_nn().parse_args(argv)
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    return args


def test_train_class_norm_weight_decay_then_run(tmp_path, capsys):
    from PIL import Image
    from ifcb_classifier_amd import neuston_net as nn_
    src = str(tmp_path / 'training-data')
    rng = np.random.default_rng(7)
    for cls, mean, n in (('big', 90, 40), ('mid', 130, 8), ('small', 170, 3)):
        os.makedirs(os.path.join(src, cls))
        for i in range(n):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(src, cls, 'roi_%s_%03d.png' % (cls, i)))
    outdir = str(tmp_path / 'training-output' / 'cn')
    _cli(['--batch', '16', '--loaders', '0', 'TRAIN', src, 'resnet18', 'cn', '--untrain', '--seed', '1', '--emax', '1', '--emin', '1',
          '--estop', '0', '--outdir', outdir, '--class-norm', '--weight-decay', '1e-4'])
    out = capsys.readouterr().out
    assert 'Class-norm POWER 1' in out and '(small)' in out and '(big)' in out
    train = open(os.path.join(outdir, 'training_images.list')).read().splitlines()
    classes = ['big', 'mid', 'small']
    counts = [sum(1 for p in train if os.path.basename(os.path.dirname(p)) == c) for c in classes]
    assert sum(counts) == len(train) and counts[0] > counts[1] > counts[2] > 0
    want = nn_.class_norm_weights(counts, 1.0)
    import yaml
    y = yaml.safe_load(open(os.path.join(outdir, 'args.yml')))
    assert y['class_norm'] == 1.0 and y['weight_decay'] == 1e-4 and y['classes'] == classes
    assert y['class_weights'] == want and want[2] > want[1] > want[0]
    ck = torch.load(os.path.join(outdir, 'cn.ptl'), map_location='cpu', weights_only=False)
    hp = ck['hyper_parameters']
    assert hp['class_norm'] == 1.0 and hp['class_weights'] == want and hp['weight_decay'] == 1e-4
    assert ck['optimizer_states'][0]['param_groups'][0]['weight_decay'] == 1e-4
    assert ck['state_dict']['criterion.weight'].tolist() == want
    rows = open(os.path.join(outdir, 'epochs.csv')).read().strip().splitlines()
    assert rows[0].split(',')[:4] == ['epoch', 'best', 'train_loss', 'val_loss'] and len(rows) == 2
    assert all(np.isfinite(float(v)) for v in rows[1].split(',')[2:4])
    # RUN of that checkpoint: the usual shape
    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '16', '--loaders', '0', 'RUN', src, os.path.join(outdir, 'cn.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'cn', 'img_results.json')))
    scores = np.array(rj['output_scores'])
    assert rj['model_id'] == 'cn' and rj['class_labels'] == classes and scores.shape == (51, 3)
    assert np.allclose(scores.sum(1), 1, atol=1e-4) and (np.array(rj['output_classes']) == scores.argmax(1)).all()
