"""TRAIN --distill on the GPU: the distillation loss kernel (ifcbk_softmax_xent_distill, csrc/loss.hip) against tests/distill_cases.py at
every shape and case of its lists, its ABI (guard words, refusals, run-to-run bits), alpha == 1 against the target, alpha == 0 against
the teacher and the smoothed hard loss's reference, and the op dispatch on p[6], plain and through a captured graph."""
import pytest
import torch

import distill_cases as dc
import loss_smooth_bounds as sb

pytestmark = pytest.mark.gpu
GUARD = -12345.0
G = 64                           # guard words on either side of dlogits
FN = 'ifcbk_softmax_xent_distill'


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def P(t):
    return _lib().ptr(t)


def st():
    return _lib().cur_stream()


def _call(ctx, ld, td, zd, cwd, N, NC, scale, eps, alpha, T, acc, with_dl, old=dc.OLD_LOSS):
    """-> (loss [1], dlogits [N, NC] or None); the words around both are checked"""
    lbuf = torch.full((3,), GUARD, device='cuda')
    if acc:
        lbuf[1] = old
    dbuf = torch.full((2 * G + N * NC,), GUARD, device='cuda') if with_dl else None
    ctx.call(FN, P(ld), P(td), P(zd), P(cwd), N, NC, scale, eps, alpha, T, P(lbuf[1:]), acc, P(dbuf[G:]) if with_dl else None, st())
    torch.cuda.synchronize()
    assert float(lbuf[0]) == GUARD and float(lbuf[2]) == GUARD
    if with_dl:
        assert bool((dbuf[:G] == GUARD).all()) and bool((dbuf[G + N * NC:] == GUARD).all())
        return lbuf[1:2].clone(), dbuf[G:G + N * NC].reshape(N, NC).clone()
    return lbuf[1:2].clone(), None


def _dev(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


@pytest.mark.parametrize('N,NC', dc.SHAPES)
def test_softmax_xent_distill(ctx, N, NC):
    worst = 0.0
    fam = 'softmax_xent_distill'
    for case in dc.CASES:
        alpha, T, eps, scale, wm, offset, acc, with_dl = case
        l, t, z, cw = dc.inputs(N, NC, wm, offset)
        ld, td, zd, cwd = _dev(l, t, z, cw)
        loss, dl = _call(ctx, ld, td, zd, cwd, N, NC, scale, eps, alpha, T, acc, with_dl)
        got = {'loss': loss, 'dlogits': dl} if with_dl else {'loss': loss}
        if wm == 'zero' and NC == 1:
            assert all(bool(torch.isnan(v).all()) for v in got.values())          # the only class weighs nothing: 0 / 0, as in torch
            continue
        want = dc.bounds(l, t, z, cw, scale, eps, alpha, T, old_loss=dc.OLD_LOSS if acc else None)
        worst = max(worst, dc.check(dc.case_name(N, NC, case), got, want, family=fam))
        loss2, dl2 = _call(ctx, ld, td, zd, cwd, N, NC, scale, eps, alpha, T, acc, with_dl)          # run to run
        assert torch.equal(loss, loss2) and (not with_dl or torch.equal(dl, dl2))
    print('%s (%d, %d): worst err/bound %.3f' % (fam, N, NC, worst))


@pytest.mark.parametrize('N,NC', [(3, 5), (257, 101)])
def test_alpha_1_does_not_read_the_target_and_alpha_0_not_the_teacher(ctx, N, NC):
    l, t, z, _ = dc.inputs(N, NC, 'none')
    z2 = dc.inputs(N, NC, 'none', seed=1)[2]
    assert not torch.equal(z, z2)
    t2 = (t + 1) % NC
    ld, td, t2d, zd, z2d = _dev(l, t, t2, z, z2)
    # alpha == 1, no class weights: the hard term is multiplied by an exact 0
    a = _call(ctx, ld, td, zd, None, N, NC, 0.4, 0.1, 1.0, 4.0, 0, 1)
    b = _call(ctx, ld, t2d, zd, None, N, NC, 0.4, 0.1, 1.0, 4.0, 0, 1)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    # alpha == 0: the soft terms are multiplied by exact zeros, and the function is the smoothed hard loss's
    for wm in ('none', 'random'):
        cw = dc.inputs(N, NC, wm)[3]
        cwd = None if cw is None else cw.cuda()
        a = _call(ctx, ld, td, zd, cwd, N, NC, 0.4, 0.1, 0.0, 4.0, 0, 1)
        b = _call(ctx, ld, td, z2d, cwd, N, NC, 0.4, 0.1, 0.0, 4.0, 0, 1)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        dc.check('alpha 0 vs distill bound', {'loss': a[0], 'dlogits': a[1]}, dc.bounds(l, t, z, cw, 0.4, 0.1, 0.0, 4.0))
        # ... within loss_smooth_bounds' own bound: at alpha == 0 the kernel runs softmax_xent_ls_kernel's operations, then * 1 and + 0
        sb.check('alpha 0 vs xent_ls', {'loss': a[0], 'dlogits': a[1]}, sb.xent_ls(l, t, cw, 0.4, 0.1))


def test_underflowed_q_adds_nothing_and_leaves_r_in_dlogits(ctx):
    N, NC, T = 3, 5, 0.5
    l, t, z, _ = dc.inputs(N, NC, 'none', True)
    ld, td, zd = _dev(l, t, z)
    loss, dl = _call(ctx, ld, td, zd, None, N, NC, 1.0, 0.0, 1.0, T, 0, 1)
    row = (N // 2 + 1) % N
    q = torch.softmax(z / T, 1)
    zero = q[row] == 0
    assert int(zero.sum()) == NC - 1 and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dl).all())
    r = torch.softmax(l.double() / T, 1)
    assert torch.allclose(dl[row].cpu().double()[zero], (T / N * r[row])[zero], rtol=1e-5, atol=0)


def test_refusals_launch_nothing(ctx):
    N, NC = 7, 5
    l, t, z, cw = dc.inputs(N, NC, 'random')
    ld, td, zd, cwd = _dev(l, t, z, cw)
    loss = torch.full((1,), GUARD, device='cuda')
    dl = torch.full((N, NC), GUARD, device='cuda')
    ok = (P(ld), P(td), P(zd), P(cwd), N, NC, 1.0, 0.1, 0.3, 4.0, P(loss), 0, P(dl), st())

    def refused(**kw):
        names = ('logits', 'target', 'teacher', 'cw', 'N', 'NC', 'weight', 'eps', 'alpha', 'T', 'loss', 'acc', 'dl', 'stream')
        args = [kw.get(k, v) for k, v in zip(names, ok)]
        with pytest.raises(RuntimeError, match=r'ifcbk_softmax_xent_distill failed \(-1\)'):
            ctx.call(FN, *args)
    for k in ('logits', 'target', 'teacher', 'loss'):
        refused(**{k: None})
    for k in ('N', 'NC'):
        refused(**{k: 0})
        refused(**{k: -1})
    for a in (-0.1, 1.5, float('nan'), float('inf')):
        refused(alpha=a)
    for T in (0.0, -1.0, float('inf'), float('-inf'), float('nan')):
        refused(T=T)
    for e in (-0.1, 1.5, float('nan'), float('inf')):
        refused(eps=e)
    torch.cuda.synchronize()
    assert float(loss) == GUARD and bool((dl == GUARD).all())
    ctx.call(FN, *ok)
    torch.cuda.synchronize()
    dc.check('after the refusals', {'loss': loss, 'dlogits': dl}, dc.bounds(l, t, z, cw, 1.0, 0.1, 0.3, 4.0))


@pytest.mark.parametrize('weights', ['none', 'random'])
def test_op_dispatch_on_p6(ctx, weights):
    """a one-op program of either kind: p[6] = the teacher's logits runs the distillation kernel with the op's operands, f[1] as eps,
    f[3] as alpha and f[4] as the temperature -- the bits of the direct call, also from a captured graph; p[6] with f[2] or with p[5] is
    refused, nothing written; p[6] NULL is the dispatch without a teacher"""
    from ifcb_classifier_amd.engine import OpList, Program
    lib = _lib()
    N, NC = 7, 5
    l, t, z, cw = dc.inputs(N, NC, weights)
    ld, td, zd, cwd = _dev(l, t, z, cw)
    lam = torch.ones(N, device='cuda')
    loss = torch.full((1,), GUARD, device='cuda')
    dl = torch.full((N, NC), GUARD, device='cuda')
    kind, c4 = (lib.OP_SOFTMAX_XENT, None) if cw is None else (lib.OP_SOFTMAX_XENT_W, P(cwd))

    def prog(f, teacher=True, mix=False):
        ops = OpList()
        ops.add(kind, 'loss', p=(P(ld), P(td), P(loss), P(dl), c4, P(lam) if mix else None, P(zd) if teacher else None), i=(N, NC), f=f)
        return Program(ops)
    for bad, what in ((prog((1.0, 0.0, 2.0, 0.3, 4.0)), r'p\[6\].*f\[2\]'), (prog((1.0, 0.1, 0.0, 0.3, 4.0), mix=True), r'p\[6\].*p\[5\]')):
        with pytest.raises(RuntimeError, match=r'\(-1\).*' + what):               # (-1: IFCBK_EINVAL)
            ctx.run_program(bad.arr, bad.n, st())
        torch.cuda.synchronize()
        assert float(loss) == GUARD and bool((dl == GUARD).all())
    for eps in (0.0, 0.1):
        good = prog((0.4, eps, 0.0, 0.3, 4.0))
        ctx.run_program(good.arr, good.n, st())
        torch.cuda.synchronize()
        dc.check('op p[6], eps %g' % eps, {'loss': loss, 'dlogits': dl}, dc.bounds(l, t, z, cw, 0.4, eps, 0.3, 4.0))
        a, b = loss.clone(), dl.clone()
        loss.fill_(GUARD)
        dl.fill_(GUARD)
        ctx.call(FN, P(ld), P(td), P(zd), P(cwd), N, NC, 0.4, eps, 0.3, 4.0, P(loss), 0, P(dl), st())
        torch.cuda.synchronize()
        assert torch.equal(a, loss) and torch.equal(b, dl)
        # the same op from a captured graph, twice
        g = ctx.capture(good.arr, good.n)
        try:
            for _ in range(2):
                loss.fill_(GUARD)
                dl.fill_(GUARD)
                ctx.graph_launch(g, st())
                torch.cuda.synchronize()
                assert torch.equal(a, loss) and torch.equal(b, dl)
        finally:
            ctx.call('ifcbk_graph_destroy', g)
    plain = prog((1.0, 0.1), teacher=False)
    ctx.run_program(plain.arr, plain.n, st())
    torch.cuda.synchronize()
    sb.check('op without p[6]', {'loss': loss, 'dlogits': dl}, sb.xent_ls(l, t, cw, 1.0, 0.1))
