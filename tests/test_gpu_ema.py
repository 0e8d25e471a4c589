"""The weight average in the optimizer kernels (ifcbk_adam_ema_flat, ifcbk_sgd_ema_flat: adam_kernel / sgd_kernel of csrc/pool_head.hip
with their `ema` operand), the plain update (ifcbk_ema_flat, csrc/ema.hip) and the op form (IFCBK_OP_ADAM p[4] / f[6], IFCBK_OP_SGD
p[3] / f[4]) against the float64 oracle and bound of tests/ema_bounds.py.

Sizes: those of test_gpu_op_bounds.ADAM that reach every path of the kernels -- 1 and 3 (scalar tail only), 4 (one 16-byte access),
5 (one access and a tail), 100003 (many blocks and a tail) -- crossed with the weights 0 (no update), 1e-4 (a late-training decay),
0.5 and 1 (the average becomes p), and with weight decay on and off."""
import ctypes as C

import pytest
import torch

import ema_bounds as eb

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 5, 100003)
WS = (0.0, 1e-4, 0.5, 1.0)
WDS = (0.0, 0.01)
CANARY = 0x7fc0dead                    # a NaN with a payload: any write behind element n changes these bits
NCAN = 9


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def P(t):
    return _lib().ptr(t)


def st():
    return _lib().cur_stream()


def _dev(t):
    """a device buffer of its own (so 16-byte aligned) holding t and a canary region behind it"""
    can = torch.full((NCAN,), CANARY, dtype=torch.int32).view(torch.float32)
    return torch.cat([t.float(), can]).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _canary_ok(t, n):
    return bool((_bits(t)[n:] == CANARY).all()) and t.numel() == n + NCAN


def _state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 10 ** (torch.rand(n, generator=g) * 6 - 4)
    gr[::7] = 0.0
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01
    e = p + torch.randn(n, generator=g) * 10 ** (torch.rand(n, generator=g) * 6 - 6)        # an average 1e-6 .. 1 away from p
    e[::5] = p[::5]                          # already at p
    e[3::11] = -0.0                          # a signed zero keeps its sign when nothing is applied
    e[1::13] *= 300.0                        # and far from it
    return p, gr, m, v, e


ADAM_ARGS = (1e-3, 0.9, 0.999, 1e-8)


@pytest.mark.parametrize('wd', WDS)
@pytest.mark.parametrize('w', WS)
@pytest.mark.parametrize('n', NS)
def test_adam_ema_flat(ctx, n, w, wd):
    p, gr, m, v, e = _state(n, n + int(w * 1e4))
    step, gs = 3, 1 / 128
    old = [_dev(t) for t in (p, gr, m, v)]
    new = [_dev(t) for t in (p, gr, m, v, e)]
    nul = [_dev(t) for t in (p, gr, m, v)]
    ctx.call('ifcbk_adam_flat', P(old[0]), P(old[1]), P(old[2]), P(old[3]), n, *ADAM_ARGS, wd, step, gs, st())
    ctx.call('ifcbk_adam_ema_flat', P(new[0]), P(new[1]), P(new[2]), P(new[3]), P(new[4]), n, *ADAM_ARGS, wd, step, gs, w, st())
    ctx.call('ifcbk_adam_ema_flat', P(nul[0]), P(nul[1]), P(nul[2]), P(nul[3]), None, n, *ADAM_ARGS, wd, step, gs, w, st())
    torch.cuda.synchronize()
    for k, name in enumerate(('p', 'g', 'm', 'v')):
        assert _same_bits(new[k], old[k]), '%s differs from ifcbk_adam_flat' % name          # (canary included)
        assert _same_bits(nul[k], old[k]), '%s with ema = NULL differs from ifcbk_adam_flat' % name
    for t in old + new + nul:
        assert _canary_ok(t, n)
    assert (n < 100 or not _same_bits(old[0][:n], p)) and torch.isfinite(new[0][:n]).all()
    if w == 0.0:
        assert _same_bits(new[4][:n], e)
    else:
        eb.check('adam_ema n=%d w=%g wd=%g' % (n, w, wd), new[4][:n].cpu(), e, new[0][:n].cpu(), eb.f32(w))
        assert n < 100 or not _same_bits(new[4][:n], e)          # (a single element may sit at p already)


@pytest.mark.parametrize('mu', (0.0, 0.9))
@pytest.mark.parametrize('wd', WDS)
@pytest.mark.parametrize('w', WS)
@pytest.mark.parametrize('n', NS)
def test_sgd_ema_flat(ctx, n, w, wd, mu):
    p, gr, mom, _v, e = _state(n, 7 * n + int(w * 1e4))
    lr, gs = 0.05, 1 / 128
    old = [_dev(t) for t in (p, gr, mom)]
    new = [_dev(t) for t in (p, gr, mom, e)]
    nul = [_dev(t) for t in (p, gr, mom)]
    ctx.call('ifcbk_sgd_flat', P(old[0]), P(old[1]), P(old[2]) if mu else None, n, lr, mu, wd, gs, st())
    ctx.call('ifcbk_sgd_ema_flat', P(new[0]), P(new[1]), P(new[2]) if mu else None, P(new[3]), n, lr, mu, wd, gs, w, st())
    ctx.call('ifcbk_sgd_ema_flat', P(nul[0]), P(nul[1]), P(nul[2]) if mu else None, None, n, lr, mu, wd, gs, w, st())
    torch.cuda.synchronize()
    for k, name in enumerate(('p', 'g', 'mom')):
        assert _same_bits(new[k], old[k]), '%s differs from ifcbk_sgd_flat' % name
        assert _same_bits(nul[k], old[k]), '%s with ema = NULL differs from ifcbk_sgd_flat' % name
    if not mu:
        assert _same_bits(new[2][:n], mom)
    for t in old + new + nul:
        assert _canary_ok(t, n)
    assert torch.isfinite(new[0][:n]).all()
    if w == 0.0:
        assert _same_bits(new[3][:n], e)
    else:
        eb.check('sgd_ema n=%d w=%g wd=%g mu=%g' % (n, w, wd, mu), new[3][:n].cpu(), e, new[0][:n].cpu(), eb.f32(w))
        assert n < 100 or not _same_bits(new[3][:n], e)


@pytest.mark.parametrize('w', WS)
@pytest.mark.parametrize('n', NS)
def test_ema_flat(ctx, n, w):
    x, _g, _m, _v, e = _state(n, 13 * n + int(w * 1e4))
    de, dx = _dev(e), _dev(x)
    ctx.call('ifcbk_ema_flat', P(de), P(dx), n, w, st())
    torch.cuda.synchronize()
    assert _canary_ok(de, n) and _canary_ok(dx, n) and _same_bits(dx[:n], x)
    if w == 0.0:
        assert _same_bits(de[:n], e)
    else:
        eb.check('ema_flat n=%d w=%g' % (n, w), de[:n].cpu(), e, x, eb.f32(w))
        assert n < 100 or not _same_bits(de[:n], e)
    # x == e is a fixed point, exactly
    de2 = _dev(x)
    ctx.call('ifcbk_ema_flat', P(de2), P(dx), n, w, st())
    torch.cuda.synchronize()
    assert _same_bits(de2[:n], x)


def test_bad_arguments_are_refused_before_anything_is_launched(ctx):
    lib = _lib()
    t = [_dev(torch.ones(8)) for _ in range(5)]
    for w in (-0.1, 1.5, float('nan')):
        assert ctx.lib.ifcbk_ema_flat(ctx.h, P(t[0]), P(t[1]), 8, w, st()) == lib.EINVAL
        assert ctx.lib.ifcbk_adam_ema_flat(ctx.h, P(t[0]), P(t[1]), P(t[2]), P(t[3]), P(t[4]), 8, *ADAM_ARGS, 0.0, 1, 1.0, w, st()) == lib.EINVAL
        assert ctx.lib.ifcbk_sgd_ema_flat(ctx.h, P(t[0]), P(t[1]), P(t[2]), P(t[4]), 8, 0.05, 0.9, 0.0, 1.0, w, st()) == lib.EINVAL
    assert ctx.lib.ifcbk_ema_flat(ctx.h, None, P(t[1]), 8, 0.5, st()) == lib.EINVAL
    assert ctx.lib.ifcbk_ema_flat(ctx.h, P(t[0]), P(t[1]), -1, 0.5, st()) == lib.EINVAL
    assert ctx.lib.ifcbk_ema_flat(ctx.h, C.c_void_p(t[0].data_ptr() + 4), P(t[1]), 4, 0.5, st()) == lib.EINVAL            # not 16-byte aligned
    assert ctx.lib.ifcbk_adam_ema_flat(ctx.h, P(t[0]), P(t[1]), P(t[2]), P(t[3]), C.c_void_p(t[4].data_ptr() + 4), 4, *ADAM_ARGS, 0.0, 1, 1.0, 0.5,
                                       st()) == lib.EINVAL                                                               # aligned unlike p
    assert ctx.lib.ifcbk_ema_flat(ctx.h, P(t[0]), P(t[1]), 0, 0.5, st()) == 0
    torch.cuda.synchronize()
    for x in t:
        assert _same_bits(x[:8], torch.ones(8)) and _canary_ok(x, 8)


@pytest.mark.parametrize('w', (0.0, 1e-4, 1.0))
@pytest.mark.parametrize('n', (5, 100003))
def test_the_op_form_equals_the_typed_calls(ctx, n, w):
    lib = _lib()
    p, gr, m, v, e = _state(n, 3 * n)
    step, gs, wd = 4, 0.5, 0.01
    # Adam: p[4] = the average, f[6] = its weight
    typed = [_dev(t) for t in (p, gr, m, v, e)]
    viaop = [_dev(t) for t in (p, gr, m, v, e)]
    ctx.call('ifcbk_adam_ema_flat', P(typed[0]), P(typed[1]), P(typed[2]), P(typed[3]), P(typed[4]), n, *ADAM_ARGS, wd, step, gs, w, st())
    o = lib.Op()
    o.kind = lib.OP_ADAM
    for k in range(5):
        o.p[k] = viaop[k].data_ptr()
    o.i[0], o.i[1] = n, step
    for k, f in enumerate(ADAM_ARGS + (wd, gs, w)):
        o.f[k] = f
    ctx.run_program((lib.Op * 1)(o), 1, st())
    torch.cuda.synchronize()
    for a, b in zip(typed, viaop):
        assert _same_bits(a, b)
    # ... and without the operand the op is the plain step
    plain = [_dev(t) for t in (p, gr, m, v)]
    o.p[4] = None
    for k in range(4):
        o.p[k] = plain[k].data_ptr()
    ctx.run_program((lib.Op * 1)(o), 1, st())
    torch.cuda.synchronize()
    for a, b in zip(typed[:4], plain):
        assert _same_bits(a, b)
    # SGD: p[3] and f[4]
    for mu in (0.0, 0.9):
        typed = [_dev(t) for t in (p, gr, m, e)]
        viaop = [_dev(t) for t in (p, gr, m, e)]
        ctx.call('ifcbk_sgd_ema_flat', P(typed[0]), P(typed[1]), P(typed[2]) if mu else None, P(typed[3]), n, 0.05, mu, wd, gs, w, st())
        o = lib.Op()
        o.kind = lib.OP_SGD
        for k in (0, 1, 3):
            o.p[k] = viaop[k].data_ptr()
        o.p[2] = viaop[2].data_ptr() if mu else None
        o.i[0], o.i[1] = n, 1
        for k, f in enumerate((0.05, mu, wd, gs, w)):
            o.f[k] = f
        ctx.run_program((lib.Op * 1)(o), 1, st())
        torch.cuda.synchronize()
        for a, b in zip(typed, viaop):
            assert _same_bits(a, b)
        if w:
            assert n < 100 or not _same_bits(viaop[3][:n], e)
