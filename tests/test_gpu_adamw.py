"""ifcbk_adamw_flat (adam_kernel<true> of csrc/pool_head.hip) on the device against the float64 twin and bound of tests/sched_cases.py,
and its bit-equalities: weight_decay = 0 is ifcbk_adam_clip_flat, the op with decoupled = 0 is the op as it was, the op with
decoupled = 1 is the typed call, nothing at or behind n is written, and a refused call launches nothing.

Sizes: 1 and 3 (scalar tail only), 4 (one 16-byte access), 5 (one access and a tail), 1023 / 1024 / 1025 (one block of 256 threads x 4
elements: its last thread on the tail, exactly full, a second block of one tail element), 4099 (several blocks and a tail)."""
import ctypes as C

import pytest
import torch

import clip_cases as cc
import ema_bounds as eb
import op_bounds as ob
import sched_cases as sc

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 5, 1023, 1024, 1025, 4099)
CANARY, NCAN = 0x7fc0dead, 9           # a NaN with a payload: any write behind element n changes these bits
ARGS = (1e-3, 0.9, 0.999, 1e-8)
WD = 0.05


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def P(t):
    return _lib().ptr(t)


def st():
    return _lib().cur_stream()


def _dev(t):
    can = torch.full((NCAN,), CANARY, dtype=torch.int32).view(torch.float32)
    return torch.cat([t.float(), can]).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
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
    e = p + torch.randn(n, generator=g) * 10 ** (torch.rand(n, generator=g) * 6 - 6)
    return p, gr, m, v, e


def _clip_state(lib):
    return torch.zeros(int(lib.ifcbk_grad_clip_state_floats()), dtype=torch.float32).cuda()


def _call(ctx, fn, bufs, n, wd, step, gs, ema_w, max_norm, cs):
    ctx.call(fn, P(bufs[0]), P(bufs[1]), P(bufs[2]), P(bufs[3]), P(bufs[4]) if len(bufs) > 4 else None, n, *ARGS, wd, step, gs, ema_w,
             max_norm, None if cs is None else P(cs), st())


@pytest.mark.parametrize('clip', (False, True))
@pytest.mark.parametrize('ema', (False, True))
@pytest.mark.parametrize('gs', (1.0, 0.5))
@pytest.mark.parametrize('step', (1, 1000))
@pytest.mark.parametrize('n', NS)
def test_adamw_flat_against_the_twin(ctx, n, step, gs, ema, clip):
    p, gr, m, v, e = _state(n, 31 * n + step)
    host = (p, gr, m, v) + ((e,) if ema else ())
    w = 0.25 if ema else 0.0
    # a bound at half the norm of gs * g, so that the coefficient is about 1/2: clipping must scale the gradient and leave the decay alone
    mx = float(torch.tensor(0.5 * gs * float(gr.double().norm()), dtype=torch.float32)) if clip else 0.0
    if clip and mx == 0.0:
        mx = 1.0                                                              # (n = 1 with a zero gradient: nothing to clip)
    dev = [_dev(t) for t in host]
    cs = _clip_state(ctx.lib) if clip else None
    _call(ctx, 'ifcbk_adamw_flat', dev, n, WD, step, gs, w, mx, cs)
    torch.cuda.synchronize()
    for t in dev:
        assert _canary_ok(t, n)                                               # nothing at or behind n is written
    assert _same(dev[1][:n], gr)
    coef = 1.0
    if clip:
        coef = float(cs[1])
        assert cc.f32_bits(coef) == cc.f32_bits(cc.host_coef(cs[0].cpu().numpy(), mx))
        assert coef < 0.75 or float(gr.abs().max()) == 0.0
    # the twin from the gradient scale the kernel formed: fl(gs * coef), one fp32 product
    scale = float(torch.tensor(gs, dtype=torch.float32) * torch.tensor(coef, dtype=torch.float32))
    want = sc.adamw(p, gr, m, v, *ARGS, WD, step, scale)
    worst = ob.check_dict('adamw n=%d step=%d gs=%g ema=%d clip=%d' % (n, step, gs, ema, clip),
                          {'p': dev[0][:n], 'm': dev[2][:n], 'v': dev[3][:n]}, want, family='adamw')
    assert worst < 1.0
    if ema:
        eb.check('adamw E n=%d' % n, dev[4][:n].cpu(), e, dev[0][:n].cpu(), eb.f32(w))        # the average of the FINAL p
    # and it is not the L2 form: the decay shows in p, never in the moments
    l2 = [_dev(t) for t in host]
    cs2 = _clip_state(ctx.lib) if clip else None
    _call(ctx, 'ifcbk_adam_clip_flat', l2, n, 0.0, step, gs, w, mx, cs2)
    torch.cuda.synchronize()
    assert _same(l2[2], dev[2]) and _same(l2[3], dev[3])
    assert n < 100 or not _same(l2[0], dev[0])
    # weight_decay = 0 is ifcbk_adam_clip_flat, bit for bit (canaries included)
    w0 = [_dev(t) for t in host]
    cs3 = _clip_state(ctx.lib) if clip else None
    _call(ctx, 'ifcbk_adamw_flat', w0, n, 0.0, step, gs, w, mx, cs3)
    torch.cuda.synchronize()
    for a, b in zip(w0, l2):
        assert _same(a, b)
    if clip:
        assert _same(cs3, cs2) and _same(cs[:2], cs2[:2])


def _op(lib, bufs, n, step, wd, gs, w, decoupled, cs=None, mx=0.0):
    o = lib.Op()
    o.kind = lib.OP_ADAM
    for k, t in enumerate(bufs):
        o.p[k] = t.data_ptr()
    if cs is not None:
        o.p[5] = cs.data_ptr()
    o.i[0], o.i[1], o.i[2] = n, step, decoupled
    for k, f in enumerate(ARGS + (wd, gs, w, mx)):
        o.f[k] = f
    return o


@pytest.mark.parametrize('n', (5, 1025, 4099))
def test_the_op_form(ctx, n):
    lib = _lib()
    p, gr, m, v, e = _state(n, 3 * n)
    step, gs, w = 4, 0.5, 0.25
    mx = float(torch.tensor(0.25 * float(gr.double().norm()), dtype=torch.float32))
    for with_e, clip in ((True, False), (False, True), (True, True), (False, False)):
        host = (p, gr, m, v) + ((e,) if with_e else ())
        ww = w if with_e else 0.0
        # decoupled = 1 through ifcbk_run_program equals the typed call
        typed, viaop = [_dev(t) for t in host], [_dev(t) for t in host]
        cs_t, cs_o = (_clip_state(ctx.lib), _clip_state(ctx.lib)) if clip else (None, None)
        _call(ctx, 'ifcbk_adamw_flat', typed, n, WD, step, gs, ww, mx, cs_t)
        ctx.run_program((lib.Op * 1)(_op(lib, viaop, n, step, WD, gs, ww, 1, cs_o, mx)), 1, st())
        # decoupled = 0 equals today's op: ifcbk_adam_clip_flat with the same operands, the L2 form
        old, zero = [_dev(t) for t in host], [_dev(t) for t in host]
        cs_a, cs_z = (_clip_state(ctx.lib), _clip_state(ctx.lib)) if clip else (None, None)
        _call(ctx, 'ifcbk_adam_clip_flat', old, n, WD, step, gs, ww, mx, cs_a)
        ctx.run_program((lib.Op * 1)(_op(lib, zero, n, step, WD, gs, ww, 0, cs_z, mx)), 1, st())
        torch.cuda.synchronize()
        for a, b in zip(typed, viaop):
            assert _same(a, b)
        for a, b in zip(old, zero):
            assert _same(a, b)
        assert not _same(typed[0][:n], old[0][:n]) and not _same(typed[2][:n], old[2][:n])      # two different updates
        if clip:
            assert _same(cs_t, cs_o) and _same(cs_a, cs_z) and _same(cs_t[:2], cs_a[:2])
    # the names and the cost the library reports for the two forms
    buf = C.create_string_buffer(64)
    o1, o0 = _op(lib, viaop, n, step, WD, gs, 0.0, 1), _op(lib, viaop, n, step, WD, gs, 0.0, 0)
    assert ctx.lib.ifcbk_op_kernel(C.byref(o1), buf, 64) == 0 and buf.value == b'adam_kernel<true>'
    assert ctx.lib.ifcbk_op_kernel(C.byref(o0), buf, 64) == 0 and buf.value == b'adam_kernel'


def test_bad_arguments_are_refused_before_anything_is_launched(ctx):
    lib = _lib()
    t = [_dev(torch.ones(8)) for _ in range(5)]
    cs = _clip_state(ctx.lib)
    f = ctx.lib.ifcbk_adamw_flat
    ptrs = [P(x) for x in t]
    for wd in (-0.01, float('nan'), float('inf'), -float('inf')):
        assert f(ctx.h, *ptrs, 8, *ARGS, wd, 1, 1.0, 0.5, 1.0, P(cs), st()) == lib.EINVAL
    assert b'weight_decay' in ctx.lib.ifcbk_last_error(ctx.h)
    for step in (0, -3):
        assert f(ctx.h, *ptrs, 8, *ARGS, WD, step, 1.0, 0.5, 1.0, P(cs), st()) == lib.EINVAL
        assert f(ctx.h, *ptrs, 8, *ARGS, 0.0, step, 1.0, 0.5, 1.0, P(cs), st()) == lib.EINVAL      # (the weight_decay = 0 route alike)
    for w in (-0.1, 1.5, float('nan')):
        assert f(ctx.h, *ptrs, 8, *ARGS, WD, 1, 1.0, w, 1.0, P(cs), st()) == lib.EINVAL
    assert f(ctx.h, *ptrs[:4], C.c_void_p(t[4].data_ptr() + 4), 4, *ARGS, WD, 1, 1.0, 0.5, 1.0, P(cs), st()) == lib.EINVAL      # aligned unlike p
    for mx in (0.0, -1.0, float('nan')):                                      # ifcbk_grad_norm's own refusal, ahead of the update
        assert f(ctx.h, *ptrs, 8, *ARGS, WD, 1, 1.0, 0.5, mx, P(cs), st()) == lib.EINVAL
    # the op form refuses alike
    o = _op(lib, t, 8, 1, -1.0, 1.0, 0.5, 1)
    with pytest.raises(RuntimeError):
        ctx.run_program((lib.Op * 1)(o), 1, st())
    torch.cuda.synchronize()
    for x in t:
        assert _same(x[:8], torch.ones(8)) and _canary_ok(x, 8)
    assert bool((cs == 0).all())
