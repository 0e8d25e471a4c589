"""ifcbk_grad_norm (csrc/grad_clip.hip) and the clipped optimizer steps (ifcbk_adam_clip_flat / ifcbk_sgd_clip_flat, the op form p[5] /
f[7] of IFCBK_OP_ADAM and p[4] / f[5] of IFCBK_OP_SGD) on the device.

The norm is held to a float64 sum of squares of the same fp32 values within tests/clip_cases.py's bound, which is derived there from
the accumulation the kernel does: ((L + 6) / 2 + 2) * 2^-24 relative, L the float4s of the busiest thread, plus the absolute term of
squares below the fp32 normal range.  The coefficient is torch's formula applied in fp32 to the device's own norm, bit for bit.

Sizes: 0, 1, 3 (tail only), 4 (one float4), 5 (one and a tail), 1023 / 1024 (four blocks, with and without a tail), and from the
geometry the library reports: one float4 less than a pass of the whole grid, exactly a pass, a pass and one element (the second pass
holds only the tail), two passes and 7 (a third pass of one float4 and a tail of 3)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clip_cases as cc
import op_bounds as ob
import option_matrix as om

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7fc00001
SMALL_NS = (0, 1, 3, 4, 5, 1023, 1024)
ADAM_ARGS = (1e-3, 0.9, 0.999, 1e-8)


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def P(t):
    return _lib().ptr(t)


def st():
    return _lib().cur_stream()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _sizes():
    blocks, per_pass = cc.geometry(_lib().load())
    assert blocks >= 256 and per_pass == blocks * 1024
    return blocks, SMALL_NS + (per_pass - 4, per_pass, per_pass + 1, 2 * per_pass + 7)


def _state(lib):
    """a clip state whose every word is a NaN with a payload: a partial that was not written would reach the norm"""
    nf = int(lib.ifcbk_grad_clip_state_floats())
    return torch.full((nf,), NAN_BITS, dtype=torch.int32).view(torch.float32).cuda()


def _zero_figures(s):
    s[:4].zero_()


_INPUTS = {}


def _input(kind, n):
    """the n first elements of one seeded array per kind (made once, at the largest size)"""
    if kind not in _INPUTS:
        nmax = max(_sizes()[1])
        g = torch.Generator().manual_seed({'normal': 1, 'wide': 2, 'zeros': 3, 'huge': 4}[kind])
        if kind == 'normal':
            t = torch.randn(nmax, generator=g)
        elif kind == 'wide':            # magnitudes 2^-60 .. 2^40, either sign: the squares span 2^-120 .. 2^80, inside the normal range
            t = torch.randn(nmax, generator=g).sign() * torch.exp2(torch.rand(nmax, generator=g) * 100 - 60)
        elif kind == 'zeros':
            t = torch.zeros(nmax)
        else:                           # one element of 2^40 among tiny ones
            t = torch.randn(nmax, generator=g) * 1e-12
            t[0] = 2.0 ** 40
        _INPUTS[kind] = t.cuda()
    return _INPUTS[kind][:n]


def _norm_call(ctx, g, n, gs, mx, state):
    ctx.call('ifcbk_grad_norm', P(g) if g is not None else None, n, gs, mx, P(state), st())
    torch.cuda.synchronize()
    return state[:4].cpu()


@pytest.mark.parametrize('kind', ('normal', 'wide', 'zeros', 'huge'))
def test_norm_within_the_derived_bound_and_coef_is_torchs_formula_bit_for_bit(ctx, kind):
    lib = _lib()
    blocks, sizes = _sizes()
    for n in sizes:
        for gs, mx in ((1.0, 1.0), (0.5, 1e-3)):
            g = _input(kind, n) if n else torch.zeros(4).cuda()
            state = _state(lib.load())
            _zero_figures(state)
            s = _norm_call(ctx, g, n, gs, mx, state)
            ref = cc.ref_norm(g[:n].cpu(), gs) if n else 0.0
            bound = cc.norm_bound(n, blocks, ref, gs)
            norm, coef = float(s[0]), float(s[1])
            print('%s n=%d gs=%g: norm %.9g ref %.9g err %.3g bound %.3g' % (kind, n, gs, norm, ref, abs(norm - ref), bound))
            assert math.isfinite(norm) and abs(norm - ref) <= bound, (kind, n, gs, norm, ref, bound)
            assert cc.f32_bits(coef) == cc.f32_bits(cc.host_coef(s[0].numpy(), mx)), (kind, n, coef)
            if n == 0 or kind == 'zeros':
                assert norm == 0.0 and coef == 1.0
            assert float(s[2]) == norm and float(s[3]) == (1.0 if coef < 1.0 else 0.0)
            # the partials were all written: none keeps the NaN the buffer was filled with
            assert not torch.isnan(state[4:].view(torch.float64)).any()
    # torch itself, on the CPU, at one size of every path (float64 copies: the norm; fp32: the coefficient's effect)
    n = sizes[-1]
    g = _input(kind, n).cpu()
    total, _ = cc.torch_clip([g], 1.0, dtype=torch.float64)
    state = _state(lib.load())
    s = _norm_call(ctx, _input(kind, n), n, 1.0, 1.0, state)
    assert abs(float(s[0]) - total) <= cc.norm_bound(n, blocks, total)


def test_same_call_twice_gives_the_same_bits_and_the_figures_accumulate(ctx):
    lib = _lib()
    blocks, sizes = _sizes()
    n = sizes[-1]
    g = _input('normal', n)
    a, b = _state(lib.load()), _state(lib.load())
    _zero_figures(a)
    _zero_figures(b)
    sa = _norm_call(ctx, g, n, 1.0, 1.0, a)
    sb = _norm_call(ctx, g, n, 1.0, 1.0, b)
    assert _same(a, b) and _same(sa, sb)
    # three calls: a small gradient under the bound, the large one over it, the small one again
    small = _input('normal', 1024)
    s1 = _norm_call(ctx, small, 1024, 1.0, 100.0, a)
    assert float(s1[1]) == 1.0 and float(s1[2]) == float(sa[0]) and float(s1[3]) == 1.0           # max kept, nothing counted
    s2 = _norm_call(ctx, g, n, 2.0, 100.0, a)
    assert float(s2[1]) < 1.0 and float(s2[2]) == float(s2[0]) > float(sa[0]) and float(s2[3]) == 2.0
    s3 = _norm_call(ctx, small, 1024, 1.0, 1.0, a)
    assert float(s3[0]) == float(s1[0]) and float(s3[2]) == float(s2[0]) and float(s3[3]) == 3.0


def test_non_finite_gradients_are_not_special_cased(ctx):
    lib = _lib()
    n = 1027
    g = torch.randn(n, generator=torch.Generator().manual_seed(5))
    g[100] = float('inf')
    state = _state(lib.load())
    _zero_figures(state)
    s = _norm_call(ctx, g.cuda(), n, 1.0, 1.0, state)
    assert float(s[0]) == math.inf and float(s[1]) == 0.0
    # what torch does with the same input: the total norm is inf and every finite element is multiplied by 0
    total, clipped = cc.torch_clip([g], 1.0)
    assert total == math.inf and float(clipped[0][0]) == 0.0 == float(g[0]) * float(s[1])
    g[100] = float('nan')
    state = _state(lib.load())
    _zero_figures(state)
    s = _norm_call(ctx, g.cuda(), n, 1.0, 1.0, state)
    assert math.isnan(float(s[0])) and math.isnan(float(s[1]))
    total, clipped = cc.torch_clip([g], 1.0)
    assert math.isnan(total) and math.isnan(float(clipped[0][0]))
    assert float(s[2]) == 0.0 and float(s[3]) == 0.0             # a NaN norm neither becomes the maximum nor counts as clipped


def test_bad_arguments_are_refused_and_leave_the_state_alone(ctx):
    lib = _lib()
    g = torch.ones(64).cuda()
    state = _state(lib.load())
    before = _bits(state).clone()
    call = lambda gp, n, gs, mx, sp: ctx.lib.ifcbk_grad_norm(ctx.h, gp, n, gs, mx, sp, st())
    assert call(None, 8, 1.0, 1.0, P(state)) == lib.EINVAL
    assert call(P(g), 8, 1.0, 1.0, None) == lib.EINVAL
    assert call(C.c_void_p(g.data_ptr() + 4), 8, 1.0, 1.0, P(state)) == lib.EINVAL            # g not 16-byte aligned
    assert call(P(g), -1, 1.0, 1.0, P(state)) == lib.EINVAL
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert call(P(g), 8, 1.0, bad, P(state)) == lib.EINVAL, bad
        assert call(P(g), 8, bad, 1.0, P(state)) == lib.EINVAL, bad
        p = [torch.ones(8).cuda() for _ in range(4)]
        assert ctx.lib.ifcbk_adam_clip_flat(ctx.h, P(p[0]), P(g), P(p[1]), P(p[2]), None, 8, *ADAM_ARGS, 0.0, 1, 1.0, 0.0, bad, P(state),
                                            st()) == lib.EINVAL
        assert ctx.lib.ifcbk_sgd_clip_flat(ctx.h, P(p[0]), P(g), None, None, 8, 0.05, 0.0, 0.0, 1.0, 0.0, bad, P(state), st()) == lib.EINVAL
        torch.cuda.synchronize()
        assert all(_same(t, torch.ones(8)) for t in p)                                          # ... and no update ran either
    torch.cuda.synchronize()
    assert torch.equal(_bits(state), before)


def _opt_state(n, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    gr = torch.randn(n, generator=g) * 10 ** (torch.rand(n, generator=g) * 4 - 3)
    m = torch.randn(n, generator=g) * 0.1
    v = torch.rand(n, generator=g) * 0.01
    e = p + torch.randn(n, generator=g) * 1e-3
    return p, gr, m, v, e


def _adam(ctx, bufs, ema, n, wd, step, gs, w, mx=None, state=None):
    if state is None:
        ctx.call('ifcbk_adam_ema_flat', P(bufs[0]), P(bufs[1]), P(bufs[2]), P(bufs[3]), P(bufs[4]) if ema else None, n, *ADAM_ARGS, wd, step,
                 gs, w, st())
    else:
        ctx.call('ifcbk_adam_clip_flat', P(bufs[0]), P(bufs[1]), P(bufs[2]), P(bufs[3]), P(bufs[4]) if ema else None, n, *ADAM_ARGS, wd, step,
                 gs, w, mx, P(state), st())


def _sgd(ctx, bufs, ema, mu, n, wd, gs, w, mx=None, state=None):
    if state is None:
        ctx.call('ifcbk_sgd_ema_flat', P(bufs[0]), P(bufs[1]), P(bufs[2]) if mu else None, P(bufs[4]) if ema else None, n, 0.05, mu, wd, gs, w,
                 st())
    else:
        ctx.call('ifcbk_sgd_clip_flat', P(bufs[0]), P(bufs[1]), P(bufs[2]) if mu else None, P(bufs[4]) if ema else None, n, 0.05, mu, wd, gs, w,
                 mx, P(state), st())


@pytest.mark.parametrize('gs', (1.0, 0.5))
@pytest.mark.parametrize('ema', (False, True))
@pytest.mark.parametrize('n', (5, 1027))
def test_adam_clip_flat(ctx, n, ema, gs):
    lib = _lib()
    host = _opt_state(n, 11 * n)
    step, wd, w = 3, 0.01, 0.25
    dev = lambda: [t.clone().cuda() for t in host]
    # a bound nothing reaches: the bits of the plain entry point
    plain, loose = dev(), dev()
    state = _state(lib.load())
    _adam(ctx, plain, ema, n, wd, step, gs, w)
    _adam(ctx, loose, ema, n, wd, step, gs, w, 1e30, state)
    torch.cuda.synchronize()
    assert float(state[1]) == 1.0
    assert all(_same(a, b) for a, b in zip(plain, loose))
    # a bound below the norm: the plain entry point with grad_scale * coef formed in fp32 on the host
    true = cc.ref_norm(host[1], gs)
    mx = 0.3 * true
    tight, twin = dev(), dev()
    state = _state(lib.load())
    _adam(ctx, tight, ema, n, wd, step, gs, w, mx, state)
    torch.cuda.synchronize()
    coef = state[1].cpu().numpy()
    assert 0.29 < float(coef) < 0.31
    _adam(ctx, twin, ema, n, wd, step, float(np.float32(gs) * coef), w)
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(tight, twin))
    if not ema:
        assert _same(tight[4], host[4])
    # ... and torch: clip_grad_norm_, then torch.optim.Adam, within the optimizer bound of tests/op_bounds.py
    want, slack, p_torch = _torch_adam(host, n, gs, mx, wd, step)
    assert bool(((p_torch.double() - want['p'][0]).abs() <= want['p'][1]).all())
    ob.check_dict('adam_clip n=%d' % n, {'p': tight[0].cpu()}, {'p': (want['p'][0], want['p'][1] + slack)})


def _scale_delta(n):
    return om.scale_delta(n, cc.geometry(_lib().load())[0])


def _reference_gradient(host, gs, mx):
    return om.reference_gradient(host[1], gs, mx)


_sensitivity = om.sensitivity                          # (the three live in tests/option_matrix.py now, with their docstrings)


def _torch_adam(host, n, gs, mx, wd, step):
    gc = _reference_gradient(host, gs, mx)
    fn = lambda g_: ob.adam(host[0], g_, host[2], host[3], *ADAM_ARGS, wd, step, 1.0)
    want = fn(gc)
    slack = _sensitivity(fn, gc, _scale_delta(n))
    pt = torch.nn.Parameter(host[0].clone())
    pt.grad = gc.clone()
    opt = torch.optim.Adam([pt], lr=ADAM_ARGS[0], betas=ADAM_ARGS[1:3], eps=ADAM_ARGS[3], weight_decay=wd)
    opt.state[pt] = dict(step=torch.tensor(float(step - 1)), exp_avg=host[2].clone(), exp_avg_sq=host[3].clone())
    opt.step()
    return want, slack, pt.detach()


def _torch_sgd(host, n, gs, mx, wd, mu, lr):
    gc = _reference_gradient(host, gs, mx)
    fn = lambda g_: ob.sgd(host[0], g_, host[2] if mu else None, lr, mu, wd, 1.0)
    want = fn(gc)
    slack = _sensitivity(fn, gc, _scale_delta(n))
    pt = torch.nn.Parameter(host[0].clone())
    pt.grad = gc.clone()
    opt = torch.optim.SGD([pt], lr=lr, momentum=mu, weight_decay=wd)
    if mu:
        opt.state[pt] = dict(momentum_buffer=host[2].clone())
    opt.step()
    return want, slack, pt.detach()


def test_the_reference_chain_on_the_cpu_is_inside_its_own_bound():
    """torch.optim behind clip_grad_norm_ against the float64 oracle, without the device: what the device tests compare with"""
    for n in (5, 1027):
        for gs in (1.0, 0.5):
            host = _opt_state(n, 11 * n)
            mx = 0.3 * cc.ref_norm(host[1], gs)
            want, slack, pt = _torch_adam(host, n, gs, mx, 0.01, 3)
            assert bool(((pt.double() - want['p'][0]).abs() <= want['p'][1]).all()) and bool((slack < 1e-6).all())
            for mu in (0.0, 0.9):
                want, slack, pt = _torch_sgd(host, n, gs, mx, 0.01, mu, 0.05)
                assert bool(((pt.double() - want['p'][0]).abs() <= want['p'][1]).all()) and bool((slack < 1e-5).all())


@pytest.mark.parametrize('gs', (1.0, 0.5))
@pytest.mark.parametrize('mu', (0.0, 0.9))
@pytest.mark.parametrize('ema', (False, True))
@pytest.mark.parametrize('n', (5, 1027))
def test_sgd_clip_flat(ctx, n, ema, mu, gs):
    lib = _lib()
    host = _opt_state(n, 13 * n)
    wd, w, lr = 0.01, 0.25, 0.05
    dev = lambda: [t.clone().cuda() for t in host]
    plain, loose = dev(), dev()
    state = _state(lib.load())
    _sgd(ctx, plain, ema, mu, n, wd, gs, w)
    _sgd(ctx, loose, ema, mu, n, wd, gs, w, 1e30, state)
    torch.cuda.synchronize()
    assert float(state[1]) == 1.0 and all(_same(a, b) for a, b in zip(plain, loose))
    true = cc.ref_norm(host[1], gs)
    mx = 0.3 * true
    tight, twin = dev(), dev()
    state = _state(lib.load())
    _sgd(ctx, tight, ema, mu, n, wd, gs, w, mx, state)
    torch.cuda.synchronize()
    coef = state[1].cpu().numpy()
    assert 0.29 < float(coef) < 0.31
    _sgd(ctx, twin, ema, mu, n, wd, float(np.float32(gs) * coef), w)
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(tight, twin))
    want, slack, p_torch = _torch_sgd(host, n, gs, mx, wd, mu, lr)
    assert bool(((p_torch.double() - want['p'][0]).abs() <= want['p'][1]).all())
    ob.check_dict('sgd_clip n=%d' % n, {'p': tight[0].cpu()}, {'p': (want['p'][0], want['p'][1] + slack)})


@pytest.mark.parametrize('n', (5, 1027))
def test_the_op_form_equals_the_typed_calls(ctx, n):
    lib = _lib()
    host = _opt_state(n, 17 * n)
    step, gs, wd, w = 4, 0.5, 0.01, 0.25
    mx = 0.3 * cc.ref_norm(host[1], gs)
    dev = lambda: [t.clone().cuda() for t in host]
    typed, viaop = dev(), dev()
    s_typed, s_op = _state(lib.load()), _state(lib.load())
    _zero_figures(s_typed)
    _zero_figures(s_op)
    _adam(ctx, typed, True, n, wd, step, gs, w, mx, s_typed)
    o = lib.Op()
    o.kind = lib.OP_ADAM
    for k in range(5):
        o.p[k] = viaop[k].data_ptr()
    o.p[5] = s_op.data_ptr()
    o.i[0], o.i[1] = n, step
    for k, f in enumerate(ADAM_ARGS + (wd, gs, w, mx)):
        o.f[k] = f
    ctx.run_program((lib.Op * 1)(o), 1, st())
    torch.cuda.synchronize()
    assert _same(s_typed, s_op) and float(s_op[1]) < 1.0 and all(_same(a, b) for a, b in zip(typed, viaop))
    for mu in (0.0, 0.9):
        typed, viaop = dev(), dev()
        s_typed, s_op = _state(lib.load()), _state(lib.load())
        _zero_figures(s_typed)
        _zero_figures(s_op)
        _sgd(ctx, typed, False, mu, n, wd, gs, 0.0, mx, s_typed)
        o = lib.Op()
        o.kind = lib.OP_SGD
        o.p[0], o.p[1] = viaop[0].data_ptr(), viaop[1].data_ptr()
        o.p[2] = viaop[2].data_ptr() if mu else None
        o.p[4] = s_op.data_ptr()
        o.i[0], o.i[1] = n, 1
        for k, f in enumerate((0.05, mu, wd, gs, 0.0, mx)):
            o.f[k] = f
        ctx.run_program((lib.Op * 1)(o), 1, st())
        torch.cuda.synchronize()
        assert _same(s_typed, s_op) and float(s_op[1]) < 1.0 and all(_same(a, b) for a, b in zip(typed, viaop))
