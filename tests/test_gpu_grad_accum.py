"""ifcbk_grad_accum_flat (csrc/grad_accum.hip) on the device: first != 0 stores g over whatever a held, first == 0 is torch's fp32 a + g bit
for bit, three calls are the left-to-right sum (g1 + g2) + g3 and lie within the sequential-sum bound of the float64 sum, a slice call
touches its slice alone, nothing at or behind n is written, g is never written, and a refused call launches nothing.

Sizes: 1 and 3 (scalar tail only), 4 (one 16-byte access), 5 (one access and a tail), 1023 / 1024 / 1025 (one block of 256 threads x 4
elements: its last thread on the tail, exactly full, a second block of one tail element), 4099 (several blocks and a tail) -- the edges
of tests/test_gpu_adamw.py, whose kernel has this one's grid shape."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (1, 3, 4, 5, 1023, 1024, 1025, 4099)
CANARY, NCAN = 0x7fc0dead, 9           # a NaN with a payload: any write behind element n changes these bits
U = 2.0 ** -24                         # unit roundoff of fp32


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def P(t):
    return _lib().ptr(t)


def st():
    return _lib().cur_stream()


def _canaries(k=NCAN):
    return torch.full((k,), CANARY, dtype=torch.int32).view(torch.float32)


def _dev(t):
    return torch.cat([t.float(), _canaries()]).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _canary_ok(t, n):
    return bool((_bits(t)[n:] == CANARY).all()) and t.numel() == n + NCAN


def _grad(n, seed):
    """magnitudes 10^-4 .. 10^2 with zeros sprinkled in, as _state of tests/test_gpu_adamw.py draws its gradient"""
    g = torch.Generator().manual_seed(seed)
    gr = torch.randn(n, generator=g) * 10 ** (torch.rand(n, generator=g) * 6 - 4)
    gr[::7] = 0.0
    return gr


def _special(t, k):
    """one +-inf and one NaN element, at n >= 1023 (body and tail elements both)"""
    if t.numel() >= 1023:
        t[5 + k] = float('inf') if k % 2 == 0 else -float('inf')
        t[t.numel() - 1 - k] = float('nan')
    return t


@pytest.mark.parametrize('n', NS)
def test_first_stores_g_over_whatever_a_held(ctx, n):
    g = _special(_grad(n, 3 * n + 1), 0)
    a, dg = _dev(_canaries(n)), _dev(g)                                       # a: NaN in every element
    ctx.call('ifcbk_grad_accum_flat', P(a), P(dg), n, 1, st())
    torch.cuda.synchronize()
    assert _same(a[:n], g) and _canary_ok(a, n)
    assert _same(dg[:n], g) and _canary_ok(dg, n)


@pytest.mark.parametrize('n', NS)
def test_add_is_torchs_fp32_sum(ctx, n):
    a0, g = _special(_grad(n, 5 * n + 2), 0), _special(_grad(n, 7 * n + 3), 1)
    if n >= 1023:
        g[5] = float('inf')                                                   # inf + inf of one sign stays inf
    a, dg = _dev(a0), _dev(g)
    ctx.call('ifcbk_grad_accum_flat', P(a), P(dg), n, 0, st())
    torch.cuda.synchronize()
    want = a0 + g                                                             # torch, CPU, fp32
    assert _same(a[:n], want) and _canary_ok(a, n)
    assert _same(dg[:n], g) and _canary_ok(dg, n)
    if n >= 1023:
        got = a[:n].cpu()
        assert got[5] == float('inf') and got[6] == -float('inf')             # inf stays inf
        assert bool(torch.isnan(got[n - 1])) and bool(torch.isnan(got[n - 2]))      # NaN stays NaN
        assert int(torch.isnan(got).sum()) == 2 and int(torch.isinf(got).sum()) == 2


@pytest.mark.parametrize('n', NS)
def test_three_calls_are_the_sequential_sum(ctx, n):
    gs = [_grad(n, 11 * n + k) for k in range(3)]
    a = _dev(_canaries(n))
    dgs = [_dev(g) for g in gs]
    for k, dg in enumerate(dgs):
        ctx.call('ifcbk_grad_accum_flat', P(a), P(dg), n, 1 if k == 0 else 0, st())
    torch.cuda.synchronize()
    assert _same(a[:n], (gs[0] + gs[1]) + gs[2]) and _canary_ok(a, n)
    for g, dg in zip(gs, dgs):
        assert _same(dg[:n], g) and _canary_ok(dg, n)
    # two roundings, each of a partial sum no larger than sum_j |g_j|: |fl-sum - sum| <= 2 u sum_j |g_j| (u = 2^-24); nothing is measured
    exact = gs[0].double() + gs[1].double() + gs[2].double()
    bound = 2 * U * (gs[0].double().abs() + gs[1].double().abs() + gs[2].double().abs())
    err = (a[:n].cpu().double() - exact).abs()
    print('n %d: worst err / bound %.3g' % (n, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())


@pytest.mark.parametrize('first', (1, 0))
@pytest.mark.parametrize('off,n', ((4, 5), (1024, 1025), (8, 4099 - 8)))
def test_a_slice_call_touches_the_slice_alone(ctx, off, n, first):
    total = off + n + 3                                                       # elements behind the slice, then the canaries
    a0, g = _grad(total, off + n), _grad(total, off + n + 1)
    a, dg = _dev(a0), _dev(g)
    ctx.call('ifcbk_grad_accum_flat', C.c_void_p(a.data_ptr() + 4 * off), C.c_void_p(dg.data_ptr() + 4 * off), n, first, st())
    torch.cuda.synchronize()
    want = a0.clone()
    want[off:off + n] = g[off:off + n] if first else a0[off:off + n] + g[off:off + n]
    assert _same(a[:total], want) and _canary_ok(a, total)
    assert _same(dg[:total], g) and _canary_ok(dg, total)


def test_refusals_launch_nothing(ctx):
    lib = _lib()
    a0, g = _grad(16, 1), _grad(16, 2)
    a, dg = _dev(a0), _dev(g)
    call = lambda pa, pg, n, first=0: ctx.lib.ifcbk_grad_accum_flat(ctx.h, pa, pg, n, first, st())
    off4 = lambda t: C.c_void_p(t.data_ptr() + 4)
    for first in (0, 1):
        assert call(None, P(dg), 8, first) == lib.EINVAL == -1
        assert call(P(a), None, 8, first) == lib.EINVAL
        assert call(off4(a), P(dg), 4, first) == lib.EINVAL                   # a not 16-byte aligned
        assert call(P(a), off4(dg), 4, first) == lib.EINVAL                   # g not 16-byte aligned
        assert call(P(a), P(dg), -1, first) == lib.EINVAL
        assert call(P(a), P(a), 8, first) == lib.EINVAL                       # a == g
        assert call(P(a), P(dg), 0, first) == 0                               # nothing to do: OK, nothing launched
    torch.cuda.synchronize()
    assert _same(a[:16], a0) and _canary_ok(a, 16)
    assert _same(dg[:16], g) and _canary_ok(dg, 16)
