"""RUN --tta on the GPU: ifcbk_softmax_acc (csrc/loss.hip).  A single call that stores is ifcbk_softmax bit for bit; eight accumulated
calls, the last scaled by 1/8, stay inside the float64 bound of tests/tta_bounds.py and equal, bit for bit, the fp32 left-to-right sum
of the eight ifcbk_softmax outputs times 0.125 (torch's elementwise fp32 add and multiply are single IEEE operations); refusals."""
import math

import pytest
import torch

import tta_bounds as tb

pytestmark = pytest.mark.gpu

CASES = [(N, NC) for N in (1, 5, 257) for NC in (1, 2, 7, 100)]
V = 8


def _views(N, NC):
    g = torch.Generator().manual_seed(100 * N + NC)
    ls = [torch.randn(N, NC, generator=g) * 3.0 for _ in range(V)]
    ls[2][N // 2, NC - 1] += 80.0                       # a row with one logit 80 above the rest (the others' exponentials flush)
    return ls


@pytest.mark.parametrize('N,NC', CASES)
def test_store_is_softmax_and_eight_views_are_their_fp32_mean(ctx, N, NC):
    from ifcb_classifier_amd import _lib as lib
    P, st = lib.ptr, lib.cur_stream
    ls = _views(N, NC)
    dev = [l.cuda() for l in ls]
    plain = [torch.empty(N, NC, device='cuda') for _ in range(V)]
    for l, p in zip(dev, plain):
        ctx.call('ifcbk_softmax', P(l), N, NC, P(p), st())
    # accumulate = 0, scale = 1: ifcbk_softmax's bits, over whatever the buffer held
    one = torch.full((N + 1, NC), float('nan'), device='cuda')
    ctx.call('ifcbk_softmax_acc', P(dev[0]), N, NC, P(one), 0, 1.0, st())
    assert torch.equal(one[:N], plain[0]) and one[N:].isnan().all().item()
    # the eight views
    acc = torch.full((N + 1, NC), float('nan'), device='cuda')
    for v in range(V):
        ctx.call('ifcbk_softmax_acc', P(dev[v]), N, NC, P(acc), int(v > 0), 0.125 if v == V - 1 else 1.0, st())
    again = torch.full((N + 1, NC), float('nan'), device='cuda')
    for v in range(V):
        ctx.call('ifcbk_softmax_acc', P(dev[v]), N, NC, P(again), int(v > 0), 0.125 if v == V - 1 else 1.0, st())
    torch.cuda.synchronize()
    assert acc[N:].isnan().all().item(), 'a row beyond N was written'
    assert torch.equal(acc[:N], again[:N]), 'two runs differ'
    s = plain[0].clone()
    for p in plain[1:]:
        s = s + p
    assert torch.equal(acc[:N], s * 0.125), 'not the fp32 left-to-right sum of the ifcbk_softmax outputs times 0.125'
    want, e = tb.mean_softmax(ls)
    r = ((acc[:N].cpu().double() - want).abs() / e).max().item()
    print('softmax_acc N %d NC %d: worst err / bound %.3f' % (N, NC, r))
    assert r <= 1.0, r


def test_refusals(ctx):
    from ifcb_classifier_amd import _lib as lib
    P, st = lib.ptr, lib.cur_stream
    l = torch.randn(4, 5, device='cuda')
    acc = torch.zeros(4, 5, device='cuda')
    ok = dict(l=P(l), N=4, NC=5, acc=P(acc), a=1, s=1.0)
    bad = [dict(ok, l=None), dict(ok, acc=None), dict(ok, N=0), dict(ok, N=-1), dict(ok, NC=0), dict(ok, s=0.0), dict(ok, s=-0.5),
           dict(ok, s=math.inf), dict(ok, s=math.nan)]
    for a in bad:
        with pytest.raises(RuntimeError, match=r'ifcbk_softmax_acc failed \(-1\)'):
            ctx.call('ifcbk_softmax_acc', a['l'], a['N'], a['NC'], a['acc'], a['a'], a['s'], st())
    torch.cuda.synchronize()
    assert not acc.any().item()
