"""RUN --tta on the GPU: ifcbk_batch_sym (csrc/batch_sym.hip) against the numpy model of tests/sym_cases.py -- exact equality for the
three buffer kinds, the three ops, every size of the case table and batches of 1 and 3; the u8 plane at every base offset 0..15 of a
larger buffer whose guard bytes must come back untouched; involutions, the walks back to the start, reproducibility, and the refusals."""
import ctypes as C

import numpy as np
import pytest
import torch

import sym_cases as sc

pytestmark = pytest.mark.gpu

G = 64                                  # guard bytes on either side of a buffer
CANARY = 0xA5


def _run(ctx, kind, x, ops, off=0):
    """x (numpy raw bits, [N, S, S, ...]) at byte offset G + off of a guarded device buffer, the ops applied in order -> (result, guards ok)"""
    from ifcb_classifier_amd import _lib as lib
    raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    host = np.full(G + off + raw.size + G, CANARY, np.uint8)
    host[G + off:G + off + raw.size] = raw
    buf = torch.from_numpy(host).cuda()
    for op in ops:
        ctx.call('ifcbk_batch_sym', C.c_void_p(buf.data_ptr() + G + off), sc.KINDS[kind][0], x.shape[0], x.shape[1], op, lib.cur_stream())
    back = buf.cpu().numpy()
    guards = bool((back[:G + off] == CANARY).all() and (back[G + off + raw.size:] == CANARY).all())
    return back[G + off:G + off + raw.size].view(x.dtype).reshape(x.shape), guards


@pytest.mark.parametrize('op', sorted(sc.OPS))
@pytest.mark.parametrize('kind', sorted(sc.KINDS))
def test_batch_sym_is_the_numpy_permutation(ctx, kind, op):
    for S in sc.SIZES:
        for N in sc.NS:
            x = sc.batch(kind, N, S)
            for off in (range(16) if kind == 'u8' else (0,)):           # (a dense tensor has to be 16-byte aligned)
                got, guards = _run(ctx, kind, x, [sc.OPS[op]], off)
                tag = 'batch_sym %s %s S %d N %d offset %d' % (kind, op, S, N, off)
                assert guards, tag + ': a guard byte was written'
                assert np.array_equal(got, sc.apply(x, sc.OPS[op])), tag


@pytest.mark.parametrize('kind', sorted(sc.KINDS))
def test_twice_is_the_identity_and_the_walks_come_home(ctx, kind):
    for S in (2, 17, 65, 299):
        x = sc.batch(kind, 3, S, seed=1)
        off = 5 if kind == 'u8' else 0
        for op in sc.OPS.values():
            got, guards = _run(ctx, kind, x, [op, op], off)
            assert guards and np.array_equal(got, x), (kind, S, op)
        for mode, walk in sc.WALKS.items():
            got, guards = _run(ctx, kind, x, list(walk), off)
            assert guards and np.array_equal(got, sc.views(x, mode)[-1]), (kind, S, mode)
            assert not np.array_equal(got, x)
            got, guards = _run(ctx, kind, x, list(walk) + [sc.RESTORE[mode]], off)
            assert guards and np.array_equal(got, x), (kind, S, mode)


@pytest.mark.parametrize('kind', sorted(sc.KINDS))
def test_two_runs_give_the_same_bits(ctx, kind):
    x = sc.batch(kind, 3, 299, seed=2)
    for op in sc.OPS.values():
        a, _ = _run(ctx, kind, x, [op], 3 if kind == 'u8' else 0)
        b, _ = _run(ctx, kind, x, [op], 3 if kind == 'u8' else 0)
        assert np.array_equal(a, b)


def test_refusals(ctx):
    from ifcb_classifier_amd import _lib as lib
    S = 17
    u8 = torch.zeros(2 * S * S + 16, dtype=torch.uint8, device='cuda')
    dense = torch.zeros(2, S, S, 8, dtype=torch.float32, device='cuda')
    ok = dict(x=lib.ptr(u8), kind=lib.MIX_U8, N=2, S=S, op=lib.SYM_HFLIP)
    bad = [dict(ok, x=None), dict(ok, N=0), dict(ok, N=-3), dict(ok, S=0), dict(ok, S=32769), dict(ok, kind=3), dict(ok, kind=-1),
           dict(ok, op=0), dict(ok, op=3), dict(ok, op=5), dict(ok, op=7), dict(ok, op=8), dict(ok, op=-1),
           dict(ok, x=C.c_void_p(dense.data_ptr() + 8), kind=lib.F32), dict(ok, x=C.c_void_p(dense.data_ptr() + 4), kind=lib.BF16)]
    for a in bad:
        with pytest.raises(RuntimeError, match=r'ifcbk_batch_sym failed \(-1\)'):
            ctx.call('ifcbk_batch_sym', a['x'], a['kind'], a['N'], a['S'], a['op'], lib.cur_stream())
    torch.cuda.synchronize()
    assert not u8.any().item() and not dense.any().item()
    # a u8 plane may start anywhere, and S == 1 is a no-op for every op and kind
    ctx.call('ifcbk_batch_sym', C.c_void_p(u8.data_ptr() + 7), lib.MIX_U8, 2, S, lib.SYM_TRANSPOSE, lib.cur_stream())
    one = torch.arange(3 * 8, dtype=torch.float32, device='cuda').reshape(3, 1, 1, 8)
    for op in sc.OPS.values():
        ctx.call('ifcbk_batch_sym', lib.ptr(one), lib.F32, 3, 1, op, lib.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(one.cpu().reshape(-1), torch.arange(24.0))
