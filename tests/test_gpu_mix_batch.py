"""TRAIN --mixup / --cutmix on the GPU: ifcbk_batch_mix (csrc/batch_mix.hip) in its three buffer forms against tests/mix_cases.py --
S 5 and 299 (25 and 89,401 bytes per image: partners aligned to nothing) and 16 (aligned), N 1, 2, 3 and 8, per-row factors with exact
0, 1 and 0.5, every box of mix_cases.boxes, guard bytes on both sides, and the refusals."""
import pytest
import torch

import mix_cases as mc

pytestmark = pytest.mark.gpu
G = 64                  # guard bytes on either side
FILL = 0xA5
FORMS = {'u8': (torch.uint8, 2), 'bf16': (torch.bfloat16, 0), 'f32': (torch.float32, 1)}          # (storage, kind of the C ABI)


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def _mix(ctx, x, form, lam, box, off=0):
    """run the kernel on a copy of ``x`` that starts ``off`` bytes behind an aligned address, between guard bytes; -> the mixed copy"""
    import ctypes as C
    lib = _lib()
    raw = x.contiguous().view(torch.uint8).reshape(-1)
    nb = raw.numel()
    buf = torch.full((G + off + nb + G,), FILL, dtype=torch.uint8, device='cuda')
    buf[G + off:G + off + nb] = raw.cuda()
    lam_d = lam.cuda()
    ctx.call('ifcbk_batch_mix', C.c_void_p(buf.data_ptr() + G + off), FORMS[form][1], x.shape[0], x.shape[1], lib.ptr(lam_d), *box, lib.cur_stream())
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[:G + off] == FILL).all()) and bool((out[G + off + nb:] == FILL).all()), 'guard bytes changed'
    return out[G + off:G + off + nb].clone().view(x.dtype).reshape(x.shape)


def _inputs(N, S, form):
    lam = mc.lam_rows(N)
    x8 = mc.u8_batch(N, S, lam=lam)
    return (x8 if form == 'u8' else mc.dense_from_u8(x8, FORMS[form][0])), lam


@pytest.mark.parametrize('S', mc.MIX_S)
@pytest.mark.parametrize('form', list(FORMS))
def test_batch_mix(ctx, form, S):
    worst = 0.0
    for N in mc.MIX_N:
        x, lam = _inputs(N, S, form)
        for k, (name, box) in enumerate(mc.boxes(S).items()):
            tag = 'batch_mix %s S %d N %d box %s' % (form, S, N, name)
            if form == 'u8':
                got = _mix(ctx, x, form, lam, box, off=(0, 3, 7, 15, 1, 9, 5, 13)[k])          # the buffer itself starts anywhere
                worst = max(worst, mc.check_mix_u8(tag, got, x, lam, box))
            else:
                got = _mix(ctx, x, form, lam, box)
                worst = max(worst, mc.check_mix_dense(tag, got, x, lam, box, form))
            # box pixels are exact copies of the partner's original pixels
            y0, y1, x0, x1 = box
            keep = [n for n in range(N) if n != N - 1 - n]
            assert torch.equal(got[keep][:, y0:y1, x0:x1].view(torch.uint8), x.flip(0)[keep][:, y0:y1, x0:x1].contiguous().view(torch.uint8)), tag
    print('batch_mix %s S %d: worst %s %.4f' % (form, S, 'ambiguous share' if form == 'u8' else 'err/bound', worst))


@pytest.mark.parametrize('form', list(FORMS))
def test_lam_1_and_an_empty_box_return_every_byte(ctx, form):
    for S in mc.MIX_S:
        for N in (1, 2, 3, 8):
            x, _ = _inputs(N, S, form)
            if form != 'u8':
                iv = x.view(torch.int16 if form == 'bf16' else torch.int32)              # -0, a NaN pattern, a denormal: bits, not values
                iv[0, 0, 0, 3:6] = torch.tensor([-0x8000, 0x7fc1, 1] if form == 'bf16' else [-0x80000000, 0x7fc00001, 1], dtype=iv.dtype)
            for box in ((0, 0, 0, 0), (2, 2, 0, S), (0, S, 3, 3)):
                got = _mix(ctx, x, form, torch.ones(N), box, off=5 if form == 'u8' else 0)
                assert torch.equal(got.view(torch.uint8), x.view(torch.uint8)), (form, S, N, box)


def test_refusals_launch_nothing(ctx):
    lib = _lib()
    N, S = 4, 16
    x = mc.u8_batch(N, S).cuda()
    keep = x.clone()
    lam = torch.tensor([0.7391, 0.1234567, 0.9183, 0.3344551], device='cuda')      # (no short fractions: lam (a - b) sits near no rounding tie)
    ok = dict(x=lib.ptr(x), kind=2, N=N, S=S, lam=lib.ptr(lam), y0=0, y1=4, x0=0, x1=4)

    def refused(**kw):
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError, match=r'ifcbk_batch_mix failed \(-1\)'):
            ctx.call('ifcbk_batch_mix', a['x'], a['kind'], a['N'], a['S'], a['lam'], a['y0'], a['y1'], a['x0'], a['x1'], lib.cur_stream())
    refused(x=None)
    refused(lam=None)
    refused(N=0)
    refused(N=-2)
    refused(S=0)
    refused(y0=-1)
    refused(y1=S + 1)
    refused(x0=-1)
    refused(x1=S + 1)
    refused(y0=5, y1=4)
    refused(x0=5, x1=4)
    refused(kind=3)
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    ctx.call('ifcbk_batch_mix', *[ok[k] for k in ('x', 'kind', 'N', 'S', 'lam', 'y0', 'y1', 'x0', 'x1')], lib.cur_stream())
    torch.cuda.synchronize()
    mc.check_mix_u8('after the refusals', x.cpu(), keep.cpu(), lam.cpu(), (0, 4, 0, 4))
