"""ifcbk_batch_blur (TRAIN --blur) on the GPU: the three storage forms against the float64 twin and the rounding-count bound of
tests/blur_cases.py, at the shapes of its case table (S = r + 1, S = 2 r + 1, odd S, the training shape, N = 1, r = 1 and r = 12), between
guard bytes, the u8 buffer at odd addresses; sigma = 0 keeps an image's bits, an image alone gets the bits it gets inside the batch, a
constant image stays constant, and every refusal launches nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import blur_cases as bc

pytestmark = pytest.mark.gpu
G, FILL = 256, 0xA5
DT = {'bf16': torch.bfloat16, 'f32': torch.float32}


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def _kind(form):
    lib = _lib()
    return {'u8': lib.MIX_U8, 'bf16': lib.BF16, 'f32': lib.F32}[form]


def _tensor(x, form):
    """a case input (numpy) as the torch tensor of its storage type"""
    t = torch.from_numpy(np.array(x))
    return t if form == 'u8' else t.to(DT[form])


def _blur(ctx, x, form, sigmas, r, off=0):
    """run the kernel on a copy of ``x`` that starts ``off`` bytes behind an aligned address, between guard bytes; -> the blurred copy"""
    lib = _lib()
    raw = x.contiguous().view(torch.uint8).reshape(-1)
    nb = raw.numel()
    buf = torch.full((G + off + nb + G,), FILL, dtype=torch.uint8, device='cuda')
    buf[G + off:G + off + nb] = raw.cuda()
    sg = torch.tensor(list(sigmas), dtype=torch.float32).cuda()
    ctx.call('ifcbk_batch_blur', C.c_void_p(buf.data_ptr() + G + off), _kind(form), x.shape[0], x.shape[1], lib.ptr(sg), int(r), lib.cur_stream())
    torch.cuda.synchronize()
    out = buf.cpu()
    assert bool((out[:G + off] == FILL).all()) and bool((out[G + off + nb:] == FILL).all()), 'guard bytes changed'
    return out[G + off:G + off + nb].clone().view(x.dtype).reshape(x.shape)


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _check(tag, got, x, form, sigmas, ref, bound):
    """-> the worst err / bound (dense) or the largest near-tie share (u8)"""
    worst = 0.0
    for n, s in enumerate(sigmas):
        if s == 0.0:
            assert torch.equal(_bits(got[n]), _bits(x[n])), '%s: image %d (sigma 0) changed' % (tag, n)
            continue
        if form == 'u8':
            wrong, share = bc.u8_verdict(got[n].numpy(), ref[n], bound[n])
            print('%s image %d sigma %g: %d near-ties of %d pixels, %d wrong' % (tag, n, s, int(round(share * wrong.size)), wrong.size, int(wrong.sum())))
            assert not wrong.any(), '%s: image %d, %d bytes are not rint(twin)' % (tag, n, int(wrong.sum()))
            assert share <= bc.TIE_CAP
            worst = max(worst, share)
        else:
            g = got[n].double().numpy()
            err = np.abs(g[..., :3] - ref[n][..., :3])
            ratio = float((err / bound[n][..., :3]).max())
            print('%s image %d sigma %g: worst err %.3e, err / bound %.3f' % (tag, n, s, float(err.max()), ratio))
            assert ratio <= 1.0, '%s: image %d err / bound %.3f' % (tag, n, ratio)
            assert torch.equal(_bits(got[n][..., 3:]), _bits(x[n][..., 3:])), '%s: image %d pad channels changed' % (tag, n)
            worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize('name', bc.CASE_IDS)
@pytest.mark.parametrize('form', bc.FORMS)
def test_batch_blur_against_the_twin(ctx, form, name):
    _, S, r, sigmas, _ = bc.CASES[bc.CASE_IDS.index(name)]
    x = _tensor(bc.case_input(name, form), form)
    ref, bound = bc.case_twin(name, form)
    off = (bc.CASE_IDS.index(name) * 2 + 1) % 16 if form == 'u8' else 0          # the u8 buffer itself starts at an odd address
    got = _blur(ctx, x, form, sigmas, r, off)
    worst = _check('batch_blur %s %s' % (form, name), got, x, form, sigmas, ref, bound)
    print('batch_blur %s %s: worst %s %.4f' % (form, name, 'near-tie share' if form == 'u8' else 'err/bound', worst))
    # each image blurred alone gives the bits it gets inside the batch
    if len(sigmas) > 1:
        for n, s in enumerate(sigmas):
            alone = _blur(ctx, x[n:n + 1], form, [s], r, off=3 if form == 'u8' else 0)
            assert torch.equal(_bits(alone[0]), _bits(got[n])), '%s %s: image %d differs alone' % (form, name, n)
    # a second run gives the same bits
    assert torch.equal(_bits(_blur(ctx, x, form, sigmas, r, off)), _bits(got))


@pytest.mark.parametrize('form', bc.FORMS)
def test_sigma_0_and_sigmas_that_are_not_numbers_keep_every_bit(ctx, form):
    S, r = 19, 4
    x = _tensor(bc.case_input('S=33 r=6', form)[:4, :S, :S].copy(), form)
    if form != 'u8':
        iv = x.view(torch.int16 if form == 'bf16' else torch.int32)              # -0, a NaN pattern, a denormal: bits, not values
        iv[0, 0, 0, 0:3] = torch.tensor([-0x8000, 0x7fc1, 1] if form == 'bf16' else [-0x80000000, 0x7fc00001, 1], dtype=iv.dtype)
    got = _blur(ctx, x, form, [0.0, -1.0, float('nan'), float('inf')], r, off=5 if form == 'u8' else 0)
    assert torch.equal(_bits(got), _bits(x))
    got = _blur(ctx, x, form, [0.0, float('-inf'), 1.0, -0.0], r, off=9 if form == 'u8' else 0)
    keep = [0, 1, 3]
    assert torch.equal(_bits(got[keep]), _bits(x[keep])) and not torch.equal(_bits(got[2]), _bits(x[2]))


@pytest.mark.parametrize('form', bc.FORMS)
def test_a_constant_image_stays_constant(ctx, form):
    S, r, sigmas = 21, 6, (2.0, 0.1, 0.9, 1.7)
    if form == 'u8':
        x = torch.tensor([255, 0, 1, 128], dtype=torch.uint8)[:, None, None].expand(4, S, S).contiguous()
        got = _blur(ctx, x, form, sigmas, r, off=7)
        assert torch.equal(got, x)                                   # exactly: the weights sum to 1 within a few u, far from a half
        return
    x = torch.tensor([2.640625, -2.1171875, 0.0078125, 1.0])[:, None, None, None].expand(4, S, S, 8).contiguous().to(DT[form])
    got = _blur(ctx, x, form, sigmas, r)
    for n, s in enumerate(sigmas):
        c = float(x[n, 0, 0, 0])
        b = float(np.max(bc.stored_bound(form, s, r, abs(c), np.array([c]))))
        assert float((got[n][..., :3].double() - c).abs().max()) <= b, (form, n)
        assert torch.equal(_bits(got[n][..., 3:]), _bits(x[n][..., 3:]))


def test_refusals_launch_nothing(ctx):
    lib = _lib()
    N, S, r = 3, 13, 6
    x = _tensor(bc.case_input('S=r+1 r=12', 'u8'), 'u8').cuda()
    keep = x.clone()
    sg = torch.tensor([1.0, 2.0, 0.5], device='cuda')
    ok = dict(x=lib.ptr(x), kind=lib.MIX_U8, N=N, S=S, sigma=lib.ptr(sg), radius=r)

    def refused(**kw):
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError, match=r'ifcbk_batch_blur failed \(-1\)'):
            ctx.call('ifcbk_batch_blur', a['x'], a['kind'], a['N'], a['S'], a['sigma'], a['radius'], lib.cur_stream())
    refused(x=None)
    refused(sigma=None)
    refused(N=0)
    refused(N=-1)
    refused(radius=0)
    refused(radius=-3)
    refused(radius=13)
    refused(radius=12, S=12)                                          # radius >= S
    refused(radius=6, S=6)
    refused(radius=1, S=1)
    refused(kind=3)
    refused(kind=-1)
    refused(radius=12, S=600)                                         # the LDS rows of this S do not fit
    d = torch.zeros(N * S * S * 8 + 8, dtype=torch.bfloat16, device='cuda')
    refused(x=C.c_void_p(d.data_ptr() + 2), kind=lib.BF16)            # a dense tensor that is not 16-byte aligned
    assert lib.load().ifcbk_batch_blur(None, ok['x'], ok['kind'], N, S, ok['sigma'], r, lib.cur_stream()) == lib.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
    ctx.call('ifcbk_batch_blur', *[ok[k] for k in ('x', 'kind', 'N', 'S', 'sigma', 'radius')], lib.cur_stream())
    torch.cuda.synchronize()
    assert not torch.equal(x, keep)
