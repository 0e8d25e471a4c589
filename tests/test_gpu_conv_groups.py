"""The image-group split of the eval forward (conv_fwd_impl in conv_igemm.hip, and the copy of that loop in
ifcbk_conv2d_fwd_affine_maxpool): a batch whose tensors pass the 2 GiB buffer-descriptor window runs as launches over groups of
G = (2^31 - 1) // bytes-per-image images, with x, y, every segment destination and the residual offset by hand.  Here with a residual,
in fp32, with segments, with a narrow channel slice at a very wide pixel stride and through the pooled entry point, at shapes where
G = 4 and the fourth image ends just under 2^31: one call over the whole batch equals, bit for bit, one call per image with the
pointers offset by the test; the last image of each group is anchored to the fp64 bound of tests/conv_bounds.py (two equal results
could both be wrong).  The splits depend on bytes per image only: a 1x1 convolution over a few very large images, or a 40-channel
slice of a 65,528-element pixel stride, costs a few milliseconds of compute.  No host tensor of the batch's size is created."""
import ctypes as C
import gc

import pytest
import torch

import conv_bounds as cb

pytestmark = pytest.mark.gpu

NAN = float('nan')
TD = {0: torch.bfloat16, 1: torch.float32}
ES = {0: 2, 1: 4}
OUT = {0: 'bf16', 1: 'f32'}
WINDOW = (1 << 31) - 1
H1, W1 = 2048, 2047                 # cases 1 to 3: a 1x1 convolution over six images of 2048 x 2047 pixels


@pytest.fixture(autouse=True)
def _free():
    gc.collect()
    torch.cuda.empty_cache()
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _desc(N, H, W, Cc, ldx, K, R, S, pad, ldy, dt):
    from ifcb_classifier_amd._lib import ConvDesc
    P, Q = H + 2 * pad - R + 1, W + 2 * pad - S + 1
    return ConvDesc(N, H, W, Cc, ldx, K, R, S, 1, 1, pad, pad, P, Q, ldy, Cc, dt)


def _one(d):
    from ifcb_classifier_amd._lib import ConvDesc
    one = ConvDesc.from_buffer_copy(d)
    one.N = 1
    return one


def _groups(N, per):
    """(G, last image of each group) for `per` bytes per image; the fourth image of a group of 4 ends within 2 MiB of 2^31"""
    G = WINDOW // per
    assert G == 4 and N > G and 0 < (1 << 31) - 4 * per <= (2 << 20), (G, per)
    return G, sorted({min(g0 + G, N) - 1 for g0 in range(0, N, G)})


def _at(t, off_elems, dt):
    return C.c_void_p(t.data_ptr() + ES[dt] * off_elems)


def _nan(shape, dt):
    return torch.full(shape, NAN, dtype=TD[dt], device='cuda')


def _randn(shape, dt, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    return torch.randn(shape, device='cuda', dtype=TD[dt], generator=g)


def _sample(npix, seed):
    """4,096 pixels of an image, its first and last among them"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, npix, (4096,), generator=g)
    idx[0], idx[-1] = 0, npix - 1
    return idx


def _as_image(rows):
    """[pixels, channels] gathered on the GPU -> NCHW [1, channels, 1, pixels] fp32 on the CPU (a 1x1 convolution sees pixels only)"""
    return rows.float().cpu().t()[None, :, None, :].contiguous()


def _same(a, b, what):
    assert torch.equal(a, b), '%s: the batch differs from its parts in %d elements' % (what, int((a != b).sum()))


@pytest.mark.parametrize('dt,Cc', [(0, 64), (1, 32)])
def test_group_split_with_residual_equals_its_parts(ctx, dt, Cc):
    """cases 1 and 2: affine + residual + ReLU, bf16 (64 channels) and fp32 (32 channels); groups of 4 + 2 images"""
    from ifcb_classifier_amd import _lib
    N, K, es = 6, 16, ES[dt]
    d = _desc(N, H1, W1, Cc, Cc, K, 1, 1, 0, K, dt)
    per = H1 * W1 * Cc * es
    assert per == 536608768 and 4 * per == 2146435072
    G, lasts = _groups(N, per)
    assert lasts == [3, 5]
    st = _lib.cur_stream()
    x = _randn((N, H1, W1, Cc), dt, 1)
    res = _randn((N, H1, W1, K), dt, 2)
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(K, Cc, 1, 1, generator=g) / Cc ** 0.5).to(TD[dt])
    scale, shift = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
    wk, scd, shd = w.permute(0, 2, 3, 1).contiguous().cuda(), scale.cuda(), shift.cuda()
    y, parts = _nan((N, H1, W1, K), dt), _nan((N, H1, W1, K), dt)
    ctx.call('ifcbk_conv2d_fwd_affine', C.byref(d), _lib.ptr(x), _lib.ptr(wk), _lib.ptr(y), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(res),
             K, 1, st)
    one = _one(d)
    for n in range(N):
        ctx.call('ifcbk_conv2d_fwd_affine', C.byref(one), _at(x, n * H1 * W1 * Cc, dt), _lib.ptr(wk), _at(parts, n * H1 * W1 * K, dt),
                 _lib.ptr(scd), _lib.ptr(shd), _at(res, n * H1 * W1 * K, dt), K, 1, st)
    torch.cuda.synchronize()
    assert torch.isfinite(y.view(-1)[-K:].float()).all() and not torch.isnan(y).any()
    _same(y, parts, 'affine + residual')
    for n in lasts:
        idx = _sample(H1 * W1, 10 + n).cuda()
        xs = _as_image(x[n].reshape(-1, Cc)[idx])
        ref, A, nred = cb.fwd(xs, w.float())
        cb.check_affine('image %d' % n, y[n].reshape(-1, K)[idx].reshape(1, 1, -1, K), ref, A, nred, scale, shift,
                        res[n].reshape(-1, K)[idx].reshape(1, 1, -1, K), relu=True, out=OUT[dt],
                        family='conv image groups %s affine+res' % OUT[dt])


def test_group_split_with_segments_equals_its_parts(ctx):
    """case 3: the segmented forward over the same input; a raw segment inside a 32-wide buffer at channel offset 8 and two affine ones"""
    from ifcb_classifier_amd import _lib
    N, Cc, K, dt = 6, 64, 48, 0
    ksegs, lds, offs, aff = [16, 24, 8], [32, 24, 8], [8, 0, 0], [0, 1, 1]
    d = _desc(N, H1, W1, Cc, Cc, K, 1, 1, 0, K, dt)
    G, lasts = _groups(N, H1 * W1 * Cc * 2)
    st = _lib.cur_stream()
    x = _randn((N, H1, W1, Cc), dt, 4)
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(K, Cc, 1, 1, generator=g) / Cc ** 0.5).to(TD[dt])
    scale, shift = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
    wk, scd, shd = w.permute(0, 2, 3, 1).contiguous().cuda(), scale.cuda(), shift.cuda()
    arr = lambda v: (C.c_int32 * 3)(*v)

    def run(dd, bufs, n0):
        ptrs = (C.c_void_p * 3)(*[b.data_ptr() + 2 * (n0 * H1 * W1 * ld + o) for b, ld, o in zip(bufs, lds, offs)])
        ctx.call('ifcbk_conv2d_fwd_affine_segments', C.byref(dd), _at(x, n0 * H1 * W1 * Cc, dt), _lib.ptr(wk), 3, ptrs, arr(lds), arr(ksegs),
                 arr(aff), _lib.ptr(scd), _lib.ptr(shd), st)

    ys = [_nan((N, H1, W1, ld), dt) for ld in lds]
    parts = [_nan((N, H1, W1, ld), dt) for ld in lds]
    run(d, ys, 0)
    one = _one(d)
    for n in range(N):
        run(one, parts, n)
    torch.cuda.synchronize()
    assert torch.isnan(ys[0][..., :8]).all() and torch.isnan(ys[0][..., 24:]).all(), 'segment 0 wrote outside its channel slice'
    for i, (ks, o) in enumerate(zip(ksegs, offs)):
        assert not torch.isnan(ys[i][..., o:o + ks]).any()
        _same(ys[i][..., o:o + ks], parts[i][..., o:o + ks], 'segment %d' % i)
    fam = 'conv image groups bf16 segments'
    for n in lasts:
        idx = _sample(H1 * W1, 20 + n).cuda()
        ref, A, nred = cb.fwd(_as_image(x[n].reshape(-1, Cc)[idx]), w.float())
        k0 = 0
        for i, (ks, ld, o) in enumerate(zip(ksegs, lds, offs)):
            got = ys[i][n].reshape(-1, ld)[idx][:, o:o + ks].reshape(1, 1, -1, ks)
            sl = slice(k0, k0 + ks)
            if aff[i]:
                cb.check_affine('image %d segment %d' % (n, i), got, ref[..., sl], A[..., sl], nred, scale[sl], shift[sl], relu=True, family=fam)
            else:
                cb.check('image %d segment %d (raw)' % (n, i), got, ref[..., sl], A[..., sl], nred, family=fam)
            k0 += ks


def test_group_split_of_a_narrow_slice_at_a_wide_pixel_stride(ctx):
    """case 4: 3x3 / pad 1 over five 64 x 64 images whose 40 channels are the last slice of a 65,528-element pixel stride: the fourth
    image's last pixel ends 16 bytes under the end of its group's window"""
    from ifcb_classifier_amd import _lib
    N, H, W, Cc, K, LDX, dt = 5, 64, 64, 40, 48, 65528, 0
    off = LDX - Cc - 8
    per = H * W * LDX * 2
    assert per == 536805376 and 4 * per == 2147221504
    G, lasts = _groups(N, per)
    assert lasts == [3, 4]
    st = _lib.cur_stream()
    xb = _nan((N, H, W, LDX), dt)
    xb[..., off:off + Cc] = _randn((N, H, W, Cc), dt, 6)
    res = _randn((N, H, W, K), dt, 7)
    g = torch.Generator().manual_seed(8)
    w = (torch.randn(K, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5).to(TD[dt])
    scale, shift = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
    wk, scd, shd = w.permute(0, 2, 3, 1).contiguous().cuda(), scale.cuda(), shift.cuda()
    y, parts = _nan((N, H, W, K + 8), dt), _nan((N, H, W, K + 8), dt)
    dd = _desc(N, H, W, Cc, LDX, K, 3, 3, 1, K + 8, dt)
    ctx.call('ifcbk_conv2d_fwd_affine', C.byref(dd), _at(xb, off, dt), _lib.ptr(wk), _lib.ptr(y), _lib.ptr(scd), _lib.ptr(shd), _lib.ptr(res),
             K, 1, st)
    one = _one(dd)
    for n in range(N):
        ctx.call('ifcbk_conv2d_fwd_affine', C.byref(one), _at(xb, n * H * W * LDX + off, dt), _lib.ptr(wk), _at(parts, n * H * W * (K + 8), dt),
                 _lib.ptr(scd), _lib.ptr(shd), _at(res, n * H * W * K, dt), K, 1, st)
    torch.cuda.synchronize()
    assert torch.isnan(y[..., K:]).all() and not torch.isnan(y[..., :K]).any()
    _same(y[..., :K], parts[..., :K], 'affine + residual')
    ref, A, nred = cb.fwd(xb[N - 1, :, :, off:off + Cc].float().cpu().permute(2, 0, 1)[None], w.float(), 1, 1)
    cb.check_affine('last image', y[N - 1:, :, :, :K], ref, A, nred, scale, shift, res[N - 1:], relu=True,
                    family='conv image groups bf16 wide stride')
    ref, A, nred = cb.fwd(xb[G - 1, :, :, off:off + Cc].float().cpu().permute(2, 0, 1)[None], w.float(), 1, 1)
    cb.check_affine('last image of the full group', y[G - 1:G, :, :, :K], ref, A, nred, scale, shift, res[G - 1:G], relu=True,
                    family='conv image groups bf16 wide stride')


def test_group_split_of_the_pooled_entry_point(ctx):
    """case 5: ifcbk_conv2d_fwd_affine_maxpool has its own group loop: five 128 x 130 images of a 32-channel slice at a pixel stride
    of 16,128 elements.  The batch equals its parts, and the last image of each group equals ifcbk_conv2d_fwd_affine +
    ifcbk_maxpool_fwd on that image bit for bit (the header's promise), whose activation is held to the fp64 affine bound"""
    from ifcb_classifier_amd import _lib
    from ifcb_classifier_amd._lib import PoolDesc
    N, H, W, Cc, K, LDX, LDP, dt = 5, 128, 130, 32, 64, 16128, 80, 0
    off = LDX - Cc - 8
    d = _desc(N, H, W, Cc, LDX, K, 3, 3, 0, K, dt)
    P, Q = d.P, d.Q
    Pp, Qp = (P - 3) // 2 + 1, (Q - 3) // 2 + 1
    assert ctx.lib.ifcbk_conv2d_fwd_affine_maxpool_ok(C.byref(d)) == 1 and Q <= 160
    per = H * W * LDX * 2
    assert per == 536739840
    G, lasts = _groups(N, per)
    assert lasts == [3, 4]
    st = _lib.cur_stream()
    xb = _nan((N, H, W, LDX), dt)
    xb[..., off:off + Cc] = _randn((N, H, W, Cc), dt, 9)
    g = torch.Generator().manual_seed(10)
    w = (torch.randn(K, Cc, 3, 3, generator=g) / (Cc * 9) ** 0.5).to(TD[dt])
    scale, shift = torch.randn(K, generator=g) * 0.7, torch.randn(K, generator=g) * 0.3            # (negative scales too)
    wk, scd, shd = w.permute(0, 2, 3, 1).contiguous().cuda(), scale.cuda(), shift.cuda()
    y, parts = _nan((N, Pp, Qp, LDP), dt), _nan((N, Pp, Qp, LDP), dt)
    ctx.call('ifcbk_conv2d_fwd_affine_maxpool', C.byref(d), _at(xb, off, dt), _lib.ptr(wk), _lib.ptr(y), LDP, _lib.ptr(scd), _lib.ptr(shd), 1, st)
    one = _one(d)
    for n in range(N):
        ctx.call('ifcbk_conv2d_fwd_affine_maxpool', C.byref(one), _at(xb, n * H * W * LDX + off, dt), _lib.ptr(wk), _at(parts, n * Pp * Qp * LDP, dt),
                 LDP, _lib.ptr(scd), _lib.ptr(shd), 1, st)
    torch.cuda.synchronize()
    assert torch.isnan(y[..., K:]).all() and not torch.isnan(y[..., :K]).any()
    _same(y[..., :K], parts[..., :K], 'pooled')
    pd = PoolDesc(1, P, Q, K, K, 3, 3, 2, 2, 0, 0, Pp, Qp, K, dt)
    for n in lasts:
        act = _nan((1, P, Q, K), dt)
        ctx.call('ifcbk_conv2d_fwd_affine', C.byref(one), _at(xb, n * H * W * LDX + off, dt), _lib.ptr(wk), _lib.ptr(act), _lib.ptr(scd),
                 _lib.ptr(shd), None, 0, 1, st)
        pooled = _nan((1, Pp, Qp, K), dt)
        ctx.call('ifcbk_maxpool_fwd', C.byref(pd), _lib.ptr(act), _lib.ptr(pooled), None, st)
        torch.cuda.synchronize()
        _same(y[n:n + 1, :, :, :K], pooled, 'image %d against conv2d_fwd_affine + maxpool_fwd' % n)
        ref, A, nred = cb.fwd(xb[n, :, :, off:off + Cc].float().cpu().permute(2, 0, 1)[None], w.float())
        cb.check_affine('image %d activation' % n, act, ref, A, nred, scale, shift, relu=True, family='conv image groups bf16 pooled (activation)')


def test_calls_that_cannot_be_split_refuse_a_batch_beyond_the_window(ctx):
    """a training forward (its statistics are per launch), the input gradient and the weight gradient do not split: with the
    descriptor of case 1 each fails in its descriptor check, before anything launches (null operands)"""
    from ifcb_classifier_amd import _lib
    d = _desc(6, H1, W1, 64, 64, 16, 1, 1, 0, 16, 0)
    part = torch.zeros(8, device='cuda')
    with pytest.raises(RuntimeError, match='2 GiB'):
        ctx.call('ifcbk_conv2d_fwd', C.byref(d), None, None, None, _lib.ptr(part), None)
    with pytest.raises(RuntimeError, match='2 GiB'):
        ctx.call('ifcbk_conv2d_dgrad', C.byref(d), None, None, None, 0, None)
    with pytest.raises(RuntimeError, match='2 GiB'):
        ctx.call('ifcbk_conv2d_wgrad', C.byref(d), None, None, None, 0, None)
