"""The fp32 parity mode (conv_igemm<float, NT, 2, 2, MODE> and conv_wgrad_f32<MT>) held to the per-element fp64 bound of
tests/conv_bounds.py on every epilogue it has: raw forward with statistics, the eval affine (scale, shift, residual, ReLU), the input
gradient as first writer, accumulating and with the BN-backward sums (MODE 3), the stride-2 forms (MODE 1, MODE 2), the segmented
forward (MODE 4), and the weight gradient plain and accumulating -- on channel slices (ld* > C), channel counts that are multiples of 4
and not of 8, N = 1 with M % 128 == 1 and Cw < C.  Then geometry that the descriptor check accepts and no other case has, in bf16 and
fp32 on the default dispatch: stride-2 input gradients with a trailing input row / column that no output pixel reaches, stride_h !=
stride_w, H < 2 at stride 2, and a stride above 2 (forward and weight gradient bounded, the input gradient refused).

Every tensor a kernel touches is a channel slice of a NaN-filled buffer: after each call nothing outside the slice has changed (and an
operand read outside its slice would surface as a NaN inside).  Each role asserts through ifcbk_op_kernel which kernel ran."""
import ctypes as C
import re

import pytest
import torch

import conv_bounds as cb
import test_gpu_conv_forced as T1

pytestmark = pytest.mark.gpu

forced = T1.forced          # (the per-launch switch fixture of the forced tests)
OFF = dict(IFCBK_CONV_BIG=0, IFCBK_CONV_FLAT=0, IFCBK_CONV_SLAB=0, IFCBK_CONV_PP3=0, IFCBK_WGRAD_PP=0, IFCBK_WGRAD_FLAT=0)
NAN = float('nan')
TD = {0: torch.bfloat16, 1: torch.float32}
ES = {0: 2, 1: 4}
OUT = {0: 'bf16', 1: 'f32'}


def pick_tile(K, maxt=4):
    """pick_nt (conv_igemm.hip) / pick_mt (conv_wgrad.hip): the 32-column multiple with the least cdiv(K, 32 t) * (32 t + 48), ties to
    the wider tile; the fp32 kernels take at most 4"""
    cost = lambda t: -(-K // (32 * t)) * (32 * t + 48)
    return min(range(1, maxt + 1), key=lambda t: (cost(t), -t))


class Row:
    def __init__(self, case, roles, Cw=None, ldx=None, ldy=None, xoff=0, yoff=0, ldr=None, roff=0, dmode=0, dist='randn'):
        self.case, self.roles, self.Cw = case, roles, Cw or case[1]
        self.dist = dist      # 'randn', or 'net': the operands of a layer inside a network (run_row)
        N, Cc, H, W, K, R, S, sh, sw, ph, pw = case
        self.ldx, self.ldy, self.xoff, self.yoff = ldx or Cc, ldy or K, xoff, yoff
        self.ldr, self.roff, self.dmode = ldr or K, roff, dmode
        self.P, self.Q = (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1

    def desc(self, dt):
        from ifcb_classifier_amd._lib import ConvDesc
        N, Cc, H, W, K, R, S, sh, sw, ph, pw = self.case
        return ConvDesc(N, H, W, Cc, self.ldx, K, R, S, sh, sw, ph, pw, self.P, self.Q, self.ldy, self.Cw, dt)


ALL = ('fwd', 'affine', 'affine+res', 'dgrad', 'dgrad +=', 'bnstat', 'wgrad', 'wgrad +=')
# the fp32 table: rows of (N, C, H, W, K, R, S, sh, sw, ph, pw); dmode: the epilogue mode of the row's input gradient
F32 = {
    # M = 385 (N = 1, M % 128 == 1), C and K multiples of 4 and not of 8, every tensor a channel slice
    'm385-slices': Row((1, 12, 35, 11, 20, 3, 3, 1, 1, 1, 1), ALL, ldx=20, ldy=28, xoff=4, yoff=4, ldr=24, roff=4),
    # the stem as the fp32 ABI allows it: 3 master channels padded to 4, stride 2, parity classes
    'stem-cw3': Row((2, 4, 31, 31, 32, 3, 3, 2, 2, 0, 0), ('fwd', 'affine', 'affine+res', 'dgrad', 'wgrad', 'wgrad +=', 'pack'), Cw=3, dmode=2),
    'mode1': Row((1, 64, 9, 9, 96, 1, 1, 2, 2, 0, 0), ('dgrad', 'dgrad +='), dmode=1),
    'mode2-mtail': Row((3, 40, 9, 10, 56, 3, 3, 2, 2, 1, 1), ('dgrad', 'dgrad +=', 'wgrad', 'wgrad +='), dmode=2),
    'mode3': Row((2, 48, 11, 13, 72, 1, 7, 1, 1, 0, 3), ('fwd', 'bnstat', 'dgrad +=', 'wgrad')),
    # K tail: 200 = 128 + 72 columns of the forward (NT = 4) and rows of the weight gradient (MT = 4); its input gradient has NT = 1
    'ktail': Row((2, 24, 9, 9, 200, 3, 3, 1, 1, 1, 1), ('fwd', 'affine+res', 'dgrad', 'wgrad', 'wgrad +='), ldx=32, ldy=208, xoff=4, yoff=8),
    # resnet18's layer4.0.downsample.0 (1x1 / stride 2, 256 -> 512: the node of the fp64 walk whose dW sits farthest from fp64, 1.6-1.8 x
    # the reference's distance) at N = 2: the same three kernels and the same single weight-gradient split (98 and 392 pixels are 4 and
    # 13 steps of 32, both under the 16 that a second split needs; run_row asserts the split), on the operands of a layer inside a
    # network: a non-negative post-ReLU input and filters with a common offset, so that the raw output's mean is ~6 of its standard
    # deviations and the statistics' sums cancel nothing; the upstream gradient has zero per-channel mean, as a BatchNorm backward
    # leaves it, but is otherwise random: its correlation with the input inside a trained network is not reproduced
    'l4ds-net': Row((2, 256, 14, 14, 512, 1, 1, 2, 2, 0, 0), ('fwd', 'dgrad', 'wgrad'), dmode=1, dist='net'),
}
SEG_CASE = (1, 64, 11, 35, 132, 1, 1, 1, 1, 0, 0)          # MODE 4: M = 385, K = 132
KINDS = {'fwd': ('OP_CONV_FWD', 0, False), 'affine': ('OP_CONV_FWD_AFFINE', 0, False), 'affine+res': ('OP_CONV_FWD_AFFINE', 0, True),
         'dgrad': ('OP_CONV_DGRAD', 0, False), 'dgrad +=': ('OP_CONV_DGRAD', 1, False), 'bnstat': ('OP_CONV_DGRAD_BNSTAT', 0, False),
         'wgrad': ('OP_CONV_WGRAD', 0, False), 'wgrad +=': ('OP_CONV_WGRAD', 0, False), 'seg': ('OP_CONV_FWD_AFFINE_SEG', 0, False)}


def role_name(ctx, row, dt, role):
    from ifcb_classifier_amd import _lib
    kind, flags, res = KINDS[role]
    return cb.kname(ctx, row.desc(dt), getattr(_lib, kind), flags, res)


def f32_names(ctx):
    """every kernel the fp32 table reaches (test_gpu_conv_bounds.test_conv_kernel_inventory holds it against its fp32 inventory)"""
    names = {role_name(ctx, row, 1, r) for row in F32.values() for r in row.roles if r in KINDS}
    names.add(role_name(ctx, Row(SEG_CASE, ('seg',)), 1, 'seg'))
    return names


def expected_f32_name(row, role):
    N, Cc, H, W, K = row.case[:5]
    if role.startswith('wgrad'):
        return 'conv_wgrad_f32<%d>' % pick_tile(K)
    if role in ('fwd', 'affine', 'affine+res'):
        return 'conv_igemm<float, %d, 2, 2, 0>' % pick_tile(K)
    if role == 'seg':
        return 'conv_igemm<float, %d, 2, 2, 4>' % pick_tile(K)
    return 'conv_igemm<float, %d, 2, 2, %d>' % (pick_tile(Cc), 3 if role == 'bnstat' else row.dmode)


def _rep(t, dt):
    return t.to(TD[dt]).float()


def _slab(data, shape, ld, off, dt):
    """a NaN-filled [*shape, ld] buffer on the GPU with `data` ([*shape, channels], or None) in the channels from `off`"""
    buf = torch.full(tuple(shape) + (ld,), NAN, dtype=TD[dt], device='cuda')
    if data is not None:
        buf[..., off:off + data.shape[-1]] = data.to(TD[dt]).cuda()
    return buf


def _at(buf, off, dt):
    return C.c_void_p(buf.data_ptr() + ES[dt] * off)


def guard(name, buf, off, Cc):
    """nothing written outside the Cc channels from `off`, everything inside written and finite"""
    assert torch.isnan(buf[..., :off]).all() and torch.isnan(buf[..., off + Cc:]).all(), name + ': wrote outside its channel slice'
    assert torch.isfinite(buf[..., off:off + Cc].float()).all(), name + ': unwritten or non-finite element inside'
    return buf[..., off:off + Cc]


def _flat_guarded(data, n, pad=4):
    """a flat fp32 tensor of n elements between `pad` NaN floats (data: its old contents, or None for NaN)"""
    b = torch.full((n + 2 * pad,), NAN)
    if data is not None:
        b[pad:-pad] = data.flatten()
    return b.cuda()


def run_row(ctx, row, dt, seed, fam, expect=None):
    """every role of the row in storage type dt.  fam(role) names the family of the measured section; expect(role, name) asserts
    the kernel.  Returns the input-gradient results for the geometry tests."""
    from ifcb_classifier_amd import _lib
    N, Cc, H, W, K, R, S, sh, sw, ph, pw = row.case
    P, Q, Cw, out = row.P, row.Q, row.Cw, OUT[dt]
    d = row.desc(dt)
    st = _lib.cur_stream()
    g = torch.Generator().manual_seed(seed)
    x = _rep(torch.randn(N, Cc, H, W, generator=g), dt)
    w = _rep(torch.randn(K, Cc, R, S, generator=g) / (Cw * R * S) ** 0.5, dt)
    if row.dist == 'net':
        x = _rep(torch.relu(x), dt)
        w = _rep(w + 2.0 / (Cw * R * S) ** 0.5, dt)
    x[:, Cw:] = 0
    w[:, Cw:] = 0
    dy = _rep(torch.randn(N, K, P, Q, generator=g), dt)
    if row.dist == 'net':
        raw = torch.nn.functional.conv2d(x, w, None, (sh, sw), (ph, pw))
        assert float((raw.mean((0, 2, 3)) / raw.std((0, 2, 3))).min()) > 4.0, 'the raw output is not mean >> spread'
        dy = _rep(dy - dy.mean((0, 2, 3), keepdim=True), dt)
        assert ctx.lib.ifcbk_conv2d_wgrad_workspace(C.byref(d)) == K * R * S * Cc * 4, 'the weight gradient is no longer one split'
    tag = '%s %s' % (out, row.case)
    for role in row.roles:
        if expect and role in KINDS:
            expect(role, role_name(ctx, row, dt, role))
    xd = _slab(x.permute(0, 2, 3, 1), (N, H, W), row.ldx, row.xoff, dt)
    dyd = _slab(dy.permute(0, 2, 3, 1), (N, P, Q), row.ldy, row.yoff, dt)
    wk = w.permute(0, 2, 3, 1).contiguous().to(TD[dt]).cuda()
    wT = w.permute(1, 2, 3, 0).flip(1, 2).contiguous().to(TD[dt]).cuda()
    if 'pack' in row.roles:
        wm = w[:, :Cw].permute(0, 2, 3, 1).contiguous().cuda()                    # the fp32 master [K][R][S][Cw]
        pk, pT = torch.full_like(wk, NAN), torch.full_like(wT, NAN)
        ctx.call('ifcbk_weight_pack', C.byref(d), _lib.ptr(wm), _lib.ptr(pk), _lib.ptr(pT), st)
        torch.cuda.synchronize()
        assert (pk[..., Cw:] == 0).all() and not torch.signbit(pk[..., Cw:]).any() and (pT[Cw:] == 0).all()
        assert torch.equal(pk[..., :Cw], wm.to(TD[dt])) and torch.equal(pk, wk) and torch.equal(pT, wT)
        wk, wT = pk, pT
    res = {}
    fref = cb.fwd(x, w, (sh, sw), (ph, pw)) if {'fwd', 'affine', 'affine+res'} & set(row.roles) else None
    if 'fwd' in row.roles:
        y = _slab(None, (N, P, Q), row.ldy, row.yoff, dt)
        mb = ctx.lib.ifcbk_conv2d_fwd_mblocks(C.byref(d))
        part = torch.full((mb + 1, 2, K), NAN, device='cuda')
        ctx.call('ifcbk_conv2d_fwd', C.byref(d), _at(xd, row.xoff, dt), _lib.ptr(wk), _at(y, row.yoff, dt), _lib.ptr(part), st)
        torch.cuda.synchronize()
        ys = guard('fwd ' + tag, y, row.yoff, K)
        assert torch.isfinite(part[:mb]).all() and torch.isnan(part[mb]).all(), 'statistics rows'
        cb.check('fwd ' + tag, ys, *fref, out=out, family=fam('fwd'))
        cb.check_bn_fwd_sums('fwd stats ' + tag, part[:mb], ys, family=fam('fwd statistics'))
    for role in ('affine', 'affine+res'):
        if role not in row.roles:
            continue
        with_res = role == 'affine+res'
        scale, shift = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
        r = _rep(torch.randn(N, P, Q, K, generator=g), dt) if with_res else None
        rd = _slab(r, (N, P, Q), row.ldr, row.roff, dt) if with_res else None
        scd, shd = scale.cuda(), shift.cuda()
        y = _slab(None, (N, P, Q), row.ldy, row.yoff, dt)
        ctx.call('ifcbk_conv2d_fwd_affine', C.byref(d), _at(xd, row.xoff, dt), _lib.ptr(wk), _at(y, row.yoff, dt), _lib.ptr(scd),
                 _lib.ptr(shd), _at(rd, row.roff, dt) if with_res else None, row.ldr if with_res else 0, int(with_res), st)
        torch.cuda.synchronize()
        ys = guard(role + ' ' + tag, y, row.yoff, K)
        cb.check_affine(role + ' ' + tag, ys, *fref, scale, shift, r, relu=with_res, out=out, family=fam(role))
    dims = ('n', 'h', 'w', 'c')
    dref = cb.dgrad(dy, w, x.shape, (sh, sw), (ph, pw)) if {'dgrad', 'dgrad +=', 'bnstat'} & set(row.roles) else None
    if dref is not None:
        res['taps'] = dref[2]
    if 'dgrad' in row.roles:
        dx = _slab(None, (N, H, W), row.ldx, row.xoff, dt)
        ctx.call('ifcbk_conv2d_dgrad', C.byref(d), _at(dyd, row.yoff, dt), _lib.ptr(wT), _at(dx, row.xoff, dt), 0, st)
        torch.cuda.synchronize()
        res['dx'] = guard('dgrad ' + tag, dx, row.xoff, Cc)
        cb.check('dgrad ' + tag, res['dx'], *dref, out=out, dims=dims, family=fam('dgrad'))
    if 'dgrad +=' in row.roles:
        old = _rep(torch.randn(N, H, W, Cc, generator=g), dt)
        dxa = _slab(old, (N, H, W), row.ldx, row.xoff, dt)
        ctx.call('ifcbk_conv2d_dgrad', C.byref(d), _at(dyd, row.yoff, dt), _lib.ptr(wT), _at(dxa, row.xoff, dt), 1, st)
        torch.cuda.synchronize()
        res['dxa'], res['old'] = guard('dgrad += ' + tag, dxa, row.xoff, Cc), old
        cb.check('dgrad += ' + tag, res['dxa'], *dref, out=out, old=old, dims=dims, family=fam('dgrad +='))
    if 'bnstat' in row.roles:
        raw = _rep(torch.randn(N, H, W, Cc, generator=g) * 1.5, dt)
        mean, invstd = torch.randn(Cc, generator=g) * 0.2, torch.rand(Cc, generator=g) + 0.5
        bsc, bsh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
        nrow = ctx.lib.ifcbk_conv2d_dgrad_bnstat_mblocks(C.byref(d))
        assert nrow > 0
        part2 = torch.full((nrow + 1, 2, Cc), NAN, device='cuda')
        dx3 = _slab(None, (N, H, W), row.ldx, row.xoff, dt)
        rawd = _slab(raw, (N, H, W), row.ldx, row.xoff, dt)
        dev = [t.cuda() for t in (mean, invstd, bsc, bsh)]
        ctx.call('ifcbk_conv2d_dgrad_bnstat', C.byref(d), _at(dyd, row.yoff, dt), _lib.ptr(wT), _at(dx3, row.xoff, dt),
                 _at(rawd, row.xoff, dt), row.ldx, *[_lib.ptr(t) for t in dev], _lib.ptr(part2), st)
        torch.cuda.synchronize()
        d3 = guard('bnstat ' + tag, dx3, row.xoff, Cc)
        assert torch.isfinite(part2[:nrow]).all() and torch.isnan(part2[nrow]).all(), 'BN-backward partial rows'
        cb.check('bnstat ' + tag, d3, *dref, out=out, dims=dims, family=fam('bnstat'))
        cb.check_bn_bwd_sums('bnstat ' + tag, part2[:nrow], d3, raw, mean, invstd, bsc, bsh, family=fam('BN-backward sums'))
    if 'wgrad' in row.roles or 'wgrad +=' in row.roles:
        wdims = ('k', 'r', 's', 'c')
        wref = cb.wgrad(x[:, :Cw], dy, (K, Cw, R, S), (sh, sw), (ph, pw))
        ctx.reserve(ctx.lib.ifcbk_conv2d_wgrad_workspace(C.byref(d)))
        n = K * R * S * Cw
        for role in ('wgrad', 'wgrad +='):
            if role not in row.roles:
                continue
            acc = role == 'wgrad +='
            old = torch.randn(K, R, S, Cw, generator=g) if acc else None
            b = _flat_guarded(old, n)
            ctx.call('ifcbk_conv2d_wgrad', C.byref(d), _at(xd, row.xoff, dt), _at(dyd, row.yoff, dt), C.c_void_p(b.data_ptr() + 16),
                     int(acc), st)
            torch.cuda.synchronize()
            assert torch.isnan(b[:4]).all() and torch.isnan(b[-4:]).all() and torch.isfinite(b[4:-4]).all(), role + ': guard floats'
            cb.check(role + ' ' + tag, b[4:-4].reshape(K, R, S, Cw), *wref, out='f32', old=old, dims=wdims, family=fam(role))
    return res


def _f32_family(role):
    return ('conv_wgrad_f32 ' if role.startswith('wgrad') else 'conv_igemm<float> ') + role


# ---------------------------------------------------------------------------------------------------- B: the fp32 table
@pytest.mark.parametrize('key', list(F32))
def test_f32_epilogue_modes(ctx, forced, key):
    forced(**OFF)
    row = F32[key]

    def expect(role, name):
        assert name == expected_f32_name(row, role), (key, role, name)

    run_row(ctx, row, 1, 40 + sum(row.case), _f32_family, expect)


def test_f32_segments_mode4(ctx, forced):
    """MODE 4 in fp32: a raw segment and two affine ones, sizes off the 32-column tile and multiples of 4, the first destination a
    slice at channel offset 4, M % 128 == 1"""
    from ifcb_classifier_amd import _lib
    forced(**OFF)
    row = Row(SEG_CASE, ('seg',))
    N, Cc, H, W, K = SEG_CASE[:5]
    P, Q = row.P, row.Q
    d = row.desc(1)
    assert role_name(ctx, row, 1, 'seg') == expected_f32_name(row, 'seg') == 'conv_igemm<float, 3, 2, 2, 4>'
    g = torch.Generator().manual_seed(17)
    x = torch.randn(N, Cc, H, W, generator=g)
    w = torch.randn(K, Cc, 1, 1, generator=g) / Cc ** 0.5
    ksegs, lds, offs, aff = [20, 100, 12], [28, 100, 12], [4, 0, 0], [0, 1, 1]
    ys = [_slab(None, (N, P, Q), ld, 0, 1) for ld in lds]
    ptrs = (C.c_void_p * 3)(*[y.data_ptr() + 4 * o for y, o in zip(ys, offs)])
    scale, shift = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
    scd, shd = scale.cuda(), shift.cuda()
    xd, wk = x.permute(0, 2, 3, 1).contiguous().cuda(), w.permute(0, 2, 3, 1).contiguous().cuda()
    ctx.call('ifcbk_conv2d_fwd_affine_segments', C.byref(d), _lib.ptr(xd), _lib.ptr(wk), 3, ptrs, (C.c_int32 * 3)(*lds),
             (C.c_int32 * 3)(*ksegs), (C.c_int32 * 3)(*aff), _lib.ptr(scd), _lib.ptr(shd), _lib.cur_stream())
    torch.cuda.synchronize()
    ref, A, n = cb.fwd(x, w)
    fam = _f32_family('segments')
    k0 = 0
    for i, (ks, off) in enumerate(zip(ksegs, offs)):
        got = guard('segment %d' % i, ys[i], off, ks)
        sl = slice(k0, k0 + ks)
        if aff[i]:
            cb.check_affine('segment %d' % i, got, ref[..., sl], A[..., sl], n, scale[sl], shift[sl], relu=True, out='f32', family=fam)
        else:
            cb.check('segment %d (raw)' % i, got, ref[..., sl], A[..., sl], n, out='f32', family=fam)
        k0 += ks


def test_f32_table_reaches_every_column_and_row_tile(ctx, forced):
    """conv_igemm<float, NT, ...> with NT = 1..4 and conv_wgrad_f32<MT> with MT = 1..4 each have a case in the table above"""
    forced(**OFF)
    nt, mt = set(), set()
    for name in f32_names(ctx):
        m = re.fullmatch(r'conv_igemm<float, (\d), 2, 2, \d>', name)
        if m:
            nt.add(int(m.group(1)))
            continue
        m = re.fullmatch(r'conv_wgrad_f32<(\d)>', name)
        assert m, name
        mt.add(int(m.group(1)))
    assert nt == {1, 2, 3, 4} and mt == {1, 2, 3, 4}, (nt, mt)


# ---------------------------------------------------------------------------------------------------- C: geometry, bf16 and fp32
def _geo(case, roles, dmode):
    """geometry rows run on slices too: ld = channels + 8, offset 8 (multiples of 8: valid for both storage types)"""
    return Row(case, roles, ldx=case[1] + 8, ldy=case[4] + 8, xoff=8, yoff=8, dmode=dmode)


def _geo_family(dt):
    return lambda role: 'conv geometry %s %s' % (OUT[dt], role)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('case,cols', [((2, 24, 12, 14, 40, 3, 3, 2, 2, 0, 0), [13]), ((1, 16, 12, 12, 24, 5, 5, 2, 2, 0, 0), [11])])
def test_stride2_input_gradient_with_unreached_trailing_row_and_column(ctx, dt, case, cols):
    """input row 11 (and the last column) lies past the last filter window: no output pixel reaches it.  The first writer stores
    +0 there, the accumulating call leaves the old value bit for bit; everything else within the bound (whose tap count is 0 there)"""
    row = _geo(case, ('dgrad', 'dgrad +='), 2)
    name = role_name(ctx, row, dt, 'dgrad')
    assert name.endswith(', 2>') and name.startswith('conv_igemm<'), name
    r = run_row(ctx, row, dt, 60 + dt, _geo_family(dt))
    dead = (r['taps'] == 0).expand(-1, -1, -1, case[1])
    assert bool(dead[:, 11].all()) and all(bool(dead[:, :, c].all()) for c in cols) and not bool(dead[:, :11, :cols[0]].any())
    dx, dxa, old = r['dx'].cpu(), r['dxa'].cpu(), r['old'].to(TD[dt])
    assert (dx[dead] == 0).all() and not torch.signbit(dx[dead]).any(), 'first writer: an unreached pixel is not +0'
    assert torch.equal(_bits(dxa[dead]), _bits(old[dead])), 'accumulate: an unreached pixel lost its old value'


@pytest.mark.parametrize('dt', [0, 1])
@pytest.mark.parametrize('sh,sw', [(2, 1), (1, 2)])
def test_mixed_strides(ctx, dt, sh, sw):
    """stride_h != stride_w: the one situation in which the dilated gather's two input strides differ"""
    row = _geo((1, 32, 12, 9, 48, 3, 3, sh, sw, 1, 1), ('fwd', 'dgrad', 'dgrad +=', 'wgrad'), 1)
    for role in ('dgrad', 'dgrad +='):
        name = role_name(ctx, row, dt, role)
        assert name.endswith(', 1>') and name.startswith('conv_igemm<'), name
    run_row(ctx, row, dt, 70 + 2 * sh + sw + dt, _geo_family(dt))


@pytest.mark.parametrize('dt', [0, 1])
def test_stride2_input_gradient_of_a_one_row_image(ctx, dt):
    """H < 2 at stride 2: the parity classes need two rows, the dilated gather serves the layer"""
    row = _geo((2, 16, 1, 9, 24, 3, 3, 2, 2, 1, 1), ('dgrad', 'dgrad +='), 1)
    for role in ('dgrad', 'dgrad +='):
        name = role_name(ctx, row, dt, role)
        assert name.endswith(', 1>') and not name.endswith(', 2>') and name.startswith('conv_igemm<'), name
    run_row(ctx, row, dt, 80 + dt, _geo_family(dt))


@pytest.mark.parametrize('dt', [0, 1])
def test_stride_above_2(ctx, dt):
    """alexnet's 11x11 / stride 4: forward and weight gradient within their bounds, the input gradient refused by the descriptor
    check before anything launches (null operands)"""
    row = _geo((1, 8, 23, 23, 16, 11, 11, 4, 4, 2, 2), ('fwd', 'wgrad'), 0)
    run_row(ctx, row, dt, 90 + dt, _geo_family(dt))
    d = row.desc(dt)
    with pytest.raises(RuntimeError, match='1 or 2 for the input gradient'):
        ctx.call('ifcbk_conv2d_dgrad', C.byref(d), None, None, None, 0, None)
