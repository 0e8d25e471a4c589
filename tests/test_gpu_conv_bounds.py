"""Conv kernels that had no case of their own, held to the per-element fp64 bound of tests/conv_bounds.py: the persistent conv_ws (one
tile per block, and more tiles than CUs so that blocks loop), every epilogue mode of conv_igemm (0 plain, 1 stride-2 input gradient,
2 parity class, 3 BN-backward sums, 4 segments) with Cw < C, N = 1 and M % 128 == 1, the weight-gradient kernels conv_wgrad_cols /
conv_wgrad_rows, ifcbk_conv2d_wgrad_segments (bf16 and fp32 kernels) and ifcbk_weight_pack_multi.  Each case asserts through
ifcbk_op_kernel which kernel ran.  test_conv_kernel_inventory lists every conv kernel family and mode the shipped library can name
and asserts that the bound-checked case tables reach each one, the fp32 modes and row tiles (table of test_gpu_conv_f32_bounds.py) included."""
import ctypes as C
import re

import pytest
import torch

import conv_bounds as cb
import test_gpu_conv as T0
import test_gpu_conv_forced as T1

pytestmark = pytest.mark.gpu

_bf = T1._bf
OFF = dict(IFCBK_CONV_BIG=0, IFCBK_CONV_FLAT=0, IFCBK_CONV_SLAB=0, IFCBK_CONV_PP3=0)      # per-launch switches: the other families off


def _desc(case, Cw=None, dtype=0):
    from ifcb_classifier_amd._lib import ConvDesc
    N, Cc, H, W, K, R, S, sh, sw, ph, pw = case
    P, Q = (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1
    return ConvDesc(N, H, W, Cc, Cc, K, R, S, sh, sw, ph, pw, P, Q, K, Cw or Cc, dtype)


def _operands(case, Cw, seed):
    """bf16-representable NCHW x (channels >= Cw zero, as the stem's padded input), KCRS w (zero past Cw), dy"""
    N, Cc, H, W, K, R, S, sh, sw, ph, pw = case
    d = _desc(case, Cw)
    g = torch.Generator().manual_seed(seed)
    x = _bf(torch.randn(N, Cc, H, W, generator=g))
    w = _bf(torch.randn(K, Cc, R, S, generator=g) / (d.Cw * R * S) ** 0.5)
    x[:, d.Cw:] = 0
    w[:, d.Cw:] = 0
    dy = _bf(torch.randn(N, K, d.P, d.Q, generator=g))
    return d, x, w, dy


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()


def _run_conv_case(ctx, case, Cw, want, seed=1):
    """forward (+ statistics), eval affine (+ residual + ReLU), input gradient (first writer, accumulate, BN-backward sums), each with
    the kernel named in `want` (role -> prefix; a role missing from `want` is not run)"""
    from ifcb_classifier_amd import _lib
    N, Cc, H, W, K, R, S, sh, sw, ph, pw = case
    d, x, w, dy = _operands(case, Cw, seed)
    P, Q = d.P, d.Q
    st = _lib.cur_stream()
    xd, dyd = _nhwc(x), _nhwc(dy)
    wk = w.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()
    wT = w.permute(1, 2, 3, 0).flip(1, 2).contiguous().to(torch.bfloat16).cuda()
    roles = {'fwd': (_lib.OP_CONV_FWD, 0, False), 'affine': (_lib.OP_CONV_FWD_AFFINE, 0, True), 'dgrad': (_lib.OP_CONV_DGRAD, 0, False),
             'dgrad +=': (_lib.OP_CONV_DGRAD, 1, False), 'bnstat': (_lib.OP_CONV_DGRAD_BNSTAT, 0, False)}
    names = {}
    for role, pre in want.items():
        kind, flags, res = roles[role]
        names[role] = cb.kname(ctx, d, kind, flags, res)
        assert re.match(pre, names[role]), (role, names[role], pre)
    fam = lambda role: cb.family_of(names[role], role)
    g = torch.Generator().manual_seed(seed + 100)
    if 'fwd' in want:
        fref = cb.fwd(x, w, (sh, sw), (ph, pw))
        y = torch.full((N, P, Q, K), float('nan'), dtype=torch.bfloat16, device='cuda')
        mb = ctx.lib.ifcbk_conv2d_fwd_mblocks(C.byref(d))
        part = torch.full((mb, 2, K), float('nan'), device='cuda')
        ctx.call('ifcbk_conv2d_fwd', C.byref(d), _lib.ptr(xd), _lib.ptr(wk), _lib.ptr(y), _lib.ptr(part), st)
        torch.cuda.synchronize()
        cb.check('fwd %s' % (case,), y, *fref, family=fam('fwd'))
        cb.check_bn_fwd_sums('fwd stats %s' % (case,), part, y, family='conv fwd statistics')
    if 'affine' in want:
        scale, shift = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
        res = _bf(torch.randn(N, P, Q, K, generator=g))
        scd, shd, resd = scale.cuda(), shift.cuda(), res.to(torch.bfloat16).cuda()
        y2 = torch.full((N, P, Q, K), float('nan'), dtype=torch.bfloat16, device='cuda')
        ctx.call('ifcbk_conv2d_fwd_affine', C.byref(d), _lib.ptr(xd), _lib.ptr(wk), _lib.ptr(y2), _lib.ptr(scd), _lib.ptr(shd),
                 _lib.ptr(resd), K, 1, st)
        torch.cuda.synchronize()
        cb.check_affine('affine+res %s' % (case,), y2, *fref, scale, shift, res, relu=True, family=fam('affine'))
    if 'dgrad' in want or 'dgrad +=' in want or 'bnstat' in want:
        dref = cb.dgrad(dy, w, x.shape, (sh, sw), (ph, pw))
        dims = ('n', 'h', 'w', 'c')
        dx = torch.full((N, H, W, Cc), float('nan'), dtype=torch.bfloat16, device='cuda')
        ctx.call('ifcbk_conv2d_dgrad', C.byref(d), _lib.ptr(dyd), _lib.ptr(wT), _lib.ptr(dx), 0, st)
        torch.cuda.synchronize()
        if 'dgrad' in want:
            cb.check('dgrad %s' % (case,), dx, *dref, dims=dims, family=fam('dgrad'))
        if 'dgrad +=' in want:
            old = _bf(torch.randn(N, H, W, Cc, generator=g))
            dxa = old.to(torch.bfloat16).cuda()
            ctx.call('ifcbk_conv2d_dgrad', C.byref(d), _lib.ptr(dyd), _lib.ptr(wT), _lib.ptr(dxa), 1, st)
            torch.cuda.synchronize()
            cb.check('dgrad += %s' % (case,), dxa, *dref, old=old, dims=dims, family=fam('dgrad +='))
        if 'bnstat' in want:
            raw = _bf(torch.randn(N, H, W, Cc, generator=g) * 1.5)
            mean, invstd = torch.randn(Cc, generator=g) * 0.2, torch.rand(Cc, generator=g) + 0.5
            bsc, bsh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
            nrow = ctx.lib.ifcbk_conv2d_dgrad_bnstat_mblocks(C.byref(d))
            assert nrow > 0
            part2 = torch.full((nrow, 2, Cc), float('nan'), device='cuda')
            dx3 = torch.full((N, H, W, Cc), float('nan'), dtype=torch.bfloat16, device='cuda')
            dev = [t.cuda() for t in (raw.to(torch.bfloat16), mean, invstd, bsc, bsh)]
            ctx.call('ifcbk_conv2d_dgrad_bnstat', C.byref(d), _lib.ptr(dyd), _lib.ptr(wT), _lib.ptr(dx3), _lib.ptr(dev[0]), Cc,
                     *[_lib.ptr(t) for t in dev[1:]], _lib.ptr(part2), st)
            torch.cuda.synchronize()
            cb.check('dgrad bnstat %s' % (case,), dx3, *dref, dims=dims, family=cb.family_of(names['bnstat'], 'dgrad bnstat'))
            cb.check_bn_bwd_sums('dgrad bnstat %s' % (case,), part2, dx3, raw, mean, invstd, bsc, bsh,
                                 family='conv dgrad BN-backward sums')
    return names


# ---------------------------------------------------------------------------------------------------- conv_ws
def _ws_cases():
    """3x3 / pad 1, 64 -> 64 channels (Kg = 576 both ways, one 64-channel column tile): 2 tiles, and 1.25 tiles per CU"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_loop = -(-160 * cus // 1600)                       # N * 40 * 40 pixels = cdiv(M, 128) in (CUs, 2 CUs]
    return [(1, 64, 12, 12, 64, 3, 3, 1, 1, 1, 1), (n_loop, 64, 40, 40, 64, 3, 3, 1, 1, 1, 1)], cus


@pytest.mark.parametrize('which', [0, 1])
def test_persistent_conv_ws(ctx, forced, which):
    forced(**OFF)
    cases, cus = _ws_cases()
    case = cases[which]
    M = case[0] * case[2] * case[3]
    tiles = -(-M // 128)
    assert (tiles <= cus) if which == 0 else (cus < tiles <= 2 * cus)
    names = _run_conv_case(ctx, case, None, {'fwd': r'conv_ws<', 'dgrad': r'conv_ws<',
                                             'affine': r'conv_igemm<unsigned short, \d, 2, 2, 0>',
                                             'dgrad +=': r'conv_igemm<unsigned short, \d, 2, 2, 0>'})
    assert ctx.lib.ifcbk_conv2d_fwd_mblocks(C.byref(_desc(case))) == 2 * tiles
    assert names['fwd'] == 'conv_ws<2>'


forced = T1.forced          # (the per-launch switch fixture of the forced tests)


# ---------------------------------------------------------------------------------------------------- conv_igemm, every mode
IGEMM = [
    # case, Cw, roles
    ((2, 8, 31, 31, 32, 3, 3, 2, 2, 0, 0), 3, {'fwd': r'conv_igemm<.*, 0>$', 'affine': r'conv_igemm<.*, 0>$',
                                               'dgrad': r'conv_igemm<.*, 2>$'}),            # stem-like: Cw = 3 of 8, stride 2
    ((1, 16, 35, 11, 48, 3, 3, 1, 1, 1, 1), None, {'fwd': r'conv_igemm<.*, 0>$', 'affine': r'conv_igemm<.*, 0>$',
                                                   'dgrad +=': r'conv_igemm<.*, 0>$', 'bnstat': r'conv_igemm<.*, 3>$'}),  # N = 1, M = 385
    ((1, 64, 9, 9, 96, 1, 1, 2, 2, 0, 0), None, {'fwd': r'conv_igemm<.*, 0>$', 'dgrad': r'conv_igemm<.*, 1>$',
                                                 'dgrad +=': r'conv_igemm<.*, 1>$'}),       # stride-2 1x1: MODE 1
    ((1, 24, 17, 17, 40, 3, 3, 2, 2, 0, 0), None, {'dgrad': r'conv_igemm<.*, 2>$', 'dgrad +=': r'conv_igemm<.*, 2>$'}),   # parity classes
    ((3, 40, 9, 10, 56, 3, 3, 2, 2, 1, 1), None, {'dgrad': r'conv_igemm<.*, 2>$'}),      # classes of 5 x 5 pixels, M tail
    ((2, 48, 11, 13, 72, 1, 7, 1, 1, 0, 3), None, {'bnstat': r'conv_igemm<.*, 3>$', 'dgrad +=': r'conv_igemm<.*, 0>$'}),
]


@pytest.mark.parametrize('case,Cw,want', IGEMM)
def test_igemm_epilogue_modes(ctx, forced, case, Cw, want):
    forced(**OFF)
    _run_conv_case(ctx, case, Cw, want, seed=sum(case))


def test_igemm_segments_mode4(ctx, forced):
    """MODE 4 of conv_igemm (the wide-tile kernel off): three segments, sizes off the 32-channel tile, M % 128 == 1"""
    from ifcb_classifier_amd import _lib
    forced(**OFF)
    case = (1, 64, 11, 35, 80, 1, 1, 1, 1, 0, 0)                      # M = 385
    d, x, w, dy = _operands(case, None, 7)
    N, P, Q, K = 1, d.P, d.Q, 80
    assert cb.kname(ctx, d, _lib.OP_CONV_FWD_AFFINE_SEG) .endswith(', 4>') and cb.kname(ctx, d, _lib.OP_CONV_FWD_AFFINE_SEG).startswith('conv_igemm<')
    fam = cb.family_of(cb.kname(ctx, d, _lib.OP_CONV_FWD_AFFINE_SEG), 'segments')
    g = torch.Generator().manual_seed(8)
    ksegs, lds, offs = [24, 40, 16], [40, 40, 16], [8, 0, 0]
    ys = [torch.full((N, P, Q, ld), float('nan'), dtype=torch.bfloat16, device='cuda') for ld in lds]
    ptrs = (C.c_void_p * 3)(*[y.data_ptr() + 2 * o for y, o in zip(ys, offs)])
    scale, shift = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
    scd, shd = scale.cuda(), shift.cuda()
    xd, wk = _nhwc(x), w.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()
    ctx.call('ifcbk_conv2d_fwd_affine_segments', C.byref(d), _lib.ptr(xd), _lib.ptr(wk), 3, ptrs, (C.c_int32 * 3)(*lds),
             (C.c_int32 * 3)(*ksegs), (C.c_int32 * 3)(0, 1, 1), _lib.ptr(scd), _lib.ptr(shd), _lib.cur_stream())
    torch.cuda.synchronize()
    ref, A, n = cb.fwd(x, w)
    cb.check('segment 0 (raw)', ys[0][..., 8:32], ref[..., :24], A[..., :24], n, family=fam)
    assert torch.isnan(ys[0][..., :8].float()).all() and torch.isnan(ys[0][..., 32:].float()).all()
    cb.check_affine('segment 1', ys[1], ref[..., 24:64], A[..., 24:64], n, scale[24:64], shift[24:64], relu=True, family=fam)
    cb.check_affine('segment 2', ys[2], ref[..., 64:], A[..., 64:], n, scale[64:], shift[64:], relu=True, family=fam)


# ---------------------------------------------------------------------------------------------------- weight gradients
WOFF = dict(IFCBK_WGRAD_PP=0, IFCBK_WGRAD_FLAT=0)
WG = [
    # case, Cw, kernel
    ((2, 48, 11, 11, 32, 3, 3, 1, 1, 1, 1), None, 'conv_wgrad_cols<1, 4>'),
    ((2, 8, 31, 31, 24, 3, 3, 2, 2, 0, 0), 3, 'conv_wgrad_cols<1, 4>'),       # stem-like: Cw = 3 of 8 (scalar reduce)
    ((3, 24, 10, 13, 64, 1, 7, 1, 1, 0, 3), None, 'conv_wgrad_cols<2, 4>'),
    ((2, 40, 9, 9, 96, 3, 3, 1, 1, 1, 1), None, 'conv_wgrad_rows<3>'),
    ((2, 24, 12, 12, 128, 3, 3, 2, 2, 1, 1), None, 'conv_wgrad_rows<4>'),
    ((1, 32, 14, 14, 200, 1, 1, 1, 1, 0, 0), None, 'conv_wgrad_rows<4>'),      # K tail: 200 = 128 + 72
]


@pytest.mark.parametrize('case,Cw,kname', WG)
def test_weight_gradient_kernels(ctx, forced, case, Cw, kname):
    from ifcb_classifier_amd import _lib
    forced(**WOFF)
    N, Cc, H, W, K, R, S, sh, sw, ph, pw = case
    d, x, w, dy = _operands(case, Cw, sum(case))
    assert cb.kname(ctx, d, _lib.OP_CONV_WGRAD) == kname, cb.kname(ctx, d, _lib.OP_CONV_WGRAD)
    st = _lib.cur_stream()
    xd, dyd = _nhwc(x), _nhwc(dy)
    ctx.reserve(ctx.lib.ifcbk_conv2d_wgrad_workspace(C.byref(d)))
    dw = torch.full((K, R, S, d.Cw), float('nan'), device='cuda')
    ctx.call('ifcbk_conv2d_wgrad', C.byref(d), _lib.ptr(xd), _lib.ptr(dyd), _lib.ptr(dw), 0, st)
    torch.cuda.synchronize()
    ref = cb.wgrad(x[:, :d.Cw], dy, (K, d.Cw, R, S), (sh, sw), (ph, pw))
    fam = kname.split(',')[0].rstrip('>') + '> wgrad'                 # conv_wgrad_cols<1> wgrad
    cb.check('wgrad %s' % (case,), dw, *ref, out='f32', dims=('k', 'r', 's', 'c'), family=fam)
    old = dw.clone()
    ctx.call('ifcbk_conv2d_wgrad', C.byref(d), _lib.ptr(xd), _lib.ptr(dyd), _lib.ptr(dw), 1, st)
    torch.cuda.synchronize()
    cb.check('wgrad += %s' % (case,), dw, *ref, old=old, out='f32', dims=('k', 'r', 's', 'c'), family=fam + ' +=')


SEGS = [((2, 24, 10, 10, 64, 3, 3, 1, 1, 1, 1), [24, 40], 4), ((2, 40, 9, 9, 96, 3, 3, 1, 1, 1, 1), [16, 56, 24], 5),
        ((2, 32, 9, 9, 200, 1, 1, 1, 1, 0, 0), [72, 128], 4)]


@pytest.mark.parametrize('dtype', [0, 1])
@pytest.mark.parametrize('case,ksegs,guard', SEGS)
@pytest.mark.parametrize('acc', [0, 1])
def test_wgrad_segments(ctx, forced, case, ksegs, guard, dtype, acc):
    """one weight-gradient GEMM whose K rows go to their own destinations; each dws[i] against its K slice of the fp64 gradient,
    NaN guards of `guard` floats around each destination (guard 5: misaligned destinations, the scalar reduce)"""
    from ifcb_classifier_amd import _lib
    forced(**WOFF)
    N, Cc, H, W, K, R, S, sh, sw, ph, pw = case
    d, x, w, dy = _operands(case, None, 3 + K)
    d.dtype = dtype
    name = cb.kname(ctx, d, _lib.OP_CONV_WGRAD_SEG)
    assert name.startswith('conv_wgrad_f32<' if dtype else 'conv_wgrad_'), name
    conv = (lambda t: t.permute(0, 2, 3, 1).contiguous().cuda()) if dtype else _nhwc
    xd, dyd = conv(x), conv(dy)
    ctx.reserve(ctx.lib.ifcbk_conv2d_wgrad_workspace(C.byref(d)))
    g = torch.Generator().manual_seed(K + acc)
    bufs, olds = [], []
    for ks in ksegs:
        b = torch.full((2 * guard + ks * R * S * Cc,), float('nan'))
        old = torch.randn(ks, R, S, Cc, generator=g)
        if acc:
            b[guard:-guard] = old.flatten()
        bufs.append(b.cuda())
        olds.append(old)
    ptrs = (C.c_void_p * len(ksegs))(*[b.data_ptr() + 4 * guard for b in bufs])
    ctx.call('ifcbk_conv2d_wgrad_segments', C.byref(d), _lib.ptr(xd), _lib.ptr(dyd), len(ksegs), ptrs,
             (C.c_int32 * len(ksegs))(*ksegs), acc, _lib.cur_stream())
    torch.cuda.synchronize()
    ref, A, n = cb.wgrad(x, dy, (K, Cc, R, S), (sh, sw), (ph, pw))
    k0 = 0
    for i, (ks, b) in enumerate(zip(ksegs, bufs)):
        bc = b.cpu()
        assert torch.isnan(bc[:guard]).all() and torch.isnan(bc[-guard:]).all(), 'segment %d wrote outside its tensor' % i
        got = bc[guard:-guard].reshape(ks, R, S, Cc)
        cb.check('wgrad segment %d of %s' % (i, ksegs), got, ref[k0:k0 + ks], A[k0:k0 + ks], n, out='f32', old=olds[i] if acc else None,
                 dims=('k', 'r', 's', 'c'), family=cb.family_of(name, 'wgrad segments' + (' +=' if acc else '')))
        k0 += ks


# ---------------------------------------------------------------------------------------------------- weight_pack_multi
# K, RS, C, Cw, fused (column offset in a shared 200-wide dgrad filter, or None)
PACK = [(40, 9, 24, 24, None), (72, 1, 48, 40, None), (56, 7, 16, 16, 64), (24, 7, 16, 16, 136), (8, 1, 8, 3, None)]


@pytest.mark.parametrize('dtype', [0, 1])
def test_weight_pack_multi(ctx, dtype):
    """the training step's bf16 / fp32 weight shadows: w and the flipped, transposed wT equal rne(master) bit for bit, padded channels
    are 0, the columns of a fused dgrad filter that belong to other convs keep their NaN sentinel; equal to ifcbk_weight_pack and to
    a CPU pack"""
    from ifcb_classifier_amd import _lib
    st = _lib.cur_stream()
    tdt = torch.float32 if dtype else torch.bfloat16
    g = torch.Generator().manual_seed(12 + dtype)
    items = (_lib.PackItem * len(PACK))()
    keep, fb = [], 0
    fusedT = torch.full((16, 7, 200), float('nan'), dtype=tdt, device='cuda')
    for i, (K, RS, Cc, Cw, col) in enumerate(PACK):
        m = torch.randn(K, RS, Cw, generator=g).cuda()
        wk = torch.full((K, RS, Cc), float('nan'), dtype=tdt, device='cuda')
        if col is None:
            wT = torch.full((Cc, RS, K), float('nan'), dtype=tdt, device='cuda')
            items[i].wT, items[i].wT_ld = wT.data_ptr(), 0
        else:
            wT = fusedT[..., col:col + K]
            items[i].wT, items[i].wT_ld = wT.data_ptr(), 200
        items[i].w_master, items[i].w = m.data_ptr(), wk.data_ptr()
        items[i].K, items[i].RS, items[i].C, items[i].Cw = K, RS, Cc, Cw
        items[i].first_block = fb
        fb += -(-K // 32) * RS * -(-Cc // 32)
        keep.append((m, wk, wT))
    dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    ctx.call('ifcbk_weight_pack_multi', _lib.ptr(dev), len(PACK), fb, dtype, st)
    torch.cuda.synchronize()
    fc = fusedT.float().cpu()
    for (K, RS, Cc, Cw, col), (m, wk, wT) in zip(PACK, keep):
        want = torch.zeros(K, RS, Cc, dtype=tdt)
        want[..., :Cw] = m.cpu().to(tdt)
        assert torch.equal(wk.cpu(), want)
        wantT = want.permute(2, 1, 0).flip(1)                  # [C][RS - 1 - rs][K]
        assert torch.equal(wT.cpu(), wantT)
        # against the single-conv pack (R = RS, S = 1)
        d = _desc((1, Cc, RS, 1, K, RS, 1, 1, 1, 0, 0), Cw, dtype)
        w1, wT1 = torch.empty(K, RS, Cc, dtype=tdt, device='cuda'), torch.empty(Cc, RS, K, dtype=tdt, device='cuda')
        ctx.call('ifcbk_weight_pack', C.byref(d), _lib.ptr(m), _lib.ptr(w1), _lib.ptr(wT1), st)
        torch.cuda.synchronize()
        assert torch.equal(w1, wk) and torch.equal(wT1.cpu(), wT.cpu())
    owned = torch.zeros(200, dtype=torch.bool)
    for K, RS, Cc, Cw, col in PACK:
        if col is not None:
            owned[col:col + K] = True
    assert torch.isnan(fc[..., ~owned]).all() and not torch.isnan(fc[..., owned]).any()


# ---------------------------------------------------------------------------------------------------- inventory
# every conv kernel family / epilogue mode ifcbk_op_kernel can name in the shipped library (IFCBK_CONV_WM=4 and the debug hooks are
# experiment-only forms and not listed).  A kernel added later without a bound-checked case fails test_conv_kernel_inventory.
INVENTORY = {
    'conv_igemm/0', 'conv_igemm/1', 'conv_igemm/2', 'conv_igemm/3', 'conv_igemm/4', 'conv_ws', 'conv_rows3x3',
    'conv_flat/0', 'conv_flat/3', 'conv_slab/0', 'conv_slab/3', 'conv_pp2/0', 'conv_pp2/3', 'conv_pp2/4', 'conv_pp3/0', 'conv_pp3/1',
    'conv_wgrad_pp', 'conv_wgrad_f32', 'conv_wgrad_flat', 'conv_wgrad_stem', 'conv_wgrad_cols<1>', 'conv_wgrad_cols<2>',
    'conv_wgrad_rows<3>', 'conv_wgrad_rows<4>', 'conv_wgrad_ppg', 'conv_wgrad_flatg',
}
# the fp32 parity mode: every epilogue mode of conv_igemm<float> and every row tile of conv_wgrad_f32, reached by the table of
# test_gpu_conv_f32_bounds.py (its names keep the element type; _key below drops it for the bf16 set above)
INVENTORY_F32 = {'conv_igemm<float>/0', 'conv_igemm<float>/1', 'conv_igemm<float>/2', 'conv_igemm<float>/3', 'conv_igemm<float>/4',
                 'conv_wgrad_f32<1>', 'conv_wgrad_f32<2>', 'conv_wgrad_f32<3>', 'conv_wgrad_f32<4>'}
# compared against fp64 or bit for bit against bound-checked kernels by their own tests (not rewritten here)
_STEM = 'test_gpu_stem_u8.py::test_stem_u8_kernels_vs_fp64_conv_of_the_three_affine_planes (conv_bounds.stem_u8_%s, per element)'
COUNTED = {'stem_u8_fwd_kernel': _STEM % 'fwd', 'stem_u8_fwd_mfma_kernel': _STEM % 'fwd', 'stem_u8_wgrad_kernel': _STEM % 'wgrad',
           'stem_u8_wgrad_mfma_kernel': _STEM % 'wgrad', 'stem_u8_wgrad_reduce_kernel': _STEM % 'wgrad',
           'conv_rows3x3/pool': 'test_gpu_conv_pool.py (bit-equal to conv_rows3x3 affine + max pool)'}


def _key(name):
    base = name.split('<')[0]
    args = [a.strip() for a in name[len(base) + 1:-1].split(',')] if '<' in name else []
    if base in ('conv_igemm', 'conv_flat', 'conv_slab', 'conv_pp2'):
        return '%s/%s' % (base, args[-1])
    if base == 'conv_pp3':
        return 'conv_pp3/%s' % args[3]
    if base in ('conv_wgrad_cols', 'conv_wgrad_rows'):
        return '%s<%s>' % (base, args[0])
    return base


def _key_f32(name):
    """'conv_igemm<float, 3, 2, 2, 4>' -> 'conv_igemm<float>/4'; 'conv_wgrad_f32<2>' stays"""
    if name.startswith('conv_igemm<float,'):
        return 'conv_igemm<float>/%s' % name[:-1].split(',')[-1].strip()
    return name


def _env(monkeypatch, env):
    for k in ('IFCBK_CONV_BIG', 'IFCBK_CONV_BIG_MT', 'IFCBK_CONV_BIG_TN', 'IFCBK_WGRAD_PP', 'IFCBK_WGRAD_PP_KH', 'IFCBK_CONV_FLAT',
              'IFCBK_CONV_PP3', 'IFCBK_CONV_PP3_GRID', 'IFCBK_CONV_SLAB', 'IFCBK_WGRAD_FLAT'):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))


def _names(ctx, monkeypatch, env, case, roles, Cw=None, dtype=0):
    from ifcb_classifier_amd import _lib
    _env(monkeypatch, env)
    d = _desc(case, Cw, dtype)
    kinds = {'fwd': (_lib.OP_CONV_FWD, 0, False), 'affine': (_lib.OP_CONV_FWD_AFFINE, 0, False),
             'affine+res': (_lib.OP_CONV_FWD_AFFINE, 0, True), 'dgrad': (_lib.OP_CONV_DGRAD, 0, False),
             'dgrad +=': (_lib.OP_CONV_DGRAD, 1, False), 'bnstat': (_lib.OP_CONV_DGRAD_BNSTAT, 0, False),
             'seg': (_lib.OP_CONV_FWD_AFFINE_SEG, 0, False), 'wgrad': (_lib.OP_CONV_WGRAD, 0, False)}
    return {_key(cb.kname(ctx, d, *kinds[r])) for r in roles}


def _group_names(ctx, monkeypatch, env, members):
    """members: (case, ldx padding, ldy padding) as the group tests build them"""
    from ifcb_classifier_amd import _lib
    _env(monkeypatch, env)
    n = len(members)
    items = (_lib.WgradItem * n)()
    for i, (c, lx, ly) in enumerate(members):
        d = _desc(c)
        d.ldx, d.ldy = d.C + lx, d.K + ly
        items[i].d = d
    op = _lib.Op()
    op.kind, op.p[0], op.i[0] = _lib.OP_CONV_WGRAD_GROUP, C.addressof(items), n
    buf = C.create_string_buffer(64)
    ctx.lib.ifcbk_op_kernel(C.byref(op), buf, 64)
    return {_key(buf.value.decode())}


def test_conv_kernel_inventory(ctx, monkeypatch):
    """the kernels the bound-checked case tables reach (computed with each table's own switches and roles) cover INVENTORY, and
    every name they reach is in INVENTORY or COUNTED"""
    seen = set()
    for case in T0.CASES:                                                       # test_conv_fwd_dgrad_wgrad: default plan
        seen |= _names(ctx, monkeypatch, {}, case, ('fwd', 'dgrad', 'dgrad +=', 'wgrad'))
    for case in T0.CASES[:10] + T0.CASES[12:14]:                                # test_conv_fp32_parity_mode
        seen |= _names(ctx, monkeypatch, {}, case, ('wgrad',), dtype=1)
    for case in [(2, 32, 20, 149, 32, 3, 3, 1, 1, 0, 0), (2, 32, 21, 19, 64, 3, 3, 1, 1, 1, 1), (2, 64, 19, 23, 32, 3, 3, 1, 1, 1, 1)]:
        seen |= _names(ctx, monkeypatch, {}, case, ('affine',))                  # test_row_streaming_kernel_affine_epilogue
    for case, mt, tn, lx, ly in T1.WIDE:
        env = dict(IFCBK_CONV_BIG=2, IFCBK_CONV_FLAT=0, IFCBK_CONV_PP3=0, IFCBK_CONV_SLAB=0)
        if mt:
            env.update(IFCBK_CONV_BIG_MT=mt, IFCBK_CONV_BIG_TN=tn)
        seen |= _names(ctx, monkeypatch, env, case, ('fwd', 'affine+res') + (('dgrad', 'bnstat') if case[7] == 1 else ()))
    seen |= _names(ctx, monkeypatch, dict(IFCBK_CONV_BIG=2, IFCBK_CONV_BIG_MT=8, IFCBK_CONV_BIG_TN=3, IFCBK_CONV_FLAT=0, IFCBK_CONV_SLAB=0),
                   (3, 168, 13, 11, 152, 1, 1, 1, 1, 0, 0), ('seg',))          # test_wide_tile_segmented_epilogue
    for case, lx, ly in T1.SLAB:
        seen |= _names(ctx, monkeypatch, dict(IFCBK_CONV_SLAB=2, IFCBK_CONV_BIG=0, IFCBK_CONV_FLAT=0, IFCBK_CONV_PP3=0), case,
                       ('fwd', 'affine+res', 'dgrad', 'bnstat'))
    for case, grid, lx, ly in T1.PP3:
        env = dict(IFCBK_CONV_PP3=2, IFCBK_CONV_FLAT=0, IFCBK_CONV_BIG=0, IFCBK_CONV_SLAB=0)
        seen |= _names(ctx, monkeypatch, env, case, ('fwd', 'affine') + (('dgrad',) if case[7] == 1 else ()))
    for case, lx, ly in T1.FLAT:
        N, Cc, H, W, K, R, S, ph, pw = case
        full = (N, Cc, H, W, K, R, S, 1, 1, ph, pw)
        seen |= _names(ctx, monkeypatch, dict(IFCBK_CONV_FLAT=2, IFCBK_CONV_BIG=0), full,
                       (('fwd', 'affine') if (Cc, K, R) != (48, 64, 5) else ()) + ('dgrad', 'bnstat'))
    for case, kh, lx, ly in T1.WGRAD:
        seen |= _names(ctx, monkeypatch, dict(IFCBK_WGRAD_PP=2, IFCBK_WGRAD_PP_KH=kh), case, ('wgrad',))
    for case, lx, ly in T1.WFLAT:
        seen |= _names(ctx, monkeypatch, dict(IFCBK_WGRAD_FLAT=2), case, ('wgrad',))
    seen |= _group_names(ctx, monkeypatch, dict(IFCBK_WGRAD_FLAT=2, IFCBK_WGRAD_PP=2),
                         [((6, 48, 15, 15, 64, 5, 5, 1, 1, 2, 2), 0, 0), ((6, 64, 15, 15, 96, 3, 3, 1, 1, 1, 1), 0, 0),
                          ((6, 96, 15, 15, 96, 3, 3, 1, 1, 1, 1), 0, 0)])
    for kh, members in T1.WGROUPS:
        seen |= _group_names(ctx, monkeypatch, dict(IFCBK_WGRAD_PP=2, IFCBK_WGRAD_PP_KH=kh), members)
    for case, Cw, want in IGEMM:                                                # this file
        seen |= _names(ctx, monkeypatch, OFF, case, tuple(r if r != 'affine' else 'affine+res' for r in want), Cw)
    for case in _ws_cases()[0]:
        seen |= _names(ctx, monkeypatch, OFF, case, ('fwd', 'dgrad', 'affine+res', 'dgrad +='))
    seen |= _names(ctx, monkeypatch, OFF, (1, 64, 11, 35, 80, 1, 1, 1, 1, 0, 0), ('seg',))
    for case, Cw, kname in WG:
        seen |= _names(ctx, monkeypatch, WOFF, case, ('wgrad',), Cw)
    missing = INVENTORY - seen
    assert not missing, 'conv kernels without a bound-checked case: %s' % sorted(missing)
    unknown = seen - INVENTORY - set(COUNTED)
    assert not unknown, 'kernels reached by the case tables but missing from INVENTORY: %s' % sorted(unknown)
    import test_gpu_conv_f32_bounds as T2
    _env(monkeypatch, T2.OFF)
    seen32 = {_key_f32(n) for n in T2.f32_names(ctx)}
    missing = INVENTORY_F32 - seen32
    assert not missing, 'fp32 conv kernels without a bound-checked case: %s' % sorted(missing)
    unknown = seen32 - INVENTORY_F32
    assert not unknown, 'kernels reached by the fp32 table but missing from INVENTORY_F32: %s' % sorted(unknown)
