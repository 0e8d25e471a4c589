"""Every kernel of bn.hip, pool_head.hip and plain.hip against a float64 reference of the same operation, element by element, under
the bounds derived in tests/op_bounds.py (its docstring is the specification).  The C ABI is called through ctx.call; every
destination -- the padding channels of a wide-stride tensor included -- is filled with NaN first, and afterwards everything outside
the C channels must still be NaN and everything inside finite: a write outside the slice or a chunk never written shows at any stride.

The case tables are module-level lists: tests/test_op_inventory_cpu.py reads them and the KERNELS table at the end (kernel ->
the cases that reach it and the dispatch condition, quoted from the source).

Out of scope: the 32-bit index paths (fdiv near 2^31, the `total >= 2^31` guards); nothing here needs more than a few hundred MB.
IFCBK_BN_BWD_ROWS is cached by the library on first use: the row tiles of bn_bwd are reached by shape."""
import ctypes as C
import os

import pytest
import torch

import op_bounds as ob

pytestmark = pytest.mark.gpu
NAN = float('nan')
TD = {0: torch.bfloat16, 1: torch.float32}
OUT = {0: 'bf16', 1: 'f32'}
CH = {0: 8, 1: 4}


def _lib():
    from ifcb_classifier_amd import _lib
    return _lib


def rt(shape, gen, dt, scale=1.0, shift=0.0):
    """random values representable in the storage type (CPU, float32)"""
    return (torch.randn(shape, generator=gen) * scale + shift).to(TD[dt]).float()


def wbuf(rows, Cc, ld, dt, data=None, off=0):
    """a NaN-filled [rows..., ld] device tensor of the storage type holding `data` in channels [off, off + Cc)"""
    buf = torch.full(tuple(rows) + (ld,), NAN, dtype=TD[dt], device='cuda')
    if data is not None:
        buf[..., off:off + Cc] = data.to(TD[dt]).cuda()
    return buf


def guard(name, buf, Cc, off=0, allow_nan=False):
    """nothing written outside the Cc channels, everything inside written"""
    assert torch.isnan(buf[..., :off]).all() and torch.isnan(buf[..., off + Cc:]).all(), name + ': wrote outside its channels'
    if not allow_nan:
        assert torch.isfinite(buf[..., off:off + Cc].float()).all(), name + ': unwritten or non-finite element inside'


def fvec(*shape, gen=None, fn=torch.randn, scale=1.0, shift=0.0):
    return fn(*shape, generator=gen) * scale + shift


def nanvec(n):
    return torch.full((n,), NAN, device='cuda')


def P(t):
    return _lib().ptr(t)


def st():
    return _lib().cur_stream()


def sync():
    torch.cuda.synchronize()


# ====================================================================================================== bn_apply
# (M, C, ldx, ldy, ldr, dtype, relu, res): chunks M * C / E of 1, 2048 +- 1 (a block handles 256 * EW_ITER chunks), a few times 2048
BN_APPLY = [
    (1, 8, 8, 8, 8, 0, 1, 0), (1, 4, 4, 12, 4, 1, 0, 1), (2047, 8, 16, 8, 8, 0, 1, 1), (2048, 8, 8, 24, 16, 0, 0, 0),
    (2049, 8, 8, 8, 8, 0, 0, 1), (2047, 4, 4, 8, 4, 1, 1, 0), (2049, 4, 8, 4, 12, 1, 1, 1), (700, 96, 160, 128, 104, 0, 1, 1),
    (700, 96, 160, 128, 104, 1, 1, 0), (5, 2048, 2048, 2056, 2048, 0, 1, 0), (3, 2048, 2052, 2048, 2048, 1, 0, 1),
    (513, 16, 16, 16, 16, 1, 1, 1), (333, 200, 200, 208, 200, 0, 0, 1), (900, 24, 24, 24, 24, 0, 0, 0),
]


@pytest.mark.parametrize('case', BN_APPLY, ids=str)
def test_bn_apply(ctx, case):
    M, Cc, ldx, ldy, ldr, dt, relu, res = case
    L = _lib()
    g = torch.Generator().manual_seed(M + Cc)
    x = rt((M, Cc), g, dt, 2.0, 0.5)
    r = rt((M, Cc), g, dt) if res else None
    s, b = fvec(Cc, gen=g, scale=0.7), fvec(Cc, gen=g, scale=0.3)
    xd, rd, yd = wbuf((M,), Cc, ldx, dt, x), (wbuf((M,), Cc, ldr, dt, r) if res else None), wbuf((M,), Cc, ldy, dt)
    sd, bd = s.cuda(), b.cuda()
    d = L.BnDesc(M, Cc, ldx, ldy, relu, dt, 1e-3, 0.1)
    ctx.call('ifcbk_bn_apply', C.byref(d), P(xd), P(sd), P(bd), P(rd), ldr, P(yd), st())
    sync()
    guard('bn_apply', yd, Cc)
    want, e = ob.affine(x, s, b, r, bool(relu))
    ob.elem('bn_apply %s' % (case,), yd[..., :Cc], want, e, OUT[dt], 'bn_apply', dims=('m', 'c'))


# ====================================================================================================== bn_finalize
# (rows, C, part_ld (0: C), |mean| / std, M == 1)
_FIN_ROWS = [1, 63, 64, 65, 255, 256, 257, 1536, 1537, 5003]
FINALIZE = [(r, [8, 16, 24, 200][i % 4], (0 if i % 3 else [8, 16, 24, 200][i % 4] + 16), [0, 10, 100][i % 3], 0) for i, r in enumerate(_FIN_ROWS)] + \
           [(1537, 8, 0, 100, 0), (5003, 24, 40, 100, 0), (1, 16, 0, 10, 1), (1536, 200, 0, 0, 0), (1537, 200, 216, 10, 0), (257, 16, 0, 100, 0)]


_VAR_REL = {}


def _synthetic_rows(rows, Cc, ratio, g, one):
    if one:
        x = torch.randn(1, Cc, generator=g) + ratio
        return torch.stack([x, x * x], 1).float(), 1
    m = ratio + torch.randn(rows, Cc, generator=g) * 0.09
    v = 1 + 0.1 * torch.randn(rows, Cc, generator=g)
    return torch.stack([128 * m, 128 * (v + m * m)], 1).float(), rows * 128


@pytest.mark.parametrize('case', FINALIZE, ids=str)
def test_bn_finalize(ctx, case):
    from conftest import MEASURED
    rows, Cc, pld, ratio, one = case
    L = _lib()
    g = torch.Generator().manual_seed(rows + Cc)
    part, M = _synthetic_rows(rows, Cc, ratio, g, one)
    ld = pld or Cc
    if pld:
        pd = torch.full((rows, 2, ld), NAN, device='cuda')             # this BatchNorm's columns inside a wider matrix
        pd[..., 8:8 + Cc] = part.cuda()
    else:
        pd = part.cuda().contiguous()
    gam, bet = fvec(Cc, gen=g, fn=torch.rand, shift=0.5), fvec(Cc, gen=g)
    rm, rv = fvec(Cc, gen=g), fvec(Cc, gen=g, fn=torch.rand, shift=0.5)
    outs = {k: nanvec(Cc) for k in ('mean', 'invstd', 'scale', 'shift')}
    rmd, rvd, gd, bd = rm.cuda(), rv.cuda(), gam.cuda(), bet.cuda()
    d = L.BnDesc(M, Cc, Cc, Cc, 1, 0, 1e-3, 0.1)
    src = pd[..., 8:] if pld else pd
    if pld:
        ctx.call('ifcbk_bn_finalize_ld', C.byref(d), P(src), rows, ld, P(gd), P(bd), P(rmd), P(rvd),
                 *[P(outs[k]) for k in ('mean', 'invstd', 'scale', 'shift')], st())
    else:
        ctx.call('ifcbk_bn_finalize', C.byref(d), P(src), rows, P(gd), P(bd), P(rmd), P(rvd),
                 *[P(outs[k]) for k in ('mean', 'invstd', 'scale', 'shift')], st())
    sync()
    want = ob.finalize(part, M, 1e-3, 0.1, gam, bet, rm, rv)
    got = dict(outs, running_mean=rmd, running_var=rvd)
    ob.check_finalize('bn_finalize %s' % (case,), got, want, family='bn_finalize' + (' (prereduce)' if rows > 1536 else ''))
    # the variance the kernel used, recovered from invstd: its error over its bound, and relative to the variance
    var, e_var = want['var']
    e_from = (e_var + 4 * ob.U * (var + ob.f32(1e-3))) * (1 + 1e-5)
    v_got = 1 / outs['invstd'].double().cpu() ** 2 - ob.f32(1e-3)
    r = ob.elem('variance', v_got, var, e_from, 'f32', 'bn_finalize variance at |mean|/std = %d' % ratio, dims=('channel',))
    if not one:
        rel = float(((v_got - var).abs() / var).max())
        row = _VAR_REL.setdefault(ratio, [0.0, len(MEASURED)])
        if row[0] == 0.0:
            MEASURED.append('')
        row[0] = max(row[0], rel, 1e-300)
        MEASURED[row[1]] = 'op bound bn_finalize: worst variance error relative to the variance at |mean|/std = %d: %.2e' % (ratio, row[0])
    assert r.ratio <= 1.0


def test_bn_finalize_eval(ctx):
    L = _lib()
    g = torch.Generator().manual_seed(1)
    for Cc in (8, 40, 300):
        gam, bet = fvec(Cc, gen=g, fn=torch.rand, shift=0.5), fvec(Cc, gen=g)
        rm, rv = fvec(Cc, gen=g), fvec(Cc, gen=g, fn=torch.rand, shift=0.1)
        sc, sh = nanvec(Cc), nanvec(Cc)
        gd, bd, rmd, rvd = gam.cuda(), bet.cuda(), rm.cuda(), rv.cuda()
        d = L.BnDesc(10, Cc, Cc, Cc, 1, 0, 1e-5, 0.1)
        ctx.call('ifcbk_bn_finalize', C.byref(d), None, 0, P(gd), P(bd), P(rmd), P(rvd), None, None, P(sc), P(sh), st())
        sync()
        ob.check_finalize('bn_finalize eval C=%d' % Cc, {'scale': sc, 'shift': sh}, ob.finalize_eval(1e-5, gam, bet, rm, rv), family='bn_finalize (eval)')
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv)


# ====================================================================================================== bn_stats
# (M, C, ld, channel offset, dtype)
STATS = [(1, 8, 8, 0, 0), (1023, 16, 48, 16, 0), (1024, 32, 32, 0, 1), (1025, 8, 24, 8, 0), (3333, 72, 288, 64, 0), (2501, 36, 64, 12, 1),
         (5, 4, 4, 0, 1)]


@pytest.mark.parametrize('case', STATS, ids=str)
def test_bn_stats(ctx, case):
    M, Cc, ld, off, dt = case
    L = _lib()
    g = torch.Generator().manual_seed(M + Cc)
    x = rt((M, Cc), g, dt, 1.5, 0.3)
    xd = wbuf((M,), Cc, ld, dt, x, off)
    rows = ctx.lib.ifcbk_bn_stats_rows(M)
    assert rows == (M + 1023) // 1024
    part = torch.full((rows + 1, 2, Cc), NAN, device='cuda')
    d = L.BnDesc(M, Cc, ld, ld, 1, dt, 1e-3, 0.1)
    ctx.call('ifcbk_bn_stats', C.byref(d), P(xd[..., off:]), P(part), st())
    sync()
    assert torch.isfinite(part[:rows]).all() and torch.isnan(part[rows]).all()
    ob.check_stats('bn_stats %s' % (case,), part[:rows], x, family='bn_stats')


# ====================================================================================================== bn_bwd
def bwd_rows(M, Cc, dt):
    """bn.hip bwd_rows(): rows per fp32 tile of the reduction pass"""
    assert 'IFCBK_BN_BWD_ROWS' not in os.environ
    cg = -(-Cc // (8 * CH[dt]))
    r = (M * cg // 3000 + 31) // 32 * 32
    return min(max(r, 256), 1024)


# (M, C, ldx, lddy, lddx, lddres, dtype, mode, dres_accumulate, param_accumulate, dy aliases dx)
# mode: 'y' = mask from y, with residual gradient; 'x' = mask recomputed from x * scale + shift; 'none' = no ReLU
BN_BWD = [
    (324, 32, 32, 32, 32, 32, 0, 'y', 0, 0, 0), (324, 32, 48, 40, 64, 56, 0, 'y', 1, 1, 0), (105, 96, 160, 96, 104, 96, 0, 'y', 2, 0, 0),
    (105, 96, 96, 128, 128, 112, 0, 'y', 3, 1, 1), (1300, 16, 16, 16, 16, 16, 0, 'x', 0, 0, 1), (1300, 16, 24, 32, 40, 16, 0, 'x', 2, 1, 0),
    (777, 64, 64, 64, 72, 64, 0, 'none', 0, 0, 0), (777, 64, 64, 64, 64, 64, 0, 'none', 2, 1, 0), (513, 20, 20, 24, 28, 32, 1, 'y', 1, 0, 0),
    (513, 20, 24, 20, 20, 20, 1, 'x', 0, 1, 0), (300, 12, 12, 12, 16, 12, 1, 'none', 3, 0, 0), (1, 8, 8, 8, 8, 8, 0, 'x', 0, 0, 0),
    (97001, 256, 256, 256, 256, 256, 1, 'x', 0, 0, 0),          # bwd_rows 288
    (30001, 3200, 3200, 3200, 3200, 3200, 1, 'x', 0, 1, 0),     # bwd_rows 1024
]


def _slabs(Cc, E):
    w = 8 * E
    if Cc <= 64:
        return [(0, Cc)]
    return sorted({(0, w), ((Cc // 2) // w * w, (Cc // 2) // w * w + w), (Cc - w, Cc)})


@pytest.mark.parametrize('case', BN_BWD, ids=str)
def test_bn_bwd(ctx, case):
    M, Cc, ldx, lddy, lddx, lddres, dt, mode, dacc, pacc, alias = case
    L = _lib()
    out = OUT[dt]
    gd = torch.Generator(device='cuda').manual_seed(M + Cc)
    g = torch.Generator().manual_seed(M + Cc)
    mk = lambda ld, sc=1.0, sh=0.0: torch.cat([(torch.randn(M, Cc, generator=gd, device='cuda') * sc + sh).to(TD[dt]),
                                               torch.full((M, ld - Cc), NAN, dtype=TD[dt], device='cuda')], 1)
    if alias:
        lddy = lddx
    xd = mk(ldx, 2.0, 0.5)
    dyd = mk(lddy)
    gam = fvec(Cc, gen=g, fn=torch.rand, shift=0.5)
    xs = xd[:, :Cc].float()
    mean = xs.mean(0).cpu() if M > 1 else torch.zeros(Cc)
    invstd = (1 / torch.sqrt(xs.var(0, unbiased=False) + 1e-3)).cpu() if M > 1 else torch.ones(Cc)
    scale = gam * invstd
    shift = fvec(Cc, gen=g, scale=0.2) - mean * scale
    relu = 0 if mode == 'none' else 1
    yd = None
    if mode == 'y':
        yd = torch.cat([(xs * scale.cuda() + shift.cuda() + torch.randn(M, Cc, generator=gd, device='cuda')).clamp_min(0).to(TD[dt]),
                        torch.full((M, ldx - Cc), NAN, dtype=TD[dt], device='cuda')], 1)
    dxd = dyd if alias else (mk(lddx) if dacc & 2 else wbuf((M,), Cc, lddx, dt))
    dresd = (mk(lddres) if dacc & 1 else wbuf((M,), Cc, lddres, dt)) if mode == 'y' else None
    old_dx = dxd[:, :Cc].clone() if dacc & 2 else None
    old_dres = dresd[:, :Cc].clone() if (dresd is not None and dacc & 1) else None
    dy_keep = dyd[:, :Cc].clone()
    old_dg, old_db = fvec(Cc, gen=g, scale=3.0), fvec(Cc, gen=g, scale=3.0)
    dgd, dbd = (old_dg.cuda(), old_db.cuda()) if pacc else (nanvec(Cc), nanvec(Cc))
    dev = [t.cuda() for t in (gam, mean, invstd, scale, shift)]
    d = L.BnDesc(M, Cc, ldx, ldx, relu, dt, 1e-3, 0.1)
    ctx.call('ifcbk_bn_bwd', C.byref(d), P(xd), P(yd), P(dyd), lddy, P(dev[0]), P(dev[1]), P(dev[2]), P(dxd), lddx, P(dresd), lddres,
             dacc, P(dgd), P(dbd), pacc, P(dev[3]) if mode == 'x' else None, P(dev[4]) if mode == 'x' else None, st())
    sync()
    guard('bn_bwd dx', dxd, Cc)
    if dresd is not None:
        guard('bn_bwd dres', dresd, Cc)
    assert torch.isfinite(dgd).all() and torch.isfinite(dbd).all()
    rows = bwd_rows(M, Cc, dt)
    name = 'bn_bwd %s' % (case,)
    fam = 'bn_bwd (row tile %d)' % rows
    for c0, c1 in _slabs(Cc, CH[dt]):
        sl = slice(c0, c1)
        ref = ob.BnBwd(xd[:, sl], dy_keep[:, sl], gam[sl], mean[sl], invstd[sl], {'none': 0, 'y': 1, 'x': 2}[mode],
                       y=None if yd is None else yd[:, sl], scale=scale[sl], shift=shift[sl], tile=rows)
        ref.check_params(name, dgd[sl], dbd[sl], old_dg[sl] if pacc else None, old_db[sl] if pacc else None, family=fam)
        ref.check_dx(name, dxd[:, sl], out, old=None if old_dx is None else old_dx[:, sl], family=fam)
        if dresd is not None:
            ref.check_dres(name, dresd[:, sl], out, old=None if old_dres is None else old_dres[:, sl], family=fam)


# (M, C, part_ld, column offset, dtype, lddx, param_accumulate)
BN_BWD_PARTIALS = [(700, 32, 96, 32, 0, 40, 0), (1000, 16, 16, 0, 0, 16, 1), (650, 24, 64, 8, 1, 24, 1)]


@pytest.mark.parametrize('case', BN_BWD_PARTIALS, ids=str)
def test_bn_bwd_partials_ld(ctx, case):
    M, Cc, pld, off, dt, lddx, pacc = case
    L = _lib()
    g = torch.Generator().manual_seed(M)
    x, dy = rt((M, Cc), g, dt, 2.0, 0.5), rt((M, Cc), g, dt)
    gam = fvec(Cc, gen=g, fn=torch.rand, shift=0.5)
    mean, invstd = x.mean(0), 1 / torch.sqrt(x.var(0, unbiased=False) + 1e-3)
    scale = gam * invstd
    shift = fvec(Cc, gen=g, scale=0.2) - mean * scale
    ref = ob.BnBwd(x, dy, gam, mean, invstd, 2, scale=scale, shift=shift)
    nt = (M + 127) // 128                                 # synthetic partial rows: 128-row tiles of the reference's own terms, as fp32
    part = torch.stack([torch.stack([ref.dz[i * 128:(i + 1) * 128].sum(0), (ref.dz * ref.xhat)[i * 128:(i + 1) * 128].sum(0)]) for i in range(nt)]).float()
    ref.use_partials(part)
    pd = torch.full((nt, 2, pld), NAN, device='cuda')
    pd[..., off:off + Cc] = part.cuda()
    xd, dyd, dxd = wbuf((M,), Cc, Cc, dt, x), wbuf((M,), Cc, Cc, dt, dy), wbuf((M,), Cc, lddx, dt)
    old_dg, old_db = fvec(Cc, gen=g), fvec(Cc, gen=g)
    dgd, dbd = (old_dg.cuda(), old_db.cuda()) if pacc else (nanvec(Cc), nanvec(Cc))
    dev = [t.cuda() for t in (gam, mean, invstd, scale, shift)]
    d = L.BnDesc(M, Cc, Cc, Cc, 1, dt, 1e-3, 0.1)
    args = [C.byref(d), P(xd), P(dyd), Cc] + [P(t) for t in dev] + [P(pd[..., off:]), nt]
    tail = [P(dxd), lddx, P(dgd), P(dbd), pacc, st()]
    if pld == Cc:
        ctx.call('ifcbk_bn_bwd_partials', *args, *tail)
    else:
        ctx.call('ifcbk_bn_bwd_partials_ld', *args, pld, *tail)
    sync()
    guard('bn_bwd_partials dx', dxd, Cc)
    ref.check_partial_params('bn_bwd_partials %s' % (case,), dgd, dbd, old_dg if pacc else None, old_db if pacc else None, family='bn_bwd_partials')
    ref.check_dx('bn_bwd_partials %s' % (case,), dxd[:, :Cc], OUT[dt], family='bn_bwd_partials')


# ====================================================================================================== pools
def pool_desc(N, H, W, Cc, ldx, ldy, R, S, sh, ph, dt, ceil=False):
    g = ob.Geo(H, W, R, S, sh, sh, ph, ph)
    if ceil:
        g = ob.Geo(H, W, R, S, sh, sh, ph, ph, -(-(H + 2 * ph - R) // sh) + 1, -(-(W + 2 * ph - S) // sh) + 1)
        assert (g.P - 1) * sh < H + ph and (g.Q - 1) * sh < W + ph
    return _lib().PoolDesc(N, H, W, Cc, ldx, R, S, sh, sh, ph, ph, g.P, g.Q, ldy, dt), g


# (N, H, W, C, ld of the raw tensor, ld of the pooled tensor, lddx, pad, dtype, ceil mode, param_accumulate, relu)
POOLED = [
    (2, 15, 13, 32, 32, 32, 32, 0, 0, 0, 0, 1), (2, 14, 11, 16, 24, 32, 40, 0, 0, 0, 1, 1), (1, 9, 12, 16, 16, 16, 24, 1, 0, 0, 1, 1),
    (2, 12, 9, 8, 16, 8, 8, 1, 1, 0, 0, 1), (2, 8, 10, 16, 16, 24, 16, 0, 0, 1, 0, 1), (1, 10, 8, 8, 8, 8, 12, 0, 1, 1, 1, 0),
    (3, 7, 7, 24, 24, 24, 24, 0, 1, 0, 0, 0), (2, 16, 10, 64, 64, 64, 64, 1, 0, 0, 0, 0), (1, 37, 36, 64, 64, 64, 64, 0, 0, 0, 0, 1),
]


@pytest.mark.parametrize('case', POOLED, ids=str)
def test_bn_apply_maxpool_and_bn_bwd_maxpool(ctx, case):
    N, H, W, Cc, ldx, ldy, lddx, pad, dt, ceil, pacc, relu = case
    L = _lib()
    out = OUT[dt]
    pd, geo = pool_desc(N, H, W, Cc, ldx, ldy, 3, 3, 2, pad, dt, ceil)
    g = torch.Generator().manual_seed(H * 100 + W + Cc)
    x = rt((N, H, W, Cc), g, dt, 2.0, 0.3)
    s, b = fvec(Cc, gen=g, scale=0.7), fvec(Cc, gen=g, scale=0.3)                 # negative scales too
    xd, sd, bd = wbuf((N, H, W), Cc, ldx, dt, x), s.cuda(), b.cuda()
    yd = wbuf((N, geo.P, geo.Q), Cc, ldy, dt)
    arg = torch.full((N, geo.P, geo.Q, Cc), 255, dtype=torch.uint8, device='cuda')
    ctx.call('ifcbk_bn_apply_maxpool', C.byref(pd), P(xd), P(sd), P(bd), relu, P(yd), P(arg), st())
    # the unfused pair on the same input: bit for bit
    bnd = L.BnDesc(N * H * W, Cc, ldx, Cc, relu, dt, 1e-3, 0.1)
    act = wbuf((N, H, W), Cc, Cc, dt)
    pd2, _ = pool_desc(N, H, W, Cc, Cc, ldy, 3, 3, 2, pad, dt, ceil)
    y2, arg2 = wbuf((N, geo.P, geo.Q), Cc, ldy, dt), torch.full_like(arg, 255)
    ctx.call('ifcbk_bn_apply', C.byref(bnd), P(xd), P(sd), P(bd), None, 0, P(act), st())
    ctx.call('ifcbk_maxpool_fwd', C.byref(pd2), P(act), P(y2), P(arg2), st())
    sync()
    guard('bn_apply_maxpool', yd, Cc)
    assert int(arg.max()) < 9
    assert torch.equal(yd[..., :Cc], y2[..., :Cc]) and torch.equal(arg, arg2)
    # values: the max of the reference activations, within the largest bound of the window (max is 1-Lipschitz); arg-max: a valid
    # tap whose reference activation is within that bound of the maximum
    a_ref, e_a = ob.affine(x, s, b, None, bool(relu))
    e_a = e_a + 0.5 * ob.ulp(a_ref.abs() + e_a, out)
    vals, errs = [], []
    for r in range(3):
        for q in range(3):
            v, ok = geo.gather(a_ref, r, q)
            ee, _ = geo.gather(e_a, r, q)
            okb = ok[None, :, :, None].expand_as(v)
            vals.append(torch.where(okb, v, torch.full_like(v, -float('inf'))))
            errs.append(torch.where(okb, ee, torch.zeros_like(ee)))
    vals, errs = torch.stack(vals), torch.stack(errs)
    want, e = vals.max(0).values, errs.max(0).values
    ob.elem('bn_apply_maxpool %s' % (case,), yd[..., :Cc], want, e, out, 'bn_apply_maxpool', dims=('n', 'p', 'q', 'c'))
    at = torch.gather(vals, 0, arg.cpu().long()[None])[0]
    assert (at >= want - 2 * e).all(), 'arg-max names a tap that is not a maximum'
    # the exact rule on the kernel's own activations
    yr, ar = ob.maxpool_fwd(act[..., :Cc], geo)
    ob.exact('bn_apply_maxpool values', yd[..., :Cc], yr, 'bn_apply_maxpool')
    ob.exact('bn_apply_maxpool arg-max', arg, ar, 'bn_apply_maxpool')
    # ---- backward through the pool
    dpool = rt((N, geo.P, geo.Q, Cc), g, dt)
    dpd = wbuf((N, geo.P, geo.Q), Cc, ldy, dt, dpool)
    gam = fvec(Cc, gen=g, fn=torch.rand, shift=0.5)
    mean, invstd = fvec(Cc, gen=g, scale=0.2), fvec(Cc, gen=g, fn=torch.rand, shift=0.5)
    dxd = wbuf((N, H, W), Cc, lddx, dt)
    old_dg, old_db = fvec(Cc, gen=g), fvec(Cc, gen=g)
    dgd, dbd = (old_dg.cuda(), old_db.cuda()) if pacc else (nanvec(Cc), nanvec(Cc))
    dev = [t.cuda() for t in (gam, mean, invstd)]
    ctx.call('ifcbk_bn_bwd_maxpool', C.byref(pd), P(xd), P(dpd), P(arg), P(dev[0]), P(dev[1]), P(dev[2]), P(sd), P(bd), relu, P(dxd), lddx,
             P(dgd), P(dbd), pacc, st())
    sync()
    guard('bn_bwd_maxpool dx', dxd, Cc)
    dy, A, _ = ob.maxpool_bwd(dpool, arg, geo, N, Cc)
    M = N * H * W
    rows = 1024 if pad == 0 else bwd_rows(M, Cc, dt)        # 2x2 blocks: 256 blocks of 4 pixels per partial row
    ref = ob.BnBwd(x.reshape(M, Cc), dy.reshape(M, Cc), gam, mean, invstd, 2 if relu else 0, scale=s, shift=b,
                   dz_abs=A.reshape(M, Cc), dz_ops=3, tile=rows)
    fam = 'bn_bwd_maxpool (%s)' % ('2x2 blocks' if pad == 0 else 'gather')
    ref.check_params('bn_bwd_maxpool %s' % (case,), dgd, dbd, old_dg if pacc else None, old_db if pacc else None, family=fam)
    ref.check_dx('bn_bwd_maxpool %s' % (case,), dxd[..., :Cc].reshape(M, Cc), out, family=fam)


# (kind, N, H, W, C, ldx, ldy, R, stride, pad, dtype, ceil mode, data)
POOL = [
    ('max', 2, 15, 13, 16, 16, 16, 3, 2, 0, 0, 0, 'relu'), ('max', 2, 14, 9, 16, 24, 32, 3, 2, 1, 0, 0, 'relu'), ('max', 1, 9, 12, 8, 16, 8, 3, 1, 1, 0, 0, 'randn'),
    ('max', 2, 8, 6, 16, 16, 24, 2, 2, 0, 0, 0, 'relu'), ('max', 2, 12, 9, 8, 12, 8, 3, 2, 0, 1, 0, 'randn'), ('max', 1, 10, 7, 12, 12, 16, 3, 2, 1, 1, 0, 'neg'),
    ('max', 2, 8, 10, 16, 16, 16, 3, 2, 0, 0, 1, 'relu'), ('max', 1, 13, 6, 8, 8, 8, 3, 2, 0, 1, 1, 'randn'), ('max', 1, 7, 9, 8, 8, 8, 3, 2, 1, 0, 0, 'equal'),
    ('max', 1, 9, 8, 8, 8, 16, 3, 2, 1, 0, 0, 'neg'), ('max', 1, 11, 9, 8, 16, 8, 3, 2, 0, 0, 0, 'nan'), ('max', 1, 6, 8, 8, 8, 8, 2, 2, 0, 1, 0, 'nan'),
    ('avg', 2, 9, 7, 16, 16, 16, 3, 1, 1, 0, 0, 'randn'), ('avg', 2, 8, 11, 16, 24, 32, 3, 1, 1, 0, 0, 'randn'), ('avg', 1, 9, 6, 8, 12, 8, 3, 1, 1, 1, 0, 'randn'),
    ('avg', 2, 8, 6, 16, 16, 24, 2, 2, 0, 0, 0, 'randn'), ('avg', 2, 6, 10, 8, 8, 8, 2, 2, 0, 1, 0, 'randn'), ('avg', 2, 17, 11, 24, 24, 40, 5, 3, 0, 0, 0, 'randn'),
    ('avg', 1, 17, 17, 8, 8, 8, 5, 3, 0, 1, 0, 'randn'), ('avg', 2, 15, 12, 16, 16, 16, 3, 2, 0, 0, 0, 'randn'), ('avg', 1, 10, 13, 8, 16, 8, 3, 2, 1, 0, 0, 'randn'),
] + [('avg', 2, h, w, 8, 8 + 8 * (w & 1), 8, 3, 1, 1, 0, 0, 'randn') for h, w in ((1, 1), (7, 3), (8, 4), (9, 5), (9, 1), (1, 5), (7, 4), (8, 3))] + \
    [('avg', 1, h, w, 4, 4, 8, 3, 1, 1, 1, 0, 'randn') for h, w in ((8, 5), (9, 4), (1, 3), (7, 1))]


def _pool_data(kind, shape, g, dt):
    x = rt(shape, g, dt)
    if kind == 'relu':
        x = x.clamp_min(0)
    elif kind == 'equal':
        x = torch.full(shape, 0.75)
    elif kind == 'neg':
        x = (-x.abs() - 0.5).to(TD[dt]).float()
    elif kind == 'nan':
        x[0, shape[1] // 2, shape[2] // 2, 3] = NAN
    return x


def _run_pool(ctx, case, fast, monkeypatch):
    kind, N, H, W, Cc, ldx, ldy, R, sh, pad, dt, ceil, data = case
    if fast is None:
        monkeypatch.delenv('IFCBK_POOL_FAST', raising=False)
    else:
        monkeypatch.setenv('IFCBK_POOL_FAST', fast)
    out = OUT[dt]
    pd, geo = pool_desc(N, H, W, Cc, ldx, ldy, R, R, sh, pad, dt, ceil)
    g = torch.Generator().manual_seed(H * 31 + W + Cc)
    x = _pool_data(data, (N, H, W, Cc), g, dt)
    dy = rt((N, geo.P, geo.Q, Cc), g, dt)
    old = rt((N, H, W, Cc), g, dt)
    xd, yd = wbuf((N, H, W), Cc, ldx, dt, x), wbuf((N, geo.P, geo.Q), Cc, ldy, dt)
    dyd, dxd, dxa = wbuf((N, geo.P, geo.Q), Cc, ldy, dt, dy), wbuf((N, H, W), Cc, ldx, dt), wbuf((N, H, W), Cc, ldx, dt, old)
    name = 'pool %s fast=%s' % (case, fast)
    fam = '%spool %dx%d/%d/%d%s' % (kind, R, R, sh, pad, '' if fast is None else ' IFCBK_POOL_FAST=' + fast)
    if kind == 'max':
        arg = torch.full((N, geo.P, geo.Q, Cc), 255, dtype=torch.uint8, device='cuda')
        ctx.call('ifcbk_maxpool_fwd', C.byref(pd), P(xd), P(yd), P(arg), st())
        ctx.call('ifcbk_maxpool_bwd', C.byref(pd), P(dyd), P(arg), P(dxd), 0, st())
        ctx.call('ifcbk_maxpool_bwd', C.byref(pd), P(dyd), P(arg), P(dxa), 1, st())
        sync()
        yr, ar = ob.maxpool_fwd(x, geo)
        ob.exact(name + ' values', yd[..., :Cc], yr, fam)
        ob.exact(name + ' arg-max', arg, ar, fam)
        ref, A, n = ob.maxpool_bwd(dy, arg, geo, N, Cc)
    else:
        arg = None
        ctx.call('ifcbk_avgpool_fwd', C.byref(pd), P(xd), P(yd), st())
        ctx.call('ifcbk_avgpool_bwd', C.byref(pd), P(dyd), P(dxd), 0, st())
        ctx.call('ifcbk_avgpool_bwd', C.byref(pd), P(dyd), P(dxa), 1, st())
        sync()
        yr, yA, yn = ob.avgpool_fwd(x, geo)
        ob.check_sum(name + ' fwd', yd[..., :Cc], yr, yA, yn, out, family=fam, dims=('n', 'p', 'q', 'c'))
        ref, A, n = ob.avgpool_bwd(dy, geo, N, Cc)
    guard(name + ' y', yd, Cc, allow_nan=data == 'nan')
    guard(name + ' dx', dxd, Cc)
    guard(name + ' dx (accumulate)', dxa, Cc)
    ob.check_sum(name + ' bwd', dxd[..., :Cc], ref, A, n, out, family=fam)
    ob.check_sum(name + ' bwd accumulate', dxa[..., :Cc], ref, A, n, out, old=old, family=fam)
    return yd, arg, dxd, dxa


@pytest.mark.parametrize('case', POOL, ids=str)
def test_pool(ctx, case, monkeypatch):
    """every pool at the library's default kernel choice; every 3x3 pool again with IFCBK_POOL_FAST=0 (the generic kernels) and 7
    (all fast paths, the opt-in 9-tap max forward included): all runs under the bound, max pool results equal bit for bit"""
    base = _run_pool(ctx, case, None, monkeypatch)
    if case[7] != 3:
        return
    for fast in ('0', '7'):
        other = _run_pool(ctx, case, fast, monkeypatch)
        if case[0] == 'max':
            for a, b in zip(base, other):
                same = (a == b) | (torch.isnan(a.float()) & torch.isnan(b.float()))
                assert same.all(), 'IFCBK_POOL_FAST=%s changes a max pool result' % fast


# (N, H, W, C, ldx, ldy, dtype, relu)
AVG_AFFINE = [(2, 9, 7, 16, 16, 16, 0, 1), (2, 8, 5, 16, 24, 32, 0, 0), (1, 7, 4, 8, 8, 12, 1, 1), (1, 1, 3, 8, 8, 8, 0, 0), (2, 17, 17, 24, 24, 24, 0, 1)]


@pytest.mark.parametrize('case', AVG_AFFINE, ids=str)
def test_avgpool3x3_affine(ctx, case):
    N, H, W, Cc, ldx, ldy, dt, relu = case
    pd, geo = pool_desc(N, H, W, Cc, ldx, ldy, 3, 3, 1, 1, dt)
    g = torch.Generator().manual_seed(H + W)
    x = rt((N, H, W, Cc), g, dt)
    s, b = fvec(Cc, gen=g), fvec(Cc, gen=g, scale=0.3)                            # negative scales too
    xd, yd, sd, bd = wbuf((N, H, W), Cc, ldx, dt, x), wbuf((N, H, W), Cc, ldy, dt), s.cuda(), b.cuda()
    ctx.call('ifcbk_avgpool3x3_affine', C.byref(pd), P(xd), P(sd), P(bd), relu, P(yd), st())
    sync()
    guard('avgpool3x3_affine', yd, Cc)
    ob.check_avg_affine('avgpool3x3_affine %s' % (case,), yd[..., :Cc], x, geo, s, b, bool(relu), OUT[dt], family='avgpool3x3_affine')


# ====================================================================================================== head
# (N, HW, C, ldx, lddx, NC, dtype, mask, param_accumulate, W == NULL)
HEAD = [
    (1, 1, 512, 512, 512, 5, 0, 0, 0, 0), (8, 7, 768, 776, 768, 100, 0, 1, 0, 0), (9, 49, 2048, 2048, 2056, 100, 0, 1, 1, 0),
    (19, 64, 256, 264, 272, 3, 0, 0, 1, 0), (5, 7, 4096, 4096, 4096, 10, 0, 1, 0, 0), (9, 64, 128, 132, 136, 7, 1, 1, 0, 0),
    (19, 1, 2048, 2048, 2048, 2, 1, 0, 1, 0), (5, 49, 4096, 4100, 4096, 3, 1, 0, 0, 0), (9, 49, 16, 24, 24, 10, 0, 0, 0, 1),
    (8, 7, 12, 12, 16, 5, 1, 0, 0, 1),
]


@pytest.mark.parametrize('case', HEAD, ids=str)
def test_head(ctx, case):
    N, HW, Cc, ldx, lddx, NC, dt, use_mask, pacc, noW = case
    L = _lib()
    g = torch.Generator().manual_seed(Cc + NC + N)
    x = (torch.rand(N, HW, Cc, generator=g)).to(TD[dt]).float()
    W, b = fvec(NC, Cc, gen=g, scale=0.05), fvec(NC, gen=g, scale=0.1)
    mask = (torch.rand(N, Cc, generator=g) > 0.5).to(torch.uint8) if use_mask else None
    xd = wbuf((N, HW), Cc, ldx, dt, x)
    md = mask.cuda() if use_mask else None
    Wd, bd = (None, None) if noW else (W.cuda(), b.cuda())
    feat, lg = torch.full((N, Cc), NAN, device='cuda'), torch.full((N, NC), NAN, device='cuda')
    d = L.HeadDesc(N, HW, Cc, ldx, NC, dt, 2.0)
    ctx.call('ifcbk_head_fwd', C.byref(d), P(xd), P(md), P(Wd), P(bd), P(feat), P(lg), st())
    sync()
    name = 'head %s' % (case,)
    ref, A, n = ob.gap(x, mask, 2.0)
    ob.check_sum(name + ' gap', feat, ref, A, n, 'f32', family='head gap', dims=('n', 'c'))
    if noW:
        ob.exact(name + ' pooled logits', lg, feat[:, :NC], 'head fc')
    else:
        ref, A, n = ob.fc_fwd(feat, W, b)                 # from the features the kernel read
        ob.check_sum(name + ' fc', lg, ref, A, n, 'f32', family='head fc', dims=('n', 'j'))
    dl = fvec(N, NC, gen=g, scale=1.0 / N)
    dld = dl.cuda()
    old_W, old_b = fvec(NC, Cc, gen=g), fvec(NC, gen=g)
    dW, db = (old_W.cuda(), old_b.cuda()) if pacc else (torch.full((NC, Cc), NAN, device='cuda'), nanvec(NC))
    dxd = wbuf((N, HW), Cc, lddx, dt)
    ctx.call('ifcbk_head_bwd', C.byref(d), P(dld), P(feat), P(md), P(Wd), None if noW else P(dW), None if noW else P(db), P(dxd), lddx, pacc, st())
    sync()
    guard(name + ' dx', dxd, Cc)
    if not noW:
        ref, A, n = ob.fc_wgrad(dl, feat)
        ob.check_sum(name + ' dW', dW, ref, A, n, 'f32', old=old_W if pacc else None, family='head fc_wgrad', dims=('j', 'c'))
        ref, A, n = ob.fc_bgrad(dl)
        ob.check_sum(name + ' db', db, ref, A, n, 'f32', old=old_b if pacc else None, family='head fc_bgrad', dims=('j',))
    ref, A, n = ob.head_dx(dl, None if noW else W, mask, 2.0, HW, Cc)
    ex = lambda t: t[:, None, :].expand(N, HW, Cc)
    ob.check_sum(name + ' dx', dxd[..., :Cc], ex(ref), ex(A), n, OUT[dt], family='head dx', dims=('n', 'hw', 'c'))


# ====================================================================================================== softmax, cross-entropy
# (N, NC, spread, shift, target: 'argmax' | 'least' | 'rand', loss_accumulate, dlogits given)
XENT = [
    (1, 1, 1, 0, 'rand', 0, 1), (255, 2, 8, 0, 'argmax', 1, 1), (256, 3, 1, 80, 'least', 0, 1), (257, 5, 8, -80, 'rand', 1, 1),
    (600, 100, 1, 0, 'rand', 0, 1), (19, 1001, 8, 0, 'least', 0, 1), (600, 5, 8, 80, 'argmax', 1, 0), (1, 1001, 1, -80, 'argmax', 0, 1),
    (257, 100, 8, 80, 'least', 0, 0), (255, 3, 1, 0, 'rand', 1, 1),
]


@pytest.mark.parametrize('case', XENT, ids=str)
def test_softmax_xent_and_softmax(ctx, case):
    N, NC, spread, shift, tmode, acc, with_dl = case
    g = torch.Generator().manual_seed(N + NC)
    l = torch.randn(N, NC, generator=g) * spread + shift
    tgt = {'argmax': l.argmax(1), 'least': l.argmin(1), 'rand': torch.randint(0, NC, (N,), generator=g)}[tmode]
    ld, td = l.cuda(), tgt.cuda()
    loss = torch.full((1,), 5.0 if acc else NAN, device='cuda')
    dl = torch.full((N + 1, NC), NAN, device='cuda') if with_dl else None
    probs = torch.full((N + 1, NC), NAN, device='cuda')
    ctx.call('ifcbk_softmax_xent', P(ld), P(td), N, NC, 0.4, P(loss), acc, P(dl), st())
    ctx.call('ifcbk_softmax', P(ld), N, NC, P(probs), st())
    sync()
    assert torch.isnan(probs[N]).all() and torch.isfinite(probs[:N]).all()
    want = ob.xent(l, tgt, 0.4, old_loss=5.0 if acc else None)
    got = {'loss': loss}
    if with_dl:
        assert torch.isnan(dl[N]).all() and torch.isfinite(dl[:N]).all()
        got['dlogits'] = dl[:N]
    ob.check_dict('softmax_xent %s' % (case,), got, want, family='softmax_xent')
    p, e, _ = ob.softmax(l)
    ob.elem('softmax %s' % (case,), probs[:N], p, e, 'f32', 'softmax', dims=('n', 'j'))


# ====================================================================================================== optimizers
# (n, step, weight_decay, grad_scale)
ADAM = [(1, 1, 0.0, 1.0), (3, 2, 0.01, 1.0), (4, 1000, 0.0, 1 / 128), (5, 1, 0.01, 1 / 128), (100003, 1, 0.0, 1.0), (100003, 2, 0.01, 1 / 128),
        (100003, 1000, 0.01, 1.0)]
# (n, momentum, weight_decay, grad_scale)
SGD = [(1, 0.0, 0.0, 1.0), (3, 0.9, 0.01, 1.0), (4, 0.9, 0.0, 1 / 128), (5, 0.0, 0.01, 1 / 128), (100003, 0.9, 0.01, 1 / 128), (100003, 0.0, 0.0, 1.0)]


def _grads(n, g):
    gr = torch.randn(n, generator=g) * 10 ** (torch.rand(n, generator=g) * 11 - 8)           # 1e-8 .. 1e3
    gr[::7] = 0.0
    return gr


@pytest.mark.parametrize('case', ADAM, ids=str)
def test_adam_flat(ctx, case):
    n, step, wd, gs = case
    g = torch.Generator().manual_seed(n + step)
    p, gr = torch.randn(n, generator=g), _grads(n, g)
    m = torch.randn(n, generator=g) * 0.1 if step > 1 else torch.zeros(n)
    v = torch.rand(n, generator=g) * 0.01 if step > 1 else torch.zeros(n)
    m[::7], v[::7] = 0.0, 0.0                                                             # v = 0 and g = 0: denom = eps
    dev = [torch.cat([t, torch.full((5,), NAN)]).cuda() for t in (p, gr, m, v)]
    ctx.call('ifcbk_adam_flat', P(dev[0]), P(dev[1]), P(dev[2]), P(dev[3]), n, 1e-3, 0.9, 0.999, 1e-8, wd, step, gs, st())
    sync()
    for t in dev:
        assert torch.isnan(t[n:]).all() and torch.isfinite(t[:n]).all()
    want = ob.adam(p, gr, m, v, 1e-3, 0.9, 0.999, 1e-8, wd, step, gs)
    ob.check_dict('adam %s' % (case,), {'p': dev[0][:n], 'm': dev[2][:n], 'v': dev[3][:n]}, want, family='adam')


@pytest.mark.parametrize('case', SGD, ids=str)
def test_sgd_flat(ctx, case):
    n, mu, wd, gs = case
    g = torch.Generator().manual_seed(n)
    p, gr, mom = torch.randn(n, generator=g), _grads(n, g), torch.randn(n, generator=g)
    dev = [torch.cat([t, torch.full((5,), NAN)]).cuda() for t in (p, gr, mom)]
    ctx.call('ifcbk_sgd_flat', P(dev[0]), P(dev[1]), P(dev[2]) if mu else None, n, 0.05, mu, wd, gs, st())
    sync()
    for t in dev:
        assert torch.isnan(t[n:]).all() and torch.isfinite(t[:n]).all()
    want = ob.sgd(p, gr, mom if mu else None, 0.05, mu, wd, gs)
    got = {'p': dev[0][:n]}
    if mu:
        got['mom'] = dev[2][:n]
    else:
        assert torch.equal(dev[2][:n].cpu(), mom)
    ob.check_dict('sgd %s' % (case,), got, want, family='sgd')


# ====================================================================================================== layout, counters, plain layers
# (N, C, H, W, Cpad, dtype, transform)
NCHW = [(3, 3, 17, 19, 8, 0, 1), (2, 3, 5, 7, 8, 0, 0), (2, 3, 9, 4, 4, 1, 1), (1, 1, 6, 6, 8, 1, 0), (2, 3, 16, 17, 16, 0, 1)]


@pytest.mark.parametrize('case', NCHW, ids=str)
def test_nchw_to_nhwc(ctx, case):
    N, Cc, H, W, Cpad, dt, tr = case
    g = torch.Generator().manual_seed(H * W)
    x = torch.rand(N, Cc, H, W, generator=g)
    sc, sh = [0.458, 0.448, 0.45], [-0.03, -0.088, -0.188]
    y = torch.full((N * H * W + 1, Cpad), NAN, dtype=TD[dt], device='cuda')
    xd = x.cuda()
    ctx.call('ifcbk_nchw_to_nhwc', P(xd), N, Cc, H, W, Cpad, dt, (C.c_float * 3)(*sc) if tr else None, (C.c_float * 3)(*sh) if tr else None, P(y), st())
    sync()
    assert torch.isnan(y[-1]).all() and torch.isfinite(y[:-1].float()).all()
    yy = y[:-1].reshape(N, H, W, Cpad)
    assert (yy[..., Cc:] == 0).all()
    s = torch.tensor([ob.f32(v) for v in sc])[:Cc] if tr else torch.ones(Cc)
    b = torch.tensor([ob.f32(v) for v in sh])[:Cc] if tr else torch.zeros(Cc)
    want, e = ob.affine(x.permute(0, 2, 3, 1), s, b)
    ob.elem('nchw_to_nhwc %s' % (case,), yy[..., :Cc], want, e if tr else 0.0, OUT[dt], 'nchw_to_nhwc', dims=('n', 'h', 'w', 'c'))


# (N, C, H, W, ldx, dtype)
NHWC = [(2, 5, 3, 7, 8, 0), (3, 16, 4, 4, 24, 0), (2, 3, 5, 5, 4, 1), (1, 10, 1, 9, 16, 1)]


@pytest.mark.parametrize('case', NHWC, ids=str)
def test_nhwc_to_nchw_f32(ctx, case):
    N, Cc, H, W, ldx, dt = case
    g = torch.Generator().manual_seed(H + W)
    x = rt((N, H, W, Cc), g, dt)
    xd = wbuf((N, H, W), Cc, ldx, dt, x)
    y = torch.full((N * Cc * H * W + 3,), NAN, device='cuda')
    ctx.call('ifcbk_nhwc_to_nchw_f32', P(xd), N, Cc, H, W, ldx, dt, P(y), st())
    sync()
    assert torch.isnan(y[-3:]).all()
    ob.exact('nhwc_to_nchw_f32 %s' % (case,), y[:-3].reshape(N, Cc, H, W), x.permute(0, 3, 1, 2), 'nhwc_to_nchw_f32')


# (number of BatchNorms, counters given, loss sum given)
COUNTERS = [(300, 1, 1), (7, 1, 0), (0, 0, 1), (257, 1, 1)]


@pytest.mark.parametrize('case', COUNTERS, ids=str)
def test_step_counters(ctx, case):
    n, with_nbt, with_loss = case
    nbt = torch.arange(n + 2, dtype=torch.int64).cuda() * 3
    before = nbt.clone()
    ls, lo = torch.tensor([1.25], device='cuda'), torch.tensor([0.3], device='cuda')
    ctx.call('ifcbk_step_counters', P(nbt) if with_nbt else None, n, P(ls) if with_loss else None, P(lo), st())
    sync()
    inc = torch.zeros_like(before)
    inc[:n] = 1 if with_nbt else 0
    assert torch.equal(nbt, before + inc)
    want = torch.tensor([1.25]).double() + (torch.tensor([0.3]).double() if with_loss else 0.0)
    ob.elem('step_counters %s' % (case,), ls, want, ob.U * want.abs(), 'f32', 'step_counters')
    assert float(lo) == ob.f32(0.3)


# (M, K, ldy, lddy, lddz, relu, dtype, param_accumulate)
BIAS_RELU = [(1000, 64, 72, 64, 80, 1, 0, 0), (37, 4096, 4096, 4104, 4096, 1, 0, 1), (5000, 24, 40, 24, 28, 1, 1, 1), (300, 104, 104, 112, 104, 0, 0, 0),
             (17, 8, 8, 8, 16, 1, 0, 0)]


@pytest.mark.parametrize('case', BIAS_RELU, ids=str)
def test_bias_relu_bwd(ctx, case):
    M, K, ldy, lddy, lddz, relu, dt, pacc = case
    g = torch.Generator().manual_seed(M + K)
    y, dy = rt((M, K), g, dt), rt((M, K), g, dt)
    yd, dyd, dzd = wbuf((M,), K, ldy, dt, y), wbuf((M,), K, lddy, dt, dy), wbuf((M,), K, lddz, dt)
    old = fvec(K, gen=g, scale=3.0)
    db = old.cuda() if pacc else nanvec(K)
    rows = ctx.lib.ifcbk_bias_relu_bwd_rows(M)
    assert rows == max(16, (M + 1023) // 1024)
    assert ctx.lib.ifcbk_bias_relu_bwd_workspace(M, K) == -(-M // rows) * K * 4
    ctx.reserve(ctx.lib.ifcbk_bias_relu_bwd_workspace(M, K))
    ctx.call('ifcbk_bias_relu_bwd', M, K, dt, P(yd), ldy, P(dyd), lddy, P(dzd), lddz, relu, P(db), pacc, st())
    sync()
    guard('bias_relu_bwd dz', dzd, K)
    dz = torch.where(y > 0, dy, torch.zeros(())) if relu else dy
    ob.exact('bias_relu_bwd dz %s' % (case,), dzd[..., :K], dz, 'bias_relu_bwd')
    ob.sums('bias_relu_bwd dbias %s' % (case,), db, dz, ops=1, old=old if pacc else None, family='bias_relu_bwd')


# (chunks, dtype, mask, accumulate)
DROPOUT = [(1, 0, 1, 0), (255, 0, 1, 1), (257, 1, 1, 0), (1234, 0, 0, 1), (513, 1, 0, 0), (1000, 1, 1, 1)]


@pytest.mark.parametrize('case', DROPOUT, ids=str)
def test_dropout_apply(ctx, case):
    nch, dt, use_mask, acc = case
    n = nch * CH[dt]
    g = torch.Generator().manual_seed(nch)
    x, old = rt((n,), g, dt), rt((n,), g, dt)
    mask = (torch.rand(n, generator=g) > 0.5).to(torch.uint8)
    pad = torch.full((CH[dt],), NAN)
    xd = torch.cat([x, pad]).to(TD[dt]).cuda()
    yd = torch.cat([old if acc else torch.full((n,), NAN), pad]).to(TD[dt]).cuda()
    md = mask.cuda() if use_mask else None
    ctx.call('ifcbk_dropout_apply', n, dt, P(xd), P(md), 1.7, P(yd), acc, st())
    sync()
    assert torch.isnan(yd[n:].float()).all() and torch.isfinite(yd[:n].float()).all()
    k = mask.double() * ob.f32(1.7) if use_mask else 1.0
    want = x.double() * k
    e = ob.U * want.abs() if use_mask else torch.zeros(n).double()
    if acc:
        e = e + ob.U * (want.abs() + old.double().abs())
        want = want + old.double()
    ob.elem('dropout_apply %s' % (case,), yd[:n], want, e, OUT[dt], 'dropout_apply')


# (N, HW, C, ldx, dtype)
FLATTEN = [(3, 36, 16, 24, 0), (2, 49, 8, 8, 0), (2, 9, 12, 20, 1), (1, 1, 4, 8, 1)]


@pytest.mark.parametrize('case', FLATTEN, ids=str)
def test_flatten_chw(ctx, case):
    N, HW, Cc, ldx, dt = case
    g = torch.Generator().manual_seed(HW + Cc)
    x, old = rt((N, HW, Cc), g, dt), rt((N, HW, Cc), g, dt)
    xd = wbuf((N, HW), Cc, ldx, dt, x)
    flat = torch.full((N * Cc * HW + 2,), NAN, dtype=TD[dt], device='cuda')
    ctx.call('ifcbk_flatten_chw', N, HW, Cc, dt, P(xd), ldx, P(flat), 1, 0, st())
    sync()
    assert torch.isnan(flat[-2:].float()).all()
    ob.exact('flatten_chw %s' % (case,), flat[:-2].reshape(N, Cc, HW), x.permute(0, 2, 1), 'flatten_chw')
    for acc in (0, 1):
        back = wbuf((N, HW), Cc, ldx, dt, old if acc else None)
        ctx.call('ifcbk_flatten_chw', N, HW, Cc, dt, P(back), ldx, P(flat), 0, acc, st())
        sync()
        guard('flatten_chw back', back, Cc)
        want = x.double() + (old.double() if acc else 0.0)
        ob.elem('flatten_chw back %s' % (case,), back[..., :Cc], want, ob.U * (x.double().abs() + old.double().abs()) if acc else 0.0, OUT[dt],
                'flatten_chw', dims=('n', 'hw', 'c'))


# (n, p, seed, offset)
DROPOUT_MASK = [(1000, 0.5, 42, 0), (777, 0.2, 7, 12345), (1, 0.9, 0, 2 ** 40)]


@pytest.mark.parametrize('case', DROPOUT_MASK, ids=str)
def test_dropout_mask_is_the_documented_generator(ctx, case):
    """splitmix64 of (seed, offset + i), the top 24 bits as a uniform in [0, 1): keep where u >= p"""
    n, p, seed, offset = case
    m = torch.full((n + 3,), 9, dtype=torch.uint8, device='cuda')
    ctx.call('ifcbk_dropout_mask', P(m), n, p, seed, offset, st())
    sync()
    K = (1 << 64) - 1
    want = []
    for i in range(n):
        z = (seed + 0x9E3779B97F4A7C15 * (offset + i + 1)) & K
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & K
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & K
        z ^= z >> 31
        want.append(1 if (z >> 40) / 16777216.0 >= ob.f32(p) else 0)
    assert m[:n].cpu().tolist() == want and (m[n:] == 9).all()


# ====================================================================================================== inventory
# kernel -> (source file, case table, which of its cases reach the kernel, the dispatch condition as the source states it)
KERNELS = {
    'bn_finalize_kernel': ('bn.hip', 'FINALIZE', lambda c: True, 'if (part) {'),
    'bn_prereduce_kernel': ('bn.hip', 'FINALIZE', lambda c: c[0] > 1536, 'mblocks > 1536'),
    'bn_eval_scale_kernel': ('bn.hip', 'FINALIZE', lambda c: True, 'eval (part==NULL)'),          # test_bn_finalize_eval
    'bn_stats_kernel': ('bn.hip', 'STATS', lambda c: True, 'd->dtype == IFCBK_F32) hipLaunchKernelGGL(bn_stats_kernel<float>'),
    'bn_apply_kernel': ('bn.hip', 'BN_APPLY', lambda c: True, 'd->relu && rr'),
    'bn_bwd_reduce_pool2x2_kernel': ('bn.hip', 'POOLED', lambda c: c[7] == 0, 'pool && pg.ph == 0 && pg.pw == 0'),
    'bn_bwd_dx_pool2x2_kernel': ('bn.hip', 'POOLED', lambda c: c[7] == 0, 'pool && pg.ph == 0 && pg.pw == 0'),
    'bn_bwd_reduce_kernel': ('bn.hip', 'BN_BWD', lambda c: True, 'else if (mask == 1)'),
    'bn_bwd_finalize_kernel': ('bn.hip', 'BN_BWD_PARTIALS', lambda c: c[2] > c[1], '(part_in && part_ld_in > 0) ? part_ld_in : C'),
    'bn_bwd_dx_kernel': ('bn.hip', 'BN_BWD', lambda c: c[8] & 2, 'dres_acc & 2'),
    'bn_apply_maxpool_kernel': ('bn.hip', 'POOLED', lambda c: True, 'pooled_check(ctx, d, "bn_apply_maxpool")'),
    'maxpool_fwd_kernel': ('pool_head.hip', 'POOL', lambda c: c[0] == 'max', 'if (make_pool3(d, 1, &f))'),
    'maxpool3x3_fwd_kernel': ('pool_head.hip', 'POOL', lambda c: c[0] == 'max' and c[7] == 3, 'if (!((m >> mode) & 1)) return false;'),
    'maxpool_bwd_kernel': ('pool_head.hip', 'POOL', lambda c: c[0] == 'max' and (c[7] != 3 or c[8] != 2), 'if (make_pool3(d, 2, &f))'),
    'maxpool3x3s2_bwd_kernel': ('pool_head.hip', 'POOL', lambda c: c[0] == 'max' and c[7] == 3 and c[8] == 2,
                                'mode == 2 && !(d->stride_h == 2 && d->stride_w == 2 && d->pad_h <= 1 && d->pad_w <= 1)'),
    'avgpool_fwd_kernel': ('pool_head.hip', 'POOL', lambda c: c[0] == 'avg' and (c[7] != 3 or c[8] != 1), 'if (make_pool3(d, 0, &f))'),
    'avgpool_bwd_kernel': ('pool_head.hip', 'POOL', lambda c: c[0] == 'avg' and (c[7] != 3 or c[8] != 1), 'if (make_pool3(d, 0, &f))'),
    'avgpool3x3s1_kernel': ('pool_head.hip', 'POOL', lambda c: c[0] == 'avg' and c[7] == 3 and c[8] == 1 and c[9] == 1,
                            'mode == 0 && !(d->stride_h == 1 && d->stride_w == 1 && d->pad_h == 1 && d->pad_w == 1'),
    'gap_kernel': ('pool_head.hip', 'HEAD', lambda c: True, 'gap_kernel<float>'),
    'fc_fwd_kernel': ('pool_head.hip', 'HEAD', lambda c: c[2] > 2048 and not c[9], 'if (d->C <= 2048)'),
    'fc_wgrad_kernel': ('pool_head.hip', 'HEAD', lambda c: not c[9], 'if (W) {'),
    'fc_bgrad_kernel': ('pool_head.hip', 'HEAD', lambda c: not c[9], 'if (W) {'),
    'head_dx_kernel': ('pool_head.hip', 'HEAD', lambda c: c[9], 'if (!W) {'),
    'dropout_mask_kernel': ('pool_head.hip', 'DROPOUT_MASK', lambda c: True, 'dropout_mask_kernel, dim3(cdiv(n, 256))'),
    'softmax_xent_kernel': ('pool_head.hip', 'XENT', lambda c: c[0] > 256, 'for (int n0 = 0; n0 < N; n0 += 256)'),
    'softmax_kernel': ('pool_head.hip', 'XENT', lambda c: True, 'softmax_kernel, dim3(cdiv(N, 64))'),
    'step_counters_kernel': ('pool_head.hip', 'COUNTERS', lambda c: True, 'n < 0 || (loss_sum && !loss)'),
    'adam_kernel': ('pool_head.hip', 'ADAM', lambda c: c[0] % 4 != 0, 'if (i + 4 <= n) {'),
    'sgd_kernel': ('pool_head.hip', 'SGD', lambda c: True, 'sgd_kernel, dim3(cdiv(n, 256))'),
    'nchw_to_nhwc_kernel': ('pool_head.hip', 'NCHW', lambda c: True, 'Cpad % dtype_chunk(dtype)'),
    'nhwc_to_nchw_kernel': ('pool_head.hip', 'NHWC', lambda c: True, 'nhwc_to_nchw_kernel<float>'),
    'bias_relu_bwd_kernel': ('plain.hip', 'BIAS_RELU', lambda c: True, 'if (!dz && !dbias) return 0;'),
    'colsum_finalize_kernel': ('plain.hip', 'BIAS_RELU', lambda c: True, 'if (dbias) {'),
    'dropout_apply_kernel': ('plain.hip', 'DROPOUT', lambda c: True, 'dropout_apply_kernel<float>'),
    'flatten_chw_kernel': ('plain.hip', 'FLATTEN', lambda c: True, 'flatten_chw_kernel<float>'),
}
