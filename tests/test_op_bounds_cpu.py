"""The checkers of tests/op_bounds.py are neither blind nor too tight (CPU): for every family a correct float32 evaluation of the same
formula -- in a summation order of its own (shuffled, or 256-row tiles combined in double), with the multiply-add contracted and
split into two roundings -- passes, and simulated kernel faults are flagged."""
import pytest
import torch

import op_bounds as ob


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _store(t, out):
    return _bf(t.float()) if out == 'bf16' else t.float()


def _fma(a, b, c, fused):
    """fp32 a * b + c: one rounding (the product of two fp32 values is exact in double) or two"""
    if fused:
        return (a.double() * b.double() + c.double()).float()
    return a.float() * b.float() + c.float()


def _shuffled_sum(t, dim, seed=1):
    """sequential fp32 sum along dim in a shuffled order"""
    g = torch.Generator().manual_seed(seed)
    t = t.float().movedim(dim, 0)
    acc = torch.zeros_like(t[0])
    for i in torch.randperm(t.shape[0], generator=g).tolist():
        acc = acc + t[i]
    return acc


def _tile_sum(t, tile=256):
    """fp32 sums of row tiles (shuffled inside a tile), combined in double, rounded once"""
    parts = [_shuffled_sum(t[i:i + tile], 0, seed=i).double() for i in range(0, t.shape[0], tile)]
    return torch.stack(parts).sum(0).float()


def _flagged(fn):
    with pytest.raises(AssertionError):
        fn()


# ------------------------------------------------------------------------------------------------------ elementwise affine
@pytest.mark.parametrize('out', ['bf16', 'f32'])
@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('relu,res', [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_affine_float32_passes_and_an_unwritten_chunk_is_flagged(out, fused, relu, res):
    g = torch.Generator().manual_seed(3)
    x = _store(torch.randn(300, 40, generator=g) * 2 + 0.5, out)
    s, b = torch.randn(40, generator=g), torch.randn(40, generator=g) * 0.3
    r = _store(torch.randn(300, 40, generator=g), out) if res else None
    y = _fma(x, s, b, fused)
    if res:
        y = y + r
    if relu:
        y = y.clamp_min(0)
    y = _store(y, out)
    want, e = ob.affine(x, s, b, r, bool(relu))
    res_ = ob.elem('affine', y, want, e, out)
    assert res_.ratio < 1.0
    bad = y.clone()
    bad[-1, -8:] = 0.0                                  # one channel chunk of 8 left unwritten in the last pixel (zero-filled buffer)
    _flagged(lambda: ob.elem('affine', bad, want, e, out))
    bad[-1, -8:] = float('nan')                         # ... (NaN-filled buffer)
    _flagged(lambda: ob.elem('affine', bad, want, e, out))
    if out == 'bf16':                                   # a bf16-rounded product before the add
        y2 = _bf(x * s) + b
        y2 = y2 + r if res else y2
        _flagged(lambda: ob.elem('affine', _bf(y2.clamp_min(0) if relu else y2), want, e, out))


# ------------------------------------------------------------------------------------------------------ pools
GEOS = [(9, 7, 3, 3, 2, 2, 0, 0), (8, 11, 3, 3, 2, 2, 1, 1), (7, 6, 3, 3, 1, 1, 1, 1), (8, 6, 2, 2, 2, 2, 0, 0), (11, 17, 5, 5, 3, 3, 0, 0)]


def _taps(x, g):
    vs = []
    for r in range(g.R):
        for s in range(g.S):
            v, ok = g.gather(x, r, s)
            vs.append(torch.where(ok[None, :, :, None], v, torch.zeros(())))
    return torch.stack(vs)


@pytest.mark.parametrize('geo', GEOS)
@pytest.mark.parametrize('out', ['bf16', 'f32'])
def test_average_pool_float32_passes_and_faults_are_flagged(geo, out):
    g = ob.Geo(*geo)
    gen = torch.Generator().manual_seed(5)
    x = _store(torch.randn(2, g.H, g.W, 16, generator=gen) + 0.3, out)
    ref, A, n = ob.avgpool_fwd(x, g)
    inv = torch.tensor(1.0 / (g.R * g.S), dtype=torch.float32)
    acc = _shuffled_sum(_taps(x, g), 0)
    y = _store(acc * inv, out)
    assert ob.check_sum('avg', y, ref, A, n, out).ratio < 1.0
    old = _store(torch.randn(y.shape, generator=gen), out)
    assert ob.check_sum('avg acc', _store(acc * inv + old, out), ref, A, n, out, old=old).ratio < 1.0
    _flagged(lambda: ob.check_sum('avg acc', y, ref, A, n, out, old=old))                  # overwritten where it should accumulate
    if out == 'f32' or g.R * g.S != 4:           # (bf16 storage and 1 / 4: rounding before or after a power of two is the same rounding)
        _flagged(lambda: ob.check_sum('avg', _store(_bf(acc) * inv, out), ref, A, n, out))     # the pooled sum rounded to bf16 before * inv
    if g.ph:                                                                               # a window that reads its neighbour instead of padding
        xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2), (g.pw, g.pw, g.ph, g.ph), mode='replicate').permute(0, 2, 3, 1)
        g2 = ob.Geo(g.H + 2 * g.ph, g.W + 2 * g.pw, g.R, g.S, g.sh, g.sw, 0, 0)
        yb = _store(_shuffled_sum(_taps(xp, g2), 0) * inv, out)
        _flagged(lambda: ob.check_sum('avg', yb, ref, A, n, out))
    # backward: the windows of a pixel, fp32
    dy = _store(torch.randn(2, g.P, g.Q, 16, generator=gen), out)
    bref, bA, bn = ob.avgpool_bwd(dy, g, 2, 16)
    dx = torch.zeros(2, g.H, g.W, 16)
    for r in reversed(range(g.R)):
        for s in range(g.S):
            g.scatter(dy, r, s, dx)
    assert ob.check_sum('avg bwd', _store(dx * inv, out), bref, bA, bn, out).ratio < 1.0


@pytest.mark.parametrize('geo', GEOS)
def test_max_pool_rule_ties_padding_and_backward(geo):
    g = ob.Geo(*geo)
    gen = torch.Generator().manual_seed(7)
    x = _bf(torch.randn(2, g.H, g.W, 8, generator=gen)).clamp_min(0)          # after ReLU: many ties
    y, arg = ob.maxpool_fwd(x, g)
    want = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), (g.R, g.S), (g.sh, g.sw), (g.ph, g.pw)).permute(0, 2, 3, 1)
    ob.exact('max', y, want)
    y2, arg2 = ob.maxpool_fwd(x, g, last_on_tie=True)                       # arg-max of the last instead of the first maximum
    ob.exact('max', y2, y)
    _flagged(lambda: ob.exact('arg', arg2, arg))
    xn = x.clone()
    xn[0, 2, 2, 3] = float('nan')                                           # NaN takes every window it lies in
    yn, _ = ob.maxpool_fwd(xn, g)
    assert torch.isnan(yn[0, :, :, 3]).any() and not torch.isnan(yn[1]).any()
    neg = -x - 1.0                                                          # all negative: a padding tap read as 0 would win
    yneg, _ = ob.maxpool_fwd(neg, g)
    assert (yneg < 0).all()
    dy = _bf(torch.randn(2, g.P, g.Q, 8, generator=gen))
    ref, A, n = ob.maxpool_bwd(dy, arg, g, 2, 8)
    dx = torch.zeros(2, g.H, g.W, 8)
    for r in reversed(range(g.R)):
        for s in range(g.S):
            g.scatter(torch.where(arg == r * g.S + s, dy, torch.zeros(())), r, s, dx)
    assert ob.check_sum('max bwd', _bf(dx), ref, A, n, 'bf16').ratio < 1.0
    ref2, _, _ = ob.maxpool_bwd(dy, arg2, g, 2, 8)
    _flagged(lambda: ob.check_sum('max bwd', _bf(ref2.float()), ref, A, n, 'bf16'))


@pytest.mark.parametrize('relu', [0, 1])
def test_average_pool_with_affine_accepts_the_designed_rounding(relu):
    g = ob.Geo(9, 6, 3, 3, 1, 1, 1, 1)
    gen = torch.Generator().manual_seed(2)
    x = _bf(torch.randn(2, 9, 6, 16, generator=gen))
    s, b = torch.randn(16, generator=gen), torch.randn(16, generator=gen) * 0.2
    avg = _bf(_shuffled_sum(_taps(x, g), 0) * torch.tensor(1 / 9.0))
    for fused in (True, False):
        y = _fma(avg, s, b, fused)
        r = ob.check_avg_affine('avg affine', _bf(y.clamp_min(0) if relu else y), x, g, s, b, bool(relu), 'bf16')
        assert r.ratio < 1.0
    y = _fma(avg, s.abs(), b, True)                                        # the sign of a negative scale lost
    _flagged(lambda: ob.check_avg_affine('avg affine', _bf(y.clamp_min(0) if relu else y), x, g, s, b, bool(relu), 'bf16'))


# ------------------------------------------------------------------------------------------------------ BatchNorm statistics
def _rows(x, tile):
    return torch.stack([torch.stack([_shuffled_sum(x[i:i + tile], 0, i), _shuffled_sum(x[i:i + tile] ** 2, 0, i + 1)])
                        for i in range(0, x.shape[0], tile)])


def _finalize_like(part, M, eps, mom, gam, bet, rm, rv, fused, prereduce=False, biased=False):
    """the arithmetic of bn_finalize_kernel: double sums, one rounding to fp32, fp32 scale / shift / running statistics"""
    p = part.double()
    if prereduce:
        p = torch.stack([p[i:i + 64].sum(0).float().double() for i in range(0, p.shape[0], 64)])
    S = p.sum(0)
    mean = S[0] / M
    var = (S[1] / M - mean * mean).clamp_min(0)
    invstd = (1 / torch.sqrt(var + ob.f32(eps))).float()
    sc = gam * invstd
    sh = _fma(-mean.float(), sc, bet, fused)
    unb = 1.0 if biased or M == 1 else M / (M - 1.0)
    c1, m_ = torch.tensor(1.0) - torch.tensor(mom), torch.tensor(mom)
    nrm = _fma(m_, mean.float(), c1 * rm, fused)
    nrv = _fma(m_, (var * unb).float(), c1 * rv, fused)
    return {'mean': mean.float(), 'invstd': invstd, 'scale': sc, 'shift': sh, 'running_mean': nrm, 'running_var': nrv}


@pytest.mark.parametrize('ratio', [0, 10, 100])
@pytest.mark.parametrize('fused', [True, False])
def test_finalize_float32_passes_and_biased_running_var_is_flagged(ratio, fused):
    gen = torch.Generator().manual_seed(ratio + 1)
    M, Cc = 1500, 24
    x = _bf(torch.randn(M, Cc, generator=gen) + ratio)
    part = _rows(x, 128)
    gam, bet = torch.rand(Cc, generator=gen) + 0.5, torch.randn(Cc, generator=gen)
    rm, rv = torch.randn(Cc, generator=gen), torch.rand(Cc, generator=gen) + 0.5
    want = ob.finalize(part, M, 1e-3, 0.1, gam, bet, rm, rv)
    got = _finalize_like(part, M, 1e-3, 0.1, gam, bet, rm, rv, fused)
    assert ob.check_finalize('finalize', got, want) < 1.0
    e_var, var = want['var'][1], want['var'][0]
    assert float((e_var / var).max()) < 1e-6                     # the double sums keep the variance even at |mean| / std = 100
    bad = _finalize_like(part, M, 1e-3, 0.1, gam, bet, rm, rv, fused, biased=True)
    _flagged(lambda: ob.check_finalize('finalize', bad, want))
    # the prereduce route stores fp32 intermediate rows: within its own bound, and (at a large mean) outside the direct route's
    pre = _finalize_like(part, M, 1e-3, 0.1, gam, bet, rm, rv, fused, prereduce=True)
    assert ob.check_finalize('finalize', pre, ob.finalize(part, M, 1e-3, 0.1, gam, bet, rm, rv, prereduce=True)) < 1.0
    # variance in fp32 (E[x^2] - mean^2 cancels): flagged once the mean is large
    if ratio == 100:
        S = part.double().sum(0)
        meanf = (S[0] / M).float()
        varf = ((S[1] / M).float() - meanf * meanf).clamp_min(0)
        b2 = dict(got)
        b2['invstd'] = 1 / torch.sqrt(varf + 1e-3)
        _flagged(lambda: ob.check_finalize('finalize', b2, want))


@pytest.mark.parametrize('M', [1, 700, 1024, 2500])
def test_stats_float32_passes_and_a_dropped_row_is_flagged(M):
    gen = torch.Generator().manual_seed(M)
    x = _bf(torch.randn(M, 16, generator=gen) * 1.5 + 0.3)
    part = _rows(x, 1024)
    assert ob.check_stats('stats', part, x) < 1.0
    if M > 1:
        keep = torch.ones(M, dtype=torch.bool)
        keep[M - 2] = False                                      # one dropped row in the last (partial) tile
        bad = part.clone()
        last = x[(M - 1) // 1024 * 1024:][keep[(M - 1) // 1024 * 1024:]]
        bad[-1, 0], bad[-1, 1] = last.sum(0), (last * last).sum(0)
        _flagged(lambda: ob.check_stats('stats', bad, x))


# ------------------------------------------------------------------------------------------------------ BatchNorm backward
def _bn_bwd_like(x, dy, on, gam, mean, invstd, M, fused, tile=256, drop=None, bf16_dg=False):
    dz = torch.where(on, dy, torch.zeros(()))
    xh = (x - mean) * invstd
    t1, t2 = dz.clone(), dz * xh
    if drop is not None:
        t1[drop], t2[drop] = 0.0, 0.0
    db, dg = _tile_sum(t1, tile), _tile_sum(t2, tile)
    invM = torch.tensor(1.0 / M, dtype=torch.float32)
    a = gam * invstd
    dgm, dbm = dg * invM, db * invM
    if bf16_dg:
        dgm = _bf(dgm)
    B = -a * invstd * dgm
    K = a * _fma(mean * invstd, dgm, -dbm, fused)
    dx = _fma(a, dz, _fma(B, x, K, fused), fused)
    return dg, db, dx, dz


@pytest.mark.parametrize('out', ['bf16', 'f32'])
@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('mask', [0, 1, 2])
def test_bn_bwd_float32_passes_and_faults_are_flagged(out, fused, mask):
    gen = torch.Generator().manual_seed(11 + mask)
    M, Cc = 650, 16
    x = _store(torch.randn(M, Cc, generator=gen) * 2 + 0.5, out)
    dy = _store(torch.randn(M, Cc, generator=gen), out)
    gam = torch.rand(Cc, generator=gen) + 0.5
    mean, var = x.mean(0), x.var(0, unbiased=False)
    invstd = 1 / torch.sqrt(var + 1e-3)
    scale = gam * invstd
    shift = torch.randn(Cc, generator=gen) * 0.2 - mean * scale
    y = _store((x * scale + shift).clamp_min(0), out)
    ref = ob.BnBwd(x, dy, gam, mean, invstd, mask, y=y, scale=scale, shift=shift, tile=256)
    assert ref.amb_frac == 0.0
    on = torch.ones_like(x, dtype=torch.bool) if mask == 0 else (y > 0 if mask == 1 else _fma(x, scale, shift, fused) > 0)
    dg, db, dx, dz = _bn_bwd_like(x, dy, on, gam, mean, invstd, M, fused)
    ref.check_params('bn_bwd', dg, db)
    r = ref.check_dx('bn_bwd', _store(dx, out), out)
    assert r.ratio < 1.0 and (r.frac is None or r.frac <= ob.MISMATCH_MAX)
    # accumulating forms
    old = _store(torch.randn(M, Cc, generator=gen), out)
    ref.check_dx('bn_bwd', _store(dx + old, out), out, old=old)
    ref.check_dres('bn_bwd', _store(dz + old, out), out, old=old)
    ref.check_params('bn_bwd', dg + 3.0, db - 2.0, old_dgamma=torch.full((Cc,), 3.0), old_dbeta=torch.full((Cc,), -2.0))
    _flagged(lambda: ref.check_dres('bn_bwd', _store(dz, out), out, old=old))              # dres overwritten where it should accumulate
    _flagged(lambda: ref.check_dx('bn_bwd', _store(dx, out), out, old=old))
    _flagged(lambda: ref.check_params('bn_bwd', dg, db, old_dgamma=torch.full((Cc,), 3.0), old_dbeta=torch.full((Cc,), -2.0)))
    # one dropped row in the last, partial tile
    dg2, db2, _, _ = _bn_bwd_like(x, dy, on, gam, mean, invstd, M, fused, drop=M - 3)
    _flagged(lambda: ref.check_params('bn_bwd', dg2, db2))
    # dgamma / M rounded to bf16
    _, _, dx3, _ = _bn_bwd_like(x, dy, on, gam, mean, invstd, M, fused, bf16_dg=True)
    _flagged(lambda: ref.check_dx('bn_bwd', _store(dx3, out), out))


def test_bn_bwd_ambiguous_mask_accepts_both_sides_and_is_counted():
    x = torch.tensor([[1.0], [2.0], [3.0], [-1.0]])
    scale, shift = torch.tensor([0.5]), torch.tensor([-1.0])               # x = 2: the pre-activation is exactly 0
    dy = torch.tensor([[1.0], [1.0], [1.0], [1.0]])
    ref = ob.BnBwd(x, dy, torch.ones(1), torch.tensor([1.25]), torch.tensor([0.7]), 2, scale=scale, shift=shift)
    assert ref.amb_frac == 0.25
    with pytest.raises(AssertionError, match='ambiguous'):
        ref.check_params('amb', ref.dgamma, ref.dbeta)
    for dz in (ref.dz, torch.where(ref.amb, dy.double(), ref.dz)):
        assert ref.check_dres('amb', dz, 'f32').ratio <= 1.0


# ------------------------------------------------------------------------------------------------------ head
@pytest.mark.parametrize('C,NC,N', [(2048, 100, 9), (4096, 10, 5), (512, 2, 19)])
def test_head_float32_passes_and_a_dropped_term_is_flagged(C, NC, N):
    gen = torch.Generator().manual_seed(C)
    x = _bf(torch.rand(N, 7, C, generator=gen))
    mask = (torch.rand(N, C, generator=gen) > 0.5).float()
    feat = _shuffled_sum(x, 1) * torch.tensor(1 / 7.0) * (mask * 2.0)
    ref, A, n = ob.gap(x, mask, 2.0)
    assert ob.check_sum('gap', feat, ref, A, n, 'f32', dims=('n', 'c')).ratio < 1.0
    _flagged(lambda: ob.check_sum('gap', _bf(_shuffled_sum(x, 1)) * torch.tensor(1 / 7.0) * (mask * 2.0), ref, A, n, 'f32', dims=('n', 'c')))
    W, b = torch.randn(NC, C, generator=gen) * 0.05, torch.randn(NC, generator=gen) * 0.1
    prod = feat[:, None, :] * W[None]
    lg = _shuffled_sum(prod, 2) + b
    ref, A, n = ob.fc_fwd(feat, W, b)
    assert ob.check_sum('fc', lg, ref, A, n, 'f32', dims=('n', 'j')).ratio < 1.0
    if C <= 2048:           # (detection limit, as for the convs: past a few thousand terms one term hides inside gamma_n * A)
        prod[N - 1, NC - 1, int(prod[N - 1, NC - 1].abs().argmax())] = 0
        _flagged(lambda: ob.check_sum('fc', _shuffled_sum(prod, 2) + b, ref, A, n, 'f32', dims=('n', 'j')))
    dl = torch.randn(N, NC, generator=gen) / N
    ref, A, n = ob.fc_wgrad(dl, feat)
    dW = _shuffled_sum(dl[:, :, None] * feat[:, None, :], 0)
    assert ob.check_sum('wgrad', dW, ref, A, n, 'f32', dims=('j', 'c')).ratio < 1.0
    assert ob.check_sum('wgrad', dW + 1.0, ref, A, n, 'f32', old=torch.ones_like(dW), dims=('j', 'c')).ratio < 1.0
    ref, A, n = ob.head_dx(dl, W, mask, 2.0, 7, C)
    g = _shuffled_sum(dl[:, :, None] * W[None], 1) * torch.tensor(1 / 7.0) * (mask * 2.0)
    assert ob.check_sum('head_dx', _bf(g), ref, A, n, 'bf16', dims=('n', 'c')).ratio < 1.0


# ------------------------------------------------------------------------------------------------------ softmax, cross-entropy
def _softmax32(l):
    mx = l.max(1, keepdim=True).values
    ex = torch.exp(l - mx)
    return ex / _shuffled_sum(ex, 1)[:, None]


def test_softmax_spread_8_and_1000_classes_needs_the_argument_term():
    gen = torch.Generator().manual_seed(8)
    l = torch.randn(64, 1000, generator=gen) * 8
    for p32 in (torch.softmax(l, 1), _softmax32(l)):
        p, e, _ = ob.softmax(l)
        r = ob.elem('softmax', p32, p, e, 'f32', dims=('n', 'j'))
        assert r.ratio < 1.0
        rel = ((p32.double() - p).abs() / p)[p > 1e-30].max().item() / ob.U
        print('spread 8, 1000 classes: worst relative error of a float32 softmax %.1f u' % rel)
        assert rel > 2 * ob.E_LIBM + 2                  # more than exp's own error explains: the rounding of l_j - max
    # with few classes gamma_NC is small, and without the argument term a correct float32 softmax is refused
    l = torch.randn(4000, 5, generator=gen) * 8
    p, e, _ = ob.softmax(l)
    assert ob.elem('softmax', torch.softmax(l, 1), p, e, 'f32', dims=('n', 'j')).ratio < 1.0
    p, e0, _ = ob.softmax(l, arg_term=False)
    _flagged(lambda: ob.elem('softmax', torch.softmax(l, 1), p, e0, 'f32', dims=('n', 'j')))


@pytest.mark.parametrize('N,NC,shift', [(7, 100, 0.0), (300, 5, 80.0), (33, 3, -80.0), (1, 1, 0.0)])
def test_xent_float32_passes_and_faults_are_flagged(N, NC, shift):
    gen = torch.Generator().manual_seed(N)
    l = torch.randn(N, NC, generator=gen) * 3 + shift
    t = torch.randint(0, NC, (N,), generator=gen)
    w = 0.4
    want = ob.xent(l, t, w, old_loss=5.0)
    p32 = _softmax32(l)
    oh = torch.nn.functional.one_hot(t, NC).float()
    dl = torch.tensor(w) * torch.tensor(1.0 / N) * (p32 - oh)
    mx = l.max(1).values
    li = mx + torch.log(_shuffled_sum(torch.exp(l - mx[:, None]), 1)) - l[torch.arange(N), t]
    loss = _shuffled_sum(li, 0) * torch.tensor(1.0 / N) * torch.tensor(w) + 5.0
    assert ob.check_dict('xent', {'dlogits': dl, 'loss': loss.reshape(1)}, want) < 1.0
    if NC > 1:
        _flagged(lambda: ob.check_dict('xent', {'dlogits': torch.tensor(w / N) * (_bf(p32) - oh)}, want))       # a bf16-rounded probability
    _flagged(lambda: ob.check_dict('xent', {'loss': loss.reshape(1) - 5.0}, want))                              # loss overwritten


def test_softmax_without_max_subtraction_is_flagged_near_90():
    l = torch.tensor([[90.0, 89.0, 88.5], [91.0, 60.0, 90.5]])
    p, e, _ = ob.softmax(l)
    ex = torch.exp(l)                                        # exp(90) overflows fp32
    _flagged(lambda: ob.elem('softmax', ex / ex.sum(1, keepdim=True), p, e, 'f32', dims=('n', 'j')))
    assert ob.elem('softmax', _softmax32(l), p, e, 'f32', dims=('n', 'j')).ratio < 1.0


# ------------------------------------------------------------------------------------------------------ optimizers
def _adam32(p, g, m, v, lr, b1, b2, eps, wd, step, gs, fused, eps_inside=False, wd_after=False):
    T = lambda s: torch.tensor(s, dtype=torch.float32)
    bc1 = T(1.0) - T(float(T(b1)) ** step)
    sbc2 = torch.sqrt(T(1.0) - T(float(T(b2)) ** step))
    gr = g * T(gs) if wd_after else _fma(g, T(gs), T(wd) * p, fused)
    m2 = _fma(T(b1), m, (T(1.0) - T(b1)) * gr, fused)
    v2 = _fma(T(b2), v, (T(1.0) - T(b2)) * gr * gr, fused)
    den = torch.sqrt(v2 + T(eps)) / sbc2 if eps_inside else torch.sqrt(v2) / sbc2 + T(eps)
    p2 = _fma(-(T(lr) / bc1), m2 / den, p, fused)
    if wd_after:
        p2 = p2 - T(lr) * T(wd) * p
    return {'p': p2, 'm': m2, 'v': v2}


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('step', [1, 2, 1000])
@pytest.mark.parametrize('wd,gs', [(0.0, 1.0), (0.01, 1 / 128)])
def test_adam_float32_passes_and_faults_are_flagged(fused, step, wd, gs):
    gen = torch.Generator().manual_seed(step)
    n = 4001
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 10 ** (torch.rand(n, generator=gen) * 11 - 8)       # 1e-8 .. 1e3
    g[::7] = 0.0
    m = torch.randn(n, generator=gen) * 0.1 if step > 1 else torch.zeros(n)
    v = torch.rand(n, generator=gen) * 0.01 if step > 1 else torch.zeros(n)
    v[::7], m[::7] = 0.0, 0.0                                                              # v = 0: denom = eps
    a = (1e-3, 0.9, 0.999, 1e-8, wd, step, gs)
    want = ob.adam(p, g, m, v, *a)
    assert ob.check_dict('adam', _adam32(p, g, m, v, *a, fused), want) < 1.0
    _flagged(lambda: ob.check_dict('adam', _adam32(p, g, m, v, *a, fused, eps_inside=True), want))      # eps inside the square root
    if wd:
        _flagged(lambda: ob.check_dict('adam', _adam32(p, g, m, v, *a, fused, wd_after=True), want))    # weight decay after the moments


@pytest.mark.parametrize('mu', [0.0, 0.9])
@pytest.mark.parametrize('wd,gs', [(0.0, 1.0), (0.01, 1 / 128)])
def test_sgd_float32_passes(mu, wd, gs):
    gen = torch.Generator().manual_seed(4)
    n = 1003
    p, g, mom = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    T = lambda s: torch.tensor(s, dtype=torch.float32)
    for fused in (True, False):
        gr = _fma(g, T(gs), T(wd) * p, fused)
        got = {}
        if mu:
            gr = _fma(T(mu), mom, gr, fused)
            got['mom'] = gr
        got['p'] = _fma(-T(0.05), gr, p, fused)
        want = ob.sgd(p, g, mom if mu else None, 0.05, mu, wd, gs)
        assert ob.check_dict('sgd', got, want) < 1.0
        if mu:
            _flagged(lambda: ob.check_dict('sgd', {'p': _fma(-T(0.05), _fma(T(mu), mom, gr, fused), p, fused)}, want))   # momentum twice
