"""The per-element checker of tests/conv_bounds.py is not vacuous: simulated kernel faults, built with torch on the CPU from an exact
float64 result, are flagged, and a correct fp32 accumulation in a shuffled order, rounded once, passes.

Reduction lengths are those of the GPU case tables: 288 (32 x 3x3), 1344 (192 x 1x7), 2048 (1x1 over 2048 channels), 4032 (448 x 3x3)
for the forward; N*P*Q up to 2000 for weight gradients, where a single term is still larger than 2 * gamma_n * A64 (past about
N*P*Q = 5000 one dropped term of a unit-variance weight gradient hides inside the bound; see the module docstring)."""
import pytest
import torch

import conv_bounds as cb


def _bf(t):
    return t.to(torch.bfloat16).to(torch.float32)


def _fwd_case(C, R, S, K=8, N=1, H=6, W=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = _bf(torch.randn(N, C, H, W, generator=g))
    w = _bf(torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5)
    return x, w


def _products(x, w, pad):
    """fp32 products [N*P*Q, K, C*R*S] (exact for bf16 operands) and the output shape"""
    N, C, H, W = x.shape
    K, _, R, S = w.shape
    cols = torch.nn.functional.unfold(x, (R, S), padding=pad)             # [N, C*R*S, L]
    P, Q = H + 2 * pad[0] - R + 1, W + 2 * pad[1] - S + 1
    prod = cols.permute(0, 2, 1).reshape(-1, 1, C * R * S) * w.reshape(1, K, -1)
    return prod, (N, P, Q, K)


def _fp32_sum(prod, seed=1, splits=1, round_partials=False):
    """sequential fp32 sum over the last axis in a shuffled order, optionally in `splits` partial sums"""
    g = torch.Generator().manual_seed(seed)
    n = prod.shape[-1]
    perm = torch.randperm(n, generator=g)
    p = prod[..., perm].float()
    parts = []
    for chunk in torch.tensor_split(torch.arange(n), splits):
        acc = torch.zeros(p.shape[:-1], dtype=torch.float32)
        for i in chunk.tolist():
            acc = acc + p[..., i]
        parts.append(_bf(acc) if round_partials else acc)
    out = torch.zeros_like(parts[0])
    for q in parts:
        out = out + q
    return out


def _kernel_like(prod, shape, **kw):
    return _fp32_sum(prod, **kw).reshape(shape)


FWD = [(32, 3, 3), (192, 1, 7), (2048, 1, 1), (448, 3, 3)]


@pytest.mark.parametrize('C,R,S', FWD)
def test_correct_shuffled_fp32_accumulation_passes(C, R, S):
    x, w = _fwd_case(C, R, S, H=6 if R > 1 else 4, W=8 if S > 1 else 4)
    ref, A, n = cb.fwd(x, w)
    prod, shape = _products(x, w, (0, 0))
    y = _bf(_kernel_like(prod, shape))
    r = cb.check('fwd', y, ref, A, n)
    assert r.ratio < 1.0 and r.frac <= cb.MISMATCH_MAX


@pytest.mark.parametrize('C,R,S', FWD)
def test_dropped_reduction_term_is_flagged(C, R, S):
    x, w = _fwd_case(C, R, S, H=6 if R > 1 else 4, W=8 if S > 1 else 4, seed=2)
    ref, A, n = cb.fwd(x, w)
    prod, shape = _products(x, w, (0, 0))
    m, k = prod.shape[0] // 2, 3
    i = int(prod[m, k].abs().argmax())                # the largest term of one output element goes missing
    prod[m, k, i] = 0
    y = _bf(_kernel_like(prod, shape))
    r = cb.check('fwd', y, ref, A, n, raise_=False)
    assert r.nbad >= 1 and r.ratio > 1.0, r


def test_missing_last_channel_chunk_in_m_tail_row_is_flagged():
    C, R, S = 72, 1, 7                                # 72 = 64 + a chunk tail of 8
    x, w = _fwd_case(C, R, S, K=16, N=3, H=5, W=9, seed=3)
    ref, A, n = cb.fwd(x, w, 1, (0, 3))
    prod, shape = _products(x, w, (0, 3))
    taps = torch.arange(C * R * S).reshape(C, R * S)[C - 8:].flatten()       # unfold order: c major
    prod[-1, :, taps] = 0                             # the last pixel (M tail) misses channels 64..71 of every tap
    y = _bf(_kernel_like(prod, shape))
    r = cb.check('fwd', y, ref, A, n, raise_=False)
    assert r.nbad >= 1, r
    assert r.msg.split('worst at (n, p, q, k) = ')[1].startswith('(2, 4, 8,')      # reported at the faulty pixel


def test_split_k_partials_rounded_to_bf16_are_flagged():
    x, w = _fwd_case(192, 1, 7, K=16, H=5, W=10, seed=4)
    ref, A, n = cb.fwd(x, w)
    prod, shape = _products(x, w, (0, 0))
    y = _bf(_kernel_like(prod, shape, splits=4, round_partials=True))
    r = cb.check('fwd', y, ref, A, n, raise_=False)
    assert r.frac > cb.MISMATCH_MAX, r
    # the same split with fp32 partials is fine
    assert cb.check('fwd', _bf(_kernel_like(prod, shape, splits=4)), ref, A, n).frac <= cb.MISMATCH_MAX


def test_swapped_output_channels_are_flagged():
    x, w = _fwd_case(96, 3, 3, K=32, seed=5)
    ref, A, n = cb.fwd(x, w)
    prod, shape = _products(x, w, (0, 0))
    y = _bf(_kernel_like(prod, shape))
    y[..., [17, 18]] = y[..., [18, 17]]
    r = cb.check('fwd', y, ref, A, n, raise_=False)
    assert r.nbad > 0 and r.frac > cb.MISMATCH_MAX, r


def test_padding_tap_read_as_neighbour_is_flagged():
    x, w = _fwd_case(64, 3, 3, K=8, H=7, W=7, seed=6)
    ref, A, n = cb.fwd(x, w, 1, 1)
    y = _bf(ref.float())
    # output (0, 0, 3, k): its tap r = 0 falls on the padding row -1 and should read zeros; it reads row 0 instead
    k = 5
    y[0, 0, 3, k] = _bf(ref[0, 0, 3, k].float() + (w[k, :, 0, :].double() * x[0, :, 0, 2:5].double()).sum().float())
    r = cb.check('fwd', y, ref, A, n, raise_=False)
    assert r.nbad == 1 and 'worst at (n, p, q, k) = (0, 0, 3, 5)' in r.msg, r


@pytest.mark.parametrize('N,H,W', [(2, 10, 10), (2, 22, 22), (5, 20, 20)])
def test_weight_gradient_bounds(N, H, W):
    """fp32 weight gradient, N*P*Q = 128 / 800 / 1800: a correct split-K fp32 result passes, one dropped term fails, and so do
    bf16-rounded split partials"""
    g = torch.Generator().manual_seed(N * H)
    C, K, R, S = 16, 8, 3, 3
    x = _bf(torch.randn(N, C, H, W, generator=g))
    P, Q = H - 2, W - 2
    dy = _bf(torch.randn(N, K, P, Q, generator=g))
    ref, A, n = cb.wgrad(x, dy, (K, C, R, S))
    assert n == N * P * Q
    cols = torch.nn.functional.unfold(x, (R, S))                               # [N, C*R*S, P*Q]
    prod = (dy.reshape(N, K, 1, P * Q) * cols.reshape(N, 1, C * R * S, P * Q)).permute(1, 2, 0, 3).reshape(K, C * R * S, -1)
    to_krsc = lambda t: t.reshape(K, C, R, S).permute(0, 2, 3, 1)
    good = to_krsc(_fp32_sum(prod, splits=6))
    assert cb.check('wgrad', good, ref, A, n, out='f32', dims=('k', 'r', 's', 'c')).ratio < 1.0
    bad = prod.clone()
    i = int(bad[3, 50].abs().argmax())
    bad[3, 50, i] = 0
    r = cb.check('wgrad', to_krsc(_fp32_sum(bad, splits=6)), ref, A, n, out='f32', dims=('k', 'r', 's', 'c'), raise_=False)
    assert r.nbad >= 1, r
    r = cb.check('wgrad', to_krsc(_fp32_sum(prod, splits=6, round_partials=True)), ref, A, n, out='f32', raise_=False)
    assert r.nbad >= 1, r


def test_input_gradient_counts_the_taps_that_hit():
    g = torch.Generator().manual_seed(8)
    dy = _bf(torch.randn(1, 8, 4, 4, generator=g))
    w = _bf(torch.randn(8, 16, 3, 3, generator=g))
    ref, A, n = cb.dgrad(dy, w, (1, 16, 6, 6))
    assert float(n[0, 0, 0, 0]) == 8 and float(n[0, 2, 2, 0]) == 9 * 8 and float(n[0, 0, 2, 0]) == 3 * 8
    assert torch.allclose(ref, torch.nn.grad.conv2d_input((1, 16, 6, 6), w.double(), dy.double()).permute(0, 2, 3, 1))


def test_accumulate_and_affine_forms():
    x, w = _fwd_case(192, 1, 7, K=16, H=4, W=9, seed=9)
    ref, A, n = cb.fwd(x, w, 1, (0, 3))
    prod, shape = _products(x, w, (0, 3))
    acc = _kernel_like(prod, shape)
    g = torch.Generator().manual_seed(10)
    old = _bf(torch.randn(shape, generator=g))
    y = _bf(_bf(acc) + old)                            # the shared epilogue: contribution rounded, then added
    assert cb.check('acc', y, ref, A, n, old=old).frac <= cb.MISMATCH_MAX
    assert cb.check('acc', _bf(acc + old), ref, A, n, old=old).frac <= cb.MISMATCH_MAX
    r = cb.check('acc', _bf(acc), ref, A, n, old=old, raise_=False)                    # the old value lost
    assert r.nbad > 0
    scale, shift = torch.rand(16, generator=g) + 0.5, torch.randn(16, generator=g) * 0.3
    res = _bf(torch.randn(shape, generator=g))
    y = _bf(torch.relu(_bf(acc) * scale + shift + res))
    assert cb.check_affine('aff', y, ref, A, n, scale, shift, res, relu=True).ratio < 1.0
    y = _bf(torch.relu(_bf(acc) * scale + shift))                                     # the residual not added
    assert cb.check_affine('aff', y, ref, A, n, scale, shift, res, relu=True, raise_=False).nbad > 0


def test_statistics_sums():
    g = torch.Generator().manual_seed(11)
    y = _bf(torch.randn(5000, 24, generator=g))
    part = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in y.split(128)])     # fp32 partial rows
    cb.check_bn_fwd_sums('bn', part, y)
    part[7, :, 3] = 0                                  # one partial row of one channel not written (a 128-pixel tile lost)
    with pytest.raises(AssertionError, match='sum: 1 of 24'):
        cb.check_bn_fwd_sums('bn', part, y)


# ------------------------------------------------------------------------------------------------------ operands of a layer in a network
# The twin of test_gpu_conv_f32_bounds.F32['l4ds-net'] (resnet18's layer4.0.downsample.0: 1x1 over 256 channels, fp32): a non-negative
# post-ReLU input and filters with a common offset.  Every product is then positive: A = sum |x||w| equals |sum x w|, the raw output's
# mean is several of its standard deviations and the statistics' sums cancel nothing.  The bound must still accept a correct fp32
# accumulation in any order and still reject one dropped term, one dropped statistics row.
def _net_case(C=256, K=16, N=2, H=7, W=7, seed=20):
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(N, C, H, W, generator=g))
    w = torch.randn(K, C, 1, 1, generator=g) / C ** 0.5 + 2.0 / C ** 0.5
    raw = torch.nn.functional.conv2d(x, w)
    assert float((raw.mean((0, 2, 3)) / raw.std((0, 2, 3))).min()) > 4.0
    return x, w


def test_net_distribution_shuffled_fp32_accumulation_passes_and_a_dropped_term_is_flagged():
    x, w = _net_case()
    ref, A, n = cb.fwd(x, w)
    assert float((A / ref.abs()).max()) < 1.5          # (nothing cancels: the bound is relative to the result itself)
    prod, shape = _products(x, w, (0, 0))
    assert cb.check('fwd net', _kernel_like(prod, shape), ref, A, n, out='f32').ratio < 1.0
    assert cb.check('fwd net', _kernel_like(prod, shape, splits=4), ref, A, n, out='f32').ratio < 1.0
    m, k = prod.shape[0] // 2, 3
    prod[m, k, int(prod[m, k].abs().argmax())] = 0    # the largest term of one output element goes missing
    r = cb.check('fwd net', _kernel_like(prod, shape), ref, A, n, out='f32', raise_=False)
    assert r.nbad >= 1 and r.ratio > 1.0, r


def test_net_distribution_weight_gradient():
    """fp32 weight gradient of the same layer (N*P*Q = 98, one split in the kernel): the post-ReLU input against a zero-mean upstream
    gradient; correct passes, a dropped term fails"""
    x, _ = _net_case()
    g = torch.Generator().manual_seed(21)
    N, C, H, W = x.shape
    K = 8
    dy = torch.randn(N, K, H, W, generator=g)
    dy = dy - dy.mean((0, 2, 3), keepdim=True)          # a BatchNorm-backward output has zero per-channel mean
    ref, A, n = cb.wgrad(x, dy, (K, C, 1, 1))
    prod = (dy.reshape(N, K, 1, H * W) * x.reshape(N, 1, C, H * W)).permute(1, 2, 0, 3).reshape(K, C, -1)
    to_krsc = lambda t: t.reshape(K, C, 1, 1).permute(0, 2, 3, 1)
    assert cb.check('wgrad net', to_krsc(_fp32_sum(prod)), ref, A, n, out='f32', dims=('k', 'r', 's', 'c')).ratio < 1.0
    bad = prod.clone()
    bad[3, 50, int(bad[3, 50].abs().argmax())] = 0
    r = cb.check('wgrad net', to_krsc(_fp32_sum(bad)), ref, A, n, out='f32', dims=('k', 'r', 's', 'c'), raise_=False)
    assert r.nbad >= 1, r


def test_net_distribution_statistics_sums():
    x, w = _net_case(N=6, H=14, W=14, K=24)
    y = torch.nn.functional.conv2d(x, w).permute(0, 2, 3, 1).reshape(-1, 24)          # 1176 rows, mean >> spread
    part = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in y.split(128)])     # fp32 partial rows
    cb.check_bn_fwd_sums('bn net', part, y)
    part[7, :, 3] = 0                                  # one partial row of one channel not written
    with pytest.raises(AssertionError, match='sum: 1 of 24'):
        cb.check_bn_fwd_sums('bn net', part, y)
    part = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in y.split(128)])
    part[8, 1, 5] = part[8, 1, 5] * (1 + 2.0 ** -8)     # one row's sum of squares off in its 8th bit (a variance a little large)
    with pytest.raises(AssertionError, match='sumsq: 1 of 24'):
        cb.check_bn_fwd_sums('bn net', part, y)


# ------------------------------------------------------------------------------------------------------ the u8 stem
# conv_stem_u8.hip emulated step by step in torch on the CPU (fp32 operations as the kernels order them); the bounds of
# conv_bounds.stem_u8_fwd / stem_u8_wgrad accept the emulation and reject its subtly wrong variants.
AB = (0.458 / (255 * 0.229), 0.448 / (255 * 0.224), 0.45 / (255 * 0.225), -0.03 - 0.458 * 0.485 / 0.229, -0.088 - 0.448 * 0.456 / 0.224,
      -0.188 - 0.45 * 0.406 / 0.225)


def _fma(a, b, c):
    """fp32 a * b + c rounded once (the product of a u8 or bf16 value and an fp32 value is exact in double)"""
    return (a.double() * b.double() + c.double()).float()


def _stem_case(N=3, H=41, W=75, seed=0):
    gen = torch.Generator().manual_seed(seed)
    g = torch.randint(0, 256, (N, H, W), generator=gen, dtype=torch.uint8)
    w = torch.randn(32, 3, 3, 3, generator=gen) * 0.2
    return g, w, torch.tensor(AB, dtype=torch.float32)


def _stem_taps(w, ab):
    """the kernels' fp32 effective taps [K][9] and bias [K]"""
    wk = w.reshape(32, 9, 3)
    we = _fma(wk[..., 2], ab[2], _fma(wk[..., 1], ab[1], wk[..., 0] * ab[0]))
    b = torch.zeros(32)
    for t in range(9):
        b = b + _fma(wk[:, t, 2], ab[5], _fma(wk[:, t, 1], ab[4], wk[:, t, 0] * ab[3]))
    return we, b


def _stem_patches(g):
    N, H, W = g.shape
    cols = torch.nn.functional.unfold(g.float()[:, None], (3, 3), stride=2)        # [N, 9, P*Q]
    P, Q = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    return cols.permute(0, 2, 1).reshape(N, P, Q, 9), P, Q


def _split(x, pieces):
    out, r = [], x.clone()
    for _ in range(pieces):
        p = _bf(r)
        out.append(p)
        r = r - p
    return out


def _stem_fwd_vector(g, w, ab):
    we, b = _stem_taps(w, ab)
    pt, P, Q = _stem_patches(g)
    v = b.expand(*pt.shape[:3], 32).clone()
    for t in range(9):
        v = _fma(pt[..., t:t + 1], we[:, t], v)
    return v


def _stem_fwd_mfma(g, w, ab, pieces=3):
    """27 + 3 exact products summed in fp32, slot by slot in the order of the two MFMA operands"""
    we, b = _stem_taps(w, ab)
    pt, P, Q = _stem_patches(g)
    wp, bp = _split(we, pieces), _split(b, pieces)
    acc = torch.zeros(*pt.shape[:3], 32)
    for piece in wp[:1] + bp + wp[1:]:
        if piece.dim() == 1:
            acc = acc + piece
        else:
            for t in range(9):
                acc = acc + pt[..., t:t + 1] * piece[:, t]
    return acc


@pytest.mark.parametrize('out', ['bf16', 'fp32'])
def test_stem_forward_bound_accepts_the_vector_emulation_and_rejects_one_storage_ulp(out):
    g, w, ab = _stem_case()
    ref, e = cb.stem_u8_fwd(g, w, ab, mfma=False)
    tdt = torch.bfloat16 if out == 'bf16' else torch.float32
    y = _stem_fwd_vector(g, w, ab).to(tdt)
    r = cb.check_e('vector', y, ref, e, out)
    assert r.ratio < 1 and (r.frac is None or r.frac < cb.MISMATCH_MAX)
    bad = y.clone().float()
    x = bad[1, 7, 11, 5]
    # one storage ulp in bf16; in fp32 storage the counted roundings are themselves ~200 u of the magnitudes: 2^-15 there
    bad[1, 7, 11, 5] = x + (float(cb.ulp(x.double().abs(), out)) if out == 'bf16' else 2.0 ** -15)
    assert cb.check_e('ulp', bad, ref, e, out, raise_=False).nbad == 1
    # the eval epilogue: scale and shift of the wrong channel
    sc, sh = torch.rand(32) + 0.5, torch.randn(32) * 0.3
    want, e_lin = cb.stem_affine(ref, e, sc, sh, True)
    ya = _fma(_stem_fwd_vector(g, w, ab), sc, sh).clamp_min(0).to(tdt)
    assert cb.check_e('affine', ya, want, e_lin, out).ratio < 1
    yb = _fma(_stem_fwd_vector(g, w, ab), sc.roll(1), sh).clamp_min(0).to(tdt)
    assert cb.check_e('affine', yb, want, e_lin, out, raise_=False).nbad > 0
    # a border: the last output column computed from the column before it
    bad = y.clone()
    bad[:, :, -1] = bad[:, :, -2]
    assert cb.check_e('border', bad, ref, e, out, raise_=False).nbad > 0


def test_stem_mfma_bound_accepts_three_bf16_pieces_and_rejects_two():
    """the split of a tap into bf16 pieces: three represent it to 2^-24 (the bound's term u * mag), two only to 2^-16.  The pieces'
    error is invisible in the bf16 OUTPUT of a single element's rounding, so the bound is held against the fp32 accumulator here
    (out='fp32'), and on the GPU against the stored bf16 value, where it shows as the mismatch fraction and the bound together"""
    g, w, ab = _stem_case(N=4, H=75, W=75, seed=1)
    ref, e = cb.stem_u8_fwd(g, w, ab, mfma=True)
    acc3, acc2 = _stem_fwd_mfma(g, w, ab, 3), _stem_fwd_mfma(g, w, ab, 2)
    r3 = cb.check_e('three pieces', acc3, ref, e, 'fp32')
    assert r3.ratio < 1
    r2 = cb.check_e('two pieces', acc2, ref, e, 'fp32', raise_=False)
    assert r2.nbad > 0 and r2.ratio > 1, r2
    rb = cb.check_e('three pieces, bf16 store', acc3.to(torch.bfloat16), ref, e, 'bf16')
    assert rb.frac < cb.MISMATCH_MAX


def _stem_wgrad_emulated(g, dy, ab, drop=None):
    """fp32 partial sums per 32 pixels (sequential), combined in double, a_c A + b_c S rounded once"""
    pt, P, Q = _stem_patches(g)
    d = dy.float()
    if drop is not None:
        n, p, q0 = drop
        d = d.clone()
        d[n, p, q0:] = 0
    cols = torch.cat([pt, torch.ones(*pt.shape[:3], 1)], -1).reshape(-1, 10)                  # [M, 10]
    dm = d.reshape(-1, 32)
    tot = torch.zeros(32, 10, dtype=torch.float64)
    for i in range(0, cols.shape[0], 32):
        acc = torch.zeros(32, 10)
        for j in range(i, min(i + 32, cols.shape[0])):
            acc = acc + dm[j][:, None] * cols[j][None]
        tot += acc.double()
    a = ab.double()
    return (tot[:, :9].reshape(32, 3, 3, 1) * a[:3] + tot[:, 9].reshape(32, 1, 1, 1) * a[3:]).float()


@pytest.mark.parametrize('mfma', [False, True])
def test_stem_wgrad_bound_rejects_a_missing_last_pixel_group_of_one_row(mfma):
    g, w, ab = _stem_case(N=2, H=21, W=83, seed=2)                    # Q = 41: groups of 32 + 9
    P, Q = 10, 41
    dy = _bf(torch.randn(2, P, Q, 32, generator=torch.Generator().manual_seed(3)))
    ref, e = cb.stem_u8_wgrad(g, dy, ab, mfma)
    good = _stem_wgrad_emulated(g, dy, ab)
    assert cb.check_stem_wgrad('good', good, ref, e).ratio < 1
    bad = _stem_wgrad_emulated(g, dy, ab, drop=(1, 4, 32))
    r = cb.check_stem_wgrad('dropped group', bad, ref, e, raise_=False)
    assert r.nbad > 32 * 27 // 2, r
    one = _stem_wgrad_emulated(g, dy, ab, drop=(1, 9, 40))           # the last pixel of the last row alone
    assert cb.check_stem_wgrad('dropped pixel', one, ref, e, raise_=False).nbad > 0
    base = torch.randn(32, 3, 3, 3)
    assert cb.check_stem_wgrad('acc', base + good, ref, e, old=base).ratio < 1
    assert cb.check_stem_wgrad('acc twice', base + good + good, ref, e, old=base, raise_=False).nbad > 0


# ------------------------------------------------------------------------------------------------------ the fp32 affine epilogue
# conv_igemm<float> emulated on the CPU: the fp32 MFMA as a sequential fma chain over the reduction, then fmaf(acc, scale, shift), an
# fp32 add of the residual, the ReLU; reduction lengths Cw * R * S of the fp32 table of test_gpu_conv_f32_bounds.py
F32_AFFINE = [(12, 3, 3), (3, 3, 3), (64, 1, 1), (48, 1, 7), (24, 3, 3)]          # 108, 27, 64, 336, 216


def _f32_affine_emulated(x, w, pad, scale, shift, res, drop=None):
    N, C, H, W = x.shape
    K, _, R, S = w.shape
    cols = torch.nn.functional.unfold(x, (R, S), padding=pad).permute(0, 2, 1).reshape(-1, 1, C * R * S)      # [M, 1, n]
    wr = w.reshape(1, K, -1).expand(cols.shape[0], K, -1).clone()
    if drop is not None:
        m, k = drop
        wr[m, k, int((cols[m, 0] * wr[m, k]).abs().argmax())] = 0           # the largest product of one output element goes missing
    acc = torch.zeros(cols.shape[0], K)
    for i in range(cols.shape[-1]):
        acc = _fma(cols[..., i], wr[..., i], acc)
    P, Q = H + 2 * pad[0] - R + 1, W + 2 * pad[1] - S + 1
    v = _fma(acc.reshape(N, P, Q, K), scale, shift)
    return torch.relu(v + res)


@pytest.mark.parametrize('C,R,S', F32_AFFINE)
def test_f32_affine_bound_accepts_the_fma_chain_and_rejects_a_dropped_product(C, R, S):
    g = torch.Generator().manual_seed(20 + C * R * S)
    K, N, H, W = 8, 2, 5, 9
    pad = (R // 2, S // 2)
    x = torch.randn(N, C, H, W, generator=g)
    w = torch.randn(K, C, R, S, generator=g) / (C * R * S) ** 0.5
    scale, shift = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3
    res = torch.randn(N, H, W, K, generator=g)
    ref, A, n = cb.fwd(x, w, 1, pad)
    assert n == C * R * S
    y = _f32_affine_emulated(x, w, pad, scale, shift, res)
    r = cb.check_affine('f32 affine', y, ref, A, n, scale, shift, res, relu=True, out='f32')
    assert r.ratio < 1.0 and r.frac is None
    pre = scale.double() * ref + shift.double() + res.double()
    m = int(pre[..., 3].flatten().argmax())                                 # an element the ReLU passes
    bad = _f32_affine_emulated(x, w, pad, scale, shift, res, drop=(m, 3))
    r = cb.check_affine('f32 affine', bad, ref, A, n, scale, shift, res, relu=True, out='f32', raise_=False)
    assert r.nbad == 1 and r.ratio > 1.0, r
    # the bf16 form of the same call is unchanged by the new parameter: an fp32 result is not a bf16 store
    r = cb.check_affine('bf16 affine', _bf(y), ref, A, n, scale, shift, res, relu=True)
    assert r.frac is not None
