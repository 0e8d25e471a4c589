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
