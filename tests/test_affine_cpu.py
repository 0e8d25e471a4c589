"""The host arithmetic of a random affine (CPU): the integer model of tests/affine_cases.py against the installed Pillow's
Image.transform bit for bit on every rotated case, exact properties for the unrotated ones, the border fill, the coefficient function
of neuston_data against the twin, range parsing and refusals, and the draws: in range, reproducible, and off the global random
streams."""
import argparse
import random

import numpy as np
import pytest
import torch

import affine_cases as ac


@pytest.mark.parametrize('case', [c for c in ac.CASES if ac.rotated(c)], ids=[c['name'] for c in ac.CASES if ac.rotated(c)])
def test_model_equals_pillow_bit_for_bit(case):
    src = ac.source(case)
    want = ac.expected(case, src)
    for n, p in enumerate(case['params']):
        m = ac.matrix(case['S'], *p)
        assert m[1] != 0.0 or m[3] != 0.0                                  # Pillow's fixed-point routine
        fill = ac.border_fill(src[n]) if case['fill'] < 0 else case['fill']
        got = ac.pillow(src[n], m, fill)
        bad = got != want[n]
        assert not bad.any(), '%s image %d: %d of %d bytes differ from Pillow, first at %s' % (
            case['name'], n, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def test_random_draws_equal_pillow_bit_for_bit():
    """the ranges the command line admits: any angle, scale 0.25..4, shifts up to the whole side; grey and RGB"""
    rng = np.random.default_rng(11)
    for S, C, k in ((64, 1, 12), (64, 3, 6), (224, 1, 3), (299, 3, 2)):
        src = rng.integers(0, 256, (S, S, C), dtype=np.uint8)
        for _ in range(k):
            p = (float(rng.uniform(-180, 180)), (int(round(rng.uniform(-1, 1) * S)), int(round(rng.uniform(-1, 1) * S))), float(rng.uniform(0.25, 4)))
            fill = int(rng.integers(0, 256))
            assert np.array_equal(ac.model(src, ac.coefs(S, *p), fill), ac.pillow(src, ac.matrix(S, *p), fill)), (S, C, p)


def test_unrotated_cases_have_their_exact_properties():
    assert ac.coefs(7, 0.0, (0, 0), 1.0) == list(ac.IDENTITY) == ac.coefs(299, 0.0, (0, 0), 1.0)
    for case in ac.CASES:
        if ac.rotated(case):
            continue
        src = ac.source(case)
        got = ac.expected(case, src)
        for n, (ang, (tx, ty), sc) in enumerate(case['params']):
            assert ang == 0.0
            if sc == 1.0:                                                  # an integer shift (or none) at scale 1: a shifted copy with fill
                assert np.array_equal(got[n], ac.shifted(src[n], tx, ty, case['fill'])), (case['name'], n)
                if (tx, ty) == (0, 0):
                    assert np.array_equal(got[n], src[n])
                if abs(tx) >= case['S'] or abs(ty) >= case['S']:           # pushed out whole: nothing but fill
                    f = ac.border_fill(src[n]) if case['fill'] < 0 else [case['fill']] * case['C']
                    assert (got[n] == np.array(f, np.uint8)).all()
    # a zoom by 4 about the centre of a 5 x 5 image repeats the centre pixel over the middle 4 x 4 block's reach
    src = ac.source(ac.CASES[-1])
    z = ac.model(src[0], ac.coefs(5, 0.0, (0, 0), 4.0), 255)
    assert (z[1:4, 1:4] == src[0][2, 2]).all()


def test_border_fill_formula():
    rng = np.random.default_rng(5)
    for S, C in ((1, 1), (1, 3), (2, 1), (3, 3), (5, 1), (64, 3)):
        src = rng.integers(0, 256, (S, S, C), dtype=np.uint8)
        ring = [src[y, x] for y in range(S) for x in range(S) if y in (0, S - 1) or x in (0, S - 1)]
        assert len(ring) == (4 * S - 4 if S > 1 else 1)
        for c in range(C):
            tot = sum(int(p[c]) for p in ring)
            want = (2 * tot + len(ring)) // (2 * len(ring))
            assert ac.border_fill(src)[c] == want
            assert abs(want - np.mean([int(p[c]) for p in ring])) <= 0.5
    src = np.zeros((5, 5, 1), np.uint8)
    src[1:4, 1:4] = 200                                                    # the interior does not count
    assert ac.border_fill(src) == [0]
    # an image pushed out whole with fill = border is that level everywhere
    src[0] = 7
    out = ac.model(src, ac.coefs(5, 30.0, (5, 5), 1.0), -1)
    assert (out == ac.border_fill(src)[0]).all()


def test_affine_coefs_of_the_package_equal_the_twin():
    from ifcb_classifier_amd import neuston_data as nd
    assert tuple(nd.AFFINE_IDENTITY) == ac.IDENTITY
    for case in ac.CASES:
        for p in case['params']:
            assert nd.affine_coefs(case['S'], *p) == ac.coefs(case['S'], *p), (case['name'], p)
            assert nd.affine_matrix(case['S'], *p) == ac.matrix(case['S'], *p)
    with pytest.raises(ValueError):
        nd.affine_coefs(32768, 45.0, (32768, 32768), 0.25)                  # an offset beyond 16.16 in an int32


def test_parsing_and_refusals():
    from ifcb_classifier_amd import neuston_data as nd
    assert nd.parse_affine() is None and nd.parse_affine(0, 0.0, '1:1') is None and nd.parse_affine(None, None, [1.0, 1.0]) is None
    assert nd.parse_affine(180) == (180.0, 0.0, 1.0, 1.0)
    assert nd.parse_affine(translate='0.1') == (0.0, 0.1, 1.0, 1.0)
    assert nd.parse_affine(scale='0.8:1.2') == (0.0, 0.0, 0.8, 1.2)
    assert nd.parse_affine('15', 1, (0.25, 4)) == (15.0, 1.0, 0.25, 4.0)
    assert nd.parse_affine(scale=2) == (0.0, 0.0, 2.0, 2.0)
    for kw in (dict(rotate=-1), dict(rotate=float('inf')), dict(rotate=float('nan')), dict(rotate='a'), dict(rotate=True),
               dict(translate=-0.1), dict(translate=1.01), dict(translate=float('nan')), dict(scale='0.2:1'), dict(scale='1:4.5'),
               dict(scale='2:1'), dict(scale='1:2:3'), dict(scale='a:b'), dict(scale=float('nan')), dict(scale=[1.0, True])):
        with pytest.raises(ValueError):
            nd.parse_affine(**kw)
    with pytest.raises(ValueError):
        nd.AffineDraw()
    with pytest.raises(ValueError):
        nd.AffineDraw(rotate=10, fill=None)


def test_draws_lie_in_range_and_repeat_with_the_seed():
    from ifcb_classifier_amd import neuston_data as nd
    S = 299
    d = nd.AffineDraw(rotate=25.0, translate=0.1, scale=(0.8, 1.2), seed=9)
    ps = d.params(500, S)
    ang = np.array([p[0] for p in ps]); tx = np.array([p[1][0] for p in ps]); ty = np.array([p[1][1] for p in ps]); sc = np.array([p[2] for p in ps])
    assert (np.abs(ang) <= 25.0).all() and ang.min() < -20 and ang.max() > 20
    assert (np.abs(tx) <= round(0.1 * S)).all() and (np.abs(ty) <= round(0.1 * S)).all() and tx.min() < 0 < tx.max() and not np.array_equal(tx, ty)
    assert ((sc >= 0.8) & (sc <= 1.2)).all() and sc.min() < 0.85 and sc.max() > 1.15
    assert all(isinstance(p[1][0], int) and isinstance(p[1][1], int) for p in ps)
    # the same seed: the same draws; another seed or rank: others
    a = nd.AffineDraw(rotate=25.0, translate=0.1, scale=(0.8, 1.2), seed=9).draw(16, S)
    b = nd.AffineDraw(rotate=25.0, translate=0.1, scale=(0.8, 1.2), seed=9).draw(16, S)
    assert a.dtype == torch.int32 and tuple(a.shape) == (16, 6) and torch.equal(a, b)
    assert not torch.equal(a, nd.AffineDraw(rotate=25.0, translate=0.1, scale=(0.8, 1.2), seed=10).draw(16, S))
    assert not torch.equal(a, nd.AffineDraw(rotate=25.0, translate=0.1, scale=(0.8, 1.2), seed=9, rank=1).draw(16, S))
    # a flag that is off draws nothing and gives its neutral value
    only = nd.AffineDraw(translate=0.2, seed=1).params(50, 64)
    assert all(p[0] == 0.0 and p[2] == 1.0 for p in only) and any(p[1] != (0, 0) for p in only)
    fixed = nd.AffineDraw(scale='2:2', seed=1).params(5, 64)
    assert all(p == (0.0, (0, 0), 2.0) for p in fixed)
    # every coefficient set of the widest admitted ranges fits, and is what the twin gives
    wide = nd.AffineDraw(rotate=180.0, translate=1.0, scale=(0.25, 4.0), seed=2)
    ps = nd.AffineDraw(rotate=180.0, translate=1.0, scale=(0.25, 4.0), seed=2).params(64, S)
    assert wide.draw(64, S).tolist() == [ac.coefs(S, *p) for p in ps]


def test_the_draw_leaves_the_global_random_streams_alone():
    """the draw owns its generator: random, numpy's and torch's global streams stay where they were"""
    from ifcb_classifier_amd import neuston_data as nd
    random.seed(3); np.random.seed(3); torch.manual_seed(3)
    s0 = (random.getstate(), np.random.get_state()[1].copy(), torch.get_rng_state().clone())
    d = nd.AffineDraw(rotate=180.0, translate=0.1, scale=[0.8, 1.2], seed=5)
    c = d.draw(2, 299)
    assert c.dtype == torch.int32 and tuple(c.shape) == (2, 6) and d.fill == 'border'
    assert random.getstate() == s0[0] and np.array_equal(np.random.get_state()[1], s0[1]) and torch.equal(torch.get_rng_state(), s0[2])
    # no transform carries a draw: nothing applies one yet
    tr, va = nd.get_trainval_transforms(argparse.Namespace(MODEL='inception_v3', img_norm=None, flip='xy', seed=5))
    assert not hasattr(tr, 'affine') and not hasattr(va, 'affine')
