"""CPU twin of tests/test_gpu_roi_paths.py: the oracle the GPU planes are compared with equals the installed Pillow on every shape of
the case table, on the committed pass-order boundary and on the golden vectors; the path predicates of roi_bounds.py still quote
roi.hip and every path is reached with and without flips; and the checkers reject subtly wrong planes (emulated in numpy)."""
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

import roi_bounds as rb
from oracle import pil_resize as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
CSRC = os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc')
Image = pytest.importorskip('PIL.Image')


def _norm(s):
    return re.sub(r'\s+', ' ', s)


def _pil_L(a, S):
    return np.asarray(Image.fromarray(a, 'L').resize((S, S), Image.BILINEAR))


def _shapes():
    seen = {}
    for c in rb.ROI:
        for h, w in c['rois']:
            seen.setdefault((h, w, c['S'], c['cin']), c['name'])
    return sorted(seen)


def test_oracle_equals_installed_pillow_on_every_case_shape():
    shapes = _shapes()
    assert len(shapes) > 80
    rng = np.random.default_rng(7)
    for h, w, S, cin in shapes:
        if cin == 1:
            a = rng.integers(0, 256, (h, w), dtype=np.uint8)
            o = PR.resize_bilinear_u8(a, S, S)
            assert np.array_equal(o, _pil_L(a, S)), (h, w, S)
            chain = np.asarray(Image.fromarray(a, 'L').convert('RGB').resize((S, S), Image.BILINEAR))
            assert np.array_equal(chain, np.repeat(o[:, :, None], 3, 2)), (h, w, S)
        else:
            a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            assert np.array_equal(PR.resize_bilinear_u8(a, S, S), np.asarray(Image.fromarray(a, 'RGB').resize((S, S), Image.BILINEAR))), (h, w, S)


def test_flipped_cases_equal_pillow_of_the_flipped_image():
    """expected_u8 flips first, then resizes: the order of neuston_data.py's train transforms"""
    case = [c for c in rb.ROI if c['name'] == 'mid299'][0]
    rois = rb.pixels(case)
    want = rb.expected_u8(case, rois)
    for i, (r, f) in enumerate(zip(rois, case['flips'])):
        im = Image.fromarray(r, 'L')
        if f & 1:
            im = im.transpose(Image.FLIP_TOP_BOTTOM)
        if f & 2:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        assert np.array_equal(want[i, :, :, 0], np.asarray(im.resize((299, 299), Image.BILINEAR))), i


def test_pass_order_rule_on_the_committed_boundary_and_goldens():
    """the sweep's outcome (tests/golden/sweep_pass_order.py): vertical pass first <=> h > 100 w and h > S.  Each boundary pair is
    re-measured against Pillow: reverting oracle.pil_resize.vertical_first fails here."""
    sw = json.load(open(os.path.join(GOLD, 'pass_order_sweep.json')))
    assert sw['rule_fits_every_point'] and sw['counts']['N'] == 0 and sw['points'] > 14000 and len(sw['boundary']) >= 15
    rng = np.random.default_rng(3)
    for b in sw['boundary']:
        S, w = b['S'], b['w']
        lo, hi = b['last_horizontal_first'], b['first_vertical_first']
        assert hi == lo + 1 == max(100 * w, S) + 1, b
        assert not PR.vertical_first(lo, w, S) and PR.vertical_first(hi, w, S)
        for h in (lo, hi):
            a = rng.integers(0, 256, (h, w), dtype=np.uint8)
            p = _pil_L(a, S)
            assert np.array_equal(PR.resize_bilinear_u8(a, S, S), p), (S, h, w)
            if w > 1 and h != S:                         # (h == S: no vertical pass; w == 1: constant rows)
                other = PR.resize_bilinear_u8(a, S, S, 'hv' if h == hi else 'vh')
                assert 0 < np.abs(other.astype(int) - p).max() <= 1, (S, h, w)             # the orders differ, by one level
    z = np.load(os.path.join(GOLD, 'pil_resize_order_cases.npz'))
    meta = json.load(open(os.path.join(GOLD, 'pil_resize_order_cases.json')))['cases']
    for S in (224, 299):
        m = [c for c in meta if c['S'] == S]
        assert sum(c['vertical_first'] for c in m) >= 4 and sum(not c['vertical_first'] for c in m) >= 2
    for c in meta:
        a = z['in_%d' % c['case']]
        assert PR.vertical_first(c['h'], c['w'], c['S']) == c['vertical_first']
        assert hashlib.sha256(PR.resize_bilinear_u8(a, c['S'], c['S']).tobytes()).hexdigest() == c['sha256'], c
        assert hashlib.sha256(_pil_L(a, c['S']).tobytes()).hexdigest() == c['sha256'], c


def test_path_predicates_quote_the_source_and_every_path_has_cases():
    src = _norm(open(os.path.join(CSRC, 'roi.hip')).read())
    for name, (pred, cond) in rb.PATHS.items():
        assert _norm(cond) in src, '%s: %r is no longer in roi.hip' % (name, cond)
    for q in rb.QUOTED:
        assert _norm(q) in src, q
    shared = _norm(open(os.path.join(CSRC, 'roi_resample.h')).read())
    for q in rb.QUOTED_SHARED:
        assert _norm(q) in shared, q
    reached = {p: [set(), set()] for p in rb.PATHS}           # path -> [flip codes seen, (flipped, not flipped)]
    vfirst = set()
    for c in rb.ROI:
        ps = rb.paths(c)
        for i, ((h, w), p) in enumerate(zip(c['rois'], ps)):
            fl = c['flips'][i] if c['flips'] else None
            for q in (p, 'roi_coeffs_kernel'):
                reached[q][1].add(fl is not None)
                if fl and h != w:
                    reached[q][0].add(fl)
            if PR.vertical_first(h, w, c['S']):
                vfirst.add((p, fl is not None))
    for p, (codes, modes) in reached.items():
        assert modes == {True, False}, '%s: needs a case with flips and one without' % p
        assert codes == {1, 2, 3}, '%s: flip codes on non-square ROIs %s' % (p, codes)
    # the vertical-first ROIs exist only above S: in the lds_ok and generic paths, with and without flips
    assert vfirst == {(p, f) for p in ('roi_resize_kernel lds_ok', 'roi_resize_kernel generic') for f in (True, False)}
    # the shapes a kmax == 3 batch must hold
    for c in rb.ROI:
        if rb.kmax(c) == 3 and c['maxima'] is None and c['cin'] == 1:
            S = c['S']
            assert {(1, 1), (1, S), (S, 1), (S, S), (S - 1, S), (2, 3)} <= set(c['rois']), c['name']
            if S == 299:                                 # three-tap windows on both axes (see roi_bounds._small)
                n3 = lambda size: int((PR._coeffs(size, S)[0][:, 1] == 3).sum())
                assert any(n3(w) for h, w in c['rois']) and any(n3(h) for h, w in c['rois']), c['name']
    S3 = {c['S'] for c in rb.ROI if set(rb.paths(c)) == {'roi_resize3_kernel'}}
    assert {224, 299, 40} <= S3 and rb.block_x(40) == 64
    k5 = [c for c in rb.ROI if rb.kmax(c) == 5 and c['maxima'] is None]
    assert all((2 * c['S'], 2 * c['S']) in c['rois'] and (c['S'] + 1, c['S']) in c['rois'] for c in k5) and len(k5) >= 3
    assert any(w == 640 for c in k5 for h, w in c['rois']) and any(w == 641 for c in rb.ROI for h, w in c['rois'])
    assert any(rb.kmax(c) == 7 and c['cin'] == 1 for c in rb.ROI) and any(c['cin'] == 3 for c in rb.ROI)
    assert any(c['cout'] == 16 for c in rb.ROI) and any(not c['out'] for c in rb.ROI) and any(not c['u8'] for c in rb.ROI)
    assert {c['dtype'] for c in rb.ROI} == {'bf16', 'fp32'}


def test_workspace_formula_covers_the_coefficient_table():
    """roi_coeffs_kernel writes fields 0 .. 1 + kmax of [image][axis][field][S]: the last word is index n * 2 * (2 + kmax) * S - 1"""
    src = _norm(open(os.path.join(CSRC, 'roi.hip')).read())
    for q in ('return (size_t)d->n_img * 2 * d->S * (2 + kmax) * sizeof(int32_t);', 'if (i >= n_img * 2 * S) return;',
              'int32_t* row = tab + ((size_t)(img * 2 + axis) * (2 + kmax)) * S + xx;', 'roi_taps(inSize, S, xx, kmax, row, S);'):
        assert _norm(q) in src, q
    shared = _norm(open(os.path.join(CSRC, 'roi_resample.h')).read())           # roi_taps: the writes behind `row`
    for q in ('row[(size_t)(2 + x) * fieldStride] = kq;', 'for (int x = 0; x < kmax; ++x) {', 'row[0] = xmin;', 'row[fieldStride] = xmax;'):
        assert _norm(q) in shared, q
    n, S, k = 5, 299, 7
    last = ((n - 1) * 2 + 1) * (2 + k) * S + (S - 1) + (2 + k - 1) * S
    assert last == n * 2 * S * (2 + k) - 1


def test_the_resampler_arithmetic_is_written_once():
    """the tap rounding and the float stage's division stand once under csrc/ (roi_resample.h): a resize feature that pastes a
    further copy instead of calling the shared one fails here"""
    text = {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(('.hip', '.h'))}
    assert len(text) > 20 and 'roi_resample.h' in text
    rounding = r'\(int\)\s*\(\s*0\.5\s*\+\s*\w+\s*\*\s*\(double\)\s*\(\s*1\s*<<\s*PRECISION_BITS\s*\)\s*\)'
    for what, pat in (('tap rounding', rounding), ('float stage', r'/\s*255\.0f')):
        hits = [f for f, t in text.items() for _ in re.finditer(pat, t)]
        assert hits == ['roi_resample.h'], '%s: %s' % (what, hits)


# ---------------------------------------------------------------------------------------------- the checkers can fail
def _plane():
    case = [c for c in rb.ROI if c['name'] == 'small299'][0]
    rois = rb.pixels(case)
    return case, rois, rb.expected_u8(case, rois)


def test_check_u8_rejects_one_level_in_one_pixel_and_a_wrong_row_tail():
    case, rois, want = _plane()
    rb.check_u8('same', want.copy(), want)
    bad = want.copy()
    i = (8, 150, 17, 0)
    bad[i] = bad[i] + 1 if bad[i] < 255 else 254
    with pytest.raises(AssertionError, match='1 of'):
        rb.check_u8('one level', bad, want)
    bad = want.copy()
    bad[:, 296:] = bad[:, 295:296]                      # the 3-row tail block (299 = 37 * 8 + 3) repeats the last full block's row
    with pytest.raises(AssertionError):
        rb.check_u8('row tail', bad, want)


def test_check_u8_rejects_a_flip_applied_to_the_window_but_not_to_its_taps():
    """the kernel flips the tap's COLUMN (col = w - 1 - (xmin + k)); flipping the window start and walking it forwards pairs the
    taps with the wrong columns"""
    S, h, w = 299, 40, 90
    a = np.random.default_rng(1).integers(0, 256, (h, w), dtype=np.uint8)
    bounds, kk = PR._coeffs(w, S)
    good = np.zeros((h, S), np.int64)
    bad = np.zeros((h, S), np.int64)
    for x in range(S):
        x0, n = bounds[x]
        for k in range(n):
            good[:, x] += a[:, w - 1 - (x0 + k)].astype(np.int64) * kk[x, k]
            bad[:, x] += a[:, w - 1 - (x0 + n - 1) + k].astype(np.int64) * kk[x, k]
    good, bad = (PR._clip8(t + (1 << (PR.PRECISION_BITS - 1))).astype(np.uint8) for t in (good, bad))
    want = PR.resize_bilinear_u8(np.ascontiguousarray(a[:, ::-1]), h, S)
    rb.check_u8('flip before the taps', good[None, :, :, None], want[None, :, :, None])
    with pytest.raises(AssertionError):
        rb.check_u8('flip after the taps', bad[None, :, :, None], want[None, :, :, None])


def _emulate_float(u3, mean, std, tsc, tsh, out, contract=True):
    """the kernel's float stage in fp32 steps"""
    f = torch.from_numpy(u3.astype(np.float32)) / torch.tensor(255.0)
    m, s, t, b = (torch.tensor(x, dtype=torch.float32) for x in (mean, std, tsc, tsh))
    v = (f - m) / s
    v = (v.double() * t.double() + b.double()).float() if contract else v * t + b
    return v.to(torch.bfloat16 if out == 'bf16' else torch.float32)


@pytest.mark.parametrize('out', ['bf16', 'fp32'])
def test_check_float_accepts_the_emulation_and_rejects_swapped_mean_and_std(out):
    case = dict(rb._case('f', [(1, 1)], 16, dtype=out, mean=rb.MEAN, std=rb.STD, tsc=rb.TSC, tsh=rb.TSH, cout=16))
    u8 = np.random.default_rng(2).integers(0, 256, (2, 16, 16, 1), dtype=np.uint8)
    u3 = np.repeat(u8, 3, -1)
    for contract in (True, False):
        got = torch.zeros(2, 16, 16, 16)
        got[..., :3] = _emulate_float(u3, case['mean'], case['std'], case['tsc'], case['tsh'], out, contract).float()
        rb.check_float('good', got, u8, case, family=None)
    m, s = list(case['mean']), list(case['std'])
    m[1], s[1] = s[1], m[1]                              # channel 1: (v - std) / mean
    bad = got.clone()
    bad[..., :3] = _emulate_float(u3, m, s, case['tsc'], case['tsh'], out).float()
    with pytest.raises(AssertionError):
        rb.check_float('swapped', bad, u8, case, family=None)
    bad = got.clone()
    bad[1, 3, 5, 9] = 2.0 ** -20                         # a pad channel that is not zero
    with pytest.raises(AssertionError):
        rb.check_float('pad', bad, u8, case, family=None)
    # one bf16 ulp off in one element (in fp32 storage the four fp32 roundings of the stage are themselves a few ulps)
    if out == 'bf16':
        bad = got.clone()
        x = bad[0, 7, 7, 2]
        bad[0, 7, 7, 2] = x + float(rb.ob.ulp(x.double().abs(), out))
        with pytest.raises(AssertionError):
            rb.check_float('one ulp', bad, u8, case, family=None)
    # the identity stage is exact: fl32(r / 255) rounded to storage, nothing else
    ident = dict(rb._case('i', [(1, 1)], 16, dtype=out))
    got = torch.zeros(2, 16, 16, 8)
    got[..., :3] = _emulate_float(u3, (0, 0, 0), (1, 1, 1), (1, 1, 1), (0, 0, 0), out).float()
    rb.check_float('identity', got, u8, ident, family=None)
    if out == 'fp32':
        bad = got.clone()
        bad[..., :3] = (torch.from_numpy(u3.astype(np.float32)) * torch.tensor(1.0 / 255.0, dtype=torch.float32))      # a multiply by fl(1/255)
        assert not torch.equal(bad, got)
        with pytest.raises(AssertionError):
            rb.check_float('reciprocal', bad, u8, ident, family=None)
