"""RUN --tta without a GPU: the walks of tests/sym_cases.py visit every view once and one more op restores the batch, the flag's
argparse surface, the declarations of the two entry points, the order of calls of NeustonModel.eval_current_tta on a recording engine,
and the bound of tests/tta_bounds.py against an fp32 emulation of the accumulate order -- with all views, and with one dropped.  The
kernels run in tests/test_gpu_batch_sym.py, test_gpu_softmax_acc.py, test_gpu_tta_model.py and test_gpu_tta_cli.py."""
import os
import re
import types

import numpy as np
import pytest
import torch

import sym_cases as sc
import tta_bounds as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _asym():
    return np.arange(25, dtype=np.int64).reshape(1, 5, 5)          # no symmetry of the square maps it to itself


def test_the_all_walk_visits_the_eight_symmetries_once_and_one_more_hflip_restores():
    x = _asym()
    vs = sc.views(x, 'all')
    assert len(vs) == 8
    keys = [v.tobytes() for v in vs]
    assert len(set(keys)) == 8
    want = set()
    for k in range(4):
        r = np.rot90(x[0], k)
        want.add(np.ascontiguousarray(r)[None].tobytes())
        want.add(np.ascontiguousarray(np.fliplr(r))[None].tobytes())
    assert len(want) == 8 and set(keys) == want
    assert np.array_equal(sc.apply(vs[-1], sc.RESTORE['all']), x) and sc.RESTORE['all'] == sc.HFLIP


def test_the_flips_walk_visits_e_h_vh_v_and_one_more_vflip_restores():
    x = _asym()
    vs = sc.views(x, 'flips')
    H, V = x[:, :, ::-1], x[:, ::-1]
    assert len(vs) == 4
    assert np.array_equal(vs[0], x) and np.array_equal(vs[1], H) and np.array_equal(vs[2], H[:, ::-1]) and np.array_equal(vs[3], V)
    assert len({v.tobytes() for v in vs}) == 4
    assert np.array_equal(sc.apply(vs[-1], sc.RESTORE['flips']), x) and sc.RESTORE['flips'] == sc.VFLIP


def test_every_op_is_an_involution_and_moves_a_dense_pixel_whole():
    x = sc.batch('bf16', 2, 5)
    for op in sc.OPS.values():
        y = np.ascontiguousarray(sc.apply(x, op))
        assert np.array_equal(sc.apply(y, op), x)
        assert sorted(map(bytes, y.reshape(-1, 8).view(np.uint8).reshape(-1, 16))) == sorted(map(bytes, x.reshape(-1, 8).view(np.uint8).reshape(-1, 16)))
    with pytest.raises(ValueError):
        sc.apply(x, sc.HFLIP | sc.VFLIP)
    s = sc.symmetrised(sc.batch('u8', 2, 7))
    assert all(np.array_equal(v, s) for v in sc.views(s, 'all'))


def test_the_engine_walks_and_the_binding_agree_with_the_case_table():
    from ifcb_classifier_amd import _lib
    from ifcb_classifier_amd.engine import Engine
    assert (_lib.SYM_HFLIP, _lib.SYM_VFLIP, _lib.SYM_TRANSPOSE) == (sc.HFLIP, sc.VFLIP, sc.TRANSPOSE) == (1, 2, 4)
    assert Engine.TTA_WALKS == sc.WALKS
    assert len(_lib._PROTOS['ifcbk_batch_sym'][1]) == 7 and len(_lib._PROTOS['ifcbk_softmax_acc'][1]) == 8
    assert sc.KINDS['u8'][0] == _lib.MIX_U8 and sc.KINDS['bf16'][0] == _lib.BF16 and sc.KINDS['f32'][0] == _lib.F32


def test_the_header_declares_both_entry_points_and_the_build_holds_the_new_file():
    hdr = open(os.path.join(ROOT, 'include', 'ifcbk.h')).read()
    flat = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S))
    assert 'IFCBK_API int ifcbk_batch_sym(ifcbk_ctx*, void* x, int kind , int N, int S, int op, void* stream);' in flat
    assert ('IFCBK_API int ifcbk_softmax_acc(ifcbk_ctx*, const float* logits, int N, int NC, float* acc, int accumulate, float scale, '
            'void* stream);') in flat
    for name, val in (('IFCBK_SYM_HFLIP', 1), ('IFCBK_SYM_VFLIP', 2), ('IFCBK_SYM_TRANSPOSE', 4)):
        assert re.search(r'#define %s\s+%d\b' % (name, val), hdr), name
    csrc = os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc')
    assert 'batch_sym.hip' in open(os.path.join(csrc, 'Makefile')).read()
    assert 'extern "C" int ifcbk_batch_sym(' in open(os.path.join(csrc, 'batch_sym.hip')).read()
    assert 'extern "C" int ifcbk_softmax_acc(' in open(os.path.join(csrc, 'loss.hip')).read()


def test_the_flag_is_runs_alone_needs_a_value_and_defaults_to_none():
    from ifcb_classifier_amd import neuston_net as nn_
    p = nn_.argparse_nn()
    assert p.parse_args(['RUN', 'src', 'm.ptl', 'rid']).tta is None
    for mode in ('flips', 'all'):
        a = p.parse_args(['RUN', '--tta', mode, 'src', 'm.ptl', 'rid'])
        assert a.tta == mode and (a.SRC, a.MODEL, a.RUN_ID) == ('src', 'm.ptl', 'rid')
        assert p.parse_args(['RUN', 'src', 'm.ptl', 'rid', '--tta', mode]).tta == mode
    for bad in (['RUN', 'src', 'm.ptl', 'rid', '--tta', 'rot'], ['RUN', 'src', 'm.ptl', 'rid', '--tta'],
                ['RUN', '--tta', 'src', 'm.ptl', 'rid'],                                  # (a positional is not taken for the value)
                ['TRAIN', 'src', 'resnet18', 'tid', '--tta', 'all']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    assert not hasattr(p.parse_args(['TRAIN', 'src', 'resnet18', 'tid']), 'tta')


class _Recorder:
    """stands where the engine stands in NeustonModel.eval_current_tta and writes down what it is asked to do"""

    def __init__(self):
        from ifcb_classifier_amd.engine import Engine
        self.TTA_WALKS = Engine.TTA_WALKS
        self.calls = []
        self.probs = torch.arange(12.0).reshape(4, 3)

    def forward_eval(self, N):
        self.calls.append(('fwd', N))

    def sym_batch(self, N, op, slot=None):
        self.calls.append(('sym', N, op, slot))

    def softmax_acc(self, N, first, scale=1.0):
        self.calls.append(('acc', N, bool(first), scale))


@pytest.mark.parametrize('mode', ['flips', 'all'])
def test_eval_current_tta_runs_forward_and_softmax_per_view_and_scales_the_last(mode):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    eng = _Recorder()
    evals = []
    me = types.SimpleNamespace(model=types.SimpleNamespace(engine=eng, eval=lambda: evals.append(1)))
    out = NeustonModel.eval_current_tta(me, 3, mode)
    walk = sc.WALKS[mode]
    V = len(walk) + 1
    want = [('fwd', 3), ('acc', 3, True, 1.0)]
    for k, op in enumerate(walk):
        want += [('sym', 3, op, None), ('fwd', 3), ('acc', 3, False, 1.0 / V if k == len(walk) - 1 else 1.0)]
    assert eng.calls == want and evals == [1]
    assert torch.equal(out, eng.probs[:3]) and out.data_ptr() != eng.probs.data_ptr()
    with pytest.raises(ValueError, match='mode'):
        NeustonModel.eval_current_tta(me, 3, 'rot')
    assert 'LEFT IN ITS LAST VIEW' in NeustonModel.eval_current_tta.__doc__


def _softmax32(l):
    """fp32 softmax in ifcbk_softmax's order of operations (numpy's expf in place of the device's)"""
    l = l.astype(np.float32)
    mx = l.max(1, keepdims=True)
    ex = np.exp(l - mx, dtype=np.float32)
    s = np.zeros((l.shape[0], 1), np.float32)
    for j in range(l.shape[1]):
        s = s + ex[:, j:j + 1]
    return ex * (np.float32(1) / s)


def _accumulate32(ps, scale):
    acc = ps[0].copy()
    for p in ps[1:]:
        acc = acc + p
    return acc * np.float32(scale)


def test_four_equal_views_average_to_their_bits_and_eight_do_not():
    """why test_gpu_tta_model.py compares a symmetric batch under 'all' with the sum of eight copies of the plain scores and not with
    the plain scores: p + p and fl(3p) + p are exact (a tie in fl(3p) needs an even mantissa, which then wins the tie of the next add),
    fl(5p) .. fl(7p) are not, and the left-to-right order is part of the definition"""
    p = np.random.default_rng(0).random(200000).astype(np.float32)
    assert np.array_equal(_accumulate32([p] * 4, 0.25), p)
    off = _accumulate32([p] * 8, 0.125) != p
    assert 0.3 < off.mean() < 0.6
    # the four inexact adds (5p .. 8p) each round by at most half an ulp of a number below 8p: 4 * 4 ulp(p) in the sum, 2 ulp(p) after / 8
    assert (np.abs(_accumulate32([p] * 8, 0.125) - p) <= 2 * np.spacing(p)).all()


@pytest.mark.parametrize('V', [4, 8])
def test_the_fp32_accumulate_order_stays_inside_the_bound_and_a_dropped_view_does_not(V):
    rng = np.random.default_rng(V)
    worst = 0.0
    for N, NC in ((1, 1), (5, 2), (5, 7), (257, 100)):
        logits = [rng.normal(0, 3, (N, NC)).astype(np.float32) for _ in range(V)]
        logits[0][0, 0] += 80.0                                          # a row with one logit far above the rest
        want, e = tb.mean_softmax([torch.from_numpy(l) for l in logits])
        ps = [_softmax32(l) for l in logits]
        got = _accumulate32(ps, 1.0 / V)
        assert got.dtype == np.float32
        r = ((torch.from_numpy(got).double() - want).abs() / e).max().item()
        worst = max(worst, r)
        assert r <= 1.0, (N, NC, r)
        if NC > 1:
            short = _accumulate32(ps[:-1], 1.0 / V)
            assert ((torch.from_numpy(short).double() - want).abs() / e).max().item() > 1e3, (N, NC)
    print('tta bound: fp32 emulation of %d views, worst err / bound %.3f' % (V, worst))
    assert worst > 1e-3                                                  # the bound is of the error's order, not a blanket
