"""TRAIN --mixup / --cutmix on the host: the flags and their parsers, the BatchMix draw (own generator, timm's box arithmetic), the
references and bounds of tests/mix_cases.py, the op tables Engine(plan_only=True) builds with and without mix, the header and the
binding, and the args.yml / .ptl round trip.  The kernels run in tests/test_gpu_mix_*.py."""
import argparse
import os
import random
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_plan_fingerprints as mpf  # noqa: E402

import loss_smooth_bounds as sb  # noqa: E402
import mix_cases as mc  # noqa: E402
from ifcb_classifier_amd import _lib, graph, neuston_data as nd, neuston_models, neuston_net  # noqa: E402
from ifcb_classifier_amd.engine import Engine  # noqa: E402


# ------------------------------------------------------------------------------------------------------ parsing, argparse
def _parse(*extra):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'inception_v3', 'id'] + list(extra))


def test_flags():
    a = _parse()
    assert a.mixup == 0.0 and a.cutmix == 0.0 and a.mix_prob == 1.0
    a = _parse('--mixup', '0.4', '--cutmix', '1', '--mix-prob', '0.5', '--label-smoothing', '0.1', '--class-norm')
    assert (a.mixup, a.cutmix, a.mix_prob, a.label_smoothing) == (0.4, 1.0, 0.5, 0.1)
    assert _parse('--mixup', '0').mixup == 0.0
    for bad in (['--mixup', '-1'], ['--mixup', 'nan'], ['--mixup', 'inf'], ['--cutmix', 'x'], ['--cutmix=-0.5'], ['--mix-prob', '1.5'],
                ['--mix-prob', '-0.1'], ['--mix-prob', 'nan']):
        with pytest.raises(SystemExit):
            _parse(*bad)


@pytest.mark.parametrize('argv', [['--mixup', '0.4', '--focal-gamma', '2'], ['--focal-gamma', '2', '--mixup', '0.4'],
                                  ['--cutmix', '1', '--focal-gamma', '2'], ['--focal-gamma', '2', '--cutmix', '1']])
def test_focal_clash_is_an_argparse_error(argv, capsys):
    with pytest.raises(SystemExit):
        _parse(*argv)
    assert '--focal-gamma do not combine' in capsys.readouterr().err
    _parse('--mixup', '0', '--focal-gamma', '2')                      # 0 is off: no clash
    _parse('--focal-gamma', '0', '--cutmix', '1')


def test_parsers():
    assert nd.parse_mix_alpha(None) == 0.0 and nd.parse_mix_alpha('0.4') == 0.4 and nd.parse_mix_alpha(2) == 2.0
    assert nd.parse_mix_prob(None) == 1.0 and nd.parse_mix_prob('0') == 0.0 and nd.parse_mix_prob(0.25) == 0.25
    for bad in (-1, float('nan'), float('inf'), 'a', True):
        with pytest.raises(ValueError):
            nd.parse_mix_alpha(bad)
    for bad in (-0.1, 1.1, float('nan'), 'p', False):
        with pytest.raises(ValueError):
            nd.parse_mix_prob(bad)
    with pytest.raises(ValueError):
        nd.BatchMix(0.0, 0.0)


# ------------------------------------------------------------------------------------------------------ BatchMix
def test_draws_are_deterministic_per_seed_and_rank_and_touch_no_global_stream():
    random.seed(5)
    np.random.seed(5)
    torch.manual_seed(5)
    st_py, st_np, st_t = random.getstate(), np.random.get_state(), torch.get_rng_state()
    a = [nd.BatchMix(0.4, 1.0, 0.8, seed=3, rank=0).draw(299) for _ in range(1)]
    m0, m0b, m1, m2 = nd.BatchMix(0.4, 1.0, 0.8, 3, 0), nd.BatchMix(0.4, 1.0, 0.8, 3, 0), nd.BatchMix(0.4, 1.0, 0.8, 3, 1), nd.BatchMix(0.4, 1.0, 0.8, 4, 0)
    d0, d0b, d1, d2 = ([m.draw(299) for _ in range(64)] for m in (m0, m0b, m1, m2))
    assert d0 == d0b and d0[0] == a[0] and d0 != d1 and d0 != d2
    assert random.getstate() == st_py and torch.equal(torch.get_rng_state(), st_t)
    now = np.random.get_state()
    assert now[0] == st_np[0] and (now[1] == st_np[1]).all() and now[2:] == st_np[2:]
    kinds = {('cut' if b is not None else ('none' if l == 1.0 else 'mix')) for l, b in d0}
    assert kinds == {'cut', 'mix', 'none'}                           # switch_prob 0.5 and prob 0.8 both show in 64 draws
    for l, b in d0:
        assert isinstance(l, float) and 0.0 <= l <= 1.0
        if b is not None:
            y0, y1, x0, x1 = b
            assert 0 <= y0 <= y1 <= 299 and 0 <= x0 <= x1 <= 299 and l == 1.0 - (y1 - y0) * (x1 - x0) / 299.0 ** 2
    assert all(b is None for _, b in (nd.BatchMix(0.4, 0.0, 1.0, 1, 0).draw(224) for _ in range(32)))
    assert all(b is not None for _, b in (nd.BatchMix(0.0, 1.0, 1.0, 1, 0).draw(224) for _ in range(32)))


def test_prob_0_never_mixes():
    m = nd.BatchMix(0.4, 1.0, 0.0, seed=1, rank=0)
    assert all(m.draw(299) == (1.0, None) for _ in range(50))


# (lam0, cy, cx, S) -> (y0, y1, x0, x1): timm's rand_bbox without margin, by hand
BOXES = [
    ((0.75, 150, 150, 299), (76, 224, 76, 224)),           # cut = int(299 * 0.5) = 149, half 74: inside the image
    ((0.75, 10, 150, 299), (0, 84, 76, 224)),              # clipped at the top
    ((0.75, 290, 150, 299), (216, 299, 76, 224)),          # ... the bottom
    ((0.75, 150, 5, 299), (76, 224, 0, 79)),               # ... the left
    ((0.75, 150, 298, 299), (76, 224, 224, 299)),          # ... the right
    ((0.99999, 100, 100, 299), (100, 100, 100, 100)),      # cut_h == 0: an empty box
    ((0.0, 8, 8, 16), (0, 16, 0, 16)),                     # the full image (cut = S, centred)
    ((0.0, 0, 0, 16), (0, 8, 0, 8)),                       # the full cut in a corner: a quarter remains
    ((0.5, 2, 2, 5), (1, 3, 1, 3)),                        # int(5 * sqrt(0.5)) = 3, half 1
]


@pytest.mark.parametrize('arg,want', BOXES)
def test_box_arithmetic(arg, want):
    lam0, cy, cx, S = arg
    box = nd.cut_box(lam0, cy, cx, S)
    assert box == want
    y0, y1, x0, x1 = want
    assert nd.box_lam(box, S) == 1.0 - (y1 - y0) * (x1 - x0) / float(S * S)
    if want[0] == want[1]:
        assert nd.box_lam(box, S) == 1.0
    if want == (0, S, 0, S):
        assert nd.box_lam(box, S) == 0.0


def test_transforms_carry_the_mix_on_the_training_side_only():
    a = argparse.Namespace(MODEL='inception_v3', img_norm=None, flip=None, seed=9)
    tr, va = nd.get_trainval_transforms(a)
    assert tr.mix is None and va.mix is None
    a = argparse.Namespace(MODEL='inception_v3', img_norm=None, flip=None, seed=9, mixup=0.4, cutmix=0.0, mix_prob=0.5)
    tr, va = nd.get_trainval_transforms(a)
    assert isinstance(tr.mix, nd.BatchMix) and va.mix is None and (tr.mix.mixup, tr.mix.cutmix, tr.mix.prob) == (0.4, 0.0, 0.5)
    with mock.patch.dict(os.environ, {'RANK': '1'}):
        tr1, _ = nd.get_trainval_transforms(a)
    tr0, _ = nd.get_trainval_transforms(a)
    assert [tr0.mix.draw(299) for _ in range(8)] == [tr.mix.draw(299) for _ in range(8)] != [tr1.mix.draw(299) for _ in range(8)]


# ------------------------------------------------------------------------------------------------------ references and bounds
def test_u8_reference_stays_under_the_ambiguity_cap_on_the_gpu_tests_inputs():
    """the share of elements whose exact value lies within AMBIG of a rounding tie, for every input test_gpu_mix_batch.py uses"""
    worst = 0.0
    for S in mc.MIX_S:
        for N in mc.MIX_N:
            lam = mc.lam_rows(N)
            x = mc.u8_batch(N, S, lam=lam)
            for name, box in mc.boxes(S).items():
                exact, copy, _ = mc.mix_reference(x, lam, box)
                wrong, share = mc.u8_verdict(torch.floor(exact + 0.5), exact)
                assert not bool(wrong.any()) and share <= mc.AMBIG_MAX, (S, N, name, share)
                worst = max(worst, share)
    print('worst ambiguous share %.5f' % worst)


def test_mix_reference_semantics():
    x = mc.u8_batch(3, 5)
    lam = torch.tensor([0.25, 0.7, 0.5])
    exact, copy, mag = mc.mix_reference(x, lam, (1, 3, 0, 5))
    xd = x.double()
    assert torch.equal(exact[0, 0], 0.25 * xd[0, 0] + 0.75 * xd[2, 0]) and torch.equal(exact[2, 4], 0.5 * xd[2, 4] + 0.5 * xd[0, 4])
    assert torch.equal(exact[0, 1:3], xd[2, 1:3]) and torch.equal(exact[2, 1:3], xd[0, 1:3])
    assert torch.equal(exact[1], xd[1]) and bool(copy[1].all()) and bool(copy[0, 1:3].all()) and not bool(copy[0, 0].any())
    # a float32 model of the dense kernel passes its own check; a value half a bf16 ulp off does not
    d = mc.dense_from_u8(x, torch.float32)
    l4 = lam.reshape(3, 1, 1, 1)
    got = torch.addcmul(d.flip(0), l4, d - d.flip(0))
    got[:, 1:3] = d.flip(0)[:, 1:3]
    got[1] = d[1]
    assert mc.check_mix_dense('model', got, d, lam, (1, 3, 0, 5), 'f32') <= 1.0
    with pytest.raises(AssertionError):
        mc.check_mix_dense('off', got * (1 + 2.0 ** -9), d, lam, (0, 0, 0, 0), 'f32')


@pytest.mark.parametrize('N', mc.LOSS_NS)
@pytest.mark.parametrize('NC', mc.LOSS_NCS)
def test_float32_emulation_of_the_loss_kernel_stays_within_the_bound(N, NC):
    worst = 0.0
    for wm in mc.WEIGHTS:
        if wm == 'zero' and NC == 1:
            continue                                        # the only class weighs nothing: 0 / 0 (the GPU test expects NaN)
        for eps in mc.EPSS:
            for lam in mc.LAMS:
                for spread, scale, acc in ((4.0, 1.0, None), (30.0, 0.4, 5.0)):
                    l, t, lm, cw = mc.loss_inputs(N, NC, wm, lam, spread)
                    want = mc.xent_mix(l, t, lm, cw, scale, eps, old_loss=acc)
                    ref_loss, ref_dl = mc.loss_reference(l, t, lm, cw, scale, eps)
                    assert torch.allclose(want['dlogits'][0], ref_dl, rtol=1e-12, atol=1e-13)          # (two float64 forms of one value: they cancel differently)
                    assert abs(float(want['loss'][0]) - float(ref_loss) - (acc or 0.0)) <= 1e-12 * (abs(float(ref_loss)) + 5)
                    got = mc.emulate_f32(l, t, lm, cw, scale, eps, old_loss=acc)
                    worst = max(worst, mc.check('emulation (%d, %d) %s eps %g lam %s' % (N, NC, wm, eps, lam), got, want))
    print('emulation (%d, %d): worst err/bound %.3f' % (N, NC, worst))
    assert 0.0 <= worst <= 1.0


def test_loss_reference_special_cases():
    N, NC = 7, 5
    l, t, lm, cw = mc.loss_inputs(N, NC, 'random', 'ones')
    # lam == 1: the smoothed one-target loss, reference and bound side by side
    for eps in (0.0, 0.1):
        a, b = mc.xent_mix(l, t, lm, cw, 0.4, eps), sb.xent_ls(l, t, cw, 0.4, eps)
        for k in ('loss', 'dlogits'):
            assert torch.allclose(a[k][0], b[k][0], rtol=1e-13, atol=1e-300)
    # no weights, no smoothing: timm's SoftTargetCrossEntropy on mixup_target
    l, t, lm, _ = mc.loss_inputs(N, NC, 'none', 'rows')
    oh = torch.nn.functional.one_hot(t, NC).double()
    tgt = lm.double()[:, None] * oh + (1 - lm.double()[:, None]) * oh.flip(0)
    want = (-tgt * torch.log_softmax(l.double(), 1)).sum(1).mean()
    assert abs(float(mc.loss_reference(l, t, lm, None, 1.0, 0.0)[0]) - float(want)) <= 1e-13 * abs(float(want))
    # the gradient is the derivative of the loss
    ld = l.double().requires_grad_(True)
    lam64, w = lm.double(), cw.double()
    logp = torch.log_softmax(ld, 1)
    r = torch.arange(N)
    ta, tb = lam64 * w[t], (1 - lam64) * w[t.flip(0)]
    loss = 0.4 / (ta + tb).sum() * (0.9 * (ta * -logp[r, t] + tb * -logp[r, t.flip(0)]) + 0.1 / NC * (w[None] * -logp).sum(1)).sum()
    loss.backward()
    _, dl = mc.loss_reference(l, t, lm, cw, 0.4, 0.1)
    assert torch.allclose(ld.grad, dl, rtol=1e-5, atol=1e-9)              # (0.4 and 0.1 are rounded to fp32 in the reference)


# ------------------------------------------------------------------------------------------------------ plans
def _plan(model, B, dtype='bf16', env=None, **kw):
    keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
    with mock.patch.dict(os.environ, dict(keep, **(env or {})), clear=True), mock.patch.object(torch, 'zeros', torch.empty), \
            mock.patch.object(torch, 'zeros_like', torch.empty_like):
        eng = Engine(graph.build(model, 7), max_batch=B, dtype=dtype, plan_only=True, **kw)
        return eng, eng.plan(B)


def _table(pl):
    out = []
    for prog in mpf.PROGRAMS:
        p = getattr(pl, prog)
        out.append((prog, [(o.kind, o.flags, tuple(o.i), tuple(o.f), bytes(o.u)) for o in (p.arr[k] for k in range(p.n))], list(p.tags)))
    return out


@pytest.mark.parametrize('kw', [dict(), dict(class_weights=[0.5, 1.0, 2.0, 1.0, 1.0, 3.0, 0.1], label_smoothing=0.1)], ids=['plain', 'cw_ls'])
def test_mix_engine_puts_the_slot_factors_into_the_train_loss_ops_only(kw):
    eng, pl = _plan('inception_v3', 2, mix=True, **kw)
    assert len(eng.mix_lam) == 2 and all(t.dtype == torch.float32 and t.numel() == 2 and t.tolist() == [1.0, 1.0] for t in eng.mix_lam)
    lam0 = eng.mix_lam[0].data_ptr()
    for prog in ('loss', 'step', 'fwd_loss', 'fwd_bwd'):
        p = getattr(pl, prog)
        ops = [p.arr[k] for k in range(p.n) if p.tags[k] in ('loss', 'loss_aux')]
        assert len(ops) == 2 and all(o.p[5] == lam0 for o in ops), prog
        assert all((o.p[4] == eng.class_weight.data_ptr()) if kw else (o.p[4] is None) for o in ops)
        assert all(o.f[2] == 0.0 and abs(o.f[1] - kw.get('label_smoothing', 0.0)) < 1e-7 for o in ops)
    ev = pl.eval_loss.arr[0]
    assert pl.eval_loss.n == 1 and ev.p[5] is None and ev.kind == ops[0].kind
    # the other slot's plan holds the other array
    eng._select_slot(1)
    pl1 = eng.plan(2)
    ops1 = [pl1.loss.arr[k] for k in range(pl1.loss.n)]
    assert all(o.p[5] == eng.mix_lam[1].data_ptr() for o in ops1) and eng.mix_lam[1].data_ptr() != lam0
    # everything but p[5] is the table of an engine without mix
    eng0, pl0 = _plan('inception_v3', 2, **kw)
    assert _table(pl) == _table(pl0)
    with pytest.raises(RuntimeError, match='without mix'):
        eng0.mix_batch(2, 0.5)
    with pytest.raises(ValueError, match='focal_gamma'):
        _plan('resnet18', 2, mix=True, focal_gamma=2.0)


@pytest.mark.parametrize('model,B', [('inception_v3', 2), ('resnet18', 4)])
def test_mix_false_is_the_default_engine(model, B):
    eng0, pl0 = _plan(model, B)
    eng1, pl1 = _plan(model, B, mix=False)
    assert not hasattr(eng1, 'mix_lam') and not hasattr(eng0, 'mix_lam')
    assert mpf.plan_text(eng1, pl1) == mpf.plan_text(eng0, pl0)
    for prog in mpf.PROGRAMS:
        p = getattr(pl1, prog)
        assert all(p.arr[k].p[5] is None for k in range(p.n) if p.arr[k].kind in (_lib.OP_SOFTMAX_XENT, _lib.OP_SOFTMAX_XENT_W))


def test_op_kernel_and_cost_name_the_mix_loss_only_with_p5():
    import ctypes as C
    eng, pl = _plan('resnet18', 2, mix=True)
    lib = _lib.load()
    name = C.create_string_buffer(128)
    fl, by = C.c_double(), C.c_double()
    o = pl.loss.arr[0]
    assert lib.ifcbk_op_kernel(C.byref(o), name, 128) == 0 and name.value == b'softmax_xent_mix_kernel'
    assert lib.ifcbk_op_cost(C.byref(o), C.byref(fl), C.byref(by)) == 0 and by.value == 2 * 7 * 8 + 2 * 12 and fl.value > 0
    e = pl.eval_loss.arr[0]
    name.value = b''
    assert lib.ifcbk_op_kernel(C.byref(e), name, 128) == 0 and name.value == b''
    assert lib.ifcbk_op_cost(C.byref(e), C.byref(fl), C.byref(by)) == 0 and by.value == 0 and fl.value == 0


# ------------------------------------------------------------------------------------------------------ header, binding
def test_the_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'ifcbk.h')).read()
    for fn in ('ifcbk_batch_mix', 'ifcbk_softmax_xent_mix'):
        assert 'IFCBK_API int %s(' % fn in hdr
        assert fn in _lib.EXPORTS and getattr(_lib.load(), fn).argtypes is not None
    assert len(_lib._PROTOS['ifcbk_batch_mix'][1]) == 11 and len(_lib._PROTOS['ifcbk_softmax_xent_mix'][1]) == 13
    assert '#define IFCBK_MIX_U8 2' in hdr and _lib.MIX_U8 == 2
    assert max(_lib.OP_NAMES) == 40                                    # no new op kind
    mk = open(os.path.join(os.path.dirname(HERE), 'ifcb_classifier_amd', 'csrc', 'Makefile')).read()
    assert 'batch_mix.hip' in mk


# ------------------------------------------------------------------------------------------------------ args.yml, .ptl
class _HostEngine(Engine):
    def __init__(self, *a, **k):
        k['plan_only'] = True
        super().__init__(*a, **k)


def _hparams(**kw):
    hp = dict(MODEL='resnet18', classes=['a', 'b', 'c'], pretrained=False, batch_size=2, precision='fp32', model_id='m', seed=1, resize=224,
              img_norm=None)
    hp.update(kw)
    return argparse.Namespace(**hp)


def test_hparams_round_trip_and_old_checkpoints(tmp_path):
    import yaml
    a = _parse('--mixup', '0.4', '--cutmix', '1.0', '--mix-prob', '0.75')
    y = yaml.safe_load(yaml.safe_dump({k: (v if isinstance(v, (int, float, str, bool, list, type(None))) else str(v)) for k, v in vars(a).items()}))
    assert (y['mixup'], y['cutmix'], y['mix_prob']) == (0.4, 1.0, 0.75)
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(_hparams(mixup=0.4, cutmix=1.0, mix_prob=0.75, label_smoothing=0.1))
        assert m.model.engine.mix and (m.mixup, m.cutmix, m.mix_prob) == (0.4, 1.0, 0.75) and m.batch_mix is None
        ck = m.checkpoint_dict()
        hp = ck['hyper_parameters']
        assert (hp['mixup'], hp['cutmix'], hp['mix_prob']) == (0.4, 1.0, 0.75)
        path = str(tmp_path / 'm.ptl')
        torch.save(ck, path)
        m2 = neuston_models.NeustonModel.load_from_checkpoint(path)
        assert m2.model.engine.mix and (m2.mixup, m2.cutmix, m2.mix_prob) == (0.4, 1.0, 0.75)
        # a checkpoint without the keys: mixing off, the engine without factors
        for k in ('mixup', 'cutmix', 'mix_prob'):
            del ck['hyper_parameters'][k]
        torch.save(ck, path)
        m3 = neuston_models.NeustonModel.load_from_checkpoint(path)
        assert not m3.model.engine.mix and (m3.mixup, m3.cutmix, m3.mix_prob) == (0.0, 0.0, 1.0) and not hasattr(m3.model.engine, 'mix_lam')
        with pytest.raises(ValueError, match='focal_gamma'):
            neuston_models.NeustonModel(_hparams(mixup=0.4, focal_gamma=2.0))
