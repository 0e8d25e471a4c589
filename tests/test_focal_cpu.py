"""TRAIN --focal-gamma on the host: loss_focal_bounds' reference against float64 autograd and, at gamma 0, torch's weighted
F.cross_entropy; the bound against a float32 emulation of the kernel's operation order; the criterion module; the flag; the op tables
Engine(plan_only=True) builds with and without it; and the .ptl / args.yml round trip.  The kernel (ifcbk_softmax_xent_focal,
csrc/loss.hip) runs in tests/test_gpu_focal.py."""
import argparse
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_focal_bounds as fb
import op_bounds as ob
import program_footprints as pf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_plan_fingerprints as mpf  # noqa: E402

from ifcb_classifier_amd import _lib, graph, neuston_models, neuston_net  # noqa: E402
from ifcb_classifier_amd.engine import Engine  # noqa: E402


# ------------------------------------------------------------------------------------------------------ reference and bound
@pytest.mark.parametrize('mode', [None, 'row120', 'peak120', 'low80'])
@pytest.mark.parametrize('N,NC', [(3, 2), (3, 5), (257, 3), (40, 101)])
def test_reference_gradient_is_float64_autograd_of_its_loss(N, NC, mode):
    """the gradient formula of the definition, to 1e-12 of each row's largest element -- the row 120 higher, the row whose target stands 120
    above it (u ~ 1e-52, a gradient of the order 1e-52 (g + 1)) and the row whose target lies 80 below (u -> 1) included"""
    for wm in ('none', 'random', 'zero'):
        for g in (0.5, 1.0, 2.0, 5.0):
            l, t, cw = fb.inputs(N, NC, wm, mode=mode)
            loss, dl = fb.reference(l, t, cw, 0.4, g)
            x = l.double().clone().requires_grad_(True)
            w = torch.ones(NC, dtype=torch.float64) if cw is None else cw.double()
            got = fb.loss64(x, t, w, ob.f32(0.4), ob.f32(g))
            got.backward()
            assert abs(float(got.detach()) - float(loss)) <= 1e-13 * abs(float(loss)), (wm, g)
            assert torch.isfinite(x.grad).all() and torch.isfinite(dl).all()
            scale = x.grad.abs().max(1, keepdim=True).values
            # (+ 1e-300: at gamma 5 the peak row's gradient, ~1e-312, is a float64 subnormal, which has no relative precision)
            assert bool(((dl - x.grad).abs() <= 1e-12 * scale + 1e-300).all()), (wm, g, float(((dl - x.grad).abs() / scale.clamp_min(1e-300)).max()))


@pytest.mark.parametrize('N,NC', fb.SHAPES)
def test_gamma_0_is_torchs_weighted_cross_entropy_in_float64(N, NC):
    for wm in fb.WEIGHTS:
        if wm == 'zero' and NC == 1:
            continue
        l, t, cw = fb.inputs(N, NC, wm)
        loss, dl = fb.reference(l, t, cw, 0.4, 0.0)
        x = l.double().clone().requires_grad_(True)
        tt = F.cross_entropy(x, t, weight=None if cw is None else cw.double()) * ob.f32(0.4)
        tt.backward()
        assert abs(float(loss) - float(tt)) <= 1e-13 * max(1.0, abs(float(tt))), wm
        assert float((dl - x.grad).abs().max()) <= 1e-14, wm
        want = fb.xent_focal(l, t, cw, 0.4, 0.0)
        assert torch.allclose(want['loss'][0], loss.reshape(1), rtol=1e-13, atol=0) and torch.allclose(want['dlogits'][0], dl, rtol=1e-13, atol=0)


@pytest.mark.parametrize('N,NC', fb.SHAPES)
def test_the_kernels_operations_in_float32_pass_the_bound(N, NC):
    """the bound is self-consistent: the kernel's operation order in float32 torch is inside it at every shape, weighting, exponent and
    special row -- so the float64 reference sits inside the bound of a correct fp32 implementation on this CPU"""
    worst = 0.0
    for wm in fb.WEIGHTS:
        if wm == 'zero' and NC == 1:
            continue
        # every exponent on the plain rows; the special rows with the weights, at an exponent below and one above 1
        for g, mode in [(g, None) for g in (0.0,) + fb.GAMMAS] + [(g, m) for m in fb.MODES[1:] for g in (0.5, 2.0) if wm == 'random']:
            l, t, cw = fb.inputs(N, NC, wm, mode=mode)
            want = fb.xent_focal(l, t, cw, 0.4, g, old_loss=5.0 if mode == 'row80' else None)
            assert all(bool(torch.isfinite(e).all()) for _, e in want.values())
            got = fb.emulate(l, t, cw, 0.4, g, old_loss=5.0 if mode == 'row80' else None)
            worst = max(worst, fb.check('focal (%d, %d) %s g %g %s' % (N, NC, wm, g, mode), got, want))
            if mode == 'peak120' and g > 0:
                assert not got['dlogits'][N // 2].any()
    print('focal (%d, %d): float32 emulation worst err/bound %.3f' % (N, NC, worst))
    assert worst < 1.0


def _variant(l, t, cw, g, norm=None, second=True, alpha=True):
    """the definition with one planted fault: the normaliser, the bracket without its second term, the gradient without w[t]"""
    l = l.double()
    N, NC = l.shape
    p, oh, u, pt, L = fb.parts(l, t)
    w = cw.double()
    wt = w[t][:, None]
    W = wt.sum() if norm is None else norm
    B = u ** g + (g * pt * u ** (g - 1.0) * L if second else 0.0)
    return {'loss': ((wt * u ** g * L).sum() / W).reshape(1), 'dlogits': (wt if alpha else 1.0) * torch.where(oh > 0, -u, p) * B / W}


FAULTS = {'normaliser N': lambda N: dict(norm=float(N)), 'bracket without its second term': lambda N: dict(second=False),
          'gradient without alpha': lambda N: dict(alpha=False)}


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_planted_faults_are_flagged(fault):
    flagged = []
    shapes = [(N, NC) for N, NC in fb.SHAPES if NC >= 2]
    for N, NC in shapes:
        l, t, cw = fb.inputs(N, NC, 'random')
        want = fb.xent_focal(l, t, cw, 1.0, 2.0)
        assert fb.check('no fault', _variant(l, t, cw, 2.0), want) < 1e-3
        bad = _variant(l, t, cw, 2.0, **FAULTS[fault](N))
        if fb.check(fault, bad, want, raise_=False) > 1.0:
            flagged.append((N, NC))
    print('%s: flagged at %d of %d shapes' % (fault, len(flagged), len(shapes)))
    assert (600, 100) in flagged and (3, 5) in flagged and len(flagged) >= 20, flagged


# ------------------------------------------------------------------------------------------------------ the criterion module
@pytest.mark.parametrize('N,NC', [(3, 5), (257, 3), (40, 101)])
def test_criterion_module_in_float64_is_the_reference(N, NC):
    for wm in fb.WEIGHTS:
        for g in fb.GAMMAS:
            for mode in (None, 'peak120', 'low80'):
                l, t, cw = fb.inputs(N, NC, wm, mode=mode)
                crit = neuston_models.FocalLoss(g, None if cw is None else cw.clone())
                assert crit.gamma == g and (crit.weight is None) == (cw is None)
                assert list(crit.state_dict()) == ([] if cw is None else ['weight'])
                x = l.double().clone().requires_grad_(True)
                got = crit(x, t)
                got.backward()
                loss, dl = fb.reference(l, t, cw, 1.0, g)
                assert abs(float(got.detach()) - float(loss)) <= 1e-12 * abs(float(loss)) + 1e-300, (wm, g, mode)
                scale = dl.abs().max(1, keepdim=True).values
                big = scale[:, 0] > 1e-30                         # (the module forms L from log s: rows with u below 1e-16 lose it; they weigh nothing)
                assert bool(((dl - x.grad).abs()[big] <= 1e-9 * scale[big]).all()), (wm, g, mode)
                # float32, as training_step runs it: inside the kernel's bound
                fb.check('criterion float32', {'loss': crit(l, t).reshape(1)}, fb.xent_focal(l, t, cw, 1.0, g))


# ------------------------------------------------------------------------------------------------------ argparse
def _parse(*extra):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'inception_v3', 'id'] + list(extra))


def test_flag(capsys):
    assert _parse().focal_gamma == 0.0 and _parse().label_smoothing == 0.0
    assert _parse('--focal-gamma', '2').focal_gamma == 2.0 and _parse('--focal-gamma', '0.5', '--class-norm').class_norm == 1.0
    assert _parse('--focal-gamma', '0').focal_gamma == 0.0
    assert _parse('--focal-gamma', '0', '--label-smoothing', '0.1').label_smoothing == 0.1
    assert _parse('--focal-gamma', '2', '--label-smoothing', '0').focal_gamma == 2.0
    for bad in ('-1', 'nan', 'inf', '-inf', 'two'):
        with pytest.raises(SystemExit):
            _parse('--focal-gamma=' + bad)
    capsys.readouterr()
    for argv in (('--focal-gamma', '2', '--label-smoothing', '0.1'), ('--label-smoothing', '0.1', '--focal-gamma', '2')):
        with pytest.raises(SystemExit):
            _parse(*argv)
        err = capsys.readouterr().err
        assert '--focal-gamma' in err and '--label-smoothing' in err


# ------------------------------------------------------------------------------------------------------ plans
def _plan(model, B, dtype='bf16', **kw):
    """Engine(plan_only=True) and its plan, built the way tests/golden/make_plan_fingerprints.py builds them"""
    keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
    with mock.patch.dict(os.environ, keep, clear=True), mock.patch.object(torch, 'zeros', torch.empty), \
            mock.patch.object(torch, 'zeros_like', torch.empty_like):
        eng = Engine(graph.build(model, 7), max_batch=B, dtype=dtype, plan_only=True, **kw)
        return eng, eng.plan(B)


def _ops(eng, pl):
    """[(program, index, kind, flags, tag, i, f, descriptor bytes, symbolic pointers)] of every program of the plan"""
    owners = mpf.Owners(eng, pl)
    out = []
    for prog in mpf.PROGRAMS:
        p = getattr(pl, prog)
        for k in range(p.n):
            o = p.arr[k]
            host = o.kind == _lib.OP_CONV_WGRAD_GROUP
            ptrs = tuple('host' if (j == 0 and host) else owners.sym(o.p[j]) for j in range(12))
            out.append((prog, k, o.kind, o.flags, p.tags[k], tuple(o.i), tuple(o.f), bytes(o.u), ptrs))
    return out


W7 = [0.01, 0.5, 1.0, 2.0, 8.0, 30.0, 100.0]


@pytest.mark.parametrize('model,B', [('inception_v3', 2), ('resnet18', 2)])
def test_gamma_0_or_absent_builds_the_default_plan(model, B):
    eng0, pl0 = _plan(model, B)
    for kw in (dict(focal_gamma=0.0), dict(focal_gamma=None), dict(focal_gamma=0.0, label_smoothing=0.0)):
        eng1, pl1 = _plan(model, B, **kw)
        assert eng1.focal_gamma == 0.0
        assert mpf.plan_text(eng1, pl1) == mpf.plan_text(eng0, pl0)
        assert _ops(eng1, pl1) == _ops(eng0, pl0)
    # ... and smoothing alone still writes f[1] only
    eng2, pl2 = _plan(model, B, label_smoothing=0.1, focal_gamma=0.0)
    f = [x[6] for x in _ops(eng2, pl2) if x[2] == _lib.OP_SOFTMAX_XENT]
    assert f and all(v[1] == float(np.float32(0.1)) and v[2] == 0.0 for v in f)


@pytest.mark.parametrize('weights', [None, W7])
@pytest.mark.parametrize('model,B', [('inception_v3', 2), ('resnet18', 2)])
def test_gamma_is_f2_of_the_loss_ops_and_nothing_else_changes(model, B, weights):
    eng0, pl0 = _plan(model, B, class_weights=weights)
    eng1, pl1 = _plan(model, B, class_weights=weights, focal_gamma=2.0)
    assert eng1.focal_gamma == 2.0 and eng1.label_smoothing == 0.0
    kind = _lib.OP_SOFTMAX_XENT if weights is None else _lib.OP_SOFTMAX_XENT_W
    a, b = _ops(eng1, pl1), _ops(eng0, pl0)
    assert len(a) == len(b)
    tags = {}
    for x, y in zip(a, b):
        if y[2] == kind:
            tags.setdefault(x[0], []).append(x[4])
            a0 = float(np.float32(0.4 if x[4] == 'loss_aux' else 1.0))
            assert y[6][:3] == (a0, 0.0, 0.0) and x[6][:3] == (a0, 0.0, 2.0)
            assert x[:6] + (x[6][3:],) + x[7:] == y[:6] + (y[6][3:],) + y[7:]
        else:
            assert x == y
            assert x[2] not in (_lib.OP_SOFTMAX_XENT, _lib.OP_SOFTMAX_XENT_W)
    heads = ['loss', 'loss_aux'] if model == 'inception_v3' else ['loss']
    assert tags['loss'] == heads and tags['eval_loss'] == ['val_loss'] and tags['step'] == heads
    for prog in mpf.PROGRAMS:
        p = getattr(pl1, prog)
        assert pf.unordered_conflicts(eng1, p.arr, p.n, p.tags) == [], prog


def test_engine_refusals():
    for bad in (-1.0, float('nan'), float('inf'), -float('inf')):
        with pytest.raises(ValueError, match='focal_gamma'):
            _plan('resnet18', 2, focal_gamma=bad)
    with pytest.raises(ValueError, match='label_smoothing'):
        _plan('resnet18', 2, focal_gamma=2.0, label_smoothing=0.1)


# ------------------------------------------------------------------------------------------------------ .ptl / args.yml round trip on the host
class _HostEngine(Engine):
    """the engine NeustonModel builds, without a device: parameters, views and optimizer state live on the host"""

    def __init__(self, *a, **k):
        k['plan_only'] = True
        super().__init__(*a, **k)


def _hparams(**kw):
    hp = dict(MODEL='resnet18', classes=['a', 'b', 'c'], pretrained=False, batch_size=2, precision='fp32', model_id='m', seed=1, resize=224,
              img_norm=None)
    hp.update(kw)
    return argparse.Namespace(**hp)


def test_ptl_round_trip_on_the_host(tmp_path):
    w = [0.5, 1.0, 4.0]
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(_hparams(focal_gamma=2.0, class_weights=w))
        assert m.model.engine.focal_gamma == 2.0 and isinstance(m.criterion, neuston_models.FocalLoss)
        assert m.criterion.gamma == 2.0 and m.criterion.weight.tolist() == w
        ck = m.checkpoint_dict(epoch=1, global_step=2)
        assert ck['hyper_parameters']['focal_gamma'] == 2.0 and ck['state_dict']['criterion.weight'].tolist() == w
        path = str(tmp_path / 'm.ptl')
        torch.save(ck, path)
        m2 = neuston_models.NeustonModel.load_from_checkpoint(path)
        assert m2.hparams.focal_gamma == 2.0 and m2.model.engine.focal_gamma == 2.0 and m2.criterion.gamma == 2.0
        assert m2.criterion.weight.tolist() == w
        for k, v in m.model.state_dict().items():
            assert torch.equal(v, m2.model.state_dict()[k]), k
        l, t, _ = fb.inputs(3, 3, 'none')
        fb.check('criterion', {'loss': m2.criterion(l, t).reshape(1)}, fb.xent_focal(l, t, torch.tensor(w), 1.0, 2.0))
        # inference ignores it: the same weights
        m3 = neuston_models.NeustonModel.load_from_checkpoint(path, inference=True)
        for k, v in m.model.state_dict().items():
            assert torch.equal(v, m3.model.state_dict()[k]), k
        # a checkpoint without the key, or with None, loads with gamma 0: torch's criterion, as before
        for drop in (True, False):
            hp = dict(ck['hyper_parameters'])
            if drop:
                del hp['focal_gamma']
            else:
                hp['focal_gamma'] = None
            old = str(tmp_path / 'old.ptl')
            torch.save(dict(ck, hyper_parameters=hp), old)
            m4 = neuston_models.NeustonModel.load_from_checkpoint(old)
            assert m4.model.engine.focal_gamma == 0.0 and isinstance(m4.criterion, torch.nn.CrossEntropyLoss)
            assert m4.criterion.weight.tolist() == w
        plain = neuston_models.NeustonModel(_hparams(focal_gamma=2.0))
        assert plain.criterion.weight is None and 'criterion.weight' not in plain.state_dict()
        plain.load_state_dict(ck['state_dict'])
        assert isinstance(neuston_models.NeustonModel(_hparams()).criterion, torch.nn.CrossEntropyLoss)
        with pytest.raises(ValueError):
            neuston_models.NeustonModel(_hparams(focal_gamma=2.0, label_smoothing=0.1))


def test_args_yml_carries_the_flag():
    """do_training dumps vars(args) to args.yml and hands the same namespace to NeustonModel as its hyper-parameters"""
    import yaml
    args = _parse('--focal-gamma', '2')
    dumped = yaml.safe_load(yaml.safe_dump({k: (v if isinstance(v, (int, float, str, bool, list, type(None))) else str(v))
                                            for k, v in vars(args).items()}))
    assert dumped['focal_gamma'] == 2.0 and dumped['label_smoothing'] == 0.0
    assert yaml.safe_load(yaml.safe_dump(vars(_parse())))['focal_gamma'] == 0.0


def test_onnx_export_ignores_it(tmp_path):
    from ifcb_classifier_amd import onnx_export
    sds = []
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        for kw in (dict(focal_gamma=2.0), dict()):
            torch.manual_seed(3)
            sds.append(neuston_models.NeustonModel(_hparams(**kw)).checkpoint_dict()['state_dict'])
    assert list(sds[0]) == list(sds[1]) and not [k for k in sds[0] if k.startswith('criterion')]
    a, b = str(tmp_path / 'a.onnx'), str(tmp_path / 'b.onnx')
    onnx_export.export(sds[0], 'resnet18', ['a', 'b', 'c'], False, a)
    onnx_export.export(sds[1], 'resnet18', ['a', 'b', 'c'], False, b)
    assert open(a, 'rb').read() == open(b, 'rb').read()


# ------------------------------------------------------------------------------------------------------ the entry point
def test_the_entry_point_is_bound():
    assert 'ifcbk_softmax_xent_focal' in _lib.EXPORTS
    fn = getattr(_lib.load(), 'ifcbk_softmax_xent_focal')
    assert fn.argtypes is not None and len(fn.argtypes) == 12                       # ctx + the 11 of the header
    root = os.path.dirname(HERE)
    hdr = open(os.path.join(root, 'include', 'ifcbk.h')).read()
    assert 'IFCBK_API int ifcbk_softmax_xent_focal(' in hdr and 'f[2] = focal-loss gamma' in hdr
    assert 'f[1] = label smoothing factor' in hdr                                  # (the sentence before it stays)
    # the export map passes every ifcbk_* symbol and the library holds this one
    assert 'global: ifcbk_*;' in open(os.path.join(root, 'ifcb_classifier_amd', 'csrc', 'exports.map')).read()
    # no new op kind
    assert _lib.OP_SOFTMAX_XENT_W == 40 and max(_lib.OP_NAMES) == 40
