"""TRAIN --label-smoothing on the host: loss_smooth_bounds' reference and bound against torch's own F.cross_entropy(weight=,
label_smoothing=), the faults the bound is there to catch, the flag, the op tables Engine(plan_only=True) builds with and without it, and
the .ptl / args.yml round trip.  The kernel (ifcbk_softmax_xent_ls, csrc/loss.hip) runs in tests/test_gpu_label_smoothing.py."""
import argparse
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_bounds as lb
import loss_smooth_bounds as sb
import op_bounds as ob
import program_footprints as pf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_plan_fingerprints as mpf  # noqa: E402

from ifcb_classifier_amd import _lib, graph, neuston_models, neuston_net  # noqa: E402
from ifcb_classifier_amd.engine import Engine  # noqa: E402

EPS = (0.1, 0.5, 1.0)


# ------------------------------------------------------------------------------------------------------ reference and bound
def _torch(l, t, cw, scale, eps, dtype):
    x = l.to(dtype).clone().requires_grad_(True)
    loss = F.cross_entropy(x, t, weight=None if cw is None else cw.to(dtype), label_smoothing=eps) * scale
    loss.backward()
    return {'dlogits': x.grad, 'loss': loss.detach().reshape(1)}


@pytest.mark.parametrize('N,NC', sb.SHAPES)
def test_reference_is_torchs_definition_in_float64(N, NC):
    for wm in sb.WEIGHTS:
        if wm == 'zero' and NC == 1:
            continue
        for eps in (0.0,) + EPS:
            l, t, cw = sb.inputs(N, NC, wm)
            loss, dl = sb.reference(l, t, cw, 0.4, eps)
            tt = _torch(l, t, cw, ob.f32(0.4), ob.f32(eps), torch.float64)
            assert abs(float(loss) - float(tt['loss'])) <= 1e-13 * max(1.0, abs(float(loss))), (wm, eps)
            assert float((dl - tt['dlogits']).abs().max()) <= 1e-14, (wm, eps)
            want = sb.xent_ls(l, t, cw, 0.4, eps)
            assert torch.allclose(want['loss'][0], loss.reshape(1), rtol=1e-13, atol=0) and float((want['dlogits'][0] - dl).abs().max()) <= 1e-15


@pytest.mark.parametrize('N,NC', sb.SHAPES)
def test_torch_float32_passes_the_bound(N, NC):
    """the condition for holding the HIP kernel to the bound: torch's own float32 value and autograd gradient are inside it"""
    worst = 0.0
    for wm in sb.WEIGHTS:
        if wm == 'zero' and NC == 1:
            continue
        for eps in (0.0,) + EPS:
            for off in (False, True):
                l, t, cw = sb.inputs(N, NC, wm, offset_row=off)
                want = sb.xent_ls(l, t, cw, 1.0, eps)
                got = _torch(l, t, cw, 1.0, eps, torch.float32)
                worst = max(worst, sb.check('xent_ls (%d, %d) %s eps %g' % (N, NC, wm, eps), got, want))
    print('smoothed xent (%d, %d): torch float32 worst err/bound %.3f' % (N, NC, worst))
    assert worst < 1.0


def _variant(l, t, cw, eps, div=None, norm=None, smooth_w=True, hard_c1=True):
    """the definition in float64 with one planted fault: div = the divisor of eps (C), norm = the normaliser (W), the smoothing term
    with / without w[j], the one-hot term with / without (1 - eps)"""
    l = l.double()
    N, NC = l.shape
    eps = ob.f32(eps)
    w = cw.double()
    ws = w if smooth_w else torch.ones_like(w)
    wt = w[t][:, None]
    W = wt.sum() if norm is None else norm
    eC = eps / (NC if div is None else div)
    c1 = 1.0 - eps if hard_c1 else 1.0
    logp = torch.log_softmax(l, 1)
    oh = F.one_hot(t, NC).double()
    loss = (c1 * wt[:, 0] * -logp[torch.arange(N), t] + eC * (ws[None] * -logp).sum(1)).sum() / W
    dl = ((c1 * wt + eC * ws.sum()) * logp.exp() - c1 * wt * oh - eC * ws[None]) / W
    return {'loss': loss.reshape(1), 'dlogits': dl}


FAULTS = {'eps / (C - 1)': lambda N, NC: dict(div=NC - 1), 'normaliser N': lambda N, NC: dict(norm=float(N)),
          'smoothing term without w[j]': lambda N, NC: dict(smooth_w=False), 'one-hot term without (1 - eps)': lambda N, NC: dict(hard_c1=False)}


@pytest.mark.parametrize('fault', sorted(FAULTS))
def test_planted_faults_are_flagged(fault):
    """each fault exceeds the bound (err / bound > 1), in the loss and in the gradient, at listed shapes; the unfaulted variant passes"""
    flagged = []
    for N, NC in sb.SHAPES:
        if NC < 2:
            continue
        l, t, cw = sb.inputs(N, NC, 'random')
        want = sb.xent_ls(l, t, cw, 1.0, 0.1)
        assert sb.check('no fault', _variant(l, t, cw, 0.1), want) < 1e-3
        bad = _variant(l, t, cw, 0.1, **FAULTS[fault](N, NC))
        r = [sb.check(fault, {k: bad[k]}, want, raise_=False) for k in ('loss', 'dlogits')]
        if min(r) > 1.0:
            flagged.append((N, NC))
    print('%s: flagged at %d of %d shapes' % (fault, len(flagged), len(sb.SHAPES)))
    assert (600, 100) in flagged and (3, 5) in flagged and len(flagged) >= 20, flagged


@pytest.mark.parametrize('N,NC', [(3, 5), (257, 101), (600, 100)])
def test_eps_0_is_the_weighted_loss_of_loss_bounds(N, NC):
    l, t, cw = sb.inputs(N, NC, 'random')
    a = sb.xent_ls(l, t, cw, 0.4, 0.0, old_loss=5.0)
    b = lb.xent_w(l, t, cw, 0.4, old_loss=5.0)
    for k in ('loss', 'dlogits'):
        assert torch.allclose(a[k][0], b[k][0], rtol=1e-13, atol=1e-300), k
    c = sb.xent_ls(l, t, None, 0.4, 0.0)
    d = ob.xent(l, t, 0.4)
    for k in ('loss', 'dlogits'):
        assert torch.allclose(c[k][0], d[k][0], rtol=1e-13, atol=1e-300), k


# ------------------------------------------------------------------------------------------------------ argparse
def _parse(*extra):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'inception_v3', 'id'] + list(extra))


def test_flag():
    assert _parse().label_smoothing == 0.0
    assert _parse('--label-smoothing', '0.1').label_smoothing == 0.1
    assert _parse('--label-smoothing', '0').label_smoothing == 0.0 and _parse('--label-smoothing', '1').label_smoothing == 1.0
    for bad in ('-0.1', '1.5', 'nan'):
        with pytest.raises(SystemExit):
            _parse('--label-smoothing=' + bad)


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


def _frozen(pl, prog):
    p = getattr(pl, prog)
    return [(o.kind, o.flags, tuple(o.i), tuple(o.f), bytes(o.u)) for o in (p.arr[k] for k in range(p.n))]


W7 = [0.01, 0.5, 1.0, 2.0, 8.0, 30.0, 100.0]


@pytest.mark.parametrize('model,B', [('inception_v3', 2), ('resnet18', 2)])
def test_eps_0_or_absent_builds_the_default_plan(model, B):
    eng0, pl0 = _plan(model, B)
    for kw in (dict(label_smoothing=0.0), dict(label_smoothing=None)):
        eng1, pl1 = _plan(model, B, **kw)
        assert eng1.label_smoothing == 0.0
        assert mpf.plan_text(eng1, pl1) == mpf.plan_text(eng0, pl0)
        assert _ops(eng1, pl1) == _ops(eng0, pl0)
        for prog in ('loss', 'eval_loss', 'step'):
            assert _frozen(pl1, prog) == _frozen(pl0, prog), prog


@pytest.mark.parametrize('weights', [None, W7])
@pytest.mark.parametrize('model,B', [('inception_v3', 2), ('resnet18', 2)])
def test_eps_changes_f1_of_the_loss_ops_and_nothing_else(model, B, weights):
    eng0, pl0 = _plan(model, B, class_weights=weights)
    eng1, pl1 = _plan(model, B, class_weights=weights, label_smoothing=0.1)
    assert eng1.label_smoothing == 0.1
    kind = _lib.OP_SOFTMAX_XENT if weights is None else _lib.OP_SOFTMAX_XENT_W
    eps = float(np.float32(0.1))
    a, b = _ops(eng1, pl1), _ops(eng0, pl0)
    assert len(a) == len(b)
    tags = {}
    for x, y in zip(a, b):
        if y[2] == kind:
            tags.setdefault(x[0], []).append(x[4])
            assert y[6][1] == 0.0 and x[6][1] == eps
            assert x[6][0] == y[6][0] == float(np.float32(0.4 if x[4] == 'loss_aux' else 1.0))
            assert x[:6] + (x[6][:1] + x[6][2:],) + x[7:] == y[:6] + (y[6][:1] + y[6][2:],) + y[7:]
        else:
            assert x == y
            assert x[2] not in (_lib.OP_SOFTMAX_XENT, _lib.OP_SOFTMAX_XENT_W)
    heads = ['loss', 'loss_aux'] if model == 'inception_v3' else ['loss']
    assert tags['loss'] == heads and tags['eval_loss'] == ['val_loss'] and tags['step'] == heads
    # the pointer footprint of either kind is what it was: the audit of the lane schedules finds nothing
    for prog in mpf.PROGRAMS:
        p = getattr(pl1, prog)
        assert pf.unordered_conflicts(eng1, p.arr, p.n, p.tags) == [], prog


def test_engine_refuses_a_factor_outside_0_1():
    for bad in (-0.1, 1.5, float('nan'), float('inf')):
        with pytest.raises(ValueError):
            _plan('resnet18', 2, label_smoothing=bad)


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
        m = neuston_models.NeustonModel(_hparams(label_smoothing=0.1, class_weights=w))
        assert m.model.engine.label_smoothing == 0.1 and m.criterion.label_smoothing == 0.1 and m.criterion.weight.tolist() == w
        ck = m.checkpoint_dict(epoch=1, global_step=2)
        assert ck['hyper_parameters']['label_smoothing'] == 0.1
        path = str(tmp_path / 'm.ptl')
        torch.save(ck, path)
        m2 = neuston_models.NeustonModel.load_from_checkpoint(path)
        assert m2.hparams.label_smoothing == 0.1 and m2.model.engine.label_smoothing == 0.1 and m2.criterion.label_smoothing == 0.1
        for k, v in m.model.state_dict().items():
            assert torch.equal(v, m2.model.state_dict()[k]), k
        # the criterion computes the reference's function
        l, t, _ = sb.inputs(3, 3, 'none')
        want = sb.xent_ls(l, t, torch.tensor(w), 1.0, 0.1)
        sb.check('criterion', {'loss': m2.criterion(l, t).reshape(1)}, want)
        # inference ignores it: the same weights, the same forward plan
        m3 = neuston_models.NeustonModel.load_from_checkpoint(path, inference=True)
        for k, v in m.model.state_dict().items():
            assert torch.equal(v, m3.model.state_dict()[k]), k
        # a checkpoint without the key loads as before: the hard loss
        hp = dict(ck['hyper_parameters'])
        del hp['label_smoothing']
        old = str(tmp_path / 'old.ptl')
        torch.save(dict(ck, hyper_parameters=hp), old)
        m4 = neuston_models.NeustonModel.load_from_checkpoint(old)
        assert not hasattr(m4.hparams, 'label_smoothing') and m4.model.engine.label_smoothing == 0.0 and m4.criterion.label_smoothing == 0.0
        plain = neuston_models.NeustonModel(_hparams())
        assert plain.criterion.label_smoothing == 0.0 and plain.criterion.weight is None and 'criterion.weight' not in plain.state_dict()
        plain.load_state_dict(ck['state_dict'])


def test_args_yml_carries_the_flag(tmp_path):
    """do_training dumps vars(args) to args.yml and hands the same namespace to NeustonModel as its hyper-parameters"""
    import yaml
    args = _parse('--label-smoothing', '0.1')
    dumped = yaml.safe_load(yaml.safe_dump({k: (v if isinstance(v, (int, float, str, bool, list, type(None))) else str(v))
                                            for k, v in vars(args).items()}))
    assert dumped['label_smoothing'] == 0.1
    assert yaml.safe_load(yaml.safe_dump(vars(_parse())))['label_smoothing'] == 0.0


def test_onnx_export_ignores_it(tmp_path):
    """neuston_onnx EXPORT reads ckpt['state_dict'] by torchvision key: a --label-smoothing checkpoint has the keys and bytes of any other"""
    from ifcb_classifier_amd import onnx_export
    sds = []
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        for kw in (dict(label_smoothing=0.1), dict()):
            torch.manual_seed(3)
            sds.append(neuston_models.NeustonModel(_hparams(**kw)).checkpoint_dict()['state_dict'])
    assert list(sds[0]) == list(sds[1]) and not [k for k in sds[0] if k.startswith('criterion')]
    a, b = str(tmp_path / 'a.onnx'), str(tmp_path / 'b.onnx')
    onnx_export.export(sds[0], 'resnet18', ['a', 'b', 'c'], False, a)
    onnx_export.export(sds[1], 'resnet18', ['a', 'b', 'c'], False, b)
    assert open(a, 'rb').read() == open(b, 'rb').read()


# ------------------------------------------------------------------------------------------------------ the entry point
def test_the_entry_point_is_bound():
    assert 'ifcbk_softmax_xent_ls' in _lib.EXPORTS
    fn = getattr(_lib.load(), 'ifcbk_softmax_xent_ls')
    assert fn.argtypes is not None and len(fn.argtypes) == 12                       # ctx + the 11 of the header
    root = os.path.dirname(HERE)
    hdr = open(os.path.join(root, 'include', 'ifcbk.h')).read()
    assert 'IFCBK_API int ifcbk_softmax_xent_ls(' in hdr and 'f[1] = label smoothing factor' in hdr
    # the export map passes every ifcbk_* symbol and the library holds this one
    assert 'global: ifcbk_*;' in open(os.path.join(root, 'ifcb_classifier_amd', 'csrc', 'exports.map')).read()
    # no new op kind
    assert _lib.OP_SOFTMAX_XENT_W == 40 and max(_lib.OP_NAMES) == 40
