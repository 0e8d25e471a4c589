"""TRAIN --class-norm / --weight-decay on the host: the weight formula, the two flags, the op tables Engine(plan_only=True) builds with
and without them, and the .ptl round trip of the hyper-parameters and the optimizer group.  The kernel behind the weighted loss
(ifcbk_softmax_xent_w, csrc/loss.hip) runs in tests/test_gpu_class_norm.py."""
import argparse
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_plan_fingerprints as mpf  # noqa: E402

from ifcb_classifier_amd import _lib, graph, neuston_models, neuston_net  # noqa: E402
from ifcb_classifier_amd.engine import Engine  # noqa: E402


# ------------------------------------------------------------------------------------------------------ the weight formula
COUNTS = [4000, 37, 512, 3, 90000, 1]


def test_power_1_is_the_balanced_weighting():
    w = neuston_net.class_norm_weights(COUNTS, 1.0)
    n = np.asarray(COUNTS, dtype=np.float64)
    want = (n.sum() / (len(n) * n)).astype(np.float32)
    assert [np.float32(v) for v in w] == list(want)
    assert all(isinstance(v, float) and float(np.float32(v)) == v for v in w)           # python floats holding float32 values


def test_power_0_is_all_ones_exactly():
    assert neuston_net.class_norm_weights(COUNTS, 0.0) == [1.0] * len(COUNTS)


@pytest.mark.parametrize('power', [0.0, 0.25, 0.5, 1.0, 2.0])
def test_mean_weight_over_training_samples_is_one(power):
    w = np.asarray(neuston_net.class_norm_weights(COUNTS, power), dtype=np.float64)
    n = np.asarray(COUNTS, dtype=np.float64)
    assert abs((n * w).sum() / n.sum() - 1.0) < 1e-6
    assert list(np.argsort(-w, kind='stable')) == list(np.argsort(n, kind='stable')) or power == 0        # smaller class, larger weight


def test_weights_follow_the_order_of_the_classes_and_empty_classes_get_zero():
    a = neuston_net.class_norm_weights([10, 1000, 100], 1.0)
    b = neuston_net.class_norm_weights([1000, 100, 10], 1.0)
    assert a == [b[2], b[0], b[1]] and a[0] > a[2] > a[1]
    z = neuston_net.class_norm_weights([10, 0, 30], 1.0)
    assert z[1] == 0.0 and abs(10 * z[0] + 30 * z[2] - 40) < 1e-4
    with pytest.raises(ValueError):
        neuston_net.class_norm_weights([10, 20], -1.0)


# ------------------------------------------------------------------------------------------------------ argparse
def _parse(*extra):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'inception_v3', 'id'] + list(extra))


def test_flags():
    a = _parse()
    assert a.class_norm is None and a.weight_decay == 0.0
    assert _parse('--class-norm').class_norm == 1.0
    assert _parse('--class-norm', '0.5').class_norm == 0.5
    assert _parse('--class-norm', '0').class_norm == 0.0
    assert _parse('--weight-decay', '1e-4').weight_decay == 1e-4
    with pytest.raises(SystemExit):
        _parse('--class-norm', '-1')
    with pytest.raises(SystemExit):
        _parse('--class-norm=-0.5')


# ------------------------------------------------------------------------------------------------------ plans
def _plan(model, B, dtype='bf16', env=None, **kw):
    """Engine(plan_only=True) and its plan, built the way tests/golden/make_plan_fingerprints.py builds them"""
    keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
    with mock.patch.dict(os.environ, dict(keep, **(env or {})), clear=True), mock.patch.object(torch, 'zeros', torch.empty), \
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


def test_weighted_loss_programs_of_inception_v3():
    eng, pl = _plan('inception_v3', 2, class_weights=W7)
    assert eng.class_weight.dtype == torch.float32 and eng.class_weight.tolist() == [float(np.float32(v)) for v in W7]
    cw = eng.class_weight.data_ptr()
    loss = [pl.loss.arr[k] for k in range(pl.loss.n)]
    assert [o.kind for o in loss] == [_lib.OP_SOFTMAX_XENT_W] * 2
    assert [o.f[0] for o in loss] == [1.0, float(np.float32(0.4))]
    assert [o.flags & 1 for o in loss] == [0, 1]
    assert [o.p[4] for o in loss] == [cw, cw]
    assert loss[0].p[2] == loss[1].p[2] == eng.loss.data_ptr() and loss[0].p[3] != loss[1].p[3] and loss[1].p[3]
    assert [int(o.i[0]) for o in loss] == [2, 2] and [int(o.i[1]) for o in loss] == [7, 7]
    ev = [pl.eval_loss.arr[k] for k in range(pl.eval_loss.n)]
    assert [o.kind for o in ev] == [_lib.OP_SOFTMAX_XENT_W] and ev[0].p[4] == cw and not ev[0].p[3] and ev[0].f[0] == 1.0
    assert _lib.OP_NAMES[_lib.OP_SOFTMAX_XENT_W] == 'softmax_xent_w'
    # nothing else of the plan moved: every other op equals the default engine's, and the loss ops differ in kind and p[4] only
    eng0, pl0 = _plan('inception_v3', 2)
    a, b = _ops(eng, pl), _ops(eng0, pl0)
    assert len(a) == len(b)
    n_loss = 0
    for x, y in zip(a, b):
        if y[2] == _lib.OP_SOFTMAX_XENT:
            n_loss += 1
            assert x[2] == _lib.OP_SOFTMAX_XENT_W and x[8][4] == 'class_weight+0' and y[8][4] is None
            assert x[:2] + x[3:8] + x[8][:4] + x[8][5:] == y[:2] + y[3:8] + y[8][:4] + y[8][5:]
        else:
            assert x == y
    assert n_loss == 2 + 1 + 2 + 2 + 2                       # loss, eval_loss, step, fwd_loss, fwd_bwd
    # the weight tensor is an input only: the loss ops are full barriers on lane 0 and no op names it as an output operand
    for x in a:
        if x[2] != _lib.OP_SOFTMAX_XENT_W:
            assert 'class_weight+0' not in x[8]
        else:
            assert (x[3] >> 8) & 7 == 0


@pytest.mark.parametrize('model,B', [('inception_v3', 2), ('resnet50', 4)])
def test_without_weights_the_plan_is_the_default_plan(model, B):
    eng0, pl0 = _plan(model, B)
    eng1, pl1 = _plan(model, B, class_weights=None, weight_decay=0.0)
    assert eng1.class_weight is None
    assert mpf.plan_text(eng1, pl1) == mpf.plan_text(eng0, pl0)
    assert not [x for x in _ops(eng1, pl1) if x[2] == _lib.OP_SOFTMAX_XENT_W]


@pytest.mark.parametrize('optimizer,env', [('adam', {}), ('sgd', {}), ('adam', {'IFCBK_OPT_BUCKETS': '1'}), ('adam', {'IFCBK_LANES': '2'})])
def test_weight_decay_reaches_every_optimizer_op_and_nothing_else(optimizer, env):
    kw = dict(optimizer=optimizer, momentum=0.9 if optimizer == 'sgd' else 0.0)
    eng0, pl0 = _plan('inception_v3', 2, env=env, **kw)
    eng1, pl1 = _plan('inception_v3', 2, env=env, weight_decay=1e-4, **kw)
    kind, slot = (_lib.OP_SGD, 2) if optimizer == 'sgd' else (_lib.OP_ADAM, 4)
    wd = float(np.float32(1e-4))
    a, b = _ops(eng1, pl1), _ops(eng0, pl0)
    assert len(a) == len(b)
    seen = {}
    for x, y in zip(a, b):
        if y[2] == kind:
            seen[x[0]] = seen.get(x[0], 0) + 1
            assert y[6][slot] == 0.0 and x[6][slot] == wd
            assert x[:6] + (x[6][:slot] + x[6][slot + 1:],) + x[7:] == y[:6] + (y[6][:slot] + y[6][slot + 1:],) + y[7:]
        else:
            assert x == y
    assert seen['adam'] == 1 and seen['adam_pack'] == 1                     # (train_step_ddp runs adam_pack)
    assert seen['step'] == (1 if env.get('IFCBK_OPT_BUCKETS') == '1' else len(pl1.step_adam_idxs)) and seen['step'] >= 1
    if not env:
        assert seen['step'] > 1                                             # the bucketed launches carry it too
    with pytest.raises(ValueError):
        _plan('resnet18', 2, weight_decay=-1.0)
    with pytest.raises(ValueError):
        _plan('resnet18', 2, class_weights=[1.0, 2.0])                      # 7 classes


# ------------------------------------------------------------------------------------------------------ .ptl round trip on the host
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
    w = neuston_net.class_norm_weights([40, 8, 3], 1.0)
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(_hparams(class_norm=1.0, class_weights=w, weight_decay=1e-4))
        assert m.model.engine.weight_decay == 1e-4 and m.model.engine.class_weight.tolist() == w
        assert m.criterion.weight.tolist() == w
        opt = m.configure_optimizers()
        assert opt.param_groups[0]['weight_decay'] == 1e-4
        ck = m.checkpoint_dict(epoch=1, global_step=2)
        hp = ck['hyper_parameters']
        assert hp['class_norm'] == 1.0 and hp['class_weights'] == w and hp['weight_decay'] == 1e-4
        assert ck['optimizer_states'][0]['param_groups'][0]['weight_decay'] == 1e-4
        assert ck['state_dict']['criterion.weight'].tolist() == w
        path = str(tmp_path / 'm.ptl')
        torch.save(ck, path)
        m2 = neuston_models.NeustonModel.load_from_checkpoint(path)
        assert m2.hparams.class_norm == 1.0 and m2.hparams.class_weights == w and m2.hparams.weight_decay == 1e-4
        assert m2.model.engine.class_weight.tolist() == w and m2.model.engine.weight_decay == 1e-4
        assert m2.checkpoint_dict()['optimizer_states'][0]['param_groups'][0]['weight_decay'] == 1e-4
        for k, v in m.model.state_dict().items():
            assert torch.equal(v, m2.model.state_dict()[k]), k
        # a checkpoint with the criterion.weight key loads into a model built without weights, and one without it into a model with
        plain = neuston_models.NeustonModel(_hparams())
        assert 'criterion.weight' not in plain.state_dict() and plain.model.engine.class_weight is None
        assert plain.checkpoint_dict()['optimizer_states'][0]['param_groups'][0]['weight_decay'] == 0
        plain.load_state_dict(ck['state_dict'])
        m2.load_state_dict(plain.state_dict())
        assert m2.criterion.weight.tolist() == w
        # SGD carries the decay too
        s = neuston_models.NeustonModel(_hparams(optimizer='SGD', momentum=0.9, weight_decay=1e-3))
        assert s.checkpoint_dict()['optimizer_states'][0]['param_groups'][0]['weight_decay'] == 1e-3
        assert s.configure_optimizers().param_groups[0]['weight_decay'] == 1e-3


def test_onnx_export_ignores_the_criterion_weight(tmp_path):
    """neuston_onnx EXPORT reads ckpt['state_dict'] by torchvision key: the extra buffer of a --class-norm checkpoint changes nothing"""
    from ifcb_classifier_amd import onnx_export
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(_hparams(class_norm=1.0, class_weights=[0.5, 1.0, 4.0]))
    sd = m.checkpoint_dict()['state_dict']
    assert 'criterion.weight' in sd
    a, b = str(tmp_path / 'a.onnx'), str(tmp_path / 'b.onnx')
    onnx_export.export(sd, 'resnet18', ['a', 'b', 'c'], False, a)
    onnx_export.export({k: v for k, v in sd.items() if k != 'criterion.weight'}, 'resnet18', ['a', 'b', 'c'], False, b)
    assert open(a, 'rb').read() == open(b, 'rb').read()


def test_the_entry_point_is_bound():
    assert 'ifcbk_softmax_xent_w' in _lib.EXPORTS
    assert getattr(_lib.load(), 'ifcbk_softmax_xent_w').argtypes is not None
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'ifcbk.h')).read()
    assert 'IFCBK_OP_SOFTMAX_XENT_W' in hdr.split('IFCBK_OP_CONV_WGRAD_GROUP')[1]          # appended: no existing kind is renumbered
