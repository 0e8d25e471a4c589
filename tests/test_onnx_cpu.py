"""ONNX export (``ifcb_classifier_amd.onnx_export``, ``neuston_onnx EXPORT``) on the CPU.

Each exported file is decoded and evaluated by tests/onnx_eval.py, which shares no code with the writer, and compared with the
oracle's eval forward.  torch's own ONNX serializer exports the same oracle modules as an independent reference: its files go
through the same decoder and evaluator, which pins that decoder's field numbers and the structure both files must share."""
import io
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import onnx_eval  # noqa: E402

from oracle.tv_models import get_namebrand_model  # noqa: E402

NC = 5
CLASSES = ['class_%d' % i for i in range(NC)]
FP32_BOUND = 1e-5          # |logit - oracle| / max|oracle logit|
# fp16 weights, input and activations against the fp32 oracle, |logit - oracle| / max|oracle logit|.  Measured on these seeds:
# inception_v3 7.4e-2 (5.6e-2 of it from the fp16 weights alone: random weights with data-calibrated statistics, eps 1e-3), resnet18
# 2.6e-3, densenet121 3.7e-3
HALF_BOUND = {'inception_v3': 1e-1, 'resnet18': 1e-2, 'densenet121': 1e-2}
FAMILIES = [('inception_v3', False), ('inception_v3', True), ('resnet18', False), ('alexnet', False), ('squeezenet', False),
            ('vgg11_bn', False), ('densenet121', False)]


def _oracle(name, pretrained, calibrate=False, seed=0):
    """seeded oracle in eval mode with random BatchNorm affine parameters and running statistics.  calibrate: running
    statistics of a random batch instead (activations stay O(1), which fp16 storage needs)"""
    torch.manual_seed(seed)
    m = get_namebrand_model(name, NC, pretrained)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.2, 0.2)
            mod.running_mean.uniform_(-0.5, 0.5)
            mod.running_var.uniform_(0.5, 2.0)
            if calibrate:
                mod.momentum = None
                mod.reset_running_stats()
    if calibrate:
        with torch.no_grad():
            m.train()(torch.rand(4, 3, _size(name), _size(name)))
    return m.eval()


def _size(name):
    return 299 if name == 'inception_v3' else 224


def _rel(y, ref):
    return float((y - ref).abs().max() / ref.abs().max())


def _torch_export(m, x, **kw):
    """torch's TorchScript exporter; its last step hands the bytes to the onnx package (not installed), bypassed here"""
    from torch.onnx._internal.torchscript_exporter import onnx_proto_utils
    f = io.BytesIO()
    orig = onnx_proto_utils._add_onnxscript_fn
    onnx_proto_utils._add_onnxscript_fn = lambda model_bytes, custom_opsets: model_bytes
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            torch.onnx.export(m, x, f, opset_version=12, input_names=['input'], output_names=['output'], dynamo=False,
                              dynamic_axes={'input': {0: 'batch_size'}, 'output': {0: 'batch_size'}}, **kw)
    finally:
        onnx_proto_utils._add_onnxscript_fn = orig
    return f.getvalue()


@pytest.mark.parametrize('name,pretrained', FAMILIES, ids=['%s%s' % (n, '-transform' if p else '') for n, p in FAMILIES])
def test_export_matches_oracle_and_torch_serializer(tmp_path, name, pretrained):
    from ifcb_classifier_amd import onnx_export
    m = _oracle(name, pretrained)
    S = _size(name)
    x = torch.rand(2, 3, S, S, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        ref = m(x)
    path = str(tmp_path / 'm.onnx')
    onnx_export.export(m.state_dict(), name, CLASSES, pretrained, path)
    mine = onnx_eval.load(path)
    with torch.no_grad():
        y = onnx_eval.evaluate(mine, x)
    assert y.shape == (2, NC)
    assert _rel(y, ref) <= FP32_BOUND, _rel(y, ref)

    # initializers are the state_dict's tensors, bit for bit, under its keys (BatchNorm unfolded); no aux head
    sd = m.state_dict()
    inits = mine['graph']['initializers']
    for k, v in inits.items():
        if k.startswith('transform_input.'):
            assert pretrained and name == 'inception_v3'
            continue
        assert np.array_equal(v, sd[k].numpy()), k
        assert mine['graph']['init_types'][k] == 1
    assert not any(k.startswith('AuxLogits') for k in inits)
    assert ('transform_input.scale' in inits) == pretrained
    ops = [n['op'] for n in mine['graph']['nodes']]
    assert 'Softmax' not in ops and ops.count('BatchNormalization') == sum(k.endswith('running_var') and not k.startswith('AuxLogits')
                                                                            for k in sd)

    # torch's serializer, read by the same decoder and evaluator, reproduces the oracle too
    theirs = onnx_eval.decode_model(_torch_export(m, x[:1]))
    with torch.no_grad():
        yt = onnx_eval.evaluate(theirs, x)
    assert _rel(yt, ref) <= FP32_BOUND, _rel(yt, ref)
    assert mine['ir_version'] == theirs['ir_version'] == 7
    assert mine['opset_import'][''] == theirs['opset_import'][''] == 12
    for a, b in ((mine['graph']['inputs'], theirs['graph']['inputs']), (mine['graph']['outputs'], theirs['graph']['outputs'])):
        assert [(v['name'], v['elem_type'], v['dims']) for v in a] == [(v['name'], v['elem_type'], v['dims']) for v in b]
    assert mine['graph']['inputs'][0]['dims'] == ['batch_size', 3, S, S]
    assert mine['graph']['outputs'][0]['dims'] == ['batch_size', NC]
    assert mine['metadata'] == {'ifcbk.model': name, 'ifcbk.num_classes': str(NC), 'ifcbk.pretrained': str(int(pretrained)),
                                'ifcbk.resize': str(S), 'ifcbk.version': onnx_export.FORMAT_VERSION}


@pytest.mark.parametrize('name', ['inception_v3', 'resnet18', 'densenet121'])
def test_half_export_within_bound(tmp_path, name):
    from ifcb_classifier_amd import onnx_export
    import conftest
    m = _oracle(name, False, calibrate=True)
    S = _size(name)
    x = torch.rand(2, 3, S, S, generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        ref = m(x)
    path = str(tmp_path / 'h.onnx')
    onnx_export.export(m.state_dict(), name, CLASSES, False, path, half=True)
    md = onnx_eval.load(path)
    g = md['graph']
    assert g['inputs'][0]['elem_type'] == g['outputs'][0]['elem_type'] == 10
    assert set(g['init_types'].values()) == {10}
    sd = m.state_dict()
    for k, v in g['initializers'].items():
        assert np.array_equal(v, sd[k].half().numpy()), k
    # the file is exactly the fp16-rounded model: fp32 arithmetic on it reproduces the oracle holding the same rounded tensors
    m16 = _oracle(name, False)
    m16.load_state_dict({k: (v.half().float() if v.is_floating_point() else v) for k, v in sd.items()})
    with torch.no_grad():
        ref16 = m16(x.half().float())
        y = onnx_eval.evaluate(md, x, half_storage=False)
    assert _rel(y, ref16) <= FP32_BOUND, _rel(y, ref16)
    # against fp32, with every activation stored as fp16 too, as an fp16 runtime would
    with torch.no_grad():
        y = onnx_eval.evaluate(md, x)
    err = _rel(y, ref)
    conftest.MEASURED.append('onnx --half %s: max|logit - fp32 oracle| / max|logit| = %.2e (bound %.0e)' % (name, err, HALF_BOUND[name]))
    assert err <= HALF_BOUND[name], err


def _fake_ptl(tmp_path, name='squeezenet', pretrained=False):
    """a checkpoint in the layout TRAIN writes (state_dict under 'model.', hyper_parameters MODEL / classes / pretrained)"""
    m = _oracle(name, pretrained)
    ck = dict(state_dict={'model.' + k: v for k, v in m.state_dict().items()},
              hyper_parameters=dict(MODEL=name, classes=CLASSES, pretrained=pretrained, seed=1))
    path = str(tmp_path / 'trained.ptl')
    torch.save(ck, path)
    return path, m


def test_cli_export_names_and_options(tmp_path, capsys):
    from ifcb_classifier_amd import neuston_onnx, onnx_export
    ptl, m = _fake_ptl(tmp_path)
    neuston_onnx.main(['EXPORT', ptl])
    out = capsys.readouterr().out
    onnx_path, cls_path = str(tmp_path / 'trained.onnx'), str(tmp_path / 'trained.classes')
    assert 'EXPORTED: %s' % onnx_path in out and 'EXPORTED: %s' % cls_path in out
    assert open(cls_path).read() == '\n'.join(CLASSES)                    # no trailing newline, as upstream
    md = onnx_eval.load(onnx_path)
    assert md['graph']['inputs'][0]['dims'] == ['batch_size', 3, 224, 224] and md['opset_import'][''] == 12
    x = torch.rand(3, 3, 224, 224, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert _rel(onnx_eval.evaluate(md, x), m(x)) <= FP32_BOUND
    # the package's own reader (RUN) sees the same tensors and metadata
    rd = onnx_export.read(onnx_path)
    assert rd['metadata']['ifcbk.model'] == 'squeezenet' and rd['opset'] == 12 and rd['ir_version'] == 7
    assert rd['inputs'][0]['dims'] == ['batch_size', 3, 224, 224] and rd['outputs'][0]['dims'] == ['batch_size', NC]
    assert sorted(rd['initializers']) == sorted(md['graph']['initializers'])
    for k, v in rd['initializers'].items():
        assert np.array_equal(v, md['graph']['initializers'][k]), k

    neuston_onnx.main(['EXPORT', ptl, '--half', '--device', 'cuda'])
    assert os.path.isfile(str(tmp_path / 'trained.FP16.onnx')) and os.path.isfile(str(tmp_path / 'trained.FP16.classes'))
    assert onnx_eval.load(str(tmp_path / 'trained.FP16.onnx'))['graph']['inputs'][0]['elem_type'] == 10

    out_path = str(tmp_path / 'deploy' / 'sub' / 'fixed.onnx')
    neuston_onnx.main(['EXPORT', ptl, '--batchsize', '8', '--opset', '13', '--output', out_path])
    md = onnx_eval.load(out_path)
    assert md['graph']['inputs'][0]['dims'] == [8, 3, 224, 224] and md['graph']['outputs'][0]['dims'] == [8, NC]
    assert md['opset_import'][''] == 13
    assert open(str(tmp_path / 'deploy' / 'sub' / 'fixed.classes')).read() == '\n'.join(CLASSES)
    with torch.no_grad():
        assert _rel(onnx_eval.evaluate(md, x), m(x)) <= FP32_BOUND


def test_export_is_deterministic_and_refuses_oversize(tmp_path, monkeypatch):
    from ifcb_classifier_amd import onnx_export
    m = _oracle('resnet18', False)
    a, b = str(tmp_path / 'a.onnx'), str(tmp_path / 'b.onnx')
    onnx_export.export(m.state_dict(), 'resnet18', CLASSES, False, a)
    onnx_export.export({'model.' + k: v for k, v in m.state_dict().items()}, 'resnet18', CLASSES, False, b)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    with pytest.raises(ValueError, match='opset'):
        onnx_export.export(m.state_dict(), 'resnet18', CLASSES, False, a, opset=9)
    monkeypatch.setattr(onnx_export, 'MAX_BYTES', 1 << 20)
    c = str(tmp_path / 'c.onnx')
    with pytest.raises(ValueError, match='2 GB'):
        onnx_export.export(m.state_dict(), 'resnet18', CLASSES, False, c)
    assert not os.path.exists(c)


def test_run_foreign_file_needs_onnxruntime(tmp_path, monkeypatch):
    """a file without the package's ifcbk.* metadata goes to onnxruntime, as upstream; without it RUN exits non-zero naming it"""
    from PIL import Image
    from ifcb_classifier_amd import neuston_onnx
    m = _oracle('squeezenet', False)
    foreign = str(tmp_path / 'foreign.onnx')
    with open(foreign, 'wb') as f:
        f.write(_torch_export(m, torch.rand(1, 3, 224, 224)))
    img = str(tmp_path / 'roi.png')
    Image.fromarray(np.full((40, 30), 128, np.uint8), 'L').save(img)
    monkeypatch.setitem(sys.modules, 'onnxruntime', None)                 # import onnxruntime -> ImportError
    with pytest.raises(SystemExit) as e:
        neuston_onnx.main(['RUN', foreign, img])
    assert 'onnxruntime' in str(e.value.code) and e.value.code not in (0, None)


def test_run_collects_images_as_upstream(tmp_path):
    from ifcb_classifier_amd.neuston_onnx import collect_images
    (tmp_path / 'a' / 'b').mkdir(parents=True)
    for p in ('a/x.png', 'a/b/y.jpg', 'a/b/notes.csv'):
        (tmp_path / p).write_bytes(b'')
    assert sorted(collect_images(str(tmp_path / 'a'))) == sorted([str(tmp_path / 'a/x.png'), str(tmp_path / 'a/b/y.jpg')])
    lst = tmp_path / 'imgs.list'
    lst.write_text('%s\n %s \n%s\n' % (tmp_path / 'a/x.png', tmp_path / 'a/b/y.jpg', tmp_path / 'a/b/notes.csv'))
    assert collect_images(str(lst)) == [str(tmp_path / 'a/x.png'), str(tmp_path / 'a/b/y.jpg')]
    assert collect_images(str(tmp_path / 'a/x.png')) == [str(tmp_path / 'a/x.png')]
