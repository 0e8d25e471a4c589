"""``TRAIN --onnx`` and ``neuston_onnx RUN`` on the GPU: the exported file holds the weights fit left in memory, evaluates on
the CPU (tests/onnx_eval.py) to the GPU's fp32 eval logits, and RUN of it on the GPU reproduces a NeustonModel bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import onnx_eval  # noqa: E402

pytestmark = pytest.mark.gpu

FP32_PARITY = 1e-3          # the project's fp32 parity bound, relative to max|logit|


def _make_dataset(root, per_class=6):
    from PIL import Image
    rng = np.random.default_rng(7)
    for cls, mean in (('cls_a', 90), ('cls_b', 170)):
        os.makedirs(os.path.join(root, cls))
        for i in range(per_class):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(root, cls, 'roi_%s_%02d.png' % (cls, i)))


def _train(tmp_path, model, monkeypatch):
    """neuston_net TRAIN ... --onnx through the CLI; returns (data dir, outdir, the NeustonModel as fit returned it)"""
    from ifcb_classifier_amd import neuston_net as nn_
    src = str(tmp_path / 'data')
    os.makedirs(src)
    _make_dataset(src)
    outdir = str(tmp_path / 'out')
    seen = []
    fit = nn_.Trainer.fit
    monkeypatch.setattr(nn_.Trainer, 'fit', lambda self, m, *a: (seen.append(m), fit(self, m, *a))[1])
    args = nn_.argparse_nn().parse_args(['--batch', '8', '--loaders', '0', '--precision', 'fp32', 'TRAIN', src, model, 'ox',
                                         '--untrain', '--seed', '1', '--emax', '1', '--emin', '1', '--estop', '0',
                                         '--outdir', outdir, '--onnx'])
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    return src, outdir, seen[0]


@pytest.mark.parametrize('model', ['inception_v3', 'vgg11_bn'])
def test_train_onnx_matches_gpu_and_run_round_trips(tmp_path, capsys, monkeypatch, model):
    from ifcb_classifier_amd import neuston_onnx
    from ifcb_classifier_amd.neuston_data import ImageDataset, collate_rois
    from ifcb_classifier_amd.neuston_models import NeustonModel
    src, outdir, trained = _train(tmp_path, model, monkeypatch)
    onnx_path = os.path.join(outdir, 'ox.onnx')
    out = capsys.readouterr().out
    assert 'EXPORTED: %s' % onnx_path in out and 'EXPORTED: %s.classes' % onnx_path in out
    assert open(onnx_path + '.classes').read() == 'cls_a\ncls_b'
    S = 299 if model == 'inception_v3' else 224

    # the file holds the in-memory weights fit returned (torchvision layout: vgg11_bn's running_mean includes the conv bias)
    md = onnx_eval.load(onnx_path)
    sd = {k: v.detach().cpu() for k, v in trained.model.state_dict().items()}
    inits = md['graph']['initializers']
    assert md['graph']['inputs'][0]['dims'] == ['batch_size', 3, S, S] and md['graph']['outputs'][0]['dims'] == ['batch_size', 2]
    assert not any(k.startswith('AuxLogits') for k in inits)
    assert sorted(inits) == sorted(k for k in sd if not k.startswith('AuxLogits') and not k.endswith('num_batches_tracked'))
    for k, v in inits.items():
        assert np.array_equal(v, sd[k].numpy()), k

    # CPU evaluation of the file == the GPU's fp32 eval logits of the same weights
    x = torch.rand(3, 3, S, S, generator=torch.Generator().manual_seed(4))
    trained.model.eval()
    with torch.no_grad():
        gpu = trained.model(x.to(trained.model.engine.dev)).float().cpu()
        cpu = onnx_eval.evaluate(md, x)
    err = float((cpu - gpu).abs().max() / gpu.abs().max())
    import conftest
    conftest.MEASURED.append('TRAIN --onnx %s: CPU eval of the file vs GPU fp32 eval, max|d logit| / max|logit| = %.2e (bound %.0e)'
                             % (model, err, FP32_PARITY))
    assert err <= FP32_PARITY, err

    # RUN of the file on the GPU == a NeustonModel holding the same weights (the .ptl: one epoch, so the best is the last)
    ck = torch.load(os.path.join(outdir, 'ox.ptl'), map_location='cpu', weights_only=False)
    assert ck['hyper_parameters']['precision'] == 'fp32'
    for k, v in inits.items():
        assert np.array_equal(v, ck['state_dict']['model.' + k].numpy()), k
    capsys.readouterr()
    res = neuston_onnx.main(['RUN', onnx_path, src, '--precision', 'fp32', '-c', onnx_path + '.classes'])
    out = capsys.readouterr().out.splitlines()
    assert len(res['images']) == 12 and res['logits'].shape == (12, 2)
    ref_model = NeustonModel.load_from_checkpoint(os.path.join(outdir, 'ox.ptl'), max_batch=neuston_onnx.RUN_BATCH, inference=True)
    ds = ImageDataset(res['images'], resize=S)
    ref_logits = []
    for i in range(0, len(ds), neuston_onnx.RUN_BATCH):
        rois, _ = collate_rois([ds[j] for j in range(i, min(i + neuston_onnx.RUN_BATCH, len(ds)))])
        n = ref_model.stage_batch(rois, ds.transform)
        ref_model.use_staged()
        ref_model.eval_current(n)
        ref_logits.append(ref_model.model._train_heads[0].logits[:n].float().cpu().numpy())
    ref_logits = np.concatenate(ref_logits)
    assert np.array_equal(res['logits'], ref_logits)
    labels = [['cls_a', 'cls_b'][i] for i in ref_logits.argmax(1)]
    assert res['labels'] == labels and out[-1] == str(labels) and out[-2] == onnx_path + '.classes'
