"""TRAIN --ema from the command line, on the GPU: two epochs on a tiny image dataset with and without the flag.  The training trajectory
(the train-loss column) is the same, validation sees the averaged model, the saved model holds the average the engine kept step by step
(checked against the oracle of tests/ema_bounds.py), not the raw weights, and RUN on it gives the scores of an eval under
Engine.ema_weights()."""
import json
import os
from unittest import mock

import numpy as np
import pytest
import torch

import ema_bounds as eb

pytestmark = pytest.mark.gpu


def _cli(argv):
    from ifcb_classifier_amd import neuston_net as nn_
    args = nn_.argparse_nn().parse_args(argv)
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    return args


def test_train_with_ema_then_run(tmp_path):
    from PIL import Image
    from ifcb_classifier_amd import neuston_net as nn_
    src = str(tmp_path / 'training-data')
    rng = np.random.default_rng(7)
    for cls, mean, n in (('big', 90, 40), ('mid', 130, 8), ('small', 170, 3)):
        os.makedirs(os.path.join(src, cls))
        for i in range(n):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(src, cls, 'roi_%s_%03d.png' % (cls, i)))

    made, steps, saved = [], [], []

    class Spy(nn_.NeustonModel):
        """the model TRAIN builds, recording the engine's P / RB / E / ERB after every step and what stood in the engine at every save"""

        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            made.append(self)

        def fit_current(self, N, *a, **k):
            eng = self.model.engine
            if eng.E is not None and not steps:
                steps.append(dict(P=eng.P.clone(), RB=eng.RB.clone()))          # what the average starts from
            out = super().fit_current(N, *a, **k)
            if eng.E is not None:
                torch.cuda.synchronize()
                steps.append({k2: getattr(eng, k2).clone() for k2 in ('P', 'RB', 'E', 'ERB')})
            return out

        def checkpoint_dict(self, *a, **k):
            eng = self.model.engine
            if eng.E is not None:
                assert eng._ema_view is not None                                   # saved from inside ema_weights()
                saved.append(dict(E=eng.E.clone(), ERB=eng.ERB.clone(), raw=eng._ema_view[0].clone(), nstep=len(steps) - 1))
            return super().checkpoint_dict(*a, **k)

    common = ['--batch', '16', '--loaders', '0', 'TRAIN', src, 'resnet18']
    tail = ['--untrain', '--seed', '1', '--emax', '2', '--emin', '2', '--estop', '0']
    out_plain, out_ema = str(tmp_path / 'training-output' / 'plain'), str(tmp_path / 'training-output' / 'avg')
    _cli(common + ['plain'] + tail + ['--outdir', out_plain])
    with mock.patch.object(nn_, 'NeustonModel', Spy):
        _cli(common + ['avg'] + tail + ['--outdir', out_ema, '--ema', '0.9'])
    rows = [open(os.path.join(d, 'epochs.csv')).read().strip().splitlines() for d in (out_plain, out_ema)]
    assert rows[0][0] == rows[1][0] and rows[0][0].split(',')[:4] == ['epoch', 'best', 'train_loss', 'val_loss'] and len(rows[0]) == len(rows[1]) == 3
    col = lambda r, j: [ln.split(',')[j] for ln in r[1:]]
    assert col(rows[0], 2) == col(rows[1], 2)                                      # the training trajectory is untouched
    assert col(rows[0], 3) != col(rows[1], 3)                                      # validation saw the averaged model
    assert all(np.isfinite(float(v)) for r in rows for v in col(r, 2) + col(r, 3))
    import yaml
    assert yaml.safe_load(open(os.path.join(out_ema, 'args.yml')))['ema'] == 0.9
    assert yaml.safe_load(open(os.path.join(out_plain, 'args.yml')))['ema'] is None
    ck = torch.load(os.path.join(out_ema, 'avg.ptl'), map_location='cpu', weights_only=False)
    assert ck['hyper_parameters']['ema'] == 0.9
    assert torch.load(os.path.join(out_plain, 'plain.ptl'), map_location='cpu', weights_only=False)['hyper_parameters']['ema'] is None

    # the recurrence the engine kept: E_k from E_(k-1) and P_k with the warm-up's weight, ERB likewise
    assert len(made) == 1 and len(steps) >= 5 and saved
    eng = made[0].model.engine
    e_prev, erb_prev = steps[0]['P'], steps[0]['RB']
    for k, s in enumerate(steps[1:], 1):
        w = eb.weight(0.9, k)
        eb.check('cli step %d E' % k, s['E'].cpu(), e_prev.cpu(), s['P'].cpu(), w)
        eb.check('cli step %d ERB' % k, s['ERB'].cpu(), erb_prev.cpu(), s['RB'].cpu(), w)
        e_prev, erb_prev = s['E'], s['ERB']
    assert eng.ema_updates == len(steps) - 1
    # the file holds the average of the best epoch's last step, not the raw weights
    best = saved[-1]
    assert torch.equal(best['E'], steps[best['nstep']]['E']) and torch.equal(best['ERB'], steps[best['nstep']]['ERB'])
    assert torch.equal(best['raw'], steps[best['nstep']]['P']) and not torch.equal(best['E'], best['raw'])
    sd = ck['state_dict']
    nchecked = 0
    for key, (o, n, shape, kind, node) in eng.poff.items():
        t = best['E'][o:o + n].cpu()
        r = best['raw'][o:o + n].cpu()
        view = (lambda x: x.view(shape[0], shape[2], shape[3], shape[1]).permute(0, 3, 1, 2)) if kind == 'conv' else (lambda x: x.view(shape))
        assert torch.equal(sd['model.' + key], view(t)), key
        nchecked += not torch.equal(view(t), view(r))
    assert nchecked > len(eng.poff) // 2
    for key, (o, n) in eng.boff.items():
        assert torch.equal(sd['model.' + key], best['ERB'][o:o + n].cpu()), key
    assert 'optimizer_states' in ck and ck['optimizer_states'][0]['state']           # (those of the raw weights, as without the flag)

    # RUN on the file: the scores of an eval under ema_weights() with that average
    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '16', '--loaders', '0', 'RUN', src, os.path.join(out_ema, 'avg.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'avg', 'img_results.json')))
    scores = np.array(rj['output_scores'], dtype=np.float32)
    assert rj['model_id'] == 'avg' and scores.shape == (51, 3) and np.allclose(scores.sum(1), 1, atol=1e-4)
    from torch.utils.data import DataLoader
    from ifcb_classifier_amd.neuston_data import ImageDataset, collate_rois
    eng.E.copy_(best['E'])
    eng.ERB.copy_(best['ERB'])
    ds = ImageDataset(list(rj['input_images']), resize=made[0].hparams.resize, input_src=src, pad=None)
    loader = DataLoader(ds, batch_size=16, num_workers=0, collate_fn=collate_rois)
    with eng.ema_weights():
        rr, _ = nn_.Trainer(0, 0, 0, run_out).test(made[0], loader, src, ds.transform, [])
    assert list(rr.inputs) == list(rj['input_images'])
    assert np.array_equal(np.asarray(rr.outputs, dtype=np.float32), scores)
    raw_rr, _ = nn_.Trainer(0, 0, 0, run_out).test(made[0], loader, src, ds.transform, [])
    assert not np.array_equal(np.asarray(raw_rr.outputs, dtype=np.float32), scores)


def test_a_decay_outside_the_unit_interval_is_refused_by_argparse(tmp_path):
    with pytest.raises(SystemExit):
        _cli(['TRAIN', str(tmp_path), 'resnet18', 'x', '--untrain', '--ema', '1.5'])
