"""RUN --tta from the command line, on the GPU: two synthetic raw bins through ``RUN --tta all`` and ``RUN --tta flips`` with .json
class files -- the same ids and layout as without the flag, scores that are NeustonModel.eval_current_tta's for the same batches and
are not the plain run's, and one file whether the bin's blob is resident on the device or goes through the per-ROI DataLoader."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
LIDS = ['D20130526T092352_IFCB013', 'D20130526T101500_IFCB013']
BATCH = 8


def _cli(argv):
    from ifcb_classifier_amd import neuston_net as nn_
    args = nn_.argparse_nn().parse_args(argv)
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    return args


def _make_bin(bdir, lid, n, seed):
    rng = np.random.default_rng(seed)
    blob, lines, off = b'', [], 0
    for k in range(n):
        h, w = (int(v) for v in rng.integers(20, 90, 2))
        a = np.clip(rng.normal(96 if k % 2 else 160, 30, (h, w)), 0, 255).astype(np.uint8)
        a[:h // 2, :w // 3] //= 2                                          # no ROI looks like one of its own views
        cols = ['0'] * 24
        cols[15], cols[16], cols[17] = str(w), str(h), str(off)
        lines.append(','.join(cols))
        blob += a.tobytes()
        off += h * w
    (bdir / (lid + '.adc')).write_text('\n'.join(lines) + '\n')
    (bdir / (lid + '.roi')).write_bytes(blob)


def _api_scores(path, root, mode):
    """eval_current_tta on the batches RUN cuts: per bin, ROIs i0..i1-1 of the resident blob"""
    from ifcb_classifier_amd.ifcb_bins import DataDirectory
    from ifcb_classifier_amd.neuston_data import IfcbBinDataset
    from ifcb_classifier_amd.neuston_models import NeustonModel
    m = NeustonModel.load_from_checkpoint(path, max_batch=BATCH, inference=True)
    out = {}
    try:
        for b in DataDirectory(root + os.sep):
            ds = IfcbBinDataset(b, m.hparams.resize, m.hparams.img_norm, pad=None)
            t = b.table
            res = m.upload_bin(b.blob, t['offs'], t['hs'], t['ws'])
            n_total, scores = len(t['targets']), []
            for i0 in range(0, n_total, BATCH):
                n = m.stage_resident(res, i0, min(i0 + BATCH, n_total), ds.transform)
                m.use_staged()
                scores.append(m.eval_current_tta(n, mode).cpu().numpy())
            out[str(b.pid.pid)] = np.concatenate(scores)
    finally:
        torch.cuda.synchronize()
        m.model.engine.close()
    return out


def test_run_tta_writes_the_usual_files_with_the_averaged_scores(tmp_path):
    from ifcb_classifier_amd.neuston_models import NeustonModel
    hp = argparse.Namespace(MODEL='resnet18', classes=['a', 'b', 'c'], pretrained=False, batch_size=BATCH, model_id='tta', resize=224,
                            img_norm=None, seed=3, cmd_timestamp='2021-01-01T00:00:00+00:00')
    torch.manual_seed(5)
    m = NeustonModel(hp)
    path = str(tmp_path / 'tta.ptl')
    torch.save(m.checkpoint_dict(epoch=0, global_step=0), path)
    torch.cuda.synchronize()
    m.model.engine.close()
    root = str(tmp_path / 'run-data')
    bdir = tmp_path / 'run-data' / 'D2013' / 'D20130526'
    bdir.mkdir(parents=True)
    _make_bin(bdir, LIDS[0], 11, 1)
    _make_bin(bdir, LIDS[1], 5, 2)

    def run(tag, extra, resident=True):
        out = str(tmp_path / ('run_' + tag))
        if not resident:
            os.environ['IFCBK_BIN_RESIDENT'] = '0'
        try:
            args = _cli(['--batch', str(BATCH), '--loaders', '0', 'RUN', root, path, tag, '--outdir', out, '--outfile', '{BIN_ID}_class.json'] + extra)
        finally:
            os.environ.pop('IFCBK_BIN_RESIDENT', None)
        assert args.tta == (extra[1] if extra else None)
        return [json.load(open(os.path.join(out, lid + '_class.json'))) for lid in LIDS]

    plain = run('plain', [])
    full = run('all', ['--tta', 'all'])
    loader = run('all_loader', ['--tta', 'all'], resident=False)
    flips = run('flips', ['--tta', 'flips'])
    for p, a, l, f in zip(plain, full, loader, flips):
        for other in (a, l, f):
            assert sorted(other) == sorted(p) and other['bin_id'] == p['bin_id'] and other['roi_numbers'] == p['roi_numbers']
            assert other['class_labels'] == p['class_labels'] and np.array(other['output_scores']).shape == np.array(p['output_scores']).shape
            assert np.allclose(np.sum(other['output_scores'], 1), 1, atol=1e-4)
            assert (np.array(other['output_classes']) == np.argmax(other['output_scores'], 1)).all()
        assert a['output_scores'] == l['output_scores'] and a['output_classes'] == l['output_classes']      # resident blob == DataLoader
        assert a['output_scores'] != p['output_scores'] and f['output_scores'] != p['output_scores'] and a['output_scores'] != f['output_scores']
    assert [len(p['roi_numbers']) for p in plain] == [11, 5]
    for mode, files in (('all', full), ('flips', flips)):
        api = _api_scores(path, root, mode)
        for lid, f in zip(LIDS, files):
            assert np.array_equal(np.array(f['output_scores'], dtype=np.float32), api[lid]), (mode, lid)
