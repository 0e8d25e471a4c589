"""TRAIN --distill from the command line, on the GPU: a resnet18 teacher, a student distilled from it (the four entries in the model
file and args.yml), RUN of the student with the teacher file deleted, a teacher with another class list, and the same command line
without --distill, which leaves no trace of the option."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
KEYS = ('distill', 'distill_alpha', 'distill_temperature', 'distill_teacher_id')


def _cli(argv):
    from ifcb_classifier_amd import neuston_net as nn_
    args = nn_.argparse_nn().parse_args(argv)
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    return args


def test_train_a_student_from_a_teacher_then_run_it_alone(tmp_path, capsys):
    from PIL import Image
    import yaml
    src = str(tmp_path / 'training-data')
    rng = np.random.default_rng(7)
    for cls, mean, n in (('big', 90, 40), ('mid', 130, 3), ('small', 170, 8)):
        os.makedirs(os.path.join(src, cls))
        for i in range(n):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(src, cls, 'roi_%s_%03d.png' % (cls, i)))

    def train(run, *extra):
        outdir = str(tmp_path / 'training-output' / run)
        _cli(['--batch', '8', '--loaders', '0', '--precision', 'fp32', 'TRAIN', src, 'resnet18', run, '--untrain', '--seed', '1', '--emax', '1',
              '--emin', '1', '--estop', '0', '--outdir', outdir] + list(extra))
        return outdir
    tdir = train('teacher')
    teacher = os.path.join(tdir, 'teacher.ptl')
    student_args = ('--label-smoothing', '0.1', '--flip', 'xy')
    sdir = train('student', '--distill', teacher, '--distill-alpha', '0.7', *student_args)
    assert 'Distilling from' in capsys.readouterr().out
    for f in ('student.ptl', 'epochs.csv', 'args.yml'):
        assert os.path.isfile(os.path.join(sdir, f)), f
    hp = torch.load(os.path.join(sdir, 'student.ptl'), map_location='cpu', weights_only=False)['hyper_parameters']
    assert tuple(hp[k] for k in KEYS) == (teacher, 0.7, 4.0, 'teacher')
    y = yaml.safe_load(open(os.path.join(sdir, 'args.yml')))
    assert tuple(y[k] for k in KEYS) == (teacher, 0.7, 4.0, 'teacher') and y['label_smoothing'] == 0.1
    rows = open(os.path.join(sdir, 'epochs.csv')).read().strip().splitlines()
    assert len(rows) == 2 and all(np.isfinite(float(v)) for v in rows[1].split(',')[2:4])
    # a teacher whose class list differs: TRAIN stops before the first step and names the class
    bdir = train('teacher2', '--class-min', '5')                  # drops 'mid'
    with pytest.raises(SystemExit) as ei:
        train('student2', '--distill', os.path.join(bdir, 'teacher2.ptl'), *student_args)
    assert ei.value.code not in (0, None) and "class 1: 'small' (teacher) != 'mid'" in str(ei.value.code)
    assert not os.path.exists(os.path.join(str(tmp_path / 'training-output' / 'student2'), 'chkpts'))
    # RUN needs the student alone
    os.remove(teacher)
    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '8', '--loaders', '0', 'RUN', src, os.path.join(sdir, 'student.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'student', 'img_results.json')))
    scores = np.array(rj['output_scores'])
    assert rj['model_id'] == 'student' and rj['class_labels'] == ['big', 'mid', 'small'] and scores.shape == (51, 3)
    assert np.allclose(scores.sum(1), 1, atol=1e-4) and (np.array(rj['output_classes']) == scores.argmax(1)).all()
    # the same command line without --distill: nothing of the option in the model file or args.yml
    pdir = train('plain', *student_args)
    hp = torch.load(os.path.join(pdir, 'plain.ptl'), map_location='cpu', weights_only=False)['hyper_parameters']
    y = yaml.safe_load(open(os.path.join(pdir, 'args.yml')))
    assert not [k for k in hp if k.startswith('distill')] and not [k for k in y if k.startswith('distill')]
