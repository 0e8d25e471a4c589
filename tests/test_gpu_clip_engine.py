"""Engine(clip_grad=...) on the device: a bound nothing reaches leaves every way a step is launched with the bits of an engine without
the flag; a bound below the norm is torch.nn.utils.clip_grad_norm_'s clip (the norm over the parameter tensors, padding excluded, within
the bound derived in tests/clip_cases.py; the update bit-equal to a plain update of the gradient times the device's coefficient); the
epoch figures count; two data-parallel replicas clip the averaged gradient by the same bits; and TRAIN --clip-grad from the command line.

Shapes: resnet18, 7 classes, batch 4, fp32 (the smallest at which the plan has its full op lists), and one inception_v3 step at batch 2
from grey ROIs, for the aux head and the u8 stem; squeezenet at batch 2 for the one kind of channel padding inside the flat buffer."""
import json
import math
import os

import numpy as np
import pytest
import torch

import clip_cases as cc
from option_matrix import bits as _bits, real_mask as _real_mask, reset as _reset, same      # noqa: F401  (moved there, unchanged)

pytestmark = pytest.mark.gpu

B, S, NC = 4, 224, 7
KEYS = ('P', 'M', 'V', 'RB', 'nbt', 'loss')


def _engine(name, b, **kw):
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    eng = Engine(graph.build(name, NC, pretrained=False), device=0, max_batch=b, **kw)
    _reset(eng)
    return eng


def _snap(eng):
    torch.cuda.synchronize()
    return {k: getattr(eng, k).clone() for k in KEYS}


class Rig:
    pass


@pytest.fixture(scope='module')
def rig():
    r = Rig()
    g = torch.Generator().manual_seed(9)
    r.xs = [torch.rand(B, 3, S, S, generator=g).cuda() for _ in range(3)]
    r.ys = [torch.randint(0, NC, (B,), generator=g) for _ in range(3)]
    r.base = _engine('resnet18', B, dtype='fp32')
    r.loose = _engine('resnet18', B, dtype='fp32', clip_grad=1e30)
    assert r.base.clip_state is None and len(r.base.plan(B).step_adam_idxs) > 1 and len(r.loose.plan(B).step_adam_idxs) == 1
    yield r
    r.base.close()
    r.loose.close()


def _load(r, eng, k):
    eng.load_input_nchw(r.xs[k])
    eng.target[:B].copy_(r.ys[k])


def _fwd_bwd(r, eng, k):
    _load(r, eng, k)
    pl = eng.forward_train(B)
    eng.run(pl.loss)
    eng.backward(B)


def _step(r, eng, k, mode):
    if mode == 'plain':
        _load(r, eng, k)
        eng.train_step(B)
    elif mode == 'graph':
        _load(r, eng, k)
        eng.graph_train = True
        try:
            pl = eng.train_step(B)
            assert 'fwd_bwd' in pl.graphs
        finally:
            eng.graph_train = False
    elif mode == 'ev':
        _load(r, eng, k)
        eng.train_step(B, ev_slot=0)
    elif mode == 'split':
        _fwd_bwd(r, eng, k)
        eng.adam_step(B)
    else:
        raise KeyError(mode)
    return _snap(eng)


_BASE = {}


def _base_steps(r):
    """three plain steps of the engine without the flag (every launch mode of it leaves these bits: tests/test_gpu_step_modes.py)"""
    if 'steps' not in _BASE:
        _reset(r.base)
        _BASE['steps'] = [_step(r, r.base, k, 'plain') for k in range(3)]
    return _BASE['steps']


@pytest.mark.parametrize('mode', ('plain', 'graph', 'ev', 'split'))
def test_a_bound_nothing_reaches_leaves_the_steps_bits_alone(rig, mode):
    want = _base_steps(rig)
    _reset(rig.loose)
    for k in range(3):
        got = _step(rig, rig.loose, k, mode)
        for key in KEYS:
            assert same(got[key], want[k][key]), (mode, k, key)
    norm, coef, top, clipped = rig.loose.grad_clip_stats()
    assert coef == 1.0 and clipped == 0 and 0.0 < norm <= top < math.inf


def _check_padding_is_zero(eng):
    torch.cuda.synchronize()
    pad = eng.G.cpu()[~_real_mask(eng)]
    assert pad.numel() == eng.nparam_padded - sum(n for (_o, n, _s, _k, _nd) in eng.poff.values())
    assert bool((pad == 0).all()), 'a pad element of G is not zero after a backward: the norm over the flat buffer would count it'
    return pad.numel()


def _tight_case(base, clipped_of, run_fwd_bwd, batch):
    """one forward + backward on the plain engine `base`; torch's clip of its gradient at half the norm; the same step on an engine built
    by clipped_of(max_norm) -> (that engine, torch's total norm)"""
    _reset(base)
    run_fwd_bwd(base)
    _check_padding_is_zero(base)
    total64, _ = cc.torch_clip([base.gviews[k] for k in base.gviews], 1.0, dtype=torch.float64)
    total32, _ = cc.torch_clip([base.gviews[k] for k in base.gviews], 1.0)
    assert 0 < total64 < math.inf and abs(total32 - total64) < 1e-4 * total64
    mx = float(np.float32(total64 / 2))
    eng = clipped_of(mx)
    _reset(eng)
    run_fwd_bwd(eng)
    torch.cuda.synchronize()
    assert same(eng.G, base.G)
    eng.adam_step(batch)
    norm, coef, top, nclipped = eng.grad_clip_stats()
    blocks = cc.geometry(eng.ctx.lib)[0]
    bound = cc.norm_bound(eng.nparam_padded, blocks, total64)
    print('norm %.9g torch %.9g (fp32 torch %.9g) err %.3g bound %.3g' % (norm, total64, total32, abs(norm - total64), bound))
    assert abs(norm - total64) <= bound
    assert cc.f32_bits(coef) == cc.f32_bits(cc.host_coef(np.float32(norm), mx)) and 0.49 < coef < 0.51
    assert top == norm and nclipped == 1
    # the twin: the plain engine's G times the device's coefficient, then its plain update
    base.G.mul_(torch.tensor(coef, dtype=torch.float32, device=base.G.device))
    base.adam_step(batch)
    torch.cuda.synchronize()
    for key in ('P', 'M', 'V'):
        assert same(getattr(eng, key), getattr(base, key)), key
    return eng, total64


def test_a_bound_below_the_norm_is_torchs_clip(rig):
    made = []

    def clipped_of(mx):
        made.append(_engine('resnet18', B, dtype='fp32', clip_grad=mx))
        return made[0]

    try:
        eng, total = _tight_case(rig.base, clipped_of, lambda e: _fwd_bwd(rig, e, 0), B)
        # reset zeroes the epoch figures and leaves the last step's
        eng.reset_grad_clip_stats()
        n2, c2, top2, k2 = eng.grad_clip_stats()
        assert (top2, k2) == (0.0, 0) and n2 > 0 and c2 < 1.0
        seen = []
        for k in range(3):
            _step(rig, eng, k, 'plain')
            seen.append(eng.grad_clip_stats())
        assert [s[3] for s in seen] == list(np.cumsum([1 if s[1] < 1.0 else 0 for s in seen]))
        assert seen[-1][2] == max(s[0] for s in seen)
    finally:
        for e in made:
            e.close()


def test_clipped_steps_counts_loose_steps_as_not_clipped(rig):
    _reset(rig.loose)
    for k in range(2):
        _step(rig, rig.loose, k, 'plain')
    norm, coef, top, clipped = rig.loose.grad_clip_stats()
    assert clipped == 0 and coef == 1.0 and top >= norm > 0
    rig.loose.reset_grad_clip_stats()
    assert rig.loose.grad_clip_stats()[2:] == (0.0, 0)


def test_inception_v3_from_grey_rois_with_its_aux_head():
    rng = np.random.default_rng(3)
    rois = [rng.integers(0, 256, (int(h), int(w)), dtype=np.uint8) for h, w in ((57, 131), (203, 88))]
    hs, ws = np.array([r.shape[0] for r in rois], np.int32), np.array([r.shape[1] for r in rois], np.int32)
    offs = np.zeros(2, np.int64)
    offs[1] = rois[0].size
    pix = torch.from_numpy(np.concatenate([r.ravel() for r in rois])).cuda()
    args = (pix, torch.from_numpy(offs).cuda(), torch.from_numpy(hs).cuda(), torch.from_numpy(ws).cuda(), int(hs.max()), int(ws.max()))
    ys = torch.tensor([1, 5])

    def run(eng):
        eng.load_rois(*args)
        if eng.stem_u8 is not None:
            assert eng.in_kind[eng.in_slot] == 'u8'
        eng.target[:2].copy_(ys)
        pl = eng.forward_train(2)
        eng.run(pl.loss)
        eng.backward(2)

    base = _engine('inception_v3', 2, dtype='fp32')
    made = []

    def clipped_of(mx):
        made.append(_engine('inception_v3', 2, dtype='fp32', clip_grad=mx))
        return made[0]

    try:
        assert len([h for h in base.heads if h.aux]) == 1
        _tight_case(base, clipped_of, run, 2)
    finally:
        base.close()
        for e in made:
            e.close()


def test_channel_padding_inside_the_flat_buffer_stays_zero():
    """squeezenet's classifier conv pads its output channels to a 16-byte chunk: rows of G that belong to no parameter view"""
    eng = _engine('squeezenet', 2, dtype='fp32', clip_grad=1.0)
    try:
        assert any(getattr(n, 'kind', '') == 'cb' and n.K != n.K_real for n in eng.net.nodes)
        g = torch.Generator().manual_seed(2)
        eng.load_input_nchw(torch.rand(2, 3, S, S, generator=g).cuda())
        eng.target[:2].copy_(torch.tensor([0, 6]))
        pl = eng.forward_train(2)
        eng.run(pl.loss)
        eng.backward(2)
        assert _check_padding_is_zero(eng) > 4
        eng.adam_step(2)
        total64, _ = cc.torch_clip([eng.gviews[k] for k in eng.gviews], 1.0, dtype=torch.float64)
        norm = eng.grad_clip_stats()[0]
        assert abs(norm - total64) <= cc.norm_bound(eng.nparam_padded, cc.geometry(eng.ctx.lib)[0], total64)
    finally:
        eng.close()


def test_two_replicas_clip_the_averaged_gradient_by_the_same_bits():
    import dp_twin
    tw = dp_twin.Twin('resnet18', B, S, nc=NC, dtype='fp32', clip_grad=1e-3)
    try:
        local = tw.local(0)
        tw.ddp_step(0, local)
        stats = [e.grad_clip_stats() for e in tw.engs]
        st = [e.clip_state[:2].clone() for e in tw.engs]
        assert same(st[0], st[1])                                   # the same norm and coefficient bits, no collective
        summed = (local[0]['G'] + local[1]['G']).cpu()              # what each replica holds behind the exchange (fp32 sum, commutative)
        real = _real_mask(tw.engs[0])
        assert bool((summed[~real] == 0).all())
        ref = cc.ref_norm(summed[real], 0.5)                        # the norm of the averaged gradient
        eng = tw.engs[0]
        assert abs(stats[0][0] - ref) <= cc.norm_bound(eng.nparam_padded, cc.geometry(eng.ctx.lib)[0], ref, 0.5)
        assert stats[0][1] < 1.0 and cc.f32_bits(stats[0][1]) == cc.f32_bits(cc.host_coef(np.float32(stats[0][0]), 1e-3))
        assert same(tw.engs[0].P, tw.engs[1].P)
    finally:
        tw.close()


def _cli(argv):
    from ifcb_classifier_amd import neuston_net as nn_
    args = nn_.argparse_nn().parse_args(argv)
    nn_.argparse_nn_runtimeparams(args)
    nn_.main(args)
    return args


def test_train_with_clip_grad_then_run(tmp_path, capsys):
    from PIL import Image
    import yaml
    src = str(tmp_path / 'training-data')
    rng = np.random.default_rng(7)
    for cls, mean, n in (('big', 90, 24), ('mid', 130, 8), ('small', 170, 4)):
        os.makedirs(os.path.join(src, cls))
        for i in range(n):
            h, w = rng.integers(32, 129, 2)
            a = np.clip(rng.normal(mean, 30, (h, w)), 0, 255).astype(np.uint8)
            Image.fromarray(a, 'L').save(os.path.join(src, cls, 'roi_%s_%03d.png' % (cls, i)))
    out = str(tmp_path / 'training-output' / 'clip')
    _cli(['--batch', '16', '--loaders', '0', 'TRAIN', src, 'resnet18', 'clip', '--untrain', '--seed', '1', '--emax', '1', '--emin', '1',
          '--estop', '0', '--outdir', out, '--clip-grad', '0.5'])
    printed = capsys.readouterr().out
    line = [ln for ln in printed.splitlines() if 'largest gradient norm before clipping' in ln]
    assert len(line) == 1 and '--clip-grad 0.5' in line[0], printed[-2000:]
    k, s = [int(v) for v in line[0].split('clipped ')[1].split(' steps')[0].split(' of ')]
    assert 0 <= k <= s and s >= 1
    assert yaml.safe_load(open(os.path.join(out, 'args.yml')))['clip_grad'] == 0.5
    ck = torch.load(os.path.join(out, 'clip.ptl'), map_location='cpu', weights_only=False)
    assert ck['hyper_parameters']['clip_grad'] == 0.5
    rows = open(os.path.join(out, 'epochs.csv')).read().strip().splitlines()
    assert rows[0].split(',')[:4] == ['epoch', 'best', 'train_loss', 'val_loss'] and 'clip' not in rows[0] and len(rows) == 2
    assert math.isfinite(float(rows[1].split(',')[2]))
    run_out = str(tmp_path / 'run-output')
    _cli(['--batch', '16', '--loaders', '0', 'RUN', src, os.path.join(out, 'clip.ptl'), 'r1', '--type', 'img',
          '--outdir', run_out + '/{RUN_ID}/v3/{MODEL_ID}', '--outfile', 'img_results.json'])
    rj = json.load(open(os.path.join(run_out, 'r1', 'v3', 'clip', 'img_results.json')))
    scores = np.array(rj['output_scores'], dtype=np.float32)
    assert rj['model_id'] == 'clip' and scores.shape == (36, 3) and np.allclose(scores.sum(1), 1, atol=1e-4)
