"""TRAIN --blur on the host: the flags and their parsers, the per-item sigma draw (own generator: no other draw moves), the float64 twin
of tests/blur_cases.py against torch's reflect pad + conv2d, the near-tie cap of the GPU tests' u8 inputs, the header / export map /
ctypes table, the --distill refusal, and an engine without the flag (plans and load_rois launches as before).  The kernel runs in
tests/test_gpu_batch_blur.py and tests/test_gpu_blur_*.py."""
import argparse
import os
import random
import re
import sys
import types
from unittest import mock

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_plan_fingerprints as mpf  # noqa: E402

import blur_cases as bc  # noqa: E402
from ifcb_classifier_amd import _lib, graph, neuston_data as nd, neuston_models, neuston_net  # noqa: E402
from ifcb_classifier_amd.engine import Engine  # noqa: E402


# ------------------------------------------------------------------------------------------------------ parsing, argparse
def _parse(*extra):
    return neuston_net.argparse_nn().parse_args(['TRAIN', 'src', 'inception_v3', 'id'] + list(extra))


def test_flags():
    a = _parse()
    assert a.blur is None and a.blur_prob == 0.5
    a = _parse('--blur', '2', '--blur-prob', '0.25')
    assert (a.blur, a.blur_prob) == (2.0, 0.25)
    assert _parse('--blur', '4').blur == 4.0 and _parse('--blur', '0.11', '--blur-prob', '0').blur_prob == 0.0
    assert _parse('--blur', '1', '--blur-prob', '1').blur_prob == 1.0
    for bad in (['--blur', '0.1'], ['--blur', '0'], ['--blur', '4.01'], ['--blur', '-1'], ['--blur', 'nan'], ['--blur', 'inf'], ['--blur', 'x'],
                ['--blur-prob', '1.5'], ['--blur-prob', '-0.1'], ['--blur-prob', 'nan'], ['--blur-prob', 'p']):
        with pytest.raises(SystemExit):
            _parse(*bad)
    helps = {a.dest: a.help for a in neuston_net.argparse_nn()._subparsers._group_actions[0].choices['TRAIN']._actions}
    assert '(MI355X path, additive)' in helps['blur'] and '(MI355X path, additive)' in helps['blur_prob']


def test_parsers_and_radius():
    assert nd.parse_blur(None) is None and nd.parse_blur('2') == 2.0 and nd.parse_blur(4) == 4.0 and nd.parse_blur(0.1001) == 0.1001
    assert nd.parse_blur_prob(None) == 0.5 and nd.parse_blur_prob('0') == 0.0 and nd.parse_blur_prob(1) == 1.0
    for bad in (0.1, 0, -2, 4.0001, float('nan'), float('inf'), 'a', True):
        with pytest.raises(ValueError):
            nd.parse_blur(bad)
    for bad in (-0.1, 1.1, float('nan'), 'p', False):
        with pytest.raises(ValueError):
            nd.parse_blur_prob(bad)
    # r = ceil(3 SIGMA_MAX): 1..12 over the whole legal range
    assert [nd.blur_radius(s) for s in (0.11, 1 / 3, 0.34, 1, 2, 2.01, 4)] == [1, 1, 2, 3, 6, 7, 12] and nd.blur_radius(None) is None


# ------------------------------------------------------------------------------------------------------ the draws
def _sigmas(n=200, **kw):
    t = nd.RoiTransform(299, **kw)
    return [t.blur_sigma() for _ in range(n)]


def test_draws_are_reproducible_float32_and_in_range():
    a, b = _sigmas(blur=2.0, blur_prob=0.5, seed=7), _sigmas(blur=2.0, blur_prob=0.5, seed=7)
    assert a == b and a != _sigmas(blur=2.0, blur_prob=0.5, seed=8) and a != _sigmas(blur=2.0, blur_prob=0.5, seed=7, rank=1)
    assert all(s == float(np.float32(s)) for s in a)
    drawn = [s for s in a if s != 0.0]
    assert 60 < len(drawn) < 140 and all(float(np.float32(0.1)) <= s <= 2.0 for s in drawn)
    assert all(s == 0.0 for s in _sigmas(blur=2.0, blur_prob=0.0, seed=7))
    assert all(s > 0.0 for s in _sigmas(blur=4.0, blur_prob=1.0, seed=7))
    assert all(s == 0.0 for s in _sigmas(seed=7))                    # unset: nothing is drawn
    # P changes which images are drawn, never the sigma an image would get
    p1 = _sigmas(blur=2.0, blur_prob=1.0, seed=7)
    assert all(s in (0.0, q) for s, q in zip(a, p1))


def test_no_other_draw_moves_and_no_global_stream_is_touched():
    def run(**kw):
        random.seed(5)
        np.random.seed(5)
        torch.manual_seed(5)
        t = nd.RoiTransform(299, vflip=True, hflip=True, rot90=True, jitter='0.2,0.3', seed=3, **kw)
        d = nd.draw_items(t, 16)
        items = [((np.zeros((4, 5), np.uint8), t.flip_code(), True) + t.jitter_factors() + ((t.blur_sigma(),) if kw else ()), 0, 'p')
                 for _ in range(8)]
        c = nd.collate_rois(items)[0]
        return d, c, (random.random(), float(np.random.rand()), float(torch.rand(1)))
    d0, c0, g0 = run()
    d1, c1, g1 = run(blur=2.0, blur_prob=1.0)
    assert g0 == g1
    for a, b in ((d0, d1), (c0, c1)):
        assert 'blur' not in a and b['blur'].dtype == torch.float32 and bool((b['blur'] > 0).all())
        for k in ('flips', 'brightness', 'contrast'):
            assert torch.equal(a[k], b[k]), k
        assert a.get('turn') == b.get('turn')
    assert d1['blur'].numel() == 16 and c1['blur'].numel() == 8
    # P = 0: the batch carries no sigmas at all, so nothing is launched for it
    d2, c2, _ = run(blur=2.0, blur_prob=0.0)
    assert 'blur' not in d2 and 'blur' not in c2


def test_dataset_items_collate_and_upload_carry_the_sigmas(tmp_path):
    from PIL import Image
    os.makedirs(tmp_path / 'a')
    for i in range(3):
        Image.fromarray(np.full((5 + i, 7), 10 * i, np.uint8)).save(str(tmp_path / 'a' / ('%d.png' % i)))
    args = argparse.Namespace(MODEL='inception_v3', img_norm=None, flip=None, blur=2.0, blur_prob=1.0, seed=9)
    train, val = nd.get_trainval_transforms(args)
    assert (train.blur, train.blur_prob) == (2.0, 1.0) and val.blur is None
    ds = nd.NeustonDataset(str(tmp_path), transforms=train)
    items = [ds[i] for i in range(3)]
    assert all(len(it[0]) == 6 and it[0][3] is None and it[0][4] is None and it[0][5] > 0 for it in items)
    batch = nd.collate_rois(items)[0]
    assert 'brightness' not in batch and batch['blur'].tolist() == [it[0][5] for it in items]
    kw = nd.rois_to_device(batch, 'cpu', train)
    assert torch.equal(kw['blur'], batch['blur']) and 'jitter' not in kw
    ds.transforms = val
    assert len(ds[0][0]) == 2 and 'blur' not in nd.collate_rois([ds[0]])[0]


# ------------------------------------------------------------------------------------------------------ the twin
@pytest.mark.parametrize('S,r,sigma', [(2, 1, 0.3), (13, 12, 4.0), (25, 12, 0.1), (33, 6, 1.3), (40, 3, 0.9)])
def test_twin_is_reflect_pad_and_conv2d_in_float64(S, r, sigma):
    import torch.nn.functional as F
    x = torch.from_numpy(np.random.default_rng(S).uniform(0, 255, (S, S)))
    w, _ = bc.weights64(sigma, r)
    assert abs(w.sum() - 1.0) < 1e-15 and np.array_equal(w, w[::-1]) and w.argmax() == r
    w2 = torch.from_numpy(np.outer(w, w))[None, None]
    want = F.conv2d(F.pad(x[None, None], (r, r, r, r), mode='reflect'), w2)[0, 0].numpy()
    got = bc.twin(x.numpy(), sigma, r)
    assert np.abs(got - want).max() <= 255 * 64 * 2.0 ** -53 * (2 * r + 1)
    # torchvision's _get_gaussian_kernel1d at kernel_size 2 r + 1
    k = 2 * r + 1
    lim = (k - 1) * 0.5
    pdf = torch.exp(-0.5 * (torch.linspace(-lim, lim, k, dtype=torch.float64) / float(np.float32(sigma))).pow(2))
    assert np.allclose(w, (pdf / pdf.sum()).numpy(), rtol=1e-13, atol=0)


def test_twin_of_an_impulse_and_of_sigma_0():
    S, r, sigma = 31, 6, 1.7
    x = np.zeros((S, S))
    x[15, 15] = 1.0
    w, _ = bc.weights64(sigma, r)
    out = bc.twin(x, sigma, r)
    assert np.allclose(out[15 - r:15 + r + 1, 15 - r:15 + r + 1], np.outer(w, w), rtol=1e-14, atol=0) and abs(out.sum() - 1.0) < 1e-14
    # an impulse on the edge: the reflected taps fold back onto their mirror images (the edge itself is not repeated)
    e = np.zeros((S, S))
    e[1, 8] = 1.0
    col = bc.twin(e, sigma, r)[:, 8]
    w1 = w[r]
    assert np.isclose(col[0], 2 * w[r + 1] * w1) and np.isclose(col[1], (w1 + w[r + 2]) * w1) and np.isclose(col[2], (w[r + 1] + w[r + 3]) * w1)
    assert list(bc.reflect_map(5, 3)) == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    for s in (0.0, -1.0, float('nan'), float('inf')):
        assert np.array_equal(bc.twin(e, s, r), e) and bc.fp32_bound(s, r, 255.0) == 0.0


def test_the_bound_follows_the_chain_length():
    u = bc.U
    for r, sigma in ((1, 1 / 3), (6, 2.0), (12, 4.0), (12, 0.1)):
        k = 2 * r + 1
        c, W = bc.pass_coef(sigma, r)
        # between the chain of the centre tap alone and the worst case of k roundings on every term plus (9 k + 1) u of weight error
        assert (r + 1) * u < c < (k + 9 * k + 1) * u * 1.001 and 0 < W < c
        b = bc.fp32_bound(sigma, r, 255.0)
        assert 2 * 255 * c <= b <= 2 * 255 * c * 1.001
    assert bc.fp32_bound(4.0, 12, 255.0) > bc.fp32_bound(1 / 3, 1, 255.0)
    ref = np.array([1.0, -2.0])
    assert np.all(bc.stored_bound('bf16', 2.0, 6, 3.0, ref) > 2.0 ** -8 * np.abs(ref))
    assert np.all(bc.stored_bound('f32', 2.0, 6, 3.0, ref) == bc.fp32_bound(2.0, 6, 3.0))


@pytest.mark.parametrize('name', bc.CASE_IDS)
def test_the_gpu_tests_u8_inputs_stay_under_the_near_tie_cap(name):
    _, S, r, sigmas, amp = bc.CASES[bc.CASE_IDS.index(name)]
    assert 0 < r < S and all(s == 0.0 or float(np.float32(0.1)) <= float(np.float32(s)) <= r / 3.0 + 1e-6 for s in sigmas)
    x = bc.case_input(name, 'u8')
    ref, bound = bc.case_twin(name, 'u8')
    assert x.shape == (len(sigmas), S, S) and x.max() < amp
    for n, s in enumerate(sigmas):
        share = float(bc.near_tie(ref[n], bound[n]).mean())
        assert share <= bc.TIE_CAP, (name, n, share)
        if s == 0.0:
            assert np.array_equal(ref[n], x[n]) and not bound[n].any()
        else:
            assert 0 < bound[n].max() < (5e-4 if x[n].max() < 128 else 2e-3)      # (the bound grows with the plane's largest level)
    # the float32 emulation of the kernel's arithmetic stays within the bound (and so does its rint, off the near-ties)
    for n, s in enumerate(sigmas):
        if s:
            emu = _emulate(x[n].astype(np.float32), s, r)
            assert np.abs(emu.astype(np.float64) - ref[n]).max() <= bound[n].max()
            wrong, _ = bc.u8_verdict(np.clip(np.rint(emu), 0, 255), ref[n], bound[n])
            assert not wrong.any()


def _emulate(img, sigma, r):
    """the kernel's order of operations in numpy float32 (products and sums rounded separately: within the same bound as the fused form)"""
    f = np.float32
    k, S = 2 * r + 1, img.shape[0]
    with np.errstate(over='ignore', under='ignore'):
        q = (np.arange(-r, r + 1).astype(f)) / f(sigma)
        e = np.exp((f(-0.5) * (q * q)).astype(np.float64)).astype(f)
    s = f(0)
    for j in range(k):
        s = f(s + e[j])
    w = (e / s).astype(f)
    idx = bc.reflect_map(S, r)
    h = np.zeros_like(img)
    for j in range(k):
        h = (h.astype(np.float64) + w[j].astype(np.float64) * img[:, idx[j:j + S]].astype(np.float64)).astype(f)      # (one rounding: fmaf)
    out = np.zeros_like(img)
    for j in range(k):
        out = (out.astype(np.float64) + w[j].astype(np.float64) * h[idx[j:j + S], :].astype(np.float64)).astype(f)
    return out


def test_dense_case_inputs():
    for name in bc.CASE_IDS[:3]:
        xb, xf = bc.case_input(name, 'bf16'), bc.case_input(name, 'f32')
        assert xb.dtype == np.float32 and xb.shape[-1] == 8 and np.all(xb[..., 3:] != 0)
        assert torch.equal(torch.from_numpy(xb.copy()).to(torch.bfloat16).float(), torch.from_numpy(xb.copy()))      # exact in bf16
        ref, bound = bc.case_twin(name, 'f32')
        assert np.array_equal(ref[..., 3:], xf[..., 3:].astype(np.float64)) and not bound[..., 3:].any()


# ------------------------------------------------------------------------------------------------------ header, export map, binding
def test_the_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'ifcbk.h')).read()
    m = re.search(r'IFCBK_API int ifcbk_batch_blur\((.*?)\);', hdr, re.S)
    assert m and len(re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S).split(',')) == 8 == len(_lib._PROTOS['ifcbk_batch_blur'][1])
    assert 'ifcbk_batch_blur' in _lib.EXPORTS and getattr(_lib.load(), 'ifcbk_batch_blur').argtypes is not None
    emap = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'exports.map')).read()
    assert re.search(r'global:\s*ifcbk_\*;', emap) and re.search(r'local:\s*\*;', emap)
    src = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'batch_blur.hip')).read()
    assert 'extern "C" int ifcbk_batch_blur(' in src and 'atomic' not in src.split('#include')[1]
    mk = open(os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc', 'Makefile')).read()
    assert 'batch_blur.hip' in mk
    assert max(_lib.OP_NAMES) == 40                                    # no new op kind


# ------------------------------------------------------------------------------------------------------ engine and model without / with it
def _plan(model, B, **kw):
    keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
    with mock.patch.dict(os.environ, keep, clear=True), mock.patch.object(torch, 'zeros', torch.empty), \
            mock.patch.object(torch, 'zeros_like', torch.empty_like):
        eng = Engine(graph.build(model, 7), max_batch=B, dtype='bf16', plan_only=True, **kw)
        return eng, eng.plan(B)


def test_blur_radius_changes_no_plan():
    eng0, pl0 = _plan('inception_v3', 2)
    eng1, pl1 = _plan('inception_v3', 2, blur_radius=6)
    assert eng0.blur_radius is None and eng1.blur_radius == 6
    assert mpf.plan_text(eng1, pl1) == mpf.plan_text(eng0, pl0)
    for bad in (0, 13, -1, 2.5):
        with pytest.raises(ValueError, match='blur_radius'):
            _plan('resnet18', 2, blur_radius=bad)


class _Calls:
    def __init__(self):
        self.calls = []

    def call(self, name, *a):
        self.calls.append((name,) + a)


def _stub(radius, kind):
    ctx, pre = _Calls(), _Calls()
    loads = []

    def load_into(target, *a, **kw):
        c, stream, tstream, slot, main = target
        loads.append((c, slot, main) + a)
    s = types.SimpleNamespace(ctx=ctx, pre_ctx=pre, pre_stream=types.SimpleNamespace(cuda_stream=77), in_slot=0,
                              in_kind=[kind, kind], in_u8=['u8_0', 'u8_1'], in_bufs=['d_0', 'd_1'], cdtype=_lib.BF16, blur_radius=radius,
                              net=types.SimpleNamespace(S=299), _load_rois_into=load_into, dev=None)
    s._slot_target, s._slot_image = types.MethodType(Engine._slot_target, s), types.MethodType(Engine._slot_image, s)
    return s, ctx, pre, loads


def test_load_rois_launches_nothing_more_without_sigmas_and_one_call_with_them():
    px = torch.zeros(12, dtype=torch.uint8)
    tabs = (torch.zeros(3, dtype=torch.int64), torch.full((3,), 2, dtype=torch.int32), torch.full((3,), 2, dtype=torch.int32))
    sig = torch.tensor([0.0, 1.0, 2.0])
    with mock.patch('ifcb_classifier_amd.engine._vp', lambda t: t), \
            mock.patch('torch.cuda.current_stream', lambda dev: types.SimpleNamespace(cuda_stream=11)):
        for more in (dict(), dict(blur=None)):
            for radius in (None, 6):
                s, ctx, pre, loads = _stub(radius, 'u8')
                assert Engine.load_rois(s, px, *tabs, 2, 2, **more) == 3
                assert len(loads) == 1 and loads[0][:3] == (ctx, 0, True) and not ctx.calls and not pre.calls
        # the current slot: behind the resize, on its ctx and stream, on the buffer the resize wrote
        s, ctx, pre, loads = _stub(6, 'u8')
        assert Engine.load_rois(s, px, *tabs, 2, 2, blur=sig) == 3
        (c,) = ctx.calls
        assert len(loads) == 1 and not pre.calls and c[:7] == ('ifcbk_batch_blur', 'u8_0', _lib.MIX_U8, 3, 299, sig, 6) and c[7].value == 11
        # a prefetch slot: the prefetch ctx and stream, the dense tensor of that slot
        s, ctx, pre, loads = _stub(12, 'nhwc')
        assert Engine.load_rois(s, px, *tabs, 2, 2, slot=1, blur=sig) == 3
        (c,) = pre.calls
        assert not ctx.calls and c[:7] == ('ifcbk_batch_blur', 'd_1', _lib.BF16, 3, 299, sig, 12) and c[7].value == 77
        assert loads[0][:3] == (pre, 1, False)
        # refusals: an engine without a radius, a tensor of the wrong type or length
        s, ctx, pre, loads = _stub(None, 'u8')
        with pytest.raises(RuntimeError, match='blur_radius'):
            Engine.load_rois(s, px, *tabs, 2, 2, blur=sig)
        s, ctx, pre, loads = _stub(6, 'u8')
        for bad in (sig.double(), sig[:2], [0.0, 1.0, 2.0]):
            with pytest.raises(ValueError, match='sigmas'):
                Engine.load_rois(s, px, *tabs, 2, 2, blur=bad)
        assert not loads and not ctx.calls


class _HostEngine(Engine):
    def __init__(self, *a, **k):
        k['plan_only'] = True
        super().__init__(*a, **k)


def _hparams(**kw):
    hp = dict(MODEL='resnet18', classes=['a', 'b', 'c'], pretrained=False, batch_size=2, precision='fp32', model_id='m', seed=1, resize=224,
              img_norm=None)
    hp.update(kw)
    return argparse.Namespace(**hp)


def test_hparams_round_trip_old_checkpoints_and_the_distill_refusal(tmp_path):
    with mock.patch.object(neuston_models, 'Engine', _HostEngine):
        m = neuston_models.NeustonModel(_hparams(blur=2.0, blur_prob=0.25))
        assert m.blur == 2.0 and m.model.engine.blur_radius == 6
        ck = m.checkpoint_dict()
        assert (ck['hyper_parameters']['blur'], ck['hyper_parameters']['blur_prob']) == (2.0, 0.25)
        path = str(tmp_path / 'm.ptl')
        torch.save(ck, path)
        assert neuston_models.NeustonModel.load_from_checkpoint(path).model.engine.blur_radius == 6
        for k in ('blur', 'blur_prob'):
            del ck['hyper_parameters'][k]
        torch.save(ck, path)
        m3 = neuston_models.NeustonModel.load_from_checkpoint(path)
        assert m3.blur is None and m3.model.engine.blur_radius is None
        with pytest.raises(ValueError, match='blur and distill do not combine'):
            neuston_models.NeustonModel(_hparams(blur=2.0, distill='teacher.ptl'))
        # the teacher never gets the student's sigmas
        assert 'blur' not in neuston_models.NeustonModel._teacher_kw(types.SimpleNamespace(_teacher_load={}), dict(pixels=1, blur=2, jitter=3))


def test_train_refuses_blur_with_distill_before_anything_is_read(tmp_path):
    a = _parse('--blur', '2', '--distill', str(tmp_path / 'nothing.ptl'), '--outdir', str(tmp_path / 'out'))
    a.cmd_timestamp = '2026-01-01T00:00:00'
    with pytest.raises(SystemExit, match='--blur and --distill do not combine'):
        neuston_net.do_training(a)
    text = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert '--blur' in text and re.search(r'--blur[^\n]*--distill|--distill[^\n]*--blur', text)
