"""RUN --tta on the GPU, whole models: NeustonModel.eval_current_tta against plain eval_current on views that the test itself writes
into the input slot with numpy (tests/sym_cases.py).  One engine per backbone, closed at the end: resnet18 fp32 on the dense route at
batch 4, inception_v3 bf16 on the u8-stem route at batch 3.

The reference is the fp32 left-to-right sum of the views' eval_current scores times 1 / V, and the comparison is bit for bit.

A batch that every symmetry of the square leaves alone shows the same input to every forward.  With four views the result is then the
plain scores bit for bit: p + p and (fl(3p) + p) are exact.  With eight it is NOT, and cannot be under the left-to-right fp32 order
the reference above fixes: fl(5p), fl(6p), fl(7p) carry roundings that do not cancel, and for 47 % of all fp32 values p the
left-to-right sum of eight copies times 0.125 differs from p in the last place (test_tta_cpu.py counts them).  For 'all' the test
therefore asserts what a symmetric batch does give: bit for bit the left-to-right sum of eight copies of the PLAIN scores times 0.125
-- every view produced the plain bits -- which is within two fp32 ulps of them (four inexact adds of at most half an ulp of 8p)."""
import argparse

import numpy as np
import pytest
import torch

import sym_cases as sc

pytestmark = pytest.mark.gpu

RIGS = {'resnet18': dict(precision='fp32', B=4, kind='nhwc'), 'inception_v3': dict(precision='bf16', B=3, kind='u8')}


def _rois(B, seed):
    from ifcb_classifier_amd.neuston_data import collate_rois
    rng = np.random.default_rng(seed)
    items = []
    for i in range(B):
        h, w = rng.integers(20, 90, 2)
        items.append(((rng.integers(0, 256, (h, w)).astype(np.uint8), 0), 0, 'roi%d' % i))
    return collate_rois(items)[0]


class _Rig:
    def __init__(self, name):
        from ifcb_classifier_amd.neuston_data import rois_to_device
        from ifcb_classifier_amd.neuston_models import NeustonModel
        cfg = RIGS[name]
        self.name, self.n = name, cfg['B']
        torch.manual_seed(11)
        self.m = NeustonModel(argparse.Namespace(MODEL=name, classes=list('abcdefg'), pretrained=False, batch_size=self.n,
                                                 precision=cfg['precision'], model_id='tta', resize=224, img_norm=None, seed=3,
                                                 learning_rate=1e-6))
        self.eng = eng = self.m.model.engine
        S = eng.net.S
        if name == 'resnet18':          # the dense route: an NCHW float batch
            g = torch.Generator().manual_seed(5)
            data = [torch.rand(self.n, 3, S, S, generator=g).cuda() for _ in range(2)]
            self.load = [lambda x=x: eng.load_input_nchw(x) for x in data]
        else:                           # grey ROIs: the resize writes the u8 plane, the stem conv reads it
            data = [rois_to_device(_rois(self.n, seed), eng.dev, None) for seed in (1, 2)]
            self.load = [lambda r=r: eng.load_rois(**r) for r in data]
        # a freshly initialised network in eval mode normalises with running statistics (0, 1) and its softmax saturates to a one-hot
        # row, the same for every view: a few train steps at a negligible learning rate bring the statistics to the data
        y = torch.arange(self.n).cuda() % 7
        for k in range(30):
            self.m.fit_batch(data[k % 2], y)
        self.load[0]()
        assert eng.in_kind[eng.in_slot] == cfg['kind']
        torch.cuda.synchronize()
        self.base = self.slot()[:self.n].cpu().numpy().copy()           # batch X as it lies in the slot

    def slot(self):
        s = self.eng.in_slot
        return self.eng.in_u8[s] if self.eng.in_kind[s] == 'u8' else self.eng.in_bufs[s]

    def write(self, arr):
        self.slot()[:self.n].copy_(torch.from_numpy(np.ascontiguousarray(arr)))

    def plain(self):
        p = self.m.eval_current(self.n)[0]
        assert torch.isfinite(p).all().item()
        return p


@pytest.fixture(scope='module', params=sorted(RIGS))
def rig(request):
    r = _Rig(request.param)
    yield r
    torch.cuda.synchronize()
    r.eng.close()


def _mean(ps):
    s = ps[0].clone()
    for p in ps[1:]:
        s = s + p
    return s * (1.0 / len(ps))


@pytest.mark.parametrize('graph', [True, False])
@pytest.mark.parametrize('mode', ['flips', 'all'])
def test_tta_is_the_fp32_mean_of_eval_current_over_numpy_views(rig, mode, graph):
    rig.eng.graph_eval = graph
    views = sc.views(rig.base, mode)
    ref = []
    for v in views:
        rig.write(v)
        ref.append(rig.plain())
    assert not torch.equal(ref[0], ref[1])
    rig.write(rig.base)
    got = rig.m.eval_current_tta(rig.n, mode)
    torch.cuda.synchronize()
    assert got.shape == (rig.n, 7) and torch.equal(got, _mean(ref)), (rig.name, mode, graph)
    assert not torch.equal(got, ref[0])                                  # an asymmetric batch: the averaged scores are not the plain ones
    # the slot is left in the walk's last view, and one more op brings the batch back
    assert np.array_equal(rig.slot()[:rig.n].cpu().numpy(), views[-1])
    rig.eng.sym_batch(rig.n, sc.RESTORE[mode])
    assert np.array_equal(rig.slot()[:rig.n].cpu().numpy(), rig.base)


def test_a_symmetric_batch_shows_every_forward_the_same_input(rig):
    rig.eng.graph_eval = True
    sym = sc.symmetrised(rig.base)
    assert all(np.array_equal(v, sym) for v in sc.views(sym, 'all'))
    rig.write(sym)
    plain = rig.plain()
    got4 = rig.m.eval_current_tta(rig.n, 'flips')
    got8 = rig.m.eval_current_tta(rig.n, 'all')
    torch.cuda.synchronize()
    assert torch.equal(got4, plain)
    assert torch.equal(got8, _mean([plain] * 8))
    ulp = torch.ldexp(torch.ones_like(plain), torch.frexp(plain)[1] - 24)
    assert ((got8 - plain).abs() <= 2 * ulp).all().item()
    assert np.array_equal(rig.slot()[:rig.n].cpu().numpy(), sym)


def test_no_state_leaks_into_the_plain_path(rig):
    rig.eng.graph_eval = True
    rig.load[1]()                                                        # batch Y, freshly loaded
    before = rig.plain()
    rig.load[0]()
    for mode in ('flips', 'all'):
        rig.m.eval_current_tta(rig.n, mode)
    rig.load[1]()
    after = rig.plain()
    torch.cuda.synchronize()
    assert torch.equal(before, after)
    with pytest.raises(ValueError, match='mode'):
        rig.m.eval_current_tta(rig.n, 'quarter')
    with pytest.raises(ValueError, match='sym_batch'):
        rig.eng.sym_batch(rig.n + 1, sc.HFLIP)
