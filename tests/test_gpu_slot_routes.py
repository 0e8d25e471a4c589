"""The two routes of an input slot on the GPU: ``Engine.load_rois`` with flips + turn + pad + jitter + blur and then ``mix_batch``, on the
current slot (the engine's ctx, the current stream) and on a prefetch slot (the prefetch ctx and stream), leave the same bits in the two
slots' input buffers -- one target choice (``_slot_target``) and one buffer choice (``_slot_image``) serve both routes and all kernels.
Batch 3, the smallest with a self-partnered middle image under mixing, fp32.  resnet18 has no u8 stem, so its grey batch goes through
the dense tensor like its RGB batch; inception_v3 is here for the grey batch through the u8 plane."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
B = 3


def _batch(ch, seed):
    """a collated batch of three ROIs of odd, mixed sizes with every per-item draw: codes with transpose bits, both factors, sigmas"""
    from ifcb_classifier_amd.neuston_data import collate_rois
    rng = np.random.default_rng(seed)
    draws = [(5, True, 0.75, 1.25, 1.3), (2, True, 1.375, 0.625, 0.0), (7, True, 0.875, 1.125, 2.0)]
    items = []
    for i, d in enumerate(draws):
        h, w = (int(v) for v in rng.integers(21, 90, 2))
        img = rng.integers(0, 256, (h, w) if ch == 1 else (h, w, 3)).astype(np.uint8)
        items.append(((img,) + d, i, 'roi%d' % i))
    rois = collate_rois(items)[0]
    assert rois['in_channels'] == ch and rois['turn'] is True and all(k in rois for k in ('brightness', 'contrast', 'blur'))
    return rois


def _bits(eng, slot):
    buf = eng.in_u8[slot] if eng.in_kind[slot] == 'u8' else eng.in_bufs[slot]
    t = buf[:B].clone().cpu()
    return t if t.dtype == torch.uint8 else t.contiguous().view(torch.int32)


@pytest.mark.parametrize('model', ['resnet18', 'inception_v3'])
def test_the_current_slot_and_a_prefetch_slot_hold_the_same_bits(model):
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    from ifcb_classifier_amd.neuston_data import RoiTransform, rois_to_device
    eng = Engine(graph.build(model, 7), max_batch=B, dtype='fp32', mix=True, blur_radius=6)
    S = eng.net.S
    tf = RoiTransform(S, ((0.4, 0.5, 0.6), (0.2, 0.25, 0.3)), rot90=True, pad='border')
    lam, box = 0.3183, (S // 4, S // 2 + 3, 0, S // 3)
    kinds = []
    for ch in (1, 3):
        rois = _batch(ch, 10 + ch)
        # the current slot
        kw = rois_to_device(rois, eng.dev, tf)
        assert sorted(kw) == sorted(['pixels', 'offs', 'hs', 'ws', 'max_h', 'max_w', 'in_channels', 'flips', 'turn', 'mean', 'std', 'pad',
                                     'jitter', 'blur'])
        assert eng.load_rois(**kw) == B and eng.mix_batch(B, lam, box) == B
        torch.cuda.synchronize()
        cur = eng.in_slot
        kinds.append(eng.in_kind[cur])
        a = _bits(eng, cur)
        # a prefetch slot: a fresh upload (the jitter maps the blob in place), the same calls with slot=
        slot, side = eng.prefetch_begin()
        assert slot == 1 - cur and bool(a.any())
        with torch.cuda.stream(side):
            assert eng.load_rois(slot=slot, **rois_to_device(rois, eng.dev, tf)) == B and eng.mix_batch(B, lam, box, slot=slot) == B
        eng.prefetch_end(slot)
        torch.cuda.synchronize()
        assert eng.in_slot == cur and eng.in_kind[slot] == eng.in_kind[cur]
        b = _bits(eng, slot)
        assert a.dtype == b.dtype and torch.equal(a, b)
        assert torch.equal(eng.mix_lam[cur][:B].cpu(), eng.mix_lam[slot][:B].cpu())
        # ... and not the bits of the plain load: the augmentations did run
        eng.load_rois(**{k: v for k, v in rois_to_device(rois, eng.dev, None).items() if k not in ('flips', 'turn', 'jitter', 'blur')})
        torch.cuda.synchronize()
        assert not torch.equal(_bits(eng, cur), a)
    assert kinds == (['u8', 'nhwc'] if model == 'inception_v3' else ['nhwc', 'nhwc'])
