"""dev tool: the ROI preprocess kernel alone at batch 256 (synthetic ROIs as in bench.py), microseconds per call.
IFCBK_LIB=<other libifcbk.so> times another build on the same box.
--turn: the quarter-turn kernels (flip_bits_valid = 2) beside the flip-only ones (flip_bits_valid = 1), writing the u8 plane only
(the training configuration) and the bf16 tensor: codes all below 4, mixed 0..7, all turned.  Under IFCBK_LIB only the
flip_bits_valid = 1 rows run (that build may predate the transpose bit)."""
import argparse
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ifcb_classifier_amd import _lib
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_rois

ap = argparse.ArgumentParser()
ap.add_argument('--turn', action='store_true', help='time flip_bits_valid = 2 with all-unturned, mixed and all-turned codes')
opts = ap.parse_args()

ctx = _lib.Context(0)


def best_of(fn):
    fn(); torch.cuda.synchronize()
    best = 1e9
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            fn()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / 10)
    return best * 1e3


for S in (299, 224):
    rois, _ = synth_rois(256, 1234, torch.device('cuda'))
    d = _lib.RoiDesc()
    d.n_img, d.S, d.in_channels, d.out_channels, d.dtype, d.flip_bits_valid = 256, S, 1, 8, 0, 0
    for k in range(3):
        d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = 0.0, 1.0, 1.0, 0.0
    ctx.reserve(ctx.lib.ifcbk_roi_preprocess_workspace(C.byref(d), rois['max_h'], rois['max_w']))
    out = torch.empty(256, S, S, 8, dtype=torch.bfloat16, device='cuda')
    if not opts.turn:
        fn = lambda: ctx.call('ifcbk_roi_preprocess', C.byref(d), _lib.ptr(rois['pixels']), _lib.ptr(rois['offs']), _lib.ptr(rois['hs']),
                              _lib.ptr(rois['ws']), None, rois['max_h'], rois['max_w'], _lib.ptr(out), None, _lib.cur_stream())
        print('S=%d  %.1f us per batch of 256 (coeffs + resize), checksum %d' % (S, best_of(fn), int(out.float().sum().item())), flush=True)
        continue
    u8 = torch.empty(256, S, S, dtype=torch.uint8, device='cuda')
    g = torch.Generator().manual_seed(5)
    low = torch.randint(0, 4, (256,), generator=g, dtype=torch.uint8)
    codes = [('flip_bits_valid=1, codes 0..3', 1, low), ('flip_bits_valid=2, codes 0..3', 2, low),
             ('flip_bits_valid=2, codes 0..7', 2, torch.randint(0, 8, (256,), generator=g, dtype=torch.uint8)),
             ('flip_bits_valid=2, codes 4..7', 2, low + 4)]
    if os.environ.get('IFCBK_LIB'):
        codes = codes[:1]
    for what, o, u in (('u8 plane', None, u8), ('bf16 tensor', out, None)):
        for name, valid, fl in codes:
            d.flip_bits_valid = valid
            fl = fl.cuda()
            fn = lambda: ctx.call('ifcbk_roi_preprocess', C.byref(d), _lib.ptr(rois['pixels']), _lib.ptr(rois['offs']), _lib.ptr(rois['hs']),
                                  _lib.ptr(rois['ws']), _lib.ptr(fl), rois['max_h'], rois['max_w'], _lib.ptr(o), _lib.ptr(u), _lib.cur_stream())
            t = best_of(fn)
            print('S=%d  %-11s  %-30s %7.1f us per batch of 256, checksum %d' % (
                S, what, name, t, int((o if o is not None else u).float().sum().item())), flush=True)
