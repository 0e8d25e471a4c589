"""dev tool: the ROI preprocess kernel alone at batch 256 (synthetic ROIs as in bench.py), microseconds per call.
IFCBK_LIB=<other libifcbk.so> times another build on the same box.
--turn: the quarter-turn kernels (flip_bits_valid = 2) beside the flip-only ones (flip_bits_valid = 1), writing the u8 plane only
(the training configuration) and the bf16 tensor: codes all below 4, mixed 0..7, all turned.
--general: the one-block-per-output-row kernels, which bench.py's batch never reaches, on two seeded batches of 256 at S = 299 --
grey ROIs of 150..598 pixels a side (kmax 5: the LDS-staged rows) and RGB ROIs of 32..299 (global loads per tap) -- through the
squash call without codes, with quarter-turn codes 0..7, and through ifcbk_roi_preprocess_fit; u8 plane only."""
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
ap.add_argument('--general', action='store_true', help='time roi_resize_kernel, roi_turn_resize_kernel and roi_fit_resize_kernel')
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


def general_batch(lo, hi, cin, seed):
    g = torch.Generator().manual_seed(seed)
    hs = torch.randint(lo, hi + 1, (256,), generator=g, dtype=torch.int32)
    ws = torch.randint(lo, hi + 1, (256,), generator=g, dtype=torch.int32)
    sizes = hs.long() * ws.long() * cin
    offs = torch.zeros(256, dtype=torch.int64)
    offs[1:] = torch.cumsum(sizes, 0)[:-1]
    pix = torch.randint(0, 256, (int(sizes.sum()),), generator=g, dtype=torch.uint8)
    return dict(pixels=pix.cuda(), offs=offs.cuda(), hs=hs.cuda(), ws=ws.cuda(), max_h=int(hs.max()), max_w=int(ws.max()))


if opts.general:
    S = 299
    codes = torch.randint(0, 8, (256,), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).cuda()
    u8 = torch.empty(256, S, S, 3, dtype=torch.uint8, device='cuda')
    for batch, cin, rois in (('grey 150..598 (kmax 5)', 1, general_batch(150, 2 * S, 1, 21)), ('RGB 32..299', 3, general_batch(32, S, 3, 22))):
        d = _lib.RoiDesc()
        d.n_img, d.S, d.in_channels, d.out_channels, d.dtype = 256, S, cin, 8, 0
        for k in range(3):
            d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = 0.0, 1.0, 1.0, 0.0
        ctx.reserve(max(ctx.lib.ifcbk_roi_preprocess_workspace(C.byref(d), rois['max_h'], rois['max_w']),
                        ctx.lib.ifcbk_roi_preprocess_fit_workspace(C.byref(d), rois['max_h'], rois['max_w'])))
        args = (C.byref(d), _lib.ptr(rois['pixels']), _lib.ptr(rois['offs']), _lib.ptr(rois['hs']), _lib.ptr(rois['ws']))
        dims = (rois['max_h'], rois['max_w'])
        for name, valid, fn in (
                ('roi_resize_kernel', 0, lambda: ctx.call('ifcbk_roi_preprocess', *args, None, *dims, None, _lib.ptr(u8), _lib.cur_stream())),
                ('roi_turn_resize_kernel', 2, lambda: ctx.call('ifcbk_roi_preprocess', *args, _lib.ptr(codes), *dims, None, _lib.ptr(u8), _lib.cur_stream())),
                ('roi_fit_resize_kernel', 2, lambda: ctx.call('ifcbk_roi_preprocess_fit', *args, _lib.ptr(codes), *dims, -1, None, _lib.ptr(u8), _lib.cur_stream()))):
            d.flip_bits_valid = valid
            t = best_of(fn)
            print('general  %-24s %-24s %8.1f us per batch of 256, checksum %d' % (batch, name, t, int(u8.view(-1)[:256 * S * S * cin].long().sum().item())), flush=True)
    sys.exit(0)

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
    for what, o, u in (('u8 plane', None, u8), ('bf16 tensor', out, None)):
        for name, valid, fl in codes:
            d.flip_bits_valid = valid
            fl = fl.cuda()
            fn = lambda: ctx.call('ifcbk_roi_preprocess', C.byref(d), _lib.ptr(rois['pixels']), _lib.ptr(rois['offs']), _lib.ptr(rois['hs']),
                                  _lib.ptr(rois['ws']), _lib.ptr(fl), rois['max_h'], rois['max_w'], _lib.ptr(o), _lib.ptr(u), _lib.cur_stream())
            t = best_of(fn)
            print('S=%d  %-11s  %-30s %7.1f us per batch of 256, checksum %d' % (
                S, what, name, t, int((o if o is not None else u).float().sum().item())), flush=True)
