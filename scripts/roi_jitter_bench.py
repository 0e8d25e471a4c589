"""dev tool: ifcbk_roi_jitter (TRAIN --jitter, brightness and contrast, in place) beside ifcbk_roi_preprocess on the same batch of 256 grey
synthetic ROIs (bench.py's input, none larger than 299), S = 299, the resize writing the u8 plane only (the training configuration).
The two calls alternate; each figure is the mean of `--calls` timed calls per round after a warm-up, with the spread over the rounds.
The factors are redrawn around 1 with a small range so that repeated in-place calls do not run the blob into one level.  Needs a GPU."""
import argparse
import ctypes as C
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ifcb_classifier_amd import _lib
from bench import synth_rois

ap = argparse.ArgumentParser()
ap.add_argument('--calls', type=int, default=20, help='timed calls per round')
ap.add_argument('--rounds', type=int, default=7)
opts = ap.parse_args()
assert torch.cuda.is_available(), 'roi_jitter_bench measures on the GPU; there is nothing to time without one'

ctx = _lib.Context(0)
S = 299
rois, _ = synth_rois(256, 1234, torch.device('cuda'))
assert rois['max_h'] <= S and rois['max_w'] <= S
d = _lib.RoiDesc()
d.n_img, d.S, d.in_channels, d.out_channels, d.dtype, d.flip_bits_valid = 256, S, 1, 8, 0, 0
for k in range(3):
    d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = 0.0, 1.0, 1.0, 0.0
ctx.reserve(max(ctx.lib.ifcbk_roi_preprocess_workspace(C.byref(d), rois['max_h'], rois['max_w']), ctx.lib.ifcbk_roi_jitter_workspace(256)))
u8 = torch.empty(256, S, S, dtype=torch.uint8, device='cuda')
g = torch.Generator(device='cuda').manual_seed(1)
fb = 1 + (torch.rand(256, generator=g, device='cuda') - 0.5) * 0.02
fc = 1 + (torch.rand(256, generator=g, device='cuda') - 0.5) * 0.02
tabs = (_lib.ptr(rois['pixels']), _lib.ptr(rois['offs']), _lib.ptr(rois['hs']), _lib.ptr(rois['ws']))
calls = {
    'squash (ifcbk_roi_preprocess)': lambda: ctx.call('ifcbk_roi_preprocess', C.byref(d), *tabs, None, rois['max_h'], rois['max_w'], None,
                                                      _lib.ptr(u8), _lib.cur_stream()),
    'jitter, both factors (ifcbk_roi_jitter)': lambda: ctx.call('ifcbk_roi_jitter', *tabs, 256, 1, rois['max_h'], rois['max_w'], _lib.ptr(fb),
                                                                _lib.ptr(fc), _lib.ptr(rois['pixels']), _lib.cur_stream()),
}
print('%d source bytes in 256 ROIs' % int((rois['hs'].long() * rois['ws'].long()).sum().item()), flush=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(opts.calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / opts.calls * 1e3


for fn in calls.values():                       # warm-up: code objects, the workspace
    for _ in range(5):
        fn()
torch.cuda.synchronize()
times = {k: [] for k in calls}
for _ in range(opts.rounds):
    for k, fn in calls.items():
        times[k].append(timed(fn))
mean = {}
for k, t in times.items():
    mean[k] = sum(t) / len(t)
    print('%-42s %7.1f us per batch of 256 (min %.1f, max %.1f over %d rounds of %d calls)' % (k, mean[k], min(t), max(t), opts.rounds, opts.calls),
          flush=True)
print('checksums: plane %d, blob %d' % (int(u8.long().sum().item()), int(rois['pixels'].long().sum().item())))
print('jitter / squash = %.3f' % (mean['jitter, both factors (ifcbk_roi_jitter)'] / mean['squash (ifcbk_roi_preprocess)']))
