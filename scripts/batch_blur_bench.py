"""dev tool: ifcbk_batch_blur (TRAIN --blur, in place) on a batch of 256 at S = 299 -- the u8 plane and the dense bf16 tensor, radius 6
and 12, every image drawn (sigma = radius / 3) -- beside ifcbk_roi_preprocess on bench.py's 256 synthetic grey ROIs (the resize that
writes the plane).  The calls alternate; each figure is the mean of `--calls` timed calls per round after a warm-up, with the spread over
the rounds, and the bytes per second of one read and one write of what the pass touches (the whole plane; of the dense tensor the three
image channels).  Repeated in-place calls keep blurring the same images, which changes the bytes and not the work.  `--once` makes one
call of each form and radius behind the warm-up, for a kernel trace.  Needs a GPU."""
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
ap.add_argument('--once', action='store_true', help='one call of each blur form behind the warm-up, nothing timed (for a kernel trace)')
opts = ap.parse_args()
assert torch.cuda.is_available(), 'batch_blur_bench measures on the GPU; there is nothing to time without one'

ctx = _lib.Context(0)
N, S = 256, 299
rois, _ = synth_rois(N, 1234, torch.device('cuda'))
d = _lib.RoiDesc()
d.n_img, d.S, d.in_channels, d.out_channels, d.dtype, d.flip_bits_valid = N, S, 1, 8, 0, 0
for k in range(3):
    d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = 0.0, 1.0, 1.0, 0.0
ctx.reserve(ctx.lib.ifcbk_roi_preprocess_workspace(C.byref(d), rois['max_h'], rois['max_w']))
u8 = torch.empty(N, S, S, dtype=torch.uint8, device='cuda')
dense = torch.randn(N, S, S, 8, device='cuda').to(torch.bfloat16)
sig = {r: torch.full((N,), r / 3.0, device='cuda') for r in (6, 12)}
tabs = (_lib.ptr(rois['pixels']), _lib.ptr(rois['offs']), _lib.ptr(rois['hs']), _lib.ptr(rois['ws']))
P, st = _lib.ptr, _lib.cur_stream
calls = {'squash (ifcbk_roi_preprocess)': lambda: ctx.call('ifcbk_roi_preprocess', C.byref(d), *tabs, None, rois['max_h'], rois['max_w'], None, P(u8), st())}
BYTES = {}
for r in (6, 12):
    calls['blur r %d, u8 plane' % r] = lambda r=r: ctx.call('ifcbk_batch_blur', P(u8), _lib.MIX_U8, N, S, P(sig[r]), r, st())
    calls['blur r %d, dense bf16' % r] = lambda r=r: ctx.call('ifcbk_batch_blur', P(dense), _lib.BF16, N, S, P(sig[r]), r, st())
    BYTES['blur r %d, u8 plane' % r] = 2.0 * N * S * S
    BYTES['blur r %d, dense bf16' % r] = 2.0 * N * S * S * 3 * 2


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(opts.calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / opts.calls * 1e3


for fn in calls.values():                       # warm-up: code objects, the workspace
    for _ in range(3):
        fn()
torch.cuda.synchronize()
if opts.once:
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    sys.exit(0)
times = {k: [] for k in calls}
for _ in range(opts.rounds):
    for k, fn in calls.items():
        times[k].append(timed(fn))
for k, t in times.items():
    mean = sum(t) / len(t)
    extra = '  %.2f TB/s of image bytes read + written' % (BYTES[k] / (mean * 1e-6) / 1e12) if k in BYTES else ''
    print('%-32s %8.1f us per batch of 256 (min %.1f, max %.1f over %d rounds of %d calls)%s' % (k, mean, min(t), max(t), opts.rounds, opts.calls, extra),
          flush=True)
print('checksums: plane %d, dense %.3f' % (int(u8.long().sum().item()), float(dense.float().abs().sum().item())))
