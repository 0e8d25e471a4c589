"""dev tool: ifcbk_batch_mix (TRAIN --mixup / --cutmix, in place) on a batch of 256 at S = 299 -- the u8 plane and the dense bf16 tensor --
beside ifcbk_roi_preprocess on bench.py's 256 synthetic grey ROIs (the resize that writes the plane), and the two-target loss op
(ifcbk_softmax_xent_mix) beside the smoothed one-target op (ifcbk_softmax_xent_ls) at 256 x 100.  The calls alternate; each figure is the
mean of `--calls` timed calls per round after a warm-up, with the spread over the rounds, and the share of the streaming bound it reaches
(one read and one write of the batch at 6 TB/s).  lam stays 0.5 with a box: repeated in-place calls keep mixing the same pairs, which
changes the bytes and not the traffic.  Needs a GPU."""
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
assert torch.cuda.is_available(), 'batch_mix_bench measures on the GPU; there is nothing to time without one'

ctx = _lib.Context(0)
N, S, NC = 256, 299, 100
rois, _ = synth_rois(N, 1234, torch.device('cuda'))
d = _lib.RoiDesc()
d.n_img, d.S, d.in_channels, d.out_channels, d.dtype, d.flip_bits_valid = N, S, 1, 8, 0, 0
for k in range(3):
    d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = 0.0, 1.0, 1.0, 0.0
ctx.reserve(ctx.lib.ifcbk_roi_preprocess_workspace(C.byref(d), rois['max_h'], rois['max_w']))
u8 = torch.empty(N, S, S, dtype=torch.uint8, device='cuda')
dense = torch.randn(N, S, S, 8, device='cuda').to(torch.bfloat16)
lam = torch.full((N,), 0.5, device='cuda')
box = (60, 200, 100, 299)
g = torch.Generator(device='cuda').manual_seed(1)
logits = torch.randn(N, NC, generator=g, device='cuda') * 4
target = torch.randint(0, NC, (N,), generator=g, device='cuda')
cw = torch.rand(NC, generator=g, device='cuda') + 0.1
loss, dl = torch.zeros(1, device='cuda'), torch.zeros(N, NC, device='cuda')
tabs = (_lib.ptr(rois['pixels']), _lib.ptr(rois['offs']), _lib.ptr(rois['hs']), _lib.ptr(rois['ws']))
P, st = _lib.ptr, _lib.cur_stream
calls = {
    'squash (ifcbk_roi_preprocess)': lambda: ctx.call('ifcbk_roi_preprocess', C.byref(d), *tabs, None, rois['max_h'], rois['max_w'], None, P(u8), st()),
    'mix, u8 plane (ifcbk_batch_mix)': lambda: ctx.call('ifcbk_batch_mix', P(u8), _lib.MIX_U8, N, S, P(lam), *box, st()),
    'mix, dense bf16 (ifcbk_batch_mix)': lambda: ctx.call('ifcbk_batch_mix', P(dense), _lib.BF16, N, S, P(lam), *box, st()),
    'smoothed loss (ifcbk_softmax_xent_ls)': lambda: ctx.call('ifcbk_softmax_xent_ls', P(logits), P(target), P(cw), N, NC, 1.0, 0.1, P(loss), 0, P(dl), st()),
    'two-target loss (ifcbk_softmax_xent_mix)': lambda: ctx.call('ifcbk_softmax_xent_mix', P(logits), P(target), P(lam), P(cw), N, NC, 1.0, 0.1, P(loss), 0,
                                                                 P(dl), st()),
}
BOUND_US = {'mix, u8 plane (ifcbk_batch_mix)': 2.0 * N * S * S / 6e12 * 1e6, 'mix, dense bf16 (ifcbk_batch_mix)': 2.0 * N * S * S * 16 / 6e12 * 1e6}


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
for k, t in times.items():
    mean = sum(t) / len(t)
    extra = '  streaming bound %.1f us: %.0f %% of it' % (BOUND_US[k], 100 * BOUND_US[k] / mean) if k in BOUND_US else ''
    print('%-42s %7.1f us per batch of 256 (min %.1f, max %.1f over %d rounds of %d calls)%s' % (k, mean, min(t), max(t), opts.rounds, opts.calls, extra),
          flush=True)
print('checksums: plane %d, dense %.3f, loss %.6f' % (int(u8.long().sum().item()), float(dense.float().abs().sum().item()), float(loss.item())))
