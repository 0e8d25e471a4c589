"""dev tool: the inception_v3 / batch 256 / bf16 train step FED the way neuston_net.Trainer feeds it -- every step uploads a pinned host
batch (bench.py's 256 synthetic grey ROIs), resizes it on the prefetch stream into the other input slot while the step in flight
computes, then steps -- without and with `--blur SIGMA_MAX` (every image drawn: --blur-prob 1, sigma uniform in [0.1, SIGMA_MAX]).
Prints the median and range of `--rounds` runs of `--steps` steps, wall clock around a synchronised run.  `--blur 0` passes no sigmas
and never names the blur, so the same file times a commit that does not have it.  Needs a GPU."""
import argparse
import math
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from bench import synth_rois

ap = argparse.ArgumentParser()
ap.add_argument('--blur', type=float, default=0.0, help='SIGMA_MAX; 0 = no blur (and no blur argument anywhere)')
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--warmup', type=int, default=8)
opts = ap.parse_args()
assert torch.cuda.is_available(), 'blur_step_bench measures on the GPU; there is nothing to time without one'

from ifcb_classifier_amd import graph
from ifcb_classifier_amd.engine import Engine
B = 256
kw = dict(blur_radius=int(math.ceil(3 * opts.blur))) if opts.blur > 0 else {}
eng = Engine(graph.build('inception_v3', 100, pretrained=False), device=0, max_batch=B, **kw)
eng.init_weights(seed=1234)
rois, _ = synth_rois(B, 1234, eng.dev)
eng.target[:B].copy_(torch.randint(0, 100, (B,), generator=torch.Generator().manual_seed(99)))
for tb in eng.tgt_bufs:
    tb[:B].copy_(eng.target[:B])
hostb = {k: (v.cpu().pin_memory() if torch.is_tensor(v) else v) for k, v in rois.items()}
if opts.blur > 0:
    g = torch.Generator().manual_seed(5)
    hostb['blur'] = (0.1 + torch.rand(B, generator=g) * (opts.blur - 0.1)).float().pin_memory()


def stage():
    slot, side = eng.prefetch_begin()
    with torch.cuda.stream(side):
        eng.load_rois(slot=slot, **{k: (v.to(eng.dev, non_blocking=True) if torch.is_tensor(v) else v) for k, v in hostb.items()})
    eng.prefetch_end(slot)


def step():
    eng.use_prefetched()
    stage()
    eng.train_step(B)


stage()
for _ in range(opts.warmup):
    step()
torch.cuda.synchronize()
ms = []
for _ in range(opts.rounds):
    t0 = time.perf_counter()
    for _ in range(opts.steps):
        step()
    torch.cuda.synchronize()
    ms.append(1e3 * (time.perf_counter() - t0) / opts.steps)
ms.sort()
print('fed step, blur %g: median %.3f ms (min %.3f, max %.3f over %d rounds of %d steps), loss %.5f'
      % (opts.blur, ms[len(ms) // 2], ms[0], ms[-1], opts.rounds, opts.steps, float(eng.loss.item())), flush=True)
