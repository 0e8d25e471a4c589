#!/usr/bin/env python
"""what TRAIN --accumulate costs on the device, two same-process, interleaved comparisons timed with device events:

1. the pass: ifcbk_grad_accum_flat (first = 0) against ifcbk_ema_flat over the same n = inception_v3's nparam_padded -- both move 12 B
   per element with one 16-byte load per operand and one 16-byte store per thread -- as LAUNCHES back-to-back launches per event pair,
   alternating between the two kernels for ROUNDS rounds; medians, their ratio, and the achieved GB/s of each.
2. the step: inception_v3 bf16 at batch 256, Engine(accumulate=1).train_step against the mean time per batch of
   Engine(accumulate=4).train_step (whole windows), BATCHES batches per event pair, alternating for ROUNDS rounds.

    python scripts/accumulate_cost.py [--rounds 10] [--launches 200] [--batches 20] [--batch 256] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ifcb_classifier_amd import _lib, graph                                     # noqa: E402
from ifcb_classifier_amd.engine import Engine                                   # noqa: E402


def timed(fn):
    """milliseconds of fn() between two events on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def kernel_cost(n, rounds, launches):
    ctx = _lib.Context(0)
    bufs = [torch.randn(n, device='cuda') for _ in range(4)]
    P, st = _lib.ptr, _lib.cur_stream
    runs = {'ema_flat': lambda: ctx.call('ifcbk_ema_flat', P(bufs[0]), P(bufs[1]), n, 0.5, st()),
            'grad_accum_flat': lambda: ctx.call('ifcbk_grad_accum_flat', P(bufs[2]), P(bufs[3]), n, 0, st())}
    bufs[3].mul_(1e-6)                      # (the sum of `launches` adds stays finite)
    ms = {k: [] for k in runs}
    for fn in runs.values():
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, fn in runs.items():
            ms[name].append(timed(lambda: [fn() for _ in range(launches)]) / launches)
    ctx.close()
    out = {}
    for name, v in ms.items():
        med = statistics.median(v)
        out[name] = dict(us=round(med * 1e3, 2), us_min=round(min(v) * 1e3, 2), us_max=round(max(v) * 1e3, 2),
                         GBps=round(12.0 * n / (med * 1e-3) / 1e9, 1))
    out['ratio'] = round(out['grad_accum_flat']['us'] / out['ema_flat']['us'], 4)
    return out


def step_cost(batch, rounds, batches, K=4):
    assert batches % K == 0, 'whole windows only'
    g = torch.Generator().manual_seed(0)
    x = torch.rand(batch, 3, 299, 299, generator=g).cuda()
    y = torch.randint(0, 10, (batch,), generator=g)
    engs = {}
    for name, kw in (('train_step', {}), ('accumulate=%d, per batch' % K, dict(accumulate=K))):
        # (a graph per engine: an engine keeps its layout on the graph's nodes)
        eng = Engine(graph.build('inception_v3', 10, pretrained=False), 0, max_batch=batch, dtype='bf16', **kw)
        eng.init_weights(seed=1)
        eng.load_input_nchw(x)
        eng.target[:batch].copy_(y)
        for _ in range(2 * K):
            eng.train_step(batch)
        engs[name] = eng
    torch.cuda.synchronize()
    ms = {k: [] for k in engs}
    for _ in range(rounds):
        for name, eng in engs.items():
            ms[name].append(timed(lambda: [eng.train_step(batch) for _ in range(batches)]) / batches)
    out = {name: dict(ms=round(statistics.median(v), 3), ms_min=round(min(v), 3), ms_max=round(max(v), 3)) for name, v in ms.items()}
    out['nparam_padded'] = engs['train_step'].nparam_padded
    for eng in engs.values():
        assert eng.acc_pending == 0
        eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('accumulate_cost: needs the GPU; nothing is measured without one')
    res = dict(device=torch.cuda.get_device_name(0), step=step_cost(a.batch, a.rounds, a.batches))
    res['kernel'] = kernel_cost(res['step']['nparam_padded'], a.rounds, a.launches)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
