"""dev tool: the cost of RUN --tta at batch 2048, all in one session on one GPU.
  1. one ifcbk_batch_sym pass per op and kind: the u8 plane at S = 299 (inception_v3's u8-stem route) and the dense bf16 / fp32 tensor at
     S = 224 (resnet18's route), with the share of the streaming bound (one read and one write of the batch at 6 TB/s);
  2. ifcbk_softmax_acc beside ifcbk_softmax at 2048 x --classes;
  3. RUN-style images/s of inception_v3 bf16 and resnet18 bf16 on bench.py's synthetic grey ROIs -- per batch the on-GPU resize, then
     the plain eval forward + softmax (the path of a RUN without the flag, whose code this feature leaves alone), or the sequence of
     NeustonModel.eval_current_tta for 'flips' and 'all'; the three alternate round by round.  The condition of the feature: the
     'all' rate is at least 1/8 of the plain rate less 5 %.
Each figure is a mean over `--rounds` rounds after a warm-up, with the spread.  Needs a GPU."""
import argparse
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ifcb_classifier_amd import _lib, graph
from ifcb_classifier_amd.engine import Engine
from bench import synth_rois

ap = argparse.ArgumentParser()
ap.add_argument('--batch', type=int, default=2048)
ap.add_argument('--classes', type=int, default=100)
ap.add_argument('--calls', type=int, default=20, help='timed kernel calls per round')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--batches', type=int, default=6, help='timed plain batches per round (the views take 4 and 8 forwards each)')
ap.add_argument('--models', default='inception_v3,resnet18')
opts = ap.parse_args()
assert torch.cuda.is_available(), 'tta_bench measures on the GPU; there is nothing to time without one'
N, NC = opts.batch, opts.classes
P, st = _lib.ptr, _lib.cur_stream
OPS = (('hflip', _lib.SYM_HFLIP), ('vflip', _lib.SYM_VFLIP), ('transpose', _lib.SYM_TRANSPOSE))


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def report(calls, bound_us=None):
    for fn in calls.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(opts.rounds):
        for k, fn in calls.items():
            times[k].append(timed(fn, opts.calls))
    for k, t in times.items():
        mean = sum(t) / len(t)
        extra = '  streaming bound %.1f us: %.0f %% of it' % (bound_us[k], 100 * bound_us[k] / mean) if bound_us and k in bound_us else ''
        print('%-44s %8.1f us (min %.1f, max %.1f over %d rounds of %d calls)%s' % (k, mean, min(t), max(t), opts.rounds, opts.calls, extra), flush=True)


# ---- 1. the passes
ctx = _lib.Context(0)
bufs = {'u8 plane S 299': (torch.randint(0, 256, (N, 299, 299), dtype=torch.uint8, device='cuda'), _lib.MIX_U8, 299, 1),
        'dense bf16 S 224': (torch.randn(N, 224, 224, 8, device='cuda').to(torch.bfloat16), _lib.BF16, 224, 16),
        'dense fp32 S 224': (torch.randn(N, 224, 224, 8, device='cuda'), _lib.F32, 224, 32)}
calls, bound = {}, {}
for name, (buf, kind, S, pix) in bufs.items():
    for opn, op in OPS:
        k = 'batch_sym %s, %s' % (opn, name)
        calls[k] = lambda buf=buf, kind=kind, S=S, op=op: ctx.call('ifcbk_batch_sym', P(buf), kind, N, S, op, st())
        bound[k] = 2.0 * N * S * S * pix / 6e12 * 1e6
print('batch %d' % N)
report(calls, bound)
del bufs, calls
torch.cuda.empty_cache()

# ---- 2. the accumulating softmax
logits = torch.randn(N, NC, device='cuda') * 4
acc = torch.zeros(N, NC, device='cuda')
report({'ifcbk_softmax %d x %d' % (N, NC): lambda: ctx.call('ifcbk_softmax', P(logits), N, NC, P(acc), st()),
        'ifcbk_softmax_acc %d x %d' % (N, NC): lambda: ctx.call('ifcbk_softmax_acc', P(logits), N, NC, P(acc), 1, 0.125, st())})
ctx.close()


# ---- 3. whole batches
def tta(eng, B, mode):
    """NeustonModel.eval_current_tta's sequence on the engine"""
    walk = eng.TTA_WALKS[mode]
    eng.forward_eval(B)
    eng.softmax_acc(B, first=True)
    for k, op in enumerate(walk):
        eng.sym_batch(B, op)
        eng.forward_eval(B)
        eng.softmax_acc(B, first=False, scale=1.0 / (len(walk) + 1) if k == len(walk) - 1 else 1.0)
    return eng.probs[:B].clone()


def plain(eng, B, mode):
    pl = eng.forward_eval(B)
    eng.run(pl.softmax)
    return eng.probs[:B].clone()


POOL = 4096
for name in opts.models.split(','):
    eng = Engine(graph.build(name, NC, pretrained=False), device=0, max_batch=N, train_batch=1)
    eng.init_weights(seed=1234)
    B = min(N, eng.max_batch)
    rois, _ = synth_rois(POOL + B, 4321, eng.dev)

    def run(fn, mode, nb):
        def batch(k):
            s0 = (k * B) % POOL
            eng.load_rois(rois['pixels'], rois['offs'][s0:s0 + B], rois['hs'][s0:s0 + B], rois['ws'][s0:s0 + B], rois['max_h'], rois['max_w'])
            return fn(eng, B, mode)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(nb):
            batch(k)
        torch.cuda.synchronize()
        return nb * B / (time.perf_counter() - t0)

    legs = {'plain': (plain, None, opts.batches), 'flips': (tta, 'flips', max(1, opts.batches // 2)), 'all': (tta, 'all', max(1, opts.batches // 3))}
    for fn, mode, _ in legs.values():                  # warm-up: plans, graphs, code objects
        run(fn, mode, 1)
    rates = {k: [] for k in legs}
    for _ in range(opts.rounds):
        for k, (fn, mode, nb) in legs.items():
            rates[k].append(run(fn, mode, nb))
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    print('%s bf16, batch %d, input route %s, hipGraph eval %s' % (name, B, eng.in_kind[eng.in_slot], bool(eng.graph_eval)))
    for k, v in rates.items():
        print('  %-6s %9.1f images/s (min %.1f, max %.1f over %d rounds)' % (k, mean[k], min(v), max(v), opts.rounds), flush=True)
    for k, V in (('flips', 4), ('all', 8)):
        print('  %-6s is %.4f of plain / %d  (%+.2f %% against %d forwards; the condition for all: >= 0.95)'
              % (k, mean[k] * V / mean['plain'], V, 100 * (mean[k] * V / mean['plain'] - 1), V))
    eng.close()
    del eng, rois
    torch.cuda.empty_cache()
