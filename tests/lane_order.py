"""Slowed-lane runs of an engine's own frozen programs (tests/test_gpu_lane_order.py).

A frozen program is an array of ifcbk_op with the lane in flags bits 8-10 and the wait mask in bits 12-19 (OpList.freeze,
ctx.hip::run_lanes).  An IFCBK_OP_MEMSET with wait mask 0 on lane L that writes a scratch buffer nothing else reads changes nothing
but the timing of lane L: `delayed` puts one in front of chosen ops.  Single-lane (flags & 0xff) is plain stream order and needs no
schedule to be right; it is the reference every delayed multi-lane run is compared with, bit for bit.

Before a run everything the step produces is overwritten (`poison`): floating buffers with a NaN pattern of their storage type, so a
consumer that runs ahead of its producer computes NaN instead of last step's plausible value; integer buffers a kernel turns into an
address (arg-max planes) with the in-range value 0.  Not poisoned, each for its reason:
  input slots [B,S,S,8]   written by load_input_nchw before every run, pad channels included (zeros): inputs, not products
  targets, dropout masks  inputs of the step (set / drawn before it), and bytes that kernels index with
  ones / zeros_k          constants (scale 1 / bias 0 of a conv without BatchNorm), written once at allocation
  class weights           an input
  Wsh of squeezenet1_1    the classifier's output channels are padded to a 16-byte chunk; the shadow rows behind the true ones are
                          zero from allocation and no pack op rewrites them (engine._pack_desc) -- everywhere else Wsh is poisoned
  G between tensors       every tensor of the flat gradient buffer is poisoned, the 16-byte alignment padding between two is not:
                          no op writes it and the optimizer's flat launch reads it (zeros from allocation)
  G of a vgg*_bn conv bias  in front of a BatchNorm the bias has an identically zero gradient and no op writes it (Engine.cbias_after): like
                          the padding, zeros from allocation that the optimizer and the data-parallel exchange read
  the ctx workspace       private to the library (per-lane arenas), not reachable from Python
"""
import ctypes as C
import random

import torch

from ifcb_classifier_amd import _lib
from ifcb_classifier_amd._lib import Op


def lanes_of(arr, n):
    return sorted({(arr[k].flags >> 8) & 7 for k in range(n)})


def single_lane(arr, n):
    out = (Op * n)(*arr)
    for k in range(n):
        out[k].flags &= 0xff
    return out


def delayed(arr, n, where, scratch, nbytes, reps=1):
    """a copy of arr with a delay (reps memsets on the lane of the op behind them, wait mask 0) in front of every op index in `where`"""
    where = set(where)
    ops = []
    for k in range(n):
        if k in where:
            d = Op()
            d.kind, d.flags = _lib.OP_MEMSET, arr[k].flags & 0x700
            d.p[0], d.i[0], d.i[1] = scratch.data_ptr(), int(nbytes), 0
            ops += [d] * reps
        ops.append(arr[k])
    return (Op * len(ops))(*ops), len(ops)


def patterns(arr, n):
    """-> {name: op indices to delay}: every op of lane L, for each lane that holds ops; three seeded random quarters"""
    out = {}
    for L in lanes_of(arr, n):
        out['slow%d' % L] = [k for k in range(n) if (arr[k].flags >> 8) & 7 == L]
    for seed in (1, 2, 3):
        rng = random.Random(seed)
        out['rand%d' % seed] = [k for k in range(n) if rng.random() < 0.25]
    return out


def snapshot(eng):
    return dict(P=eng.P.clone(), M=eng.M.clone(), V=eng.V.clone(), RB=eng.RB.clone(), nbt=eng.nbt.clone(), loss_sum=eng.loss_sum.clone(),
                step_count=eng.step_count, dropout_seed=eng.dropout_seed, dropout_calls=eng.dropout_calls)


def restore(eng, snap):
    for k in ('P', 'M', 'V', 'RB', 'nbt', 'loss_sum'):
        getattr(eng, k).copy_(snap[k])
    eng.step_count, eng.dropout_seed, eng.dropout_calls = snap['step_count'], snap['dropout_seed'], snap['dropout_calls']
    eng.packed = False                      # the bf16 shadows are rebuilt from the restored P
    eng.eval_stats_ready = False


def _nan(t):
    if t.dtype == torch.bfloat16:
        t.view(torch.int16).fill_(0x7fc1)
    elif t.dtype == torch.float32:
        t.view(torch.int32).fill_(0x7fc00001)
    else:
        raise TypeError(t.dtype)


def nan_fill(t):
    """the poison of a floating buffer, also for a slice of one (the rows behind a partial batch: tests/engine_life.py)"""
    _nan(t)


def holds_nan_fill(t):
    """every element still is the pattern nan_fill wrote"""
    if t.dtype == torch.bfloat16:
        return bool((t.view(torch.int16) == 0x7fc1).all())
    if t.dtype == torch.float32:
        return bool((t.view(torch.int32) == 0x7fc00001).all())
    raise TypeError(t.dtype)


def produced_buffers(eng):
    """-> ([(name, floating tensor)], [(name, integer tensor)]) of everything a train step or an eval forward writes"""
    fl, it = [], []
    inputs = {b.data_ptr() for b in eng.in_bufs}
    for bid, t in eng.act.items():
        if t.data_ptr() not in inputs and t.is_contiguous():
            fl.append(('act[%d]' % bid, t))
    fl += [('grad[%d]' % bid, t) for bid, t in eng.grad.items()]
    fl += [('group[%d].raw' % k, g.raw) for k, g in enumerate(eng.groups)]
    fl += [('draw[%d]' % k, t) for k, t in enumerate(eng.draw)] + [('draw_group', eng.draw_group)]
    if getattr(eng, '_draw_pool', None) is not None:
        fl.append(('_draw_pool', eng._draw_pool))
    pool = getattr(eng, '_draw_pool', None)
    for m, t in getattr(eng, 'draw_own', {}).items():
        if pool is None or t.untyped_storage().data_ptr() != pool.untyped_storage().data_ptr():
            fl.append(('draw_own[%s]' % m.name, t))
    for k, g in enumerate(eng.groups):
        t = getattr(g, 'draw_own', None)
        if t is not None and (pool is None or t.untyped_storage().data_ptr() != pool.untyped_storage().data_ptr()):
            fl.append(('group[%d].draw_own' % k, t))
    # G per parameter tensor: the alignment padding between two tensors is written by nothing and read by the optimizer's flat launch
    # (... and neither is the gradient of a conv bias in front of a BatchNorm)
    fl += [('G[%s]' % key, eng.G[o:o + n]) for key, (o, n, _shape, kind, _node) in eng.poff.items() if kind != 'bn_cbias']
    fl += [('stats', eng.stats)] + [('bn_part[%d]' % k, t) for k, t in enumerate(eng.bn_part)]
    if all(n.K == n.K_real for n in eng.plains):
        fl.append(('Wsh', eng.Wsh))
    for h in eng.heads:
        fl += [(h.name + '.feat', h.feat), (h.name + '.logits', h.logits), (h.name + '.dlogits', h.dlogits)]
    fl += [('probs', eng.probs), ('loss', eng.loss)]
    it += [('argmax[%d]' % k, t) for k, t in eng.argmax.items()]
    return fl, it


def poison(eng, clean=False):
    """clean: what freshly allocated buffers hold (zeros) instead of NaN"""
    fl, it = produced_buffers(eng)
    for _name, t in fl:
        if clean:
            t.zero_()
        else:
            _nan(t)
    for _name, t in it:
        t.zero_()                           # arg-max bytes select an address: an in-range wrong value


def run_step(eng, pl, B, x, y, make_arr, op_ms=None):
    """one train step through Context.run_program on the engine's stream; make_arr(step array, n) -> (array, n) to launch"""
    eng.load_input_nchw(x)
    eng.target[:B].copy_(y)
    eng.ensure_packed(pl)
    eng.make_dropout_mask(B)
    eng.step_count += 1
    for j in pl.step_adam_idxs:
        eng._set_update(pl.step.arr[j])
    arr, n = make_arr(pl.step.arr, pl.step.n)
    ms = (C.c_float * n)() if op_ms else None
    eng.ctx.run_program(arr, n, eng.stream(), ms)
    torch.cuda.synchronize()
    return list(ms) if op_ms else None


def run_eval(eng, pl, B, x, make_arr):
    eng.load_input_nchw(x)
    eng.ensure_packed(pl)
    eng.run(pl.evalprep)
    arr, n = make_arr(pl.fwd_eval.arr, pl.fwd_eval.n)
    eng.ctx.run_program(arr, n, eng.stream(), None)
    torch.cuda.synchronize()


def outcome(eng):
    """what a step leaves behind, cloned: compared with torch.equal on the raw bits (NaN-safe through an integer view)"""
    out = dict(loss=eng.loss, G=eng.G, P=eng.P, RB=eng.RB, M=eng.M, V=eng.V)
    for h in eng.heads:
        out[h.name + '.logits'] = h.logits
    return {k: v.clone() for k, v in out.items()}


def step_outcome(eng):
    """outcome plus the bookkeeping a step's last op writes: num_batches_tracked of every BatchNorm and the running loss sum"""
    out = outcome(eng)
    out['nbt'], out['loss_sum'] = eng.nbt.clone(), eng.loss_sum.clone()
    return out


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def differing(a, b):
    return [k for k in a if not same_bits(a[k], b[k])]


def size_delay(eng, longest_ms, cap=1 << 30):
    """-> (scratch, bytes, reps, measured ms of one delay alone): the memset grown to `cap`, then repeated back to back, until the delay
    takes at least as long as the longest op"""
    nbytes, reps = 32 << 20, 1
    while True:
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=eng.dev)
        d = Op()
        d.kind = _lib.OP_MEMSET
        d.p[0], d.i[0], d.i[1] = scratch.data_ptr(), nbytes, 0
        arr = (Op * (3 * reps))(*([d] * (3 * reps)))
        best = None
        for _ in range(2):                  # the first launch of a size pays its set-up
            ms = (C.c_float * (3 * reps))()
            eng.ctx.run_program(arr, 3 * reps, eng.stream(), ms)
            best = min(sum(ms[k * reps:(k + 1) * reps]) for k in range(3))
        if best >= longest_ms or reps >= 8:
            return scratch, nbytes, reps, best
        if nbytes < cap:
            del scratch
            nbytes *= 2
        else:
            reps += 1
