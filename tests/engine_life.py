"""One engine's whole life against a fresh engine's bits (tests/test_gpu_engine_life.py, tests/test_engine_life_cpu.py).

A TRAIN run feeds one engine full batches, a partial batch, validation batches of other sizes and then trains on: every plan of
Engine.plan(N) runs on the buffers allocated once for max_batch, and what is valid is kept in host-side flags (packed,
eval_stats_ready, in_kind[slot], the per-plan graphs).  The reference of every scenario is a FRESH engine of capacity N that was
given the same state (lane_order.restore of the long-lived engine's snapshot) and has only ever seen that one batch.

Raw bits can be demanded because the plan of N does not depend on the capacity: tests/test_engine_life_cpu.py compares the
canonical plan text of a capacity-B engine with that of a capacity-N engine for every (family, B, N, dtype) used here.

Before a partial batch runs on the long-lived engine everything behind image N is made hostile, yet in range:
  products of a step          lane_order.poison: NaN patterns over whole tensors, rows >= N included
  arg-max planes, rows >= N   ARG_TAIL (a window index every pool here has; rows < N get lane_order.poison's 0)
  the input slot behind N     NaN in the dense tensor, TAIL_BYTE in the u8 plane; the representation that is not current is
                              overwritten whole (the u8 stem must not read the dense tensor, and the other way round)
  target[N:]                  JUNK, a valid class no label uses (labels are drawn from 0 .. NC - 2)
  dropout masks, rows >= N    0 or 1, the caller's choice per run (the rows in use hold a mix of both)
Nothing of this can fault: no index leaves its range, rows >= N exist in every buffer of the long-lived engine."""
import re

import numpy as np
import torch

import lane_order as lo

NC = 7
JUNK = NC - 1
TAIL_BYTE = 0xA5
ARG_TAIL = 1

# family -> (graph.build name, capacity B of the long-lived engine, input side): the smallest shapes at which each plan has its full
# op list (tests/test_gpu_step_modes.py::FAMILIES; squeezenet1_1 at the batch of tests/test_gpu_families.py::CASES)
FAMILIES = {'inception_v3': ('inception_v3', 6, 299), 'resnet18': ('resnet18', 8, 224), 'squeezenet1_1': ('squeezenet', 4, 224)}
# partial sizes: B - 1 (odd for resnet18), for inception also 3 (odd, with a middle image), 2, and 1.  resnet18 also 5: the batch whose
# BatchNorm partial sums take more rows than those of the capacity 8 (tests/test_engine_life_cpu.py)
PARTIAL = {'inception_v3': (5, 3, 2, 1), 'resnet18': (7, 5, 2, 1), 'squeezenet1_1': (3, 2, 1)}
# inception first: the inception-only scenarios parametrise over a prefix of this list
PAIRS = ['%s-%d' % (f, n) for f in ('inception_v3', 'resnet18', 'squeezenet1_1') for n in PARTIAL[f]]
INCEPTION_PAIRS = [p for p in PAIRS if p.startswith('inception_v3-')]
DTYPES = ('bf16', 'fp32')                       # bf16: every scenario; fp32: the oracle anchor


# ---------------------------------------------------------------------------------------------- plan identity (CPU)
def carves(eng):
    """[(first byte, bytes, name)] of the d(raw) tensors carved out of the engine's pooled allocation (Engine._carve)"""
    pool = getattr(eng, '_draw_pool', None)
    if pool is None:
        return []
    base, es = pool.data_ptr(), pool.element_size()
    end = base + pool.numel() * es
    out = []
    for m, t in eng.draw_own.items():
        if base <= t.data_ptr() < end:
            out.append((t.data_ptr() - base, t.numel() * es, 'draw_own[%s]' % m.name))
    for k, g in enumerate(eng.groups):
        t = getattr(g, 'draw_own', None)
        if t is not None and base <= t.data_ptr() < end:
            out.append((t.data_ptr() - base, t.numel() * es, 'group[%d].draw_own' % k))
    return sorted(out)


def capacity_free(text, eng):
    """the plan text with every '_draw_pool+<byte offset>' rewritten as '<carved tensor>+<offset inside it>': a carve lies behind the
    earlier ones, whose sizes hold train_batch -- the one field of the text that encodes the capacity"""
    cv = carves(eng)

    def sub(m):
        off = int(m.group(1))
        for start, nbytes, name in cv:
            if start <= off < start + nbytes:
                return '%s+%d' % (name, off - start)
        return m.group(0)
    return re.sub(r'_draw_pool\+(\d+)', sub, text)


def plan_only_text(name, capacity, N, dtype):
    """-> (canonical text of plan(N) on a plan_only engine of that capacity, the same with the pool offsets normalised)"""
    import os
    import sys
    from unittest import mock
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    if golden not in sys.path:
        sys.path.insert(0, golden)
    import make_plan_fingerprints as mpf
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    # (planning reads no tensor contents: empty() keeps the host buffers untouched, as make_plan_fingerprints.build_plan does)
    with mock.patch.object(torch, 'zeros', torch.empty), mock.patch.object(torch, 'zeros_like', torch.empty_like):
        eng = Engine(graph.build(name, NC, pretrained=False), max_batch=capacity, dtype=dtype, plan_only=True)
        text = mpf.plan_text(eng, eng.plan(N))
    return text, capacity_free(text, eng)


# ---------------------------------------------------------------------------------------------- inputs
def labels(n, g):
    return torch.randint(0, NC - 1, (n,), generator=g)


def make_rois(n, seed):
    """n ragged grey ROIs as load_rois takes them (device tensors)"""
    rng = np.random.default_rng(seed)
    hs = rng.integers(20, 150, n).astype(np.int32)
    ws = rng.integers(20, 150, n).astype(np.int32)
    sizes = hs.astype(np.int64) * ws
    offs = np.zeros(n, np.int64)
    offs[1:] = np.cumsum(sizes)[:-1]
    blob = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8)
    return dict(pixels=torch.from_numpy(blob).cuda(), offs=torch.from_numpy(offs).cuda(), hs=torch.from_numpy(hs).cuda(),
                ws=torch.from_numpy(ws).cuda(), max_h=int(hs.max()), max_w=int(ws.max()))


def hostile_tail(eng, N, slot=None):
    """everything of an input slot behind image N (module docstring); on an engine of capacity N there is nothing behind it"""
    slot = eng.in_slot if slot is None else slot
    dense = eng.in_bufs[slot]
    if eng.in_kind[slot] == 'u8':
        lo.nan_fill(dense)
        eng.in_u8[slot][N:].fill_(TAIL_BYTE)
    else:
        lo.nan_fill(dense[N:])
        if eng.stem_u8 is not None:
            eng.in_u8[slot].fill_(TAIL_BYTE)
    eng.tgt_bufs[slot][N:].fill_(JUNK)


def mask_tails(eng, N, value):
    for h in eng.heads:
        if h.dropout:
            h.mask[N:].fill_(value)
    for n in eng.drops:
        n.mask[N:].fill_(value)


def stage_dense(eng, N, x, y, mask_tail=0):
    eng.load_input_nchw(x[:N].contiguous())
    eng.target[:N].copy_(y[:N])
    hostile_tail(eng, N)
    mask_tails(eng, N, mask_tail)


def stage_rois(eng, N, rois, y, mask_tail=0):
    eng.load_rois(**rois)
    eng.target[:N].copy_(y[:N])
    hostile_tail(eng, N)
    mask_tails(eng, N, mask_tail)


def stage_rois_prefetched(eng, N, rois, y, mask_tail=0):
    """the same batch through the other input slot: staged on the side stream, then made current"""
    torch.cuda.synchronize()
    slot, side = eng.prefetch_begin()
    with torch.cuda.stream(side):
        eng.load_rois(slot=slot, **rois)
        eng.tgt_bufs[slot][:N].copy_(y[:N].to(eng.dev))
        hostile_tail(eng, N, slot)
    eng.prefetch_end(slot)
    got = eng.use_prefetched()
    assert got == slot == eng.in_slot
    mask_tails(eng, N, mask_tail)
    return slot


def poison(eng, N, clean=False):
    """lane_order.poison, and (NaN run) the rows >= N of the arg-max planes at an in-range value that is not its 0"""
    lo.poison(eng, clean)
    if not clean:
        for t in eng.argmax.values():
            t[N:].fill_(ARG_TAIL)


# ---------------------------------------------------------------------------------------------- runs and what they leave
def step_outcome(eng, N):
    out = lo.step_outcome(eng)
    for h in eng.heads:
        out[h.name + '.logits'] = out[h.name + '.logits'][:N].clone()
    return out


def train(eng, N):
    eng.train_step(N)
    torch.cuda.synchronize()
    return step_outcome(eng, N)


def evaluate(eng, N):
    """forward_eval + eval loss + softmax -> probs[:N], loss and the logits[:N] of every head the eval forward runs (the auxiliary
    classifier is not part of it: plan.PlanBuilder._fwd_conv, `if not n.aux`)"""
    pl = eng.forward_eval(N)
    eng.run(pl.eval_loss)
    eng.run(pl.softmax)
    torch.cuda.synchronize()
    out = dict(probs=eng.probs[:N].clone(), loss=eng.loss.clone())
    for h in eng.heads:
        if not h.aux:
            out[h.name + '.logits'] = h.logits[:N].clone()
    return out


def all_finite(out):
    return [k for k, v in out.items() if v.is_floating_point() and not bool(torch.isfinite(v).all())]


def host_state(eng):
    """the host-side facts a refused call must leave alone (nbt and loss_sum live on the device: cloned)"""
    return dict(step_count=eng.step_count, dropout_calls=eng.dropout_calls, in_slot=eng.in_slot, packed=eng.packed,
                eval_stats_ready=eng.eval_stats_ready, plans=frozenset(eng._plans), nbt=eng.nbt.clone(), loss_sum=eng.loss_sum.clone())


def host_state_changes(a, b):
    return [k for k in a if not (torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k])]


# ---------------------------------------------------------------------------------------------- nothing behind image N is written
BATCH_LEADING = re.compile(r'^(act\[\d+\]|grad\[\d+\]|group\[\d+\]\.raw|.+\.(feat|logits|dlogits)|probs|argmax\[\d+\])$')
FLAT_SCRATCH = re.compile(r'^(draw\[\d+\]|draw_group|bn_part\[\d+\]|_draw_pool|draw_own\[.+\]|group\[\d+\]\.draw_own)$')
NO_BATCH_DIM = re.compile(r'^(G\[.+\]|stats|Wsh|loss)$')            # per parameter / per channel / scalar: wholly a product of the step


def _flat_extent(name, t, eng, fresh, N):
    """elements from the start of a flat scratch buffer that a plan at N can address: what the capacity-N engine allocated for it"""
    if name.startswith('draw['):
        return fresh.draw[int(name[5:-1])].numel()
    if name == 'draw_group':
        return fresh.draw_group.numel()
    if name.startswith('bn_part['):
        return fresh.bn_part[int(name[8:-1])].numel()           # mblocks of the N-descriptors (engine._alloc_acts)
    assert t.numel() % eng.train_batch == 0, name                 # a d(raw) tensor of its own: train_batch images
    return t.numel() // eng.train_batch * N


def written_behind(eng, fresh, N):
    """after a run at N on poisoned buffers: names of produced buffers that no longer hold the poison behind what the plan at N can
    address.  Every name of lane_order.produced_buffers must fall into one of the three classes above: a new buffer is a decision"""
    fl, it = lo.produced_buffers(eng)
    bad = []
    for name, t in fl:
        if NO_BATCH_DIM.match(name):
            continue
        if BATCH_LEADING.match(name):
            assert t.shape[0] in (eng.max_batch, eng.train_batch), (name, tuple(t.shape))
            tail = t[N:]
        elif name == '_draw_pool':
            tail = t.clone()
            es = t.element_size()
            for start, nbytes, _cn in carves(eng):
                assert start % es == 0 and (nbytes // es) % eng.train_batch == 0
                lo.nan_fill(tail[start // es:start // es + nbytes // es // eng.train_batch * N])
        elif FLAT_SCRATCH.match(name):
            tail = t.reshape(-1)[_flat_extent(name, t, eng, fresh, N):]
        else:
            raise AssertionError('%s: neither batch-leading, flat scratch nor without a batch dimension' % name)
        if not lo.holds_nan_fill(tail):
            bad.append(name)
    for name, t in it:
        assert BATCH_LEADING.match(name), name
        if not bool((t[N:] == ARG_TAIL).all()):
            bad.append(name)
    return bad
