"""Two data-parallel replicas on one device, and the static audit of the bucket plan they run (tests/test_dp_buckets_cpu.py,
tests/test_gpu_dp_world2.py).  Helpers only.

The overlapped exchange of Engine.train_step_ddp hands the tail bucket [lo, hi) of the flat gradient buffer G to the all-reduce as soon
as the backward segment that is SAID to finish it is enqueued.  What is said comes from Engine._op_param_offsets, a hand-kept table;
at world 1 (an exchange that changes nothing) a bucket handed over too early still ends with the right bits.

Static part (no device): `g_writes` takes, for every op of the backward list, the elements of G it writes from the op table alone
(program_footprints.op_footprints: pointers + descriptors), and `audit` holds a segment list and the table against them.

Device part: `PeerSum` is an all_reduce stand-in that adds the peer replica's local gradient on a side stream, handed over the way
ProcessGroupNCCL does it (the side stream waits for the caller's stream, wait() makes the caller's stream wait for the side stream);
`Twin` holds two engines built with dp_world=2 on different shards of one batch.
"""
import numpy as np
import torch

import lane_order as lo
import program_footprints as pf
from ifcb_classifier_amd import _lib

FAMILIES = ('resnet18', 'inception_v3', 'alexnet', 'vgg11', 'vgg13_bn', 'squeezenet', 'densenet121')


# ---------------------------------------------------------------------------------------------------------- static audit
def g_writes(eng, bwd):
    """-> per op of the OpList `bwd`: [(first element, end element, accumulates)] of the footprints inside G that are not read-only"""
    env = pf.allocations(eng)
    base = eng.G.data_ptr()
    end = base + 4 * eng.nparam_padded
    out = []
    for o, tag in zip(bwd.ops, bwd.tags):
        w = []
        for name, role, _span, ptr, width, pitch, rows in pf.op_footprints(env, o, tag):
            if role == pf.R or not (base <= ptr < end):
                continue
            assert rows == 1 and (ptr - base) % 4 == 0 and width % 4 == 0 and ptr + width <= end, (tag, name, ptr - base, width, pitch, rows)
            w.append(((ptr - base) // 4, (ptr - base + width) // 4, role == pf.RW))
        out.append(w)
    return out


def plain_segments(segs):
    """Engine.ddp_segments' [(Program, op end, lo, hi)] -> [(op begin, op end, lo, hi)]"""
    return [(b1 - prog.n, b1, lo, hi) for prog, b1, lo, hi in segs]


def table_offsets(eng, bwd):
    """what Engine._op_param_offsets says each backward op finishes"""
    return [list(eng._op_param_offsets(o)) for o in bwd.ops]


def tensor_extent(eng, off):
    """elements of the tensor at flat offset `off` that an op may write: its own, and for a conv whose output channels are padded to a
    16-byte chunk (squeezenet's classifier) the rows -- of the filter and of the bias -- that Engine._alloc_params reserves for the
    padded channels: the descriptors of its ops carry the padded K, and the gradient of a padded channel is zero"""
    n, shape, node = [(n, s, node) for (o, n, s, _k, node) in eng.poff.values() if o == off][0]
    if getattr(node, 'kind', '') == 'cb' and node.K != node.K_real:
        return n // shape[0] * node.K
    return n


def audit(eng, bwd, segs, offs, writes=None):
    """segs: [(op begin, op end, lo, hi)]; offs: the table (table_offsets, or a mutated copy) -> [finding], each a tuple
    (what, op tag or None, kind name or None, (lo, hi) of the bucket or None, parameter key or None, detail)"""
    writes = g_writes(eng, bwd) if writes is None else writes
    total, nops = eng.nparam_padded, len(bwd.ops)
    key_at = {o: key for key, (o, _n, _s, _k, _node) in eng.poff.items()}
    starts = sorted(key_at)
    bad = []
    kname = lambda k: _lib.OP_NAMES.get(bwd.ops[k].kind)

    def tensor_of(e):
        i = int(np.searchsorted(starts, e, side='right')) - 1
        return starts[i]

    def bucket_of(e):
        for (_b0, _b1, l, h) in segs:
            if l <= e < h:
                return (l, h)
        return None

    # ---- the segments partition the op list in order, their buckets tile [0, total) from the tail
    prev_b, prev_lo = 0, total
    for (b0, b1, l, h) in segs:
        if not (b0 == prev_b and b1 >= b0 and h == prev_lo and l < h):
            bad.append(('partition', None, None, (l, h), None, 'ops [%d, %d) behind %d, bucket behind %d' % (b0, b1, prev_b, prev_lo)))
        prev_b, prev_lo = b1, l
    if prev_b != nops or prev_lo != 0:
        bad.append(('partition', None, None, None, None, 'ends at op %d of %d, element %d' % (prev_b, nops, prev_lo)))
    seg_of = np.zeros(nops, dtype=np.int64)
    for s, (b0, b1, _l, _h) in enumerate(segs):
        seg_of[b0:b1] = s
    # ---- per element: the padding is written by nothing; the first write of a step is a plain one; which segment writes it first
    real = np.zeros(total, dtype=bool)
    for off in starts:
        real[off:off + tensor_extent(eng, off)] = True
    first_seg = np.full(total, 127, dtype=np.int8)
    written = np.zeros(total, dtype=bool)
    for k in range(nops):
        s = int(seg_of[k])
        for (a, b, acc) in writes[k]:
            if not real[a:b].all():
                e = a + int(np.argmin(real[a:b]))
                bad.append(('padding', bwd.tags[k], kname(k), bucket_of(e), key_at[tensor_of(e)], 'writes element %d behind the tensor' % e))
            if acc and not written[a:b].all():
                e = a + int(np.argmin(written[a:b]))
                bad.append(('accumulates first', bwd.tags[k], kname(k), bucket_of(e), key_at[tensor_of(e)],
                            'adds to element %d, which no op of this step has written' % e))
            written[a:b] = True
            np.minimum(first_seg[a:b], s, out=first_seg[a:b])
            # ---- no op of a later segment writes into a bucket that was handed to the exchange
            if s > 0 and b > segs[s - 1][2]:
                e = max(a, segs[s - 1][2])
                bad.append(('late write', bwd.tags[k], kname(k), bucket_of(e), key_at[tensor_of(e)],
                            'op %d of segment %d writes [%d, %d); [%d, %d) was exchanged behind segment %d'
                            % (k, s, a, b, segs[s - 1][2], total, s - 1)))
    # ---- every element of every real tensor of bucket i is written by segments 0..i; the exceptions are the conv biases in front
    #      of a BatchNorm, which nothing writes at all
    dead = sorted(o for lst in eng.cbias_after.values() for o in lst)
    for off in starts:
        key = key_at[off]
        n = eng.poff[key][1]
        bk = bucket_of(off)
        if bk is None or bucket_of(off + n - 1) != bk:
            bad.append(('straddles', None, None, bk, key, 'the tensor [%d, %d) is cut by a bucket boundary' % (off, off + n)))
            continue
        s = [i for i, sg in enumerate(segs) if (sg[2], sg[3]) == bk][0]
        if off in dead:
            if written[off:off + n].any():
                bad.append(('dead bias written', None, None, bk, key, 'a conv bias in front of a BatchNorm is written'))
            continue
        late = first_seg[off:off + n] > s
        if late.any():
            e = off + int(np.argmax(late))
            who = [bwd.tags[k] for k in range(nops) if any(a <= e < b for a, b, _acc in writes[k])]
            bad.append(('uncovered', who[0] if who else None, None, bk, key,
                        'element %d is %s when segment %d hands the bucket over' % (e, 'first written by segment %d' % first_seg[e] if who else 'never written', s)))
    # ---- the table against the footprints: an op finishes exactly the tensors it writes (+ the dead biases riding with a BatchNorm)
    for k in range(nops):
        wrote = sorted({tensor_of(a) for a, _b, _acc in writes[k]})
        said = sorted(o for o in offs[k] if o not in dead)
        rider = sorted(o for o in offs[k] if o in dead)
        if wrote != said:
            for o in sorted(set(wrote) ^ set(said)):
                bad.append(('table', bwd.tags[k], kname(k), bucket_of(o), key_at.get(o),
                            'the op %s this tensor, the table says it %s' % (('writes', 'does not') if o in wrote else ('does not write', 'does'))))
        for o in rider:
            g0 = [g for g, lst in eng.cbias_after.items() if o in lst][0]
            if g0 not in offs[k]:
                bad.append(('table', bwd.tags[k], kname(k), bucket_of(o), key_at.get(o), 'a dead bias rides with an op that is not its BatchNorm'))
    return bad


def move_cut_early(segs, writes, which=None):
    """a copy of [(op begin, op end, lo, hi)] with the cut behind segment i moved one op earlier, at the first i (or `which`) whose last
    op writes G -> (segments, i, index of the moved op)"""
    for i, (b0, b1, l, h) in enumerate(segs[:-1]):
        if (which is None or i == which) and b1 - b0 >= 2 and writes[b1 - 1]:
            out = list(segs)
            out[i] = (b0, b1 - 1, l, h)
            nb0, nb1, nl, nh = segs[i + 1]
            out[i + 1] = (b1 - 1, nb1, nl, nh)
            return out, i, b1 - 1
    raise AssertionError('no segment ends with an op that writes G')


# ---------------------------------------------------------------------------------------------------------- device
class _Handle:
    """what torch.distributed's async_op=True returns, as far as dp.run_overlapped uses it"""

    def __init__(self, side, dev, deaf=False):
        self.side, self.dev, self.deaf = side, dev, deaf

    def wait(self):
        if not self.deaf:
            torch.cuda.current_stream(self.dev).wait_stream(self.side)
        return True


class PeerSum:
    """the `all_reduce` argument of Engine.train_step_ddp for a world of two replicas in one process: adds the peer's local gradient
    into the bucket it is called with, on a side stream that first waits for the caller's stream (how ProcessGroupNCCL takes a tensor
    over); the handle's wait() makes the caller's stream wait for the side stream.
    delay: callable(side stream) that keeps the side stream busy in front of every sum.  deaf: handles whose wait() does nothing (the
    negative control of the delayed case).  eager: the caller's stream waits for the sum at once -- an exchange that is over before the
    next segment starts, which makes the outcome of a bucket handed over too early deterministic (the late writer always comes second).
    calls: [(offset, elements)] per call"""

    def __init__(self, eng, peer_grad, delay=None, deaf=False, eager=False):
        assert peer_grad.shape == eng.G.shape and peer_grad.data_ptr() != eng.G.data_ptr()
        self.eng, self.peer, self.delay, self.deaf, self.eager = eng, peer_grad, delay, deaf, eager
        self.side = torch.cuda.Stream(device=eng.dev)
        self.calls = []

    def __call__(self, t):
        eng = self.eng
        byte_off = t.data_ptr() - eng.G.data_ptr()
        n = t.numel()
        assert t.dtype == torch.float32 and t.is_contiguous() and byte_off % 4 == 0 and 0 <= byte_off and byte_off // 4 + n <= eng.G.numel()
        off = byte_off // 4
        self.calls.append((off, n))
        self.side.wait_stream(torch.cuda.current_stream(eng.dev))
        with torch.cuda.stream(self.side):
            if self.delay is not None:
                self.delay(self.side)
            t.add_(self.peer[off:off + n])
        if self.eager:
            torch.cuda.current_stream(eng.dev).wait_stream(self.side)
        return _Handle(self.side, eng.dev, self.deaf)


def memset_delay(eng, at_least_ms):
    """-> (callable(stream), measured ms of one call): lane_order's memset delay, repeated until one call outlasts `at_least_ms`"""
    import ctypes as C
    scratch, nbytes, reps, ms = lo.size_delay(eng, at_least_ms)
    reps = max(reps, int(reps * at_least_ms / max(ms, 1e-3)) + reps)
    d = _lib.Op()
    d.kind = _lib.OP_MEMSET
    d.p[0], d.i[0], d.i[1] = scratch.data_ptr(), nbytes, 0
    arr = (_lib.Op * reps)(*([d] * reps))
    t = (C.c_float * reps)()
    eng.ctx.run_program(arr, reps, eng.stream(), t)
    torch.cuda.synchronize()

    def delay(stream, _keep=scratch):
        eng.ctx.run_program(arr, reps, C.c_void_p(stream.cuda_stream), None)
    return delay, float(sum(t))


def shard(t, r, world=2):
    return t[r::world].contiguous()


class Twin:
    """two replicas of one family built with dp_world=2: same init_weights(seed), different shards of one seeded batch per step.
    masks: None, or callable(replica, B, generator) -> what Engine.external_mask takes (the dropout masks handed over)."""

    def __init__(self, name, B, S, nc=7, dtype='bf16', seed=4321, masks=None, nbatches=2, warm=True, engines=None, after_load=None, **opts):
        from ifcb_classifier_amd import graph
        from ifcb_classifier_amd.engine import Engine
        self.name, self.B, self.S, self.nc, self.opts, self.after_load = name, B, S, nc, opts, after_load
        self.engs = []
        for r in range(2):
            # engines: two engines built elsewhere (through a module wrapper) with dp_world 2 and identical weights
            eng = engines[r] if engines else Engine(graph.build(name, nc, pretrained=False), device=0, max_batch=B, dp_world=2, dtype=dtype, **opts)
            if not engines:
                eng.init_weights(seed=seed)
            eng.dropout_seed, eng.dropout_calls = 5, 0
            self.engs.append(eng)
        assert all(e.dp_world == 2 and e.NL == 2 for e in self.engs)
        g = torch.Generator().manual_seed(9)
        self.X = [torch.rand(2 * B, 3, S, S, generator=g) for _ in range(nbatches + 1)]
        self.Y = [torch.randint(0, nc, (2 * B,), generator=g) for _ in range(nbatches + 1)]
        if warm:
            # one plain step of BOTH replicas on the same shard: Adam moments, running statistics and a step count of a run in progress,
            # identical in the two (generated dropout masks: same seed, same call count)
            for eng in self.engs:
                self.load(eng, nbatches, 0)
                eng.train_step(B)
            torch.cuda.synchronize()
            for k in ('P', 'M', 'V', 'RB'):
                assert lo.same_bits(getattr(self.engs[0], k), getattr(self.engs[1], k)), k
        if masks is not None:
            for r, eng in enumerate(self.engs):
                eng.external_mask = masks(r, B, g)
        self.snaps = [lo.snapshot(e) for e in self.engs]

    def load(self, eng, k, r):
        eng.load_input_nchw(shard(self.X[k], r).cuda())
        eng.target[:self.B].copy_(shard(self.Y[k], r))
        if self.after_load is not None:
            self.after_load(r, eng)

    def reset(self):
        for e, s in zip(self.engs, self.snaps):
            lo.restore(e, s)
            if e.ema_decay is not None:
                e.ema_stale = True                   # (restore writes P from outside)

    def local(self, k):
        """per replica, from its present state: forward_train, loss, backward in plain order on shard k -> (G, loss, RB) cloned; the
        state is put back"""
        out = []
        for r, eng in enumerate(self.engs):
            snap = lo.snapshot(eng)
            self.load(eng, k, r)
            pl = eng.forward_train(self.B)
            eng.run(pl.loss)
            eng.backward(self.B)
            torch.cuda.synchronize()
            out.append(dict(G=eng.G.clone(), loss=eng.loss.clone(), RB=eng.RB.clone()))
            lo.restore(eng, snap)
        return out

    def ddp_step(self, k, local, delay=None, deaf=False, eager=False, step=None):
        """the step under test on shard k, per replica on poisoned buffers -> [PeerSum]; step: callable(replica, engine, PeerSum) in
        the place of loading the shard and Engine.train_step_ddp(B, 2, PeerSum)"""
        sums = []
        for r, eng in enumerate(self.engs):
            if step is None:
                self.load(eng, k, r)
            lo.poison(eng)
            ps = PeerSum(eng, local[1 - r]['G'], delay=delay, deaf=deaf, eager=eager)
            if step is None:
                eng.train_step_ddp(self.B, 2, ps)
            else:
                step(r, eng, ps)
            sums.append(ps)
        torch.cuda.synchronize()
        return sums

    def close(self):
        for e in self.engs:
            e.close()
        self.engs = []


def key_of(eng, e):
    """the parameter tensor (or the padding behind it) that holds flat element e"""
    best = None
    for key, (o, n, _s, _k, _node) in eng.poff.items():
        if o <= e and (best is None or o > best[1]):
            best = (key, o, n)
    key, o, n = best
    return key if e < o + n else 'padding behind ' + key


def first_difference(eng, a, b):
    """-> None, or (element, parameter key, a's value, b's value, number of differing elements) for the first element whose bits differ"""
    ne = a.view(torch.int32) != b.view(torch.int32)
    if not bool(ne.any()):
        return None
    e = int(torch.argmax(ne.to(torch.uint8)))
    return (e, key_of(eng, e), float(a[e]), float(b[e]), int(ne.sum()))
