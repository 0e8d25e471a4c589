"""The program runner's own contract (csrc/ctx.hip: run_lanes, ifcbk_run_program_ev / ifcbk_program_times, ifcbk_program_capture,
ifcbk_graph_launch), on programs of IFCBK_OP_MEMSET and IFCBK_OP_SOFTMAX ops over tensors of 64-4096 elements and private contexts:
event slots, the lane count and the per-lane arenas, the error path (host-side refusals only: nothing here launches a faulty
kernel), a graph against a workspace that moved -- and the engine's answer to that, Engine.load_rois dropping its graphs.  Last, every
op kind that no plan emits (tests/test_op_kinds_cpu.py: EXEMPT_KINDS) alone through ifcbk_run_program against its typed entry point."""
import ctypes as C
import types

import pytest
import torch

import lane_order as lo
from ifcb_classifier_amd import _lib
from ifcb_classifier_amd._lib import Op

pytestmark = pytest.mark.gpu
FILL = 0xEE                                   # what a buffer holds before a program writes it


def st():
    return _lib.cur_stream()


def sync():
    torch.cuda.synchronize()


def buf(n=4096):
    return torch.full((n,), FILL, dtype=torch.uint8, device='cuda')


def memset(t, val, lane=0, wait=0, timed=True):
    o = Op()
    o.kind, o.flags = _lib.OP_MEMSET, (0x80 if timed else 0) | (lane << 8) | (wait << 12)
    o.p[0], o.i[0], o.i[1] = t.data_ptr(), t.numel() * t.element_size(), val
    return o


def softmax(x, y, lane=0, wait=0, timed=True):
    o = Op()
    o.kind, o.flags = _lib.OP_SOFTMAX, (0x80 if timed else 0) | (lane << 8) | (wait << 12)
    o.p[0], o.p[1], o.i[0], o.i[1] = x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1]
    return o


def prog(ops):
    return (Op * len(ops))(*ops), len(ops)


def err(ctx):
    return ctx.lib.ifcbk_last_error(ctx.h).decode()


def times(ctx, slot, n):
    ms = (C.c_float * max(n, 1))(*([-1.0] * max(n, 1)))
    rc = ctx.lib.ifcbk_program_times(ctx.h, slot, n, ms)
    return rc, list(ms)[:n]


def holds(t, val):
    return bool((t == val).all())


@pytest.fixture(scope='module')
def rctx():
    c = _lib.Context(0)
    c.reserve(1 << 16)
    yield c
    c.close()


# ====================================================================================================== event slots
def test_event_slot_numbers_and_outputs_are_checked(rctx):
    b = buf()
    arr, n = prog([memset(b, 1)])
    lib, h = rctx.lib, rctx.h
    for slot in (-1, 256):
        assert lib.ifcbk_run_program_ev(h, arr, n, st(), slot) == _lib.EINVAL
        assert times(rctx, slot, 1)[0] == _lib.EINVAL
    sync()
    assert holds(b, FILL)
    assert times(rctx, 200, 1)[0] == _lib.EINVAL                          # a slot that never ran
    assert lib.ifcbk_run_program_ev(h, arr, n, st(), 201) == _lib.OK
    sync()
    assert holds(b, 1)
    assert lib.ifcbk_program_times(h, 201, 1, None) == _lib.EINVAL        # a NULL output
    rc, ms = times(rctx, 201, 1)
    assert rc == _lib.OK and ms[0] > 0


def test_a_short_run_does_not_hand_back_the_times_of_the_long_run_before_it(rctx):
    """10 ops, then 3 ops, on slot 5: asking for 10 afterwards used to return elapsed times of the first run's events"""
    bs = [buf() for _ in range(10)]
    arr, n = prog([memset(b, k + 1) for k, b in enumerate(bs)])
    rctx.call('ifcbk_run_program_ev', arr, n, st(), 5)
    sync()
    rc, ms = times(rctx, 5, 10)
    assert rc == _lib.OK and all(m > 0 and m == m and m < 1e4 for m in ms), ms
    x = torch.randn(16, 7, device='cuda')
    y = torch.full_like(x, float('nan'))
    arr, n = prog([memset(bs[0], 21), softmax(x, y, timed=False), memset(bs[2], 23)])          # the middle op is not bracketed now
    rctx.call('ifcbk_run_program_ev', arr, n, st(), 5)
    sync()
    rc, ms = times(rctx, 5, 3)
    assert rc == _lib.OK and ms[0] > 0 and ms[1] == 0.0 and ms[2] > 0, ms
    for ask in (4, 10):
        rc, _ms = times(rctx, 5, ask)
        assert rc == _lib.EINVAL, ask
        assert 'the last run on slot 5 had 3' in err(rctx)
    assert times(rctx, 5, 3)[0] == _lib.OK and times(rctx, 5, 2)[0] == _lib.OK           # fewer is a prefix
    assert holds(bs[0], 21) and holds(bs[1], 2) and holds(bs[2], 23) and holds(bs[9], 10)
    want = torch.full_like(x, float('nan'))
    rctx.call('ifcbk_softmax', _lib.ptr(x), 16, 7, _lib.ptr(want), st())
    sync()
    assert lo.same_bits(y, want)


def test_a_slot_grows(rctx):
    bs = [buf(64 + 100 * k) for k in range(40)]
    arr, n = prog([memset(b, 1) for b in bs[:3]])
    rctx.call('ifcbk_run_program_ev', arr, n, st(), 6)
    arr, n = prog([memset(b, k + 2, lane=k % 3) for k, b in enumerate(bs)])
    rctx.call('ifcbk_run_program_ev', arr, n, st(), 6)
    sync()
    rc, ms = times(rctx, 6, 40)
    assert rc == _lib.OK and all(m > 0 and m < 1e4 for m in ms), ms
    assert all(holds(b, k + 2) for k, b in enumerate(bs))
    assert times(rctx, 6, 41)[0] == _lib.EINVAL


def test_two_slots_in_flight_keep_their_own_times(rctx):
    a, b = [buf() for _ in range(4)], [buf() for _ in range(7)]
    pa, na = prog([memset(t, 30 + k, lane=k % 2) for k, t in enumerate(a)])
    pb, nb = prog([memset(t, 40 + k, lane=k % 3, timed=k != 5) for k, t in enumerate(b)])
    rctx.call('ifcbk_run_program_ev', pa, na, st(), 0)
    rctx.call('ifcbk_run_program_ev', pb, nb, st(), 1)                    # no synchronisation between the two
    sync()
    rc, ms = times(rctx, 0, 4)
    assert rc == _lib.OK and all(m > 0 for m in ms), ms
    assert times(rctx, 0, 5)[0] == _lib.EINVAL and times(rctx, 0, 7)[0] == _lib.EINVAL
    rc, ms = times(rctx, 1, 7)
    assert rc == _lib.OK and all((m > 0) == (k != 5) for k, m in enumerate(ms)) and ms[5] == 0.0, ms
    assert times(rctx, 1, 8)[0] == _lib.EINVAL
    assert all(holds(t, 30 + k) for k, t in enumerate(a)) and all(holds(t, 40 + k) for k, t in enumerate(b))


# ====================================================================================================== lanes
def test_a_lane_beyond_the_reserved_arenas_is_refused():
    c = _lib.Context(0)
    assert c.lib.ifcbk_ctx_set_lanes(c.h, 2) == _lib.OK                   # before the first reserve
    c.reserve(1 << 16)
    bs = [buf() for _ in range(3)]
    x = torch.randn(64, 5, device='cuda')
    y = torch.full_like(x, float('nan'))

    def make(lanes):
        return prog([memset(bs[0], 1, lane=lanes[0]), softmax(x, y, lane=lanes[1]), memset(bs[1], 2, lane=lanes[2]), memset(bs[2], 3, lane=lanes[0])])
    arr, n = make((0, 1, 2))
    for run in (lambda: c.lib.ifcbk_run_program(c.h, arr, n, st(), None), lambda: c.lib.ifcbk_run_program_ev(c.h, arr, n, st(), 0)):
        assert run() == _lib.EINVAL
        assert 'names a lane beyond the 2' in err(c)
    sync()
    assert all(holds(b, FILL) for b in bs) and bool(torch.isnan(y).all())          # refused before anything was launched
    arr, n = make((0, 1, 1))
    c.run_program(arr, n, st())
    sync()
    assert [holds(b, k + 1) for k, b in enumerate(bs)] == [True] * 3
    want = torch.full_like(x, float('nan'))
    c.call('ifcbk_softmax', _lib.ptr(x), 64, 5, _lib.ptr(want), st())
    sync()
    assert lo.same_bits(y, want) and bool(torch.isfinite(y).all())
    # more lanes than the reserve made arenas for: refused; fewer: fine, and the 2-lane program still runs
    assert c.lib.ifcbk_ctx_set_lanes(c.h, 4) == _lib.EINVAL
    assert 'set the lane count before ifcbk_ctx_reserve' in err(c)
    assert c.lib.ifcbk_ctx_set_lanes(c.h, 1) == _lib.OK
    for b in bs:
        b.fill_(FILL)
    c.run_program(arr, n, st())
    sync()
    assert [holds(b, k + 1) for k, b in enumerate(bs)] == [True] * 3
    c.close()


def _bias_relu_operands(seed, case):
    import test_gpu_op_bounds as T
    M, K, ldy, lddy, lddz, relu, dt, pacc = case
    g = torch.Generator().manual_seed(seed)
    y, dy = T.rt((M, K), g, dt), T.rt((M, K), g, dt)
    old = T.fvec(K, gen=g, scale=3.0)
    return T.wbuf((M,), K, ldy, dt, y), T.wbuf((M,), K, lddy, dt, dy), old


def _bias_relu_op(case, yd, dyd, dzd, db, lane):
    M, K, ldy, lddy, lddz, relu, dt, pacc = case
    o = Op()
    o.kind, o.flags = _lib.OP_BIAS_RELU_BWD, 0x80 | (pacc << 1) | (lane << 8)           # wait mask 0
    o.p[0], o.p[1], o.p[2], o.p[3] = yd.data_ptr(), dyd.data_ptr(), dzd.data_ptr(), db.data_ptr()
    o.u.bn.M, o.u.bn.C, o.u.bn.ldx, o.u.bn.ldy, o.u.bn.relu, o.u.bn.dtype = M, K, ldy, lddy, relu, dt
    o.i[0] = lddz
    return o


def _granularity():
    """the largest time between two events recorded back to back with nothing between them, over 100 pairs (ms)"""
    s = torch.cuda.current_stream()
    pairs = []
    for _ in range(100):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        b.record(s)
        pairs.append((a, b))
    sync()
    return max(a.elapsed_time(b) for a, b in pairs)


def test_two_lanes_reduce_through_arenas_of_their_own():
    """bias_relu_bwd ops (partial column sums into the ctx workspace, then a second kernel that adds them up) on lanes 1 and 2 with no
    wait between them; if the lanes shared one arena, one op's partial sums could land in the other's.
    First, without any race: the four arenas are filled with a sentinel, the op runs alone on lane 1, then on lane 2, and the arenas
    are copied out -- only the arena of the op's lane was written.
    Then the race: each lane is held back by a delay memset of the same size, sized by lane_order.size_delay (one delay alone would
    let the other lane's op run while it lasts); one op per lane, then eight per lane queued alternately.  Whether ops of the two lanes
    then ran at the same time is measured, not asserted: the ops of a lane are disjoint in time and start behind the lane's delay, so
    all of them lie in the last (outer - shorter delay) of the program, and only if their times add up to more than that (plus one
    event granularity per op) did two of different lanes overlap for certain.  On the MI355X this was written on they did not add up to
    that (ops 1.09 ms in 3.6 ms, the two 1.15 ms delays one after the other): the race rounds catch a shared arena only when the
    hardware does overlap the lanes, the sentinel check above always."""
    import test_gpu_op_bounds as T
    from conftest import MEASURED
    case = T.BIAS_RELU[2]
    M, K, ldy, lddy, lddz, relu, dt, pacc = case
    assert (M, K) == (5000, 24)                                           # its smallest case with more than one row tile
    c = _lib.Context(0)                                                   # 4 arenas, the default
    need = c.lib.ifcbk_bias_relu_bwd_workspace(M, K)
    assert need == -(-M // c.lib.ifcbk_bias_relu_bwd_rows(M)) * K * 4 > K * 4
    c.reserve(need)
    sets = []
    for seed in (11, 12):
        yd, dyd, old = _bias_relu_operands(seed, case)
        # alone, through the typed entry point
        dz0, db0 = T.wbuf((M,), K, lddz, dt), old.cuda()
        c.call('ifcbk_bias_relu_bwd', M, K, dt, _lib.ptr(yd), ldy, _lib.ptr(dyd), lddy, _lib.ptr(dz0), lddz, relu, _lib.ptr(db0), pacc, st())
        sync()
        sets.append((yd, dyd, old, dz0, db0))
    assert not lo.same_bits(sets[0][4], sets[1][4])                       # different inputs
    # ---- which arena does a lane write?  (ifcbk_ctx_workspace_ptr: the first arena; one arena of ifcbk_ctx_workspace_bytes per lane)
    per, base = c.lib.ifcbk_ctx_workspace_bytes(c.h), c.lib.ifcbk_ctx_workspace_ptr(c.h)
    assert per >= need and per % 256 == 0 and base
    arenas = torch.zeros(4, per, dtype=torch.uint8, device='cuda')
    for lane in (1, 2):
        yd, dyd, old, dz0, db0 = sets[lane - 1]
        dz, db = T.wbuf((M,), K, lddz, dt), old.cuda()
        poison, copy = Op(), Op()
        poison.kind, poison.p[0], poison.i[0], poison.i[1] = _lib.OP_MEMSET, base, 4 * per, FILL
        copy.kind, copy.p[0], copy.p[1] = _lib.OP_COPY2D, arenas.data_ptr(), base
        copy.i[0], copy.i[1], copy.i[2], copy.i[3] = 4 * per, 4 * per, 4 * per, 1
        for o in (poison, _bias_relu_op(case, yd, dyd, dz, db, lane), copy):          # three programs: each joins its lanes before the next
            c.run_program((Op * 1)(o), 1, st())
        sync()
        assert lo.same_bits(db, db0) and lo.same_bits(dz, dz0)
        for k in range(4):
            if k == lane:
                assert not holds(arenas[k, :need], FILL), 'lane %d did not write its arena' % lane
                assert holds(arenas[k, need:], FILL)
            else:
                assert holds(arenas[k], FILL), 'lane %d wrote the arena of lane %d' % (lane, k)
    ms = (C.c_float * 1)()
    warm = _bias_relu_op(case, sets[0][0], sets[0][1], T.wbuf((M,), K, lddz, dt), sets[0][2].cuda(), 0)
    for _ in range(2):
        c.run_program((Op * 1)(warm), 1, st(), ms)
    shim = types.SimpleNamespace(dev=torch.device('cuda', 0), ctx=c, stream=st)
    scratch, nbytes, reps, delay_ms = lo.size_delay(shim, 16 * ms[0])     # aimed at the 2 x 8 ops of the later rounds
    scratch2 = torch.empty_like(scratch)
    assert delay_ms >= ms[0]                                              # at least as long as the op it holds back
    g = _granularity()
    shown = []
    for rnd, per_lane in enumerate((1, 8)):
        outs = [[(T.wbuf((M,), K, lddz, dt), old.cuda()) for _ in range(per_lane)] for (_yd, _dyd, old, _dz0, _db0) in sets]
        ops = []
        for lane, sc in zip((1, 2), (scratch, scratch2)):
            ops += [memset(sc, 0, lane=lane)] * reps
        for k in range(per_lane):
            for lane, (yd, dyd, _old, _dz0, _db0), out in zip((1, 2), sets, outs):
                ops.append(_bias_relu_op(case, yd, dyd, out[k][0], out[k][1], lane))
        arr, n = prog(ops)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(torch.cuda.current_stream())
        c.call('ifcbk_run_program_ev', arr, n, st(), 3)
        b.record(torch.cuda.current_stream())                             # (behind the join of the lanes)
        sync()
        rc, t = times(c, 3, n)
        assert rc == _lib.OK and all(x > 0 for x in t), t
        for lane, (out, (_y, _dy, _old, dz0, db0)) in enumerate(zip(outs, sets), 1):
            for k, (dz, db) in enumerate(out):
                assert lo.same_bits(db, db0), ('dbias of lane %d, op %d' % (lane, k), rnd)
                assert lo.same_bits(dz, dz0), ('dz of lane %d, op %d' % (lane, k), rnd)
        outer, delays, busy = a.elapsed_time(b), (sum(t[:reps]), sum(t[reps:2 * reps])), sum(t[2 * reps:])
        shown.append(busy > outer - min(delays) + 2 * per_lane * g)
        MEASURED.append('program runner: bias_relu_bwd (%d, %d) %d per lane: alone %.4f ms, delays %.3f / %.3f ms (%d x %d MiB), ops %.4f ms in '
                        'outer %.4f ms, g %.5f ms: overlap %s' % (M, K, per_lane, ms[0], delays[0], delays[1], reps, nbytes >> 20, busy, outer, g,
                                                                   'shown' if shown[-1] else 'not shown'))
    c.close()


# ====================================================================================================== the error path
def _six_ops(bs, bad_at=3):
    ops = [memset(b, k + 1, lane=k % 3, wait=(1 << ((k + 1) % 3)) if k in (2, 5) else 0) for k, b in enumerate(bs)]
    if bad_at is not None:
        ops[bad_at].kind = 99
    return prog(ops)


def test_a_failing_op_names_itself_joins_the_lanes_and_leaves_the_ctx_usable(rctx):
    bs = [buf() for _ in range(6)]
    arr, n = _six_ops(bs)
    for run in (lambda: rctx.lib.ifcbk_run_program(rctx.h, arr, n, st(), None), lambda: rctx.lib.ifcbk_run_program_ev(rctx.h, arr, n, st(), 9)):
        for b in bs:
            b.fill_(FILL)
        assert run() == _lib.EINVAL
        assert err(rctx) == 'run_program: unknown op kind 99 [op 3 kind 99]'
        torch.cuda.current_stream().synchronize()                         # the stream alone: the lanes joined it on the error path
        assert [holds(b, k + 1) for k, b in enumerate(bs[:3])] == [True] * 3
        assert holds(bs[3], FILL) and holds(bs[4], FILL) and holds(bs[5], FILL)
    # the failed op's events are not read back: it has no stop event
    rc, ms = times(rctx, 9, 6)
    assert rc == _lib.OK and all(m > 0 for m in ms[:3]) and ms[3:] == [0.0] * 3, ms
    arr, n = _six_ops(bs, None)
    rctx.run_program(arr, n, st())
    torch.cuda.current_stream().synchronize()
    assert [holds(b, k + 1) for k, b in enumerate(bs)] == [True] * 6
    with pytest.raises(RuntimeError, match=r'ifcbk_run_program failed \(-1\): run_program: unknown op kind 0 \[op 0 kind 0\]$'):
        rctx.run_program((Op * 1)(), 1, st())                            # a zeroed op, through Context.call


def _xent_op(l, t, loss, dl, f, mixlam=None):
    o = Op()
    o.kind = _lib.OP_SOFTMAX_XENT
    o.p[0], o.p[1], o.p[2], o.p[3] = l.data_ptr(), t.data_ptr(), loss.data_ptr(), dl.data_ptr()
    if mixlam is not None:
        o.p[5] = mixlam.data_ptr()
    o.i[0], o.i[1] = l.shape
    for k, v in enumerate(f):
        o.f[k] = v
    return o


def test_refused_loss_ops_carry_the_suffix_and_a_good_one_follows(rctx):
    N, NC = 9, 5
    g = torch.Generator().manual_seed(3)
    l, t = torch.randn(N, NC, generator=g).cuda(), torch.randint(0, NC, (N,), generator=g).cuda()
    loss, dl = torch.full((1,), -7.0, device='cuda'), torch.full((N, NC), -7.0, device='cuda')
    lam = torch.full((N,), 0.5, device='cuda')
    b = buf()
    for bad, words in ((_xent_op(l, t, loss, dl, (1.0, 0.1, 2.0)), ('f[1]', 'f[2]')), (_xent_op(l, t, loss, dl, (1.0, 0.0, 2.0), lam), ('p[5]', 'f[2]'))):
        arr, n = prog([memset(b, 1), bad])
        assert rctx.lib.ifcbk_run_program(rctx.h, arr, n, st(), None) == _lib.EINVAL
        text = err(rctx)
        assert text.endswith(' [op 1 kind %d]' % _lib.OP_SOFTMAX_XENT) and all(w in text for w in words), text
        sync()
        assert float(loss) == -7.0 and bool((dl == -7.0).all())
    arr, n = prog([_xent_op(l, t, loss, dl, (0.4,))])
    rctx.run_program(arr, n, st())
    want_loss, want_dl = torch.full((1,), -7.0, device='cuda'), torch.full((N, NC), -7.0, device='cuda')
    rctx.call('ifcbk_softmax_xent', _lib.ptr(l), _lib.ptr(t), N, NC, 0.4, _lib.ptr(want_loss), 0, _lib.ptr(want_dl), st())
    sync()
    assert lo.same_bits(loss, want_loss) and lo.same_bits(dl, want_dl) and float(loss) > 0


# ====================================================================================================== graph versus workspace
def test_a_graph_is_refused_once_the_workspace_moved():
    c = _lib.Context(0)
    c.reserve(1 << 16)
    x = torch.randn(64, 9, device='cuda')
    y, want = torch.full_like(x, float('nan')), torch.full_like(x, float('nan'))
    c.call('ifcbk_softmax', _lib.ptr(x), 64, 9, _lib.ptr(want), st())
    arr, n = prog([softmax(x, y)])
    g = c.capture(arr, n)
    c.graph_launch(g, st())
    sync()
    assert lo.same_bits(y, want) and c.live_graphs() == 1
    y.fill_(float('nan'))
    have = c.lib.ifcbk_ctx_workspace_bytes(c.h)
    c.reserve(have)                                                       # not larger: nothing moves
    c.graph_launch(g, st())
    sync()
    assert lo.same_bits(y, want)
    y.fill_(float('nan'))
    c.reserve(have + 1)
    assert c.lib.ifcbk_ctx_workspace_bytes(c.h) > have
    assert c.lib.ifcbk_graph_launch(c.h, g, st()) == _lib.EINVAL
    assert 'the workspace moved' in err(c)
    sync()
    assert bool(torch.isnan(y).all())
    assert c.lib.ifcbk_graph_destroy(c.h, g) == _lib.OK and c.live_graphs() == 0
    g = c.capture(arr, n)                                                 # captured again, it replays
    c.graph_launch(g, st())
    sync()
    assert lo.same_bits(y, want)
    c.close()


def _rois(shapes, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    rois = [rng.integers(0, 256, (h, w), dtype=np.uint8) for h, w in shapes]
    hs, ws = np.array([r.shape[0] for r in rois], np.int32), np.array([r.shape[1] for r in rois], np.int32)
    offs = np.cumsum([0] + [r.size for r in rois[:-1]]).astype(np.int64)
    dev = lambda a: torch.from_numpy(a).cuda()
    return dev(np.concatenate([r.ravel() for r in rois])), dev(offs), dev(hs), dev(ws), int(hs.max()), int(ws.max())


def test_load_rois_drops_the_graphs_when_it_grows_the_arena():
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    B = 4

    def engine():
        eng = Engine(graph.build('resnet18', 7, pretrained=False), device=0, max_batch=B)
        eng.init_weights(seed=4321)
        eng.graph_eval = True
        return eng

    def probs(eng, rois):
        eng.load_rois(*rois)
        pl = eng.forward_eval(B)
        eng.run(pl.softmax)
        sync()
        return eng.probs[:B].clone()
    eng = engine()
    lib, h = eng.ctx.lib, eng.ctx.h
    small = _rois([(40, 31), (17, 40), (33, 25), (8, 12)], 1)
    assert max(small[4], small[5]) == 40
    p1 = probs(eng, small)
    pl = eng.plan(B)
    g1 = pl.graphs['fwd_eval'].value
    live = eng.ctx.live_graphs()
    assert g1 and live == 1
    # the smallest largest side whose tap tables no longer fit the arena, from the library's own sizes
    have = lib.ifcbk_ctx_workspace_bytes(h)
    d = _lib.RoiDesc()
    d.n_img, d.S, d.in_channels, d.out_channels, d.dtype = B, eng.net.S, 1, 8, eng.cdtype
    others = [(60, 50), (100, 3), (45, 45)]                              # the batch's max_w is 50: the sizes below are those load_rois asks for
    need = lambda side: lib.ifcbk_roi_preprocess_workspace(C.byref(d), side, 50)
    assert lib.ifcbk_roi_preprocess_workspace(C.byref(d), 40, 40) <= have
    side = eng.net.S
    while need(side) <= have:
        side += eng.net.S                                                 # (the tap count grows once per S pixels of input)
    assert need(side) > have >= need(side - eng.net.S) and side * 3 < (1 << 22)
    big = _rois([(side, 3)] + others, 2)
    assert (big[4], big[5]) == (side, 50)
    p2 = probs(eng, big)
    assert lib.ifcbk_ctx_workspace_bytes(h) >= need(side) > have
    g2 = pl.graphs['fwd_eval'].value
    assert g2 and eng.ctx.live_graphs() == live                           # dropped and captured again, not leaked
    assert list(pl.graphs) == ['fwd_eval']
    # The handle is the address of a host struct that the drop freed: the allocator may hand the same block to the new graph, so
    # g2 != g1 cannot be required.  Equal: the old handle IS the new graph, and launches (one that was not re-captured would be refused
    # by the epoch check).  Different: the old one must be gone -- live_graphs() unchanged with a new graph live says exactly that
    # (the count is of graphs linked into the ctx), and the old handle is not touched again: it points at freed memory.
    if g2 == g1:
        assert lib.ifcbk_graph_launch(h, C.c_void_p(g1), eng.stream()) == _lib.OK
        sync()
    fresh = engine()
    p2f = probs(fresh, big)
    assert bool(torch.isfinite(p2).all()) and lo.same_bits(p2, p2f)
    assert not lo.same_bits(p1, p2)
    fresh.close()
    eng.close()


# ====================================================================================================== kinds no plan emits
def _alone(ctx, op):
    ctx.run_program((Op * 1)(op), 1, st())
    sync()


def _case_weight_pack(ctx, monkeypatch):
    import test_gpu_conv_bounds as T
    K, RS, Cc, Cw, _col = T.PACK[0]
    d = T._desc((1, Cc, RS, 1, K, RS, 1, 1, 1, 0, 0), Cw, 0)
    m = torch.randn(K, RS, Cw, generator=torch.Generator().manual_seed(1)).cuda()
    outs = []
    for via_op in (False, True):
        w, wT = torch.full((K, RS, Cc), float('nan'), dtype=torch.bfloat16, device='cuda'), torch.full((Cc, RS, K), float('nan'), dtype=torch.bfloat16, device='cuda')
        if via_op:
            o = Op()
            o.kind, o.u.conv = _lib.OP_WEIGHT_PACK, d
            o.p[0], o.p[1], o.p[2] = m.data_ptr(), w.data_ptr(), wT.data_ptr()
            _alone(ctx, o)
        else:
            ctx.call('ifcbk_weight_pack', C.byref(d), _lib.ptr(m), _lib.ptr(w), _lib.ptr(wT), st())
        outs.append((w.view(torch.int16), wT.view(torch.int16)))
    return outs


def _xent_inputs():
    import test_gpu_op_bounds as T
    N, NC, spread, shift, _tmode, _acc, _dl = T.XENT[0]
    g = torch.Generator().manual_seed(N + NC)
    l = (torch.randn(N, NC, generator=g) * spread + shift).cuda()
    return N, NC, l, torch.randint(0, NC, (N,), generator=g).cuda()


def _case_softmax(ctx, monkeypatch):
    N, NC, l, _t = _xent_inputs()
    outs = []
    for via_op in (False, True):
        y = torch.full((N + 1, NC), float('nan'), device='cuda')
        if via_op:
            o = Op()
            o.kind, o.p[0], o.p[1], o.i[0], o.i[1] = _lib.OP_SOFTMAX, l.data_ptr(), y.data_ptr(), N, NC
            _alone(ctx, o)
        else:
            ctx.call('ifcbk_softmax', _lib.ptr(l), N, NC, _lib.ptr(y), st())
        outs.append((y.view(torch.int32),))
    return outs


def _case_softmax_xent_w(ctx, monkeypatch):
    N, NC, l, t = _xent_inputs()
    cw = (torch.rand(NC, generator=torch.Generator().manual_seed(2)) + 0.5).cuda()
    outs = []
    for via_op in (False, True):
        loss, dl = torch.full((1,), float('nan'), device='cuda'), torch.full((N + 1, NC), float('nan'), device='cuda')
        if via_op:
            o = Op()
            o.kind = _lib.OP_SOFTMAX_XENT_W
            o.p[0], o.p[1], o.p[2], o.p[3], o.p[4] = l.data_ptr(), t.data_ptr(), loss.data_ptr(), dl.data_ptr(), cw.data_ptr()
            o.i[0], o.i[1], o.f[0] = N, NC, 0.4
            _alone(ctx, o)
        else:
            ctx.call('ifcbk_softmax_xent_w', _lib.ptr(l), _lib.ptr(t), _lib.ptr(cw), N, NC, 0.4, _lib.ptr(loss), 0, _lib.ptr(dl), st())
        outs.append((loss.view(torch.int32), dl.view(torch.int32)))
    return outs


def _case_dropout_mask(ctx, monkeypatch):
    import test_gpu_op_bounds as T
    n, p, seed, offset = T.DROPOUT_MASK[0]
    outs = []
    for via_op in (False, True):
        m = torch.full((n + 16,), FILL, dtype=torch.uint8, device='cuda')
        if via_op:
            o = Op()
            o.kind, o.p[0], o.i[0], o.f[0], o.i[1], o.i[2] = _lib.OP_DROPOUT_MASK, m.data_ptr(), n, p, seed, offset
            _alone(ctx, o)
        else:
            ctx.call('ifcbk_dropout_mask', _lib.ptr(m), n, p, seed, offset, st())
        outs.append((m,))
    assert holds(outs[0][0][n:], FILL) and 0 < int(outs[0][0][:n].sum()) < n
    return outs


def _case_memset(ctx, monkeypatch):
    """no typed entry point and no kernel of the library: hipMemsetAsync, against the fill it documents"""
    m = torch.full((4096,), FILL, dtype=torch.uint8, device='cuda')
    _alone(ctx, memset(m[64:64 + 1000], 0x5a))
    want = torch.full((4096,), FILL, dtype=torch.uint8, device='cuda')
    want[64:1064] = 0x5a
    return [(want,), (m,)]


def _case_copy2d(ctx, monkeypatch):
    """no typed entry point either: hipMemcpy2DAsync (dst, dst pitch, src, src pitch, row bytes, rows), against the slice copy it is"""
    src = torch.arange(40 * 96, device='cuda').remainder(251).to(torch.uint8).view(40, 96)
    dst = torch.full((40, 128), FILL, dtype=torch.uint8, device='cuda')
    o = Op()
    o.kind, o.p[0], o.p[1] = _lib.OP_COPY2D, dst.data_ptr() + 16, src.data_ptr() + 8
    o.i[0], o.i[1], o.i[2], o.i[3] = 128, 96, 72, 37
    _alone(ctx, o)
    want = torch.full((40, 128), FILL, dtype=torch.uint8, device='cuda')
    want[:37, 16:88] = src[:37, 8:80]
    return [(want,), (dst,)]


def _case_conv_affine_maxpool(ctx, monkeypatch):
    import test_gpu_conv_pool as T
    mark = [m for m in T.test_conv_affine_maxpool_equals_the_two_kernels_it_replaces.pytestmark if m.name == 'parametrize'][0]
    assert mark.args[0] == 'N,H,W,pad,relu'
    N, H, W, pad, relu = mark.args[1][0]                                  # the first case of that file's table
    Cc, K = 32, 64
    P, Q = H + 2 * pad - 2, W + 2 * pad - 2
    Pp, Qp = (P - 3) // 2 + 1, (Q - 3) // 2 + 1
    LDX, LDP = Cc + 8, K + 16
    d = _lib.ConvDesc(N, H, W, Cc, LDX, K, 3, 3, 1, 1, pad, pad, P, Q, K, Cc, _lib.BF16)
    assert ctx.lib.ifcbk_conv2d_fwd_affine_maxpool_ok(C.byref(d)) == 1
    g = torch.Generator(device='cuda').manual_seed(5)
    xb = torch.randn(N, H, W, LDX, device='cuda', generator=g).bfloat16()
    x = xb[..., 4:4 + Cc]
    w = (torch.randn(K, 3, 3, Cc, device='cuda', generator=g) * 0.08).bfloat16()
    scale, shift = torch.randn(K, device='cuda', generator=g) * 0.7, torch.randn(K, device='cuda', generator=g) * 0.3
    outs = []
    for via_op in (False, True):
        y = torch.full((N, Pp, Qp, LDP), float('nan'), device='cuda', dtype=torch.bfloat16)
        if via_op:
            o = Op()
            o.kind, o.flags, o.u.conv = _lib.OP_CONV_FWD_AFFINE_MAXPOOL, relu << 2, d
            o.p[0], o.p[1], o.p[2], o.p[3], o.p[4], o.i[0] = x.data_ptr(), w.data_ptr(), y.data_ptr(), scale.data_ptr(), shift.data_ptr(), LDP
            _alone(ctx, o)
        else:
            ctx.call('ifcbk_conv2d_fwd_affine_maxpool', C.byref(d), _lib.ptr(x), _lib.ptr(w), _lib.ptr(y), LDP, _lib.ptr(scale), _lib.ptr(shift), relu, st())
        outs.append((y.view(torch.int16),))
    assert bool(torch.isfinite(outs[0][0].view(torch.bfloat16)[..., :K].float()).all())
    return outs


EXEMPT_CASES = {
    _lib.OP_WEIGHT_PACK: _case_weight_pack,
    _lib.OP_SOFTMAX: _case_softmax,
    _lib.OP_MEMSET: _case_memset,
    _lib.OP_COPY2D: _case_copy2d,
    _lib.OP_DROPOUT_MASK: _case_dropout_mask,
    _lib.OP_CONV_FWD_AFFINE_MAXPOOL: _case_conv_affine_maxpool,
    _lib.OP_SOFTMAX_XENT_W: _case_softmax_xent_w,
}


@pytest.mark.parametrize('kind', sorted(EXEMPT_CASES), ids=lambda k: '%d-%s' % (k, _lib.OP_NAMES[k]))
def test_a_kind_no_plan_emits_alone_equals_its_typed_entry_point(ctx, monkeypatch, kind):
    typed, through_op = EXEMPT_CASES[kind](ctx, monkeypatch)
    sync()
    assert len(typed) == len(through_op) >= 1
    for k, (a, b) in enumerate(zip(typed, through_op)):
        assert a.shape == b.shape and torch.equal(a, b), (_lib.OP_NAMES[kind], 'output %d' % k)


# ====================================================================================================== a capture that fails
# Graphs are made of IFCBK_OP_SOFTMAX ops, kernel nodes like every op of a plan.  ifcbk_program_capture refuses IFCBK_OP_MEMSET: a
# one-lane graph of four 4 KiB memsets replayed right at first and on a later launch left a non-uniform byte pattern in its first two
# buffers, with and without a failed capture before it and with no error (include/ifcbk.h, ctx.hip::ifcbk_program_capture).
def test_a_program_with_a_memset_is_not_captured(rctx):
    x = torch.randn(16, 7, device='cuda')
    y, b = torch.full_like(x, float('nan')), buf()
    live = rctx.live_graphs()
    for ops, at in (([memset(b, 1)], 0), ([softmax(x, y), memset(b, 1, lane=1)], 1)):
        arr, n = prog(ops)
        out = C.c_void_p(1)
        assert rctx.lib.ifcbk_program_capture(rctx.h, arr, n, C.byref(out)) == _lib.EUNSUPPORTED
        assert not out.value and rctx.live_graphs() == live
        assert err(rctx).startswith('program_capture: op %d is IFCBK_OP_MEMSET' % at)
        rctx.run_program(arr, n, st())                                    # the same program, launched plainly, runs
        sync()
        assert holds(b, 1)
        b.fill_(FILL)
    arr, n = prog([softmax(x, y)])                                        # and the ctx still captures
    gr = rctx.capture(arr, n)
    y.fill_(float('nan'))
    rctx.graph_launch(gr, st())
    sync()
    assert bool(torch.isfinite(y).all()) and rctx.lib.ifcbk_graph_destroy(rctx.h, gr) == _lib.OK and rctx.live_graphs() == live


def _failed_capture(lanes):
    c = _lib.Context(0)
    c.reserve(1 << 16)
    g = torch.Generator().manual_seed(len(lanes))
    xs = [torch.randn(16 + 8 * k, 7 + k, generator=g).cuda() for k in range(4)]
    ys = [torch.full_like(x, float('nan')) for x in xs]
    want = [torch.full_like(x, float('nan')) for x in xs]
    for x, w in zip(xs, want):
        c.call('ifcbk_softmax', _lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(w), st())
    good, n = prog([softmax(x, y, lane=lanes[k % len(lanes)], wait=1 if k == 3 and len(lanes) > 1 else 0) for k, (x, y) in enumerate(zip(xs, ys))])
    assert lo.lanes_of(good, n) == sorted(lanes)
    g0 = c.capture(good, n)
    live = c.live_graphs()
    assert live == 1
    bad = (Op * n)(*good)
    bad[2].kind = 99
    out = C.c_void_p(1)
    assert c.lib.ifcbk_program_capture(c.h, bad, n, C.byref(out)) == _lib.EINVAL
    assert not out.value                                                  # *out is NULL
    assert err(c) == 'run_program: unknown op kind 99 [op 2 kind 99]'
    assert c.live_graphs() == live
    sync()
    assert all(bool(torch.isnan(y).all()) for y in ys)                    # a capture runs nothing, a failed one neither
    g1 = c.capture(good, n)                                               # the capture was ended: the next one begins
    assert c.live_graphs() == live + 1
    for gr in (g1, g0, g1):
        for y in ys:
            y.fill_(float('nan'))
        c.graph_launch(gr, st())
        sync()
        assert [lo.same_bits(y, w) for y, w in zip(ys, want)] == [True] * 4
    for y in ys:
        y.fill_(float('nan'))
    c.run_program(good, n, st())                                          # and plain launches still work on this ctx
    sync()
    assert [lo.same_bits(y, w) for y, w in zip(ys, want)] == [True] * 4
    c.close()


def test_a_failed_capture_is_ended_one_lane():
    _failed_capture((0,))


def test_a_failed_capture_is_ended_two_lanes():
    """(last in the file: the only case here in which the HIP runtime ends a stream capture that forked, after an op was refused)"""
    _failed_capture((0, 1))
