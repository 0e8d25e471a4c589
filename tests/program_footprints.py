"""Audit of a frozen program against the memory its ops really touch (CPU, Engine(plan_only=True)).

The lane scheduler (engine.schedule_lanes) orders ops by the (lane, reads, writes) annotation written next to every OpList.add;
the pointers in p=(...) are written separately.  This module ignores the annotation: from the op table alone it derives, per op,
the byte footprint of every pointer slot (ROLES below: which p[k] are read / written, taken from the const-ness of the matching
parameter in include/ifcbk.h; the extent from the op's own descriptor), recomputes happens-before from the frozen lane / wait
bits exactly as ctx.hip::run_lanes executes them, and reports every pair of ops that touch common bytes, at least one writing,
without being ordered.

A footprint is (allocation, start byte, row width, row pitch, rows): `rows` runs of `width` bytes, `pitch` bytes apart.  A flat
buffer is one row.  Two footprints of one allocation conflict if at least one writes and, with equal pitch, some row of one
intersects some row of the other (exact); with different pitches, their bounding byte intervals intersect (conservative).

Out of the audit: the per-lane workspace arenas (ctx->ws: split-K slabs, BatchNorm-backward partials) -- run_lanes points ctx->ws
at the arena of the op's own lane before every launch, so two lanes never share one, and ops of one lane are stream-ordered.
"""
import ctypes as C
import weakref

from ifcb_classifier_amd import _lib

R, W, RW = 'r', 'w', 'rw'


def happens_before(sched):
    """sched: [(lane, wait mask)] in launch order -> reach[i] = set of ops that finish before op i starts (ctx.hip::run_lanes: an op
    starts after the previous op of its lane and after everything queued so far on the lanes of its wait mask)"""
    n = len(sched)
    last_on_lane = {}
    preds = [set() for _ in range(n)]
    queued = {l: [] for l in range(8)}
    for i, (lane, wait) in enumerate(sched):
        if lane in last_on_lane:
            preds[i].add(last_on_lane[lane])
        for l in range(8):
            if wait >> l & 1 and queued[l]:
                preds[i].add(queued[l][-1])          # the tail of lane l (stream order covers everything before it)
        last_on_lane[lane] = i
        queued[lane].append(i)
    # transitive closure (small n)
    reach = [set() for _ in range(n)]
    for i in range(n):
        for p in preds[i]:
            reach[i].add(p)
            reach[i] |= reach[p]
    return reach


def frozen_sched(arr, n):
    return [((arr[k].flags >> 8) & 7, (arr[k].flags >> 12) & 0xff) for k in range(n)]


# ---------------------------------------------------------------- extents
def _es(dtype):
    return 2 if dtype == _lib.BF16 else 4


# Every extent function takes (op, env) and returns (width bytes, pitch bytes, rows) or None for "slot unused"; the pointer is added
# by the caller.  e gives the library's host-side planning helpers.
def conv_x(o, e):
    d = o.u.conv
    return (d.C * _es(d.dtype), d.ldx * _es(d.dtype), d.N * d.H * d.W)


def conv_y(o, e):
    d = o.u.conv
    return (d.K * _es(d.dtype), d.ldy * _es(d.dtype), d.N * d.P * d.Q)


def conv_w(o, e):
    d = o.u.conv
    n = d.K * d.R * d.S * d.C * _es(d.dtype)
    return (n, n, 1)


def conv_dw(o, e):
    d = o.u.conv
    n = d.K * d.R * d.S * d.Cw * 4
    return (n, n, 1)


def conv_kf(o, e):
    return (o.u.conv.K * 4, o.u.conv.K * 4, 1)


def conv_cf(o, e):
    return (o.u.conv.C * 4, o.u.conv.C * 4, 1)


def bytes_(n):
    return lambda o, e: (int(n(o, e)), int(n(o, e)), 1)


def conv_res(o, e):
    d = o.u.conv
    return (d.K * _es(d.dtype), int(o.i[0]) * _es(d.dtype), d.N * d.P * d.Q)


def bn_cf(o, e):
    return (o.u.bn.C * 4, o.u.bn.C * 4, 1)


def bn_rows(ld):
    def f(o, e):
        d = o.u.bn
        return (d.C * _es(d.dtype), ld(o) * _es(d.dtype), d.M)
    return f


def bn_part(rows, ld):
    def f(o, e):
        d = o.u.bn
        return (d.C * 4, (ld(o) or d.C) * 4, 2 * rows(o, e))
    return f


def pool_x(ld=None):
    def f(o, e):
        d = o.u.pool
        return (d.C * _es(d.dtype), (ld(o) if ld else d.ldx) * _es(d.dtype), d.N * d.H * d.W)
    return f


def pool_y(o, e):
    d = o.u.pool
    return (d.C * _es(d.dtype), d.ldy * _es(d.dtype), d.N * d.P * d.Q)


def pool_cf(o, e):
    return (o.u.pool.C * 4, o.u.pool.C * 4, 1)


def pool_am(o, e):
    d = o.u.pool
    return (d.N * d.P * d.Q * d.C,) * 2 + (1,)


def head_x(ld=None):
    def f(o, e):
        d = o.u.head
        return (d.C * _es(d.dtype), (ld(o) if ld else d.ldx) * _es(d.dtype), d.N * d.HW)
    return f


def seg_dw(k):
    def f(o, e):
        d = o.u.conv
        if k >= 4 or o.i[k] <= 0 or any(o.i[j] <= 0 for j in range(k)):
            return None
        n = int(o.i[k]) * d.R * d.S * d.Cw * 4
        return (n, n, 1)
    return f


def seg_y(k):
    def f(o, e):
        d = o.u.conv
        if any((o.i[j] & 0xfffff) <= 0 for j in range(k + 1)):
            return None
        return ((o.i[k] & 0xfffff) * _es(d.dtype), ((o.i[k] >> 20) & 0xfffff) * _es(d.dtype), d.N * d.P * d.Q)
    return f


def flatten_x(o, e):
    es = _es(int(o.i[3] >> 32))
    return (int(o.i[2]) * es, int(o.i[3] & 0xffffffff) * es, int(o.i[0] * o.i[1]))


def flatten_flat(o, e):
    n = int(o.i[0] * o.i[1] * o.i[2]) * _es(int(o.i[3] >> 32))
    return (n, n, 1)


def _acc(bit):
    """written slot that also reads when flags bit `bit` is set"""
    return lambda o: RW if (o.flags >> bit) & 1 else W


_hd = lambda n: bytes_(lambda o, e: n(o.u.head) * 4)
_K = _lib

# kind -> {slot: (role(op), extent(op, env))}: one row per case of ctx.hip::run_one.  The order of the slots is that of the typed
# entry point in include/ifcbk.h; a `const` parameter is R, anything else W, and acc (flags bit 0) / pacc (bit 1) / bit 3 turn the
# slot they govern into RW.  OP_CONV_WGRAD_GROUP and OP_WEIGHT_PACK_MULTI read their pointers from an item table (op_footprints).
ROLES = {
    _K.OP_CONV_FWD: {0: (R, conv_x), 1: (R, conv_w), 2: (W, conv_y),
                     3: (W, bytes_(lambda o, e: e.lib.ifcbk_conv2d_fwd_mblocks(C.byref(o.u.conv)) * 2 * o.u.conv.K * 4))},
    _K.OP_CONV_FWD_AFFINE: {0: (R, conv_x), 1: (R, conv_w), 2: (W, conv_y), 3: (R, conv_kf), 4: (R, conv_kf), 5: (R, conv_res)},
    _K.OP_CONV_DGRAD: {0: (R, conv_y), 1: (R, conv_w), 2: (_acc(0), conv_x)},
    _K.OP_CONV_WGRAD: {0: (R, conv_x), 1: (R, conv_y), 2: (_acc(0), conv_dw)},
    _K.OP_CONV_FWD_AFFINE_MAXPOOL: {0: (R, conv_x), 1: (R, conv_w), 3: (R, conv_kf), 4: (R, conv_kf),
                                    2: (W, lambda o, e: (o.u.conv.K * _es(o.u.conv.dtype), int(o.i[0]) * _es(o.u.conv.dtype),
                                                         o.u.conv.N * ((o.u.conv.P - 3) // 2 + 1) * ((o.u.conv.Q - 3) // 2 + 1)))},
    _K.OP_STEM_U8_FWD: {0: (R, bytes_(lambda o, e: o.u.conv.N * o.u.conv.H * o.u.conv.W)), 1: (R, conv_dw), 2: (R, bytes_(lambda o, e: 24)),
                        3: (W, conv_y), 4: (W, bytes_(lambda o, e: e.lib.ifcbk_stem_u8_rows(C.byref(o.u.conv)) * 2 * o.u.conv.K * 4)),
                        5: (R, conv_kf), 6: (R, conv_kf)},
    _K.OP_STEM_U8_WGRAD: {0: (R, bytes_(lambda o, e: o.u.conv.N * o.u.conv.H * o.u.conv.W)), 1: (R, conv_y), 2: (R, bytes_(lambda o, e: 24)),
                          3: (_acc(0), conv_dw)},
    _K.OP_CONV_WGRAD_SEG: {0: (R, conv_x), 1: (R, conv_y), 2: (_acc(0), seg_dw(0)), 3: (_acc(0), seg_dw(1)), 4: (_acc(0), seg_dw(2)),
                           5: (_acc(0), seg_dw(3))},
    _K.OP_WEIGHT_PACK_MULTI: {},
    _K.OP_WEIGHT_PACK: {0: (R, conv_dw), 1: (W, conv_w),
                        2: (W, lambda o, e: (o.u.conv.K * _es(o.u.conv.dtype), (int(o.i[0]) or o.u.conv.K) * _es(o.u.conv.dtype),
                                             o.u.conv.C * o.u.conv.R * o.u.conv.S))},
    _K.OP_BN_FINALIZE: {0: (R, bn_part(lambda o, e: int(o.i[0]), lambda o: int(o.i[1]))), 1: (R, bn_cf), 2: (R, bn_cf), 3: (RW, bn_cf),
                        4: (RW, bn_cf), 5: (W, bn_cf), 6: (W, bn_cf), 7: (W, bn_cf), 8: (W, bn_cf)},
    _K.OP_BN_APPLY: {0: (R, bn_rows(lambda o: o.u.bn.ldx)), 1: (R, bn_cf), 2: (R, bn_cf), 3: (R, bn_rows(lambda o: int(o.i[0]))),
                     4: (W, bn_rows(lambda o: o.u.bn.ldy))},
    _K.OP_BN_BWD: {0: (R, bn_rows(lambda o: o.u.bn.ldx)), 1: (R, bn_rows(lambda o: o.u.bn.ldy)), 2: (R, bn_rows(lambda o: int(o.i[0]))),
                   3: (R, bn_cf), 4: (R, bn_cf), 5: (R, bn_cf), 6: (_acc(3), bn_rows(lambda o: int(o.i[1]))),
                   7: (_acc(0), bn_rows(lambda o: int(o.i[2]))), 8: (_acc(1), bn_cf), 9: (_acc(1), bn_cf), 10: (R, bn_cf), 11: (R, bn_cf)},
    _K.OP_CONV_DGRAD_BNSTAT: {0: (R, conv_y), 1: (R, conv_w), 2: (W, conv_x),
                              3: (R, lambda o, e: (o.u.conv.C * _es(o.u.conv.dtype), int(o.i[0]) * _es(o.u.conv.dtype),
                                                   o.u.conv.N * o.u.conv.H * o.u.conv.W)),
                              4: (R, conv_cf), 5: (R, conv_cf), 6: (R, conv_cf), 7: (R, conv_cf),
                              8: (W, bytes_(lambda o, e: e.lib.ifcbk_conv2d_dgrad_bnstat_mblocks(C.byref(o.u.conv)) * 2 * o.u.conv.C * 4))},
    _K.OP_BN_BWD_PARTIALS: {0: (R, bn_rows(lambda o: o.u.bn.ldx)), 1: (R, bn_rows(lambda o: int(o.i[0]))), 2: (R, bn_cf), 3: (R, bn_cf),
                            4: (R, bn_cf), 5: (R, bn_cf), 6: (R, bn_cf), 7: (R, bn_part(lambda o, e: int(o.i[1]), lambda o: int(o.i[3]))),
                            8: (W, bn_rows(lambda o: int(o.i[2]))), 9: (_acc(1), bn_cf), 10: (_acc(1), bn_cf)},
    _K.OP_CONV_FWD_AFFINE_SEG: {0: (R, conv_x), 1: (R, conv_w), 2: (W, seg_y(0)), 3: (W, seg_y(1)), 4: (W, seg_y(2)), 5: (W, seg_y(3)),
                                6: (R, conv_kf), 7: (R, conv_kf)},
    _K.OP_BN_STATS: {0: (R, bn_rows(lambda o: o.u.bn.ldx)),
                     1: (W, bytes_(lambda o, e: e.lib.ifcbk_bn_stats_rows(o.u.bn.M) * 2 * o.u.bn.C * 4))},
    _K.OP_AVGPOOL_AFFINE: {0: (R, pool_x()), 1: (R, pool_cf), 2: (R, pool_cf), 3: (W, pool_y)},
    _K.OP_BN_APPLY_MAXPOOL: {0: (R, pool_x()), 1: (R, pool_cf), 2: (R, pool_cf), 3: (W, pool_y), 4: (W, pool_am)},
    _K.OP_BN_BWD_MAXPOOL: {0: (R, pool_x()), 1: (R, pool_y), 2: (R, pool_am), 3: (R, pool_cf), 4: (R, pool_cf), 5: (R, pool_cf),
                           6: (R, pool_cf), 7: (R, pool_cf), 8: (W, pool_x(lambda o: int(o.i[1]))), 9: (_acc(1), pool_cf),
                           10: (_acc(1), pool_cf)},
    _K.OP_MAXPOOL_FWD: {0: (R, pool_x()), 1: (W, pool_y), 2: (W, pool_am)},
    _K.OP_MAXPOOL_BWD: {0: (R, pool_y), 1: (R, pool_am), 2: (_acc(0), pool_x())},
    _K.OP_AVGPOOL_FWD: {0: (R, pool_x()), 1: (W, pool_y)},
    _K.OP_AVGPOOL_BWD: {0: (R, pool_y), 1: (_acc(0), pool_x())},
    _K.OP_HEAD_FWD: {0: (R, head_x()), 1: (R, bytes_(lambda o, e: o.u.head.N * o.u.head.C)), 2: (R, _hd(lambda d: d.NC * d.C)),
                     3: (R, _hd(lambda d: d.NC)), 4: (W, _hd(lambda d: d.N * d.C)), 5: (W, _hd(lambda d: d.N * d.NC))},
    _K.OP_HEAD_BWD: {0: (R, _hd(lambda d: d.N * d.NC)), 1: (R, _hd(lambda d: d.N * d.C)), 2: (R, bytes_(lambda o, e: o.u.head.N * o.u.head.C)),
                     3: (R, _hd(lambda d: d.NC * d.C)), 4: (_acc(1), _hd(lambda d: d.NC * d.C)), 5: (_acc(1), _hd(lambda d: d.NC)),
                     6: (W, head_x(lambda o: int(o.i[0])))},
    _K.OP_SOFTMAX_XENT: {0: (R, bytes_(lambda o, e: o.i[0] * o.i[1] * 4)), 1: (R, bytes_(lambda o, e: o.i[0] * 8)), 2: (_acc(0), bytes_(lambda o, e: 4)),
                         3: (W, bytes_(lambda o, e: o.i[0] * o.i[1] * 4))},
    _K.OP_SOFTMAX_XENT_W: {0: (R, bytes_(lambda o, e: o.i[0] * o.i[1] * 4)), 1: (R, bytes_(lambda o, e: o.i[0] * 8)),
                           2: (_acc(0), bytes_(lambda o, e: 4)), 3: (W, bytes_(lambda o, e: o.i[0] * o.i[1] * 4)),
                           4: (R, bytes_(lambda o, e: o.i[1] * 4))},
    _K.OP_SOFTMAX: {0: (R, bytes_(lambda o, e: o.i[0] * o.i[1] * 4)), 1: (W, bytes_(lambda o, e: o.i[0] * o.i[1] * 4))},
    _K.OP_ADAM: {0: (RW, bytes_(lambda o, e: o.i[0] * 4)), 1: (R, bytes_(lambda o, e: o.i[0] * 4)), 2: (RW, bytes_(lambda o, e: o.i[0] * 4)),
                 3: (RW, bytes_(lambda o, e: o.i[0] * 4))},
    _K.OP_SGD: {0: (RW, bytes_(lambda o, e: o.i[0] * 4)), 1: (R, bytes_(lambda o, e: o.i[0] * 4)), 2: (RW, bytes_(lambda o, e: o.i[0] * 4))},
    _K.OP_MEMSET: {0: (W, bytes_(lambda o, e: o.i[0]))},
    _K.OP_COPY2D: {0: (W, lambda o, e: (int(o.i[2]), int(o.i[0]), int(o.i[3]))), 1: (R, lambda o, e: (int(o.i[2]), int(o.i[1]), int(o.i[3])))},
    _K.OP_DROPOUT_MASK: {0: (W, bytes_(lambda o, e: o.i[0]))},
    _K.OP_BIAS_RELU_BWD: {0: (R, bn_rows(lambda o: o.u.bn.ldx)), 1: (R, bn_rows(lambda o: o.u.bn.ldy)), 2: (W, bn_rows(lambda o: int(o.i[0]))),
                          3: (_acc(1), bn_cf)},
    _K.OP_DROPOUT: {0: (R, bytes_(lambda o, e: o.i[0] * _es(int(o.i[1])))), 1: (R, bytes_(lambda o, e: o.i[0])),
                    2: (_acc(0), bytes_(lambda o, e: o.i[0] * _es(int(o.i[1]))))},
    # flags bit 2 (to_chw): x -> flat, else flat -> x (+= with bit 0)
    _K.OP_FLATTEN_CHW: {0: (lambda o: R if (o.flags >> 2) & 1 else _acc(0)(o), flatten_x),
                        1: (lambda o: W if (o.flags >> 2) & 1 else R, flatten_flat)},
    _K.OP_STEP_COUNTERS: {0: (RW, bytes_(lambda o, e: o.i[0] * 8)), 1: (RW, bytes_(lambda o, e: 4)), 2: (R, bytes_(lambda o, e: 4))},
    _K.OP_CONV_WGRAD_GROUP: {},
}


class _ItemOp:
    """a descriptor in the place of an op, for the members of an item table"""

    def __init__(self, conv, i0=0):
        class U:
            pass
        self.u = U()
        self.u.conv = conv
        self.i = [i0, 0, 0, 0]
        self.flags = 0


class Allocations:
    """every tensor the engine, its nodes, groups and plans hold, by storage: (start, end, name).  A view resolves to its storage, so
    two slices of one buffer are compared inside the same allocation."""

    def __init__(self, eng):
        import torch
        seen = {}

        def walk(name, v, depth=0):
            if isinstance(v, torch.Tensor):
                st = v.untyped_storage()
                if st.nbytes():
                    seen.setdefault(st.data_ptr(), (st.data_ptr() + st.nbytes(), name))
            elif depth > 3:
                return
            elif isinstance(v, (list, tuple)):
                for k, x in enumerate(v):
                    walk('%s[%d]' % (name, k), x, depth + 1)
            elif isinstance(v, dict):
                for k, x in v.items():
                    walk('%s[%s]' % (name, getattr(k, 'name', k)), x, depth + 1)

        for a in sorted(vars(eng)):
            if a != '_plans':
                walk(a, vars(eng)[a])
        for k, n in enumerate(eng.net.nodes):
            for a in sorted(vars(n)):
                walk('node[%s].%s' % (n.name, a), vars(n)[a])
        for k, g in enumerate(eng.groups):
            for a in sorted(vars(g)):
                walk('group[%d].%s' % (k, a), vars(g)[a])
        self.spans = sorted((s, e, name) for s, (e, name) in seen.items())
        self.starts = [s for s, _e, _n in self.spans]
        self.lib = eng.ctx.lib
        self.eng = eng

    def find(self, ptr):
        import bisect
        k = bisect.bisect_right(self.starts, ptr) - 1
        if k >= 0 and self.spans[k][0] <= ptr < self.spans[k][1]:
            return self.spans[k]
        return None


def _pack_items(eng, o):
    import numpy as np
    tabs = [v[0] for v in eng._pack_tables.values() if v[0].data_ptr() == o.p[0]]
    assert len(tabs) == 1, 'OP_WEIGHT_PACK_MULTI: its item table is not one of the engine\'s'
    raw = tabs[0].cpu().numpy().astype(np.uint8).tobytes()
    return (_lib.PackItem * int(o.i[0])).from_buffer_copy(raw)


def op_footprints(env, o, tag=''):
    """-> [(slot name, role, allocation span, start, width, pitch, rows)] of one op; raises on a kind without a row, a pointer outside
    every allocation or an extent that leaves its allocation"""
    if o.kind not in ROLES:
        raise AssertionError('op kind %d (%s, %r) has no row in program_footprints.ROLES' % (o.kind, _lib.OP_NAMES.get(o.kind), tag))
    slots = []          # (name, role, ptr, extent)
    if o.kind == _lib.OP_CONV_WGRAD_GROUP:
        n = int(o.i[0])
        items = (_lib.WgradItem * n).from_address(o.p[0])
        for k, it in enumerate(items):
            io = _ItemOp(it.d)
            assert it.dw == o.p[1 + k], '%s: p[%d] is not member %d\'s dw' % (tag, 1 + k, k)
            slots += [('item%d.x' % k, R, it.x, conv_x(io, env)), ('item%d.dy' % k, R, it.dy, conv_y(io, env)),
                      ('item%d.dw' % k, _acc(0)(o), it.dw, conv_dw(io, env))]
    elif o.kind == _lib.OP_WEIGHT_PACK_MULTI:
        es = _es(int(o.i[2]))
        for k, it in enumerate(_pack_items(env.eng, o)):
            nm, ns = it.K * it.RS * it.Cw * 4, it.K * it.RS * it.C * es
            slots += [('item%d.w_master' % k, R, it.w_master, (nm, nm, 1)), ('item%d.w' % k, W, it.w, (ns, ns, 1))]
            if it.wT:
                slots.append(('item%d.wT' % k, W, it.wT, (it.K * es, (it.wT_ld or it.K) * es, it.C * it.RS)))
    else:
        for k in range(12):
            if k in ROLES[o.kind]:
                role, ext = ROLES[o.kind][k]
                if o.p[k]:
                    e = ext(o, env)
                    if e is not None:
                        slots.append(('p[%d]' % k, role(o) if callable(role) else role, o.p[k], e))
            elif o.p[k]:
                raise AssertionError('%s (kind %d): p[%d] is set but has no role' % (tag, o.kind, k))
    out = []
    for name, role, ptr, (width, pitch, rows) in slots:
        if width <= 0 or rows <= 0:
            continue
        if width == pitch:
            width, pitch, rows = width * rows, width * rows, 1
        span = env.find(ptr)
        if span is None:
            raise AssertionError('%s (kind %d) %s: pointer outside every tensor the engine holds' % (tag, o.kind, name))
        end = ptr + (rows - 1) * pitch + width
        if end > span[1]:
            raise AssertionError('%s (kind %d) %s: the extent ends %d bytes behind its allocation %s' % (tag, o.kind, name, end - span[1], span[2]))
        out.append((name, role, span, ptr, width, pitch, rows))
    return out


_ALLOCS = weakref.WeakKeyDictionary()


def allocations(eng):
    """the Allocations of an engine, built once (the plans of an engine share its tensors)"""
    if eng not in _ALLOCS:
        _ALLOCS[eng] = Allocations(eng)
    return _ALLOCS[eng]


def _touch(a, b):
    """do two footprints of one allocation share a byte?  a, b: (start, width, pitch, rows)"""
    sa, wa, pa, na = a
    sb, wb, pb, nb = b
    if sa + (na - 1) * pa + wa <= sb or sb + (nb - 1) * pb + wb <= sa:
        return False
    if pa != pb or (na == 1 and nb == 1):
        return True                                   # different pitches: the bounding intervals (conservative)
    if sb < sa:
        sa, wa, na, sb, wb, nb = sb, wb, nb, sa, wa, na
    q, r = divmod(sb - sa, pa)                        # b's row 0 starts r bytes into a's row q
    if r < wa and q < na:                             # rows of b against rows q.. of a
        return True
    return r + wb > pa and q + 1 < na                 # b's row runs over into a's next row


def unordered_conflicts(eng, arr, n, tags, sched=None):
    """-> [((tag, kind name, slot), (tag, kind name, slot), allocation)] of op pairs that share bytes, at least one writing, without
    happens-before between them.  sched: [(lane, wait)] to audit instead of the frozen flags (the negative controls)."""
    env = allocations(eng)
    sched = sched or frozen_sched(arr, n)
    reach = happens_before(sched)
    by_alloc = {}
    for k in range(n):
        for name, role, span, ptr, width, pitch, rows in op_footprints(env, arr[k], tags[k]):
            by_alloc.setdefault(span[0], []).append((ptr, ptr + (rows - 1) * pitch + width, k, name, role, (ptr, width, pitch, rows), span[2]))
    bad = []
    seen = set()
    for fps in by_alloc.values():
        fps.sort(key=lambda f: f[0])
        live = []
        for f in fps:
            live = [g for g in live if g[1] > f[0]]
            for g in live:
                i, j = (g[2], f[2]) if g[2] < f[2] else (f[2], g[2])
                if i == j or (g[4] == R and f[4] == R) or i in reach[j] or (i, j) in seen:
                    continue
                if _touch(g[5], f[5]):
                    seen.add((i, j))
                    a, b = (g, f) if g[2] < f[2] else (f, g)
                    bad.append(((tags[a[2]], _lib.OP_NAMES[arr[a[2]].kind], a[3]), (tags[b[2]], _lib.OP_NAMES[arr[b[2]].kind], b[3]), f[6]))
            live.append(f)
    return bad


def audit_oplist(eng, oplist, meta=None):
    """the audit over an OpList with the schedule its (possibly mutated) annotations give"""
    from ifcb_classifier_amd.engine import schedule_lanes
    arr = (_lib.Op * len(oplist.ops))(*oplist.ops)
    return unordered_conflicts(eng, arr, len(oplist.ops), oplist.tags, sched=schedule_lanes(meta if meta is not None else oplist.meta))
