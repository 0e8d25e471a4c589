"""The op tables of an engine: ``OpList`` (ops + scheduling annotations), ``schedule_lanes`` (lane and wait bits from the static data
flow), ``Program`` (a frozen table), ``Plan`` (the thirteen programs of one batch size) and ``PlanBuilder``, which writes them in five
stages (DESIGN, "How a plan is built"): analysis of the graph, forward emitters in node order, grouping of weight gradients, backward
emitters in reverse node order, assembly.  A builder lives for one ``Engine.plan`` call; what outlives a plan is the engine's."""
import ctypes as C
import os

from . import _lib, ops
from ._lib import Op, ConvDesc, BnDesc, PoolDesc, HeadDesc


def _vp(t, byte_off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + byte_off)


# operand slots the planner reads back from ops it has emitted
_PACK_MASTER, _PACK_WT = (ops.slot(_lib.OP_WEIGHT_PACK, name) for name in ('w_master', 'wT'))
_DGRAD_WT = {kind: ops.slot(kind, 'wT') for kind in (_lib.OP_CONV_DGRAD, _lib.OP_CONV_DGRAD_BNSTAT)}


class OpList:
    """ops + tags + scheduling metadata: (lane, reads, writes) per op.  A resource is (key..., lo, hi): a channel range
    of a tensor.  An op without annotations is a full barrier on lane 0 (loss, head, Adam, pack ...).  ``add`` takes p, i and f each
    as a tuple in the slot order of the kind's row in ops.OPERANDS or as a dict keyed by its slot names (an unknown name or a tuple
    longer than the row raises; None or an absent name leaves the zero of a fresh op)."""

    def __init__(self):
        self.ops = []
        self.tags = []
        self.meta = []

    def add(self, kind, tag, p=(), i=(), f=(), flags=0, conv=None, bn=None, pool=None, head=None, lane=0, reads=None, writes=None):
        o = Op()
        o.kind, o.flags = kind, flags
        ops.fill(kind, 'p', o.p, p, lambda v: v if isinstance(v, int) else v.value)
        ops.fill(kind, 'i', o.i, i, int)
        ops.fill(kind, 'f', o.f, f, float)
        if conv is not None:
            o.u.conv = conv
        elif bn is not None:
            o.u.bn = bn
        elif pool is not None:
            o.u.pool = pool
        elif head is not None:
            o.u.head = head
        self.ops.append(o)
        self.tags.append(tag)
        self.meta.append((lane, reads, writes))
        return o

    def extend(self, other):
        self.ops.extend(other.ops)
        self.tags.extend(other.tags)
        self.meta.extend(other.meta)

    def slice(self, b0, b1):
        sub = OpList()
        sub.ops, sub.tags, sub.meta = self.ops[b0:b1], self.tags[b0:b1], self.meta[b0:b1]
        return sub

    def freeze(self):
        arr = (Op * len(self.ops))(*self.ops)
        for k, (lane, wait) in enumerate(schedule_lanes(self.meta)):
            arr[k].flags = (arr[k].flags & 0xff) | (lane << 8) | (wait << 12)
        return arr


def _overlap(a, b):
    return a[:-2] == b[:-2] and a[-2] < b[-1] and b[-2] < a[-1]


def schedule_lanes(meta):
    """(lane, wait mask) per op from the static data flow: an op waits for the lanes that hold an unfinished producer of
    something it reads, or an unfinished reader / writer of something it writes.  A wait covers everything queued on the
    waited lane so far (and, transitively, whatever that lane had waited for), which is remembered to skip redundant waits."""
    NL = 8
    count = [0] * NL                              # ops queued per lane
    synced = [[0] * NL for _ in range(NL)]        # synced[L][j]: lane L is ordered after the first synced[L][j] ops of lane j
    table = {}                                    # resource -> [writer (lane, pos) or None, readers [(lane, pos)]]
    star = ('*', 0, 1)
    out = []
    for lane, reads, writes in meta:
        if reads is None and writes is None:
            lane, reads, writes = 0, [star], [star]           # barrier
        else:
            reads, writes = list(reads or ()) + [star], list(writes or ())
        deps = set()
        for r in reads:
            for res, (w, _rd) in table.items():
                if w is not None and _overlap(r, res):
                    deps.add(w)
        for wres in writes:
            for res, (w, rd) in table.items():
                if _overlap(wres, res):
                    if w is not None:
                        deps.add(w)
                    deps.update(rd)
        wait = 0
        for (lj, pj) in deps:
            if lj != lane and pj >= synced[lane][lj]:
                wait |= 1 << lj
        for lj in range(NL):
            if wait >> lj & 1:
                synced[lane][lj] = count[lj]
                for k in range(NL):
                    if k != lane:
                        synced[lane][k] = max(synced[lane][k], synced[lj][k])
        me = (lane, count[lane])
        count[lane] += 1
        for r in reads:
            table.setdefault(r, [None, []])[1].append(me)
        for wres in writes:
            for res in [res for res in table if _overlap(wres, res)]:
                table[res] = [me, []]
            table[wres] = [me, []]
        out.append((lane, wait))
    return out


class Program:
    def __init__(self, oplist):
        self.tags = list(oplist.tags)
        self.n = len(oplist.ops)
        self.arr = oplist.freeze()
        self.lanes = sorted({m[0] for m in oplist.meta if not (m[1] is None and m[2] is None)} | {0})

    def find(self, kind):
        return [k for k in range(self.n) if self.arr[k].kind == kind]

    def timed(self, which=None, single_lane=False):
        """a copy of the op table in which the ops `which` (indices; None = all) carry flags bit 7: ifcbk_run_program_ev
        brackets exactly those with HIP events.  single_lane: drop the lane / wait bits, i.e. run every op back to back
        on the caller's stream (per-kernel durations without another lane's kernel sharing the GPU)"""
        arr = (Op * self.n)(*self.arr)
        for k in (range(self.n) if which is None else which):
            arr[k].flags |= ops.FLAG_TIMED
        if single_lane:
            for k in range(self.n):
                arr[k].flags &= 0xff
        return arr


def _program(*lists):
    ol = OpList()
    for part in lists:
        ol.extend(part)
    return Program(ol)


class Plan:
    """what Engine.plan(N) hands out: thirteen programs (an accumulating engine's: two more, acc_update and acc_count), where the optimizer ops sit in ``step`` (step_adam_idxs), the backward list the
    data-parallel step cuts (bwd_list -> ddp_segs), the graphs captured from the programs, the host tables the ops point into (keep)
    and the dispatch switches in force when it was built (dispatch_env, set by Engine.plan)"""

    def __init__(self, N):
        self.N = N
        self.graphs = {}
        self.ddp_segs = None
        self.dispatch_env = None


class WgradGroup:
    """conv layers of one block whose weight gradients run as ONE split-K grid, behind the last of them in backward order"""

    def __init__(self, members, descs, ws, kh, key):
        self.members, self.descs, self.ws, self.kh, self.key = members, descs, ws, kh, key
        self.seen = 0                  # members whose d(raw) the backward emitted so far has written


# ---- resources for the lane scheduler: channel ranges of tensors (activation, its gradient, a member's slice of its sibling GEMM's
# merged output and of the merged d(raw), a conv's raw output, BatchNorm statistics, a lane's partial sums, an arg-max plane)
ra = lambda v: ('a', v.buf.id, v.coff, v.coff + v.C)
rg = lambda v: ('g', v.buf.id, v.coff, v.coff + v.C)
rpre = lambda m: ('gr', id(m.group), m.koff, m.koff + m.K)
rdg = lambda m: ('dg', id(m.group), m.koff, m.koff + m.K)
rraw = lambda m: rpre(m) if (m.group is not None and m.cpool is None) else ('r', m.raw.id, 0, m.K)
rst = lambda m: ('s', id(m), 0, 1)
rbp = lambda L: ('bp', L, 0, 1)
ram = lambda k: ('am', k, 0, 1)


class PlanBuilder:
    """writes the plan of engine `eng` at batch N (for its current input slot and kind): ``PlanBuilder(eng, N).build()``, once"""

    def __init__(self, eng, N):
        self.e, self.N, self.net = eng, N, eng.net
        self.fwd_t, self.fwd_e, self.bwd, self.pack, self.evalprep = (OpList() for _ in range(5))
        self.keep = []                 # host tables the op tables point into
        self.written = set()           # grad buffers already written in this backward pass
        self.bnstat_done = {}          # producer conv -> dict(part: partials pointer, rows: their count, res: the buffer's resource)
        self.wl_next = 0               # round-robin over the weight-gradient lanes, per conv node in backward order
        self.wg_of = {}                # conv node -> its WgradGroup
        # the builder's switches, read once.  IFCBK_FUSE_POOL: the TRAINING conv + max-pool fusion, IFCBK_FUSE_POOL_EVAL: the eval one --
        # two switches, two decisions.  IFCBK_FUSE_BNSTAT: 1 (default) fuses, 0 is the unfused reference of the parity tests.
        # IFCBK_WGRAD_GROUP=0: every weight gradient on its own launch.  IFCBK_OPT_BUCKETS: optimizer buckets (6), <= 1 = one launch
        env = os.environ.get
        self.fuse_pool = env('IFCBK_FUSE_POOL', '1') != '0'
        self.fuse_pool_eval = env('IFCBK_FUSE_POOL_EVAL', '1') != '0'
        self.fuse_bnstat = env('IFCBK_FUSE_BNSTAT', '1')
        if self.fuse_bnstat not in ('0', '1'):
            raise ValueError('IFCBK_FUSE_BNSTAT must be 0 or 1, got %r' % self.fuse_bnstat)
        self.group_wgrads = env('IFCBK_WGRAD_GROUP', '1') != '0' and eng.dtype == 'bf16'
        self.opt_buckets = int(env('IFCBK_OPT_BUCKETS', '6'))
        # the stem conv on the resized u8 plane of this slot (conv_stem_u8.hip) instead of the [N,S,S,8] tensor: that node, or None
        self.u8 = eng.stem_u8 if (eng.stem_u8 is not None and eng.in_kind[eng.in_slot] == 'u8') else None
        self.readers, self.producers = self._readers_producers()
        pool_cand = self._pool_candidates()
        self.fused_pool = dict(pool_cand) if self.fuse_pool else {}       # conv node -> (pool node, its index)
        self.fused_pool_nodes = {v[0] for v in self.fused_pool.values()}
        self.fused_pool_eval = self._fused_pool_eval(pool_cand)           # conv node -> pool node
        self.fused_pool_eval_nodes = set(self.fused_pool_eval.values())
        self.bnstat_of = self._bnstat_consumers()                         # consumer conv -> producer conv
        # training and eval programs get their own lane counts: measured (B=256) 2 / 3 / 4 lanes = 25.9 / 25.5 / 25.3 ms per
        # train step but 6.12 / 6.63 / 6.78 ms per eval forward (its kernels are few and wide: more lanes only add waits)
        self.WLs = list(range(eng.NL - eng.wgrad_lane, eng.NL))           # the weight-gradient lanes
        self.lane_of = self._assign_lanes(eng.NL - eng.wgrad_lane)
        self.lane_eval = self._assign_lanes(eng.NL_eval)

    def build(self):
        e = self.e
        e.fused_pool = self.fused_pool
        fwd = dict(conv=self._fwd_conv, max=self._fwd_pool, avg=self._fwd_pool, head=self._fwd_head, cb=self._fwd_cb,
                   drop=self._fwd_drop, flat=self._fwd_flat, bnr=self._fwd_bnr)
        bwd = dict(conv=self._bwd_conv, max=self._bwd_pool, avg=self._bwd_pool, head=self._bwd_head, cb=self._bwd_cb,
                   drop=self._bwd_drop, flat=self._bwd_flat, bnr=self._bwd_bnr)
        nodes = [(k, n) for k, n in enumerate(self.net.nodes) if n.kind in fwd]
        for k, n in nodes:
            fwd[n.kind](k, n)
        e.wgrad_groups = self._group_weight_gradients()
        # backward in reverse node order, resolving first-writer / accumulate flags
        for k, n in reversed(nodes):
            bwd[n.kind](k, n)
        return self._assemble()

    # ------------------------------------------------------------------ analysis
    def _readers_producers(self):
        """-> (buffer id -> the nodes that read it, buffer id -> the nodes that write it)"""
        readers, producers = {}, {}
        for m in self.net.nodes:
            for v in ((m.x, getattr(m, 'residual', None)) if m.kind == 'conv' else (m.x,)):
                if v is not None:
                    readers.setdefault(v.buf.id, []).append(m)
            if m.kind != 'head':
                producers.setdefault(m.y.buf.id, []).append(m)
        return readers, producers

    def _conv_producer(self, buf_id):
        """the one conv -> BN -> ReLU whose whole, private output tensor `buf_id` is (None: there is none, or not that simple)"""
        prod = [c for c in self.net.nodes if c.kind == 'conv' and c.y.buf.id == buf_id]
        if len(prod) == 1 and prod[0].y.is_full and prod[0].relu and prod[0].residual is None:
            return prod[0]
        return None

    def _pool_candidates(self):
        """conv node -> (pool node, its index): conv -> BN -> ReLU whose activation feeds ONLY a 3x3/stride-2 max pool (inception
        Conv2d_2b / Conv2d_4a, the resnet stem) -- in training the activation and its gradient are never materialised
        (bn_apply_maxpool / bn_bwd_maxpool).  The candidates, whatever the switches say"""
        cand = {}
        for kk, m in enumerate(self.net.nodes):
            if (m.kind == 'max' and m.R == 3 and m.S == 3 and m.sh == 2 and m.sw == 2 and m.ph <= 1 and m.pw <= 1
                    and m.x.is_full and len(self.readers.get(m.x.buf.id, ())) == 1):
                prod = self._conv_producer(m.x.buf.id)
                if prod is not None and prod.group is None and bool(prod.aux) == bool(m.aux):
                    cand[prod] = (m, kk)
        return cand

    def _fused_pool_eval(self, pool_cand):
        """eval twin: conv + folded BatchNorm + ReLU + that max pool in ONE kernel where the row-streaming conv serves the layer
        (inception Conv2d_2b -> maxpool1): the 708 MB activation of a batch of 256 is neither written nor read back"""
        e, fused = self.e, {}
        if self.fuse_pool_eval:
            for cn, (pn, _pk) in pool_cand.items():
                if (pn.ph == 0 and pn.pw == 0 and cn.y.buf.C == cn.K
                        and e.ctx.lib.ifcbk_conv2d_fwd_affine_maxpool_ok(C.byref(e._conv_desc(cn, self.N)))):
                    fused[cn] = pn
        return fused

    def _bnstat_consumers(self):
        """conv c whose input is the private BN+ReLU activation of conv n: c's input-gradient kernel also reduces n's BN
        backward sums in its epilogue (ifcbk_conv2d_dgrad_bnstat) and n's BN backward skips its reduction pass"""
        e, of = self.e, {}
        if self.fuse_bnstat != '1':
            return of
        for c in self.net.nodes:
            if c.kind != 'conv' or c.group is not None or c.x.buf.is_input or not c.x.is_full:
                continue
            if len(self.readers.get(c.x.buf.id, ())) != 1:
                continue
            prod = self._conv_producer(c.x.buf.id)
            if (prod is not None and prod not in self.fused_pool and bool(prod.aux) == bool(c.aux)
                    and e._conv_desc(c, self.N).C == c.x.C      # not the flattened full-cover form: its 'channels' are (tap, c)
                    and e.ctx.lib.ifcbk_conv2d_dgrad_bnstat_mblocks(C.byref(e._conv_desc(c, self.N))) > 0):
                of[c] = prod
        return of

    def _assign_lanes(self, nl):
        """node -> lane: every chain of nodes that hangs off a shared tensor (an Inception block input, a resnet block input) gets a
        lane, round-robin; a node fed by a private tensor stays on its producer's lane.  Chains in order of appearance -- lane 0 (the
        caller's stream, where the sibling GEMMs and their gradients run) takes the light 1x1 branch, the heavy chains land on lanes 1
        and 2.  Putting the HEAVIEST chain of every block on lane 0 (round 2) or rotating the lanes so that a block's GEMM follows the
        previous block's heaviest chain on the same stream (round 3) both lose ~1 ms per step: the event wait they save
        is cheaper than what they serialise."""
        nodes = self.net.nodes
        head_of = {}
        for m in nodes:                           # forward order: a follower's producer is already resolved
            if m.aux or m.kind == 'head':
                continue
            prods = self.producers.get(m.x.buf.id, [])
            follows = (len(prods) == 1 and prods[0].y.is_full and m.x.is_full and len(self.readers.get(m.x.buf.id, ())) == 1
                       and not prods[0].aux and prods[0] in head_of)
            head_of[m] = head_of[prods[0]] if follows else m
        by_tensor = {}
        for m in nodes:
            if head_of.get(m) is m:
                by_tensor.setdefault(m.x.buf.id, []).append(m)
        rank = {h: k for heads in by_tensor.values() for k, h in enumerate(heads)}
        # (the auxiliary classifier -- pool, 2 convs, fc -- runs beside Mixed_7a..7c on lane 1)
        return {m: 1 % nl if m.aux else 0 if m.kind == 'head' else rank[head_of[m]] % nl for m in nodes}

    # ------------------------------------------------------------------ what the emitters share
    def _a(self, view, grad=False):
        return self.e._aptr(view, grad)

    def _wk(self, n):
        return _vp(self.e.Wsh, self.e.esize * n.w_off)

    def _wT(self, n):
        return _vp(self.e.Wsh, self.e.esize * n.wT_off)

    def _acc(self, buf):
        """accumulate flag of a write into the gradient of `buf`: 0 for its first writer of this backward pass"""
        a = ops.FLAG_ACC if buf.id in self.written else 0
        self.written.add(buf.id)
        return a

    def _bn_desc(self, n):
        return BnDesc(self.N * n.P * n.Q, n.K, self.e._raw_ptr(n)[1], n.y.buf.C, 1 if n.relu else 0, self.e.cdtype, n.eps, 0.1)

    def _bnr_desc(self, n):
        return BnDesc(self.N * n.x.H * n.x.W, n.K, n.x.buf.C, n.K, 1 if n.relu else 0, self.e.cdtype, n.eps, 0.1)

    def _bn_finalize(self, lst, n, bnd, part=None, i=(0,), lane=0, rpart=None):
        """BatchNorm finalize of n: batch statistics from the partial sums `part` (resource `rpart`) into the training scale / shift, or
        -- no partials, evalprep -- the running statistics folded into the eval scale / shift"""
        e, bk = self.e, n.bn_key
        st = [e._stat(n, j) for j in range(4)] if part is not None else [None, None, e._stat(n, 4), e._stat(n, 5)]
        rs, rv = _vp(e.bviews[bk + '.running_mean']), _vp(e.bviews[bk + '.running_var'])
        lst.add(_lib.OP_BN_FINALIZE, n.name, p=[part, e._pptr(bk + '.weight'), e._pptr(bk + '.bias'), rs, rv] + st, i=i, bn=bnd, lane=lane,
                reads=None if part is None else [rpart], writes=None if part is None else [rst(n)])

    def _bn_apply(self, lst, n, bnd, x, train, lane, reads, res=None, ldr=0):
        lst.add(_lib.OP_BN_APPLY, n.name, p=(x, self.e._stat(n, 2 if train else 4), self.e._stat(n, 3 if train else 5), res, self._a(n.y)),
                i=(ldr,), bn=bnd, lane=lane, reads=reads, writes=[ra(n.y)])

    def _pool_affine(self, n, lane):
        """eval, commuted pool branch: the average pool on the branch's slice of the sibling tensor, eval-BN affine + ReLU in its epilogue"""
        e, cp = self.e, n.cpool
        pre, ldpre = e._pre_ptr(n)
        ppd = PoolDesc(self.N, cp.x.H, cp.x.W, n.K, ldpre, 3, 3, 1, 1, 1, 1, cp.P, cp.Q, n.y.buf.C, e.cdtype)
        self.fwd_e.add(_lib.OP_AVGPOOL_AFFINE, cp.name + '(' + n.name + ')', p=(pre, e._stat(n, 4), e._stat(n, 5), self._a(n.y)),
                       flags=ops.FLAG_RELU if n.relu else 0, pool=ppd, lane=lane, reads=[rpre(n)], writes=[ra(n.y)])

    def _pack_op(self, n, d):
        """the weight_pack of a conv / plain layer: fp32 master -> shadow (and its transpose, where an input gradient reads one)"""
        e, wT = self.e, (None if n.x.buf.is_input else self._wT(n))
        if n.kind == 'conv':
            key, ld, dp = n.conv_key, n.wT_ld, d
        else:
            key, ld, dp = n.key, (n.K if n.K != n.K_real else 0), e._pack_desc(n, d)      # wT rows keep the PADDED stride
        self.pack.add(_lib.OP_WEIGHT_PACK, n.name, p=(e._pptr(key + '.weight'), self._wk(n), wT), i=(ld,), conv=dp)

    # ------------------------------------------------------------------ forward emitters, one per node kind
    def _fwd_conv(self, k, n):
        d = self.e._conv_desc(n, self.N)
        self._train_conv(n, d)
        if not n.aux:
            self._eval_conv(n, d)
        self._bn_finalize(self.evalprep, n, self._bn_desc(n))
        self._pack_op(n, d)

    def _eval_conv(self, n, d):
        """inference: eval-BN affine (+residual) + ReLU fused into the conv epilogue; no raw tensor"""
        e, lst, Le, g = self.e, self.fwd_e, self.lane_eval[n], n.group
        relu, scale, shift = (ops.FLAG_RELU if n.relu else 0), e._stat(n, 4), e._stat(n, 5)
        if g is not None and e.eval_groups:
            if g.members[0] is n:
                self._eval_siblings(g, Le)
            if n.cpool is not None:
                self._pool_affine(n, Le)
        elif n.cpool is not None:
            # the commuted pool branch without the sibling GEMM: plain 1x1 conv of the block input into the branch's slice of the
            # sibling tensor, then its pool
            cp = n.cpool
            pre, ldpre = e._pre_ptr(n)
            dpre = ConvDesc(self.N, cp.x.H, cp.x.W, cp.x.C, cp.x.buf.C, n.K, 1, 1, 1, 1, 0, 0, n.P, n.Q, ldpre, n.Cw, e.cdtype)
            lst.add(_lib.OP_CONV_FWD, n.name, p=(self._a(cp.x), self._wk(n), pre, None), conv=dpre, lane=Le, reads=[ra(cp.x)], writes=[rpre(n)])
            self._pool_affine(n, Le)
        elif self.u8 is n:
            lst.add(_lib.OP_STEM_U8_FWD, n.name,
                    p=(_vp(e.in_u8[e.in_slot]), e._pptr(n.conv_key + '.weight'), _vp(e.in_ab[e.in_slot]), self._a(n.y), None, scale, shift),
                    flags=relu, conv=d, lane=Le, reads=[ra(n.x)], writes=[ra(n.y)])
        elif n in self.fused_pool_eval:
            pn = self.fused_pool_eval[n]
            lst.add(_lib.OP_CONV_FWD_AFFINE_MAXPOOL, n.name + '+' + pn.name, p=(self._a(n.x), self._wk(n), self._a(pn.y), scale, shift),
                    i=(pn.y.buf.C,), flags=relu, conv=d, lane=Le, reads=[ra(n.x)], writes=[ra(pn.y)])
        else:
            res = n.residual
            lst.add(_lib.OP_CONV_FWD_AFFINE, n.name,
                    p=(self._a(n.x), self._wk(n), self._a(n.y), scale, shift, self._a(res) if res is not None else None),
                    i=(res.buf.C if res is not None else 0,), flags=relu, conv=d, lane=Le,
                    reads=[ra(n.x)] + ([ra(res)] if res is not None else []), writes=[ra(n.y)])

    def _eval_siblings(self, g, lane):
        """inference: the sibling 1x1 convs of a block as ONE GEMM with per-segment destinations (ifcbk_conv2d_fwd_affine_segments):
        members with their folded BatchNorm + ReLU straight into their output tensors, a commuted pool branch raw into its slice of
        the sibling tensor (its pool applies the affine)"""
        e, ys, iv, wr = self.e, [], [], []
        for m in g.members:
            if m.cpool is not None:
                pre, ldpre = e._pre_ptr(m)
                ys.append(pre); iv.append(m.K | (ldpre << 20)); wr.append(rpre(m))
            else:
                ys.append(self._a(m.y)); iv.append(m.K | (m.y.buf.C << 20) | (1 << 40)); wr.append(ra(m.y))
        ys += [None] * (4 - len(ys))
        iv += [0] * (4 - len(iv))
        self.fwd_e.add(_lib.OP_CONV_FWD_AFFINE_SEG, '+'.join(m.name for m in g.members),
                       p=[self._a(g.x), _vp(e.Wsh, e.esize * g.w_off)] + ys + [e._stat(g.members[0], 4), e._stat(g.members[0], 5)],
                       i=iv, conv=e._group_desc(g, self.N), lane=lane, reads=[ra(g.x)], writes=wr)

    def _train_conv(self, n, d):
        """training: the conv writes its raw output and partial BatchNorm sums, finalize, then apply (+residual) (+ReLU)"""
        e, lst, L = self.e, self.fwd_t, self.lane_of[n]
        if n.group is not None:
            if n.group.members[0] is n:
                self._train_siblings(n.group)         # (the other members are emitted with the group's first)
            return
        raw, ldraw = e._raw_ptr(n)
        dfw = ConvDesc.from_buffer_copy(d)
        dfw.ldy = ldraw
        bnd, part = self._bn_desc(n), _vp(e.bn_part[L])
        if self.u8 is n:
            mb = e.ctx.lib.ifcbk_stem_u8_rows(C.byref(d))
            lst.add(_lib.OP_STEM_U8_FWD, n.name,
                    p=(_vp(e.in_u8[e.in_slot]), e._pptr(n.conv_key + '.weight'), _vp(e.in_ab[e.in_slot]), raw, part, None, None),
                    conv=dfw, lane=L, reads=[ra(n.x)], writes=[rraw(n), rbp(L)])
        else:
            mb = e.ctx.lib.ifcbk_conv2d_fwd_mblocks(C.byref(d))
            lst.add(_lib.OP_CONV_FWD, n.name, p=(self._a(n.x), self._wk(n), raw, part), conv=dfw, lane=L, reads=[ra(n.x)], writes=[rraw(n), rbp(L)])
        self._bn_finalize(lst, n, bnd, part, (mb,), L, rbp(L))
        if n in self.fused_pool:
            pn, pk = self.fused_pool[n]
            ppd = PoolDesc(self.N, pn.x.H, pn.x.W, pn.x.C, ldraw, 3, 3, 2, 2, pn.ph, pn.pw, pn.P, pn.Q, pn.y.buf.C, e.cdtype)
            lst.add(_lib.OP_BN_APPLY_MAXPOOL, n.name + '+' + pn.name, p=(raw, e._stat(n, 2), e._stat(n, 3), self._a(pn.y), _vp(e.argmax[pk])),
                    i=(1,), pool=ppd, lane=L, reads=[rraw(n), rst(n)], writes=[ra(pn.y), ram(pk)])
            return
        res = n.residual
        self._bn_apply(lst, n, bnd, raw, True, L, [rraw(n), rst(n)] + ([ra(res)] if res is not None else []),
                       self._a(res) if res is not None else None, res.buf.C if res is not None else 0)

    def _train_siblings(self, g):
        """training: ONE GEMM for all sibling 1x1 convs (lane 0), then each branch's BatchNorm on its channel slice, on its lane"""
        e, lst, N = self.e, self.fwd_t, self.N
        gd = e._group_desc(g, N)
        gmb = e.ctx.lib.ifcbk_conv2d_fwd_mblocks(C.byref(gd))
        lst.add(_lib.OP_CONV_FWD, '+'.join(m.name for m in g.members), p=(self._a(g.x), _vp(e.Wsh, e.esize * g.w_off), _vp(g.raw), _vp(e.bn_part[0])),
                conv=gd, lane=0, reads=[ra(g.x)], writes=[('gr', id(g), 0, g.Ktot), rbp(0)])
        for m in g.members:
            Lm, mbnd = self.lane_of[m], self._bn_desc(m)
            mraw, mld = e._raw_ptr(m)
            if m.cpool is not None:
                # commuted pool branch: pool the conv's slice of the merged tensor, then BatchNorm the pooled tensor
                pn = m.cpool
                pre, ldpre = e._pre_ptr(m)
                ppd = PoolDesc(N, pn.x.H, pn.x.W, m.K, ldpre, 3, 3, 1, 1, 1, 1, pn.P, pn.Q, mld, e.cdtype)
                lst.add(_lib.OP_AVGPOOL_FWD, pn.name + '(' + m.name + ')', p=(pre, mraw), pool=ppd, lane=Lm, reads=[rpre(m)], writes=[rraw(m)])
                lst.add(_lib.OP_BN_STATS, m.name, p=(mraw, _vp(e.bn_part[Lm])), bn=mbnd, lane=Lm, reads=[rraw(m)], writes=[rbp(Lm)])
                self._bn_finalize(lst, m, mbnd, _vp(e.bn_part[Lm]), (e.ctx.lib.ifcbk_bn_stats_rows(mbnd.M), m.K), Lm, rbp(Lm))
            else:
                # (one finalize per member, not per group: with all 29 member finalizes of the training forward REMOVED
                # -- timing only -- the step gains 0.15-0.22 ms; merging them into 11 launches could recover part of that)
                self._bn_finalize(lst, m, mbnd, _vp(e.bn_part[0], 4 * m.koff), (gmb, g.Ktot), Lm, rbp(0))
            self._bn_apply(lst, m, mbnd, mraw, True, Lm, [rraw(m), rst(m)])

    def _fwd_pool(self, k, n):
        if n in self.e.absorbed_pools:
            return                    # runs behind its 1x1 conv, on that conv's output (Engine._alloc_params)
        pd = self._pool_desc(n)
        # a fused max pool is done by the producing conv: its bn_apply_maxpool in training, its epilogue in eval
        if n not in self.fused_pool_nodes:
            self._pool_fwd(self.fwd_t, k, n, pd, self.lane_of[n], _vp(self.e.argmax[k]) if n.kind == 'max' else None)
        if not n.aux and n not in self.fused_pool_eval_nodes:
            self._pool_fwd(self.fwd_e, k, n, pd, self.lane_eval[n], None)

    def _pool_desc(self, n):
        return PoolDesc(self.N, n.x.H, n.x.W, n.x.C, n.x.buf.C, n.R, n.S, n.sh, n.sw, n.ph, n.pw, n.P, n.Q, n.y.buf.C, self.e.cdtype)

    def _pool_fwd(self, lst, k, n, pd, lane, argmax):
        if n.kind == 'max':
            lst.add(_lib.OP_MAXPOOL_FWD, n.name, p=(self._a(n.x), self._a(n.y), argmax), pool=pd, lane=lane, reads=[ra(n.x)],
                    writes=[ra(n.y), ram(k)])
        else:
            lst.add(_lib.OP_AVGPOOL_FWD, n.name, p=(self._a(n.x), self._a(n.y)), pool=pd, lane=lane, reads=[ra(n.x)], writes=[ra(n.y)])

    def _head_desc(self, n):
        return HeadDesc(self.N, n.HW, n.C, n.x.buf.C, n.NC, self.e.cdtype, 2.0)

    def _fwd_head(self, k, n):
        e = self.e
        for lst, lane, mask in ((self.fwd_t, self.lane_of[n], _vp(n.mask) if n.dropout else None),) + \
                (() if n.aux else ((self.fwd_e, self.lane_eval[n], None),)):
            lst.add(_lib.OP_HEAD_FWD, n.name,
                    p=(self._a(n.x), mask, e._pptr(n.key + '.weight') if n.fc else None, e._pptr(n.key + '.bias') if n.fc else None,
                       _vp(n.feat), _vp(n.logits)), head=self._head_desc(n), lane=lane, reads=[ra(n.x)], writes=[('hd', id(n), 0, 1)])

    def _fwd_cb(self, k, n):
        """conv (+bias) (+ReLU) without BatchNorm: the bias is the epilogue's shift (scale = 1), read from the fp32 master"""
        e, d = self.e, self.e._conv_desc(n, self.N)
        for lst, lane in ((self.fwd_t, self.lane_of[n]), (self.fwd_e, self.lane_eval[n])):
            if n.bias or n.relu:
                lst.add(_lib.OP_CONV_FWD_AFFINE, n.name, p=(self._a(n.x), self._wk(n), self._a(n.y), _vp(e.ones),
                           e._pptr(n.key + '.bias') if n.bias else _vp(e.zeros_k(n.K)), None),
                        i=(0,), flags=ops.FLAG_RELU if n.relu else 0, conv=d, lane=lane, reads=[ra(n.x)], writes=[ra(n.y)])
            else:
                lst.add(_lib.OP_CONV_FWD, n.name, p=(self._a(n.x), self._wk(n), self._a(n.y), None), conv=d, lane=lane,
                        reads=[ra(n.x)], writes=[ra(n.y)])
        self._pack_op(n, d)

    def _fwd_drop(self, k, n):
        for lst, lane, mask in ((self.fwd_t, self.lane_of[n], _vp(n.mask)), (self.fwd_e, self.lane_eval[n], None)):
            lst.add(_lib.OP_DROPOUT, n.name, p=(self._a(n.x), mask, self._a(n.y)), i=(self.N * n.x.H * n.x.W * n.x.C, self.e.cdtype),
                    f=(1.0 / (1.0 - n.p),), lane=lane, reads=[ra(n.x), ('dm', id(n), 0, 1)], writes=[ra(n.y)])

    def _flat_i(self, n):
        return (self.N, n.x.H * n.x.W, n.x.C, n.x.buf.C | (self.e.cdtype << 32))

    def _fwd_flat(self, k, n):
        for lst, lane in ((self.fwd_t, self.lane_of[n]), (self.fwd_e, self.lane_eval[n])):
            lst.add(_lib.OP_FLATTEN_CHW, n.name, p=(self._a(n.x), self._a(n.y)), i=self._flat_i(n), flags=ops.FLAG_TO_CHW, lane=lane,
                    reads=[ra(n.x)], writes=[ra(n.y)])

    def _fwd_bnr(self, k, n):
        """BatchNorm -> ReLU in FRONT of a conv, on a channel slice of a concatenation (densenet)"""
        e, L, bnd, xp = self.e, self.lane_of[n], self._bnr_desc(n), self._a(n.x)
        self.fwd_t.add(_lib.OP_BN_STATS, n.name, p=(xp, _vp(e.bn_part[L])), bn=bnd, lane=L, reads=[ra(n.x)], writes=[rbp(L)])
        self._bn_finalize(self.fwd_t, n, bnd, _vp(e.bn_part[L]), (e.ctx.lib.ifcbk_bn_stats_rows(bnd.M), n.K), L, rbp(L))
        self._bn_apply(self.fwd_t, n, bnd, xp, True, L, [ra(n.x), rst(n)])
        self._bn_apply(self.fwd_e, n, bnd, xp, False, self.lane_eval[n], [ra(n.x), rst(n)])
        self._bn_finalize(self.evalprep, n, bnd)

    # ------------------------------------------------------------------ weight-gradient groups
    def _group_weight_gradients(self):
        """-> the WgradGroups of this plan (round 4): the wide-tile wgrads of one block that share a channel tile run as ONE split-K
        grid (ifcbk_conv2d_wgrad_group) behind the block's LAST such layer -- 1/n of the slab traffic and reduce work per layer.  Each
        member keeps its d(raw) in a buffer of its own until the group has run: carved here, members first, in group order"""
        e, groups = self.e, []
        if not self.group_wgrads:
            return groups
        buckets = {}
        for n in reversed(e.convs):
            if n.group is not None or n.aux or self.u8 is n:
                continue
            dbw = e._conv_desc(n, self.N)
            dbw.ldy = n.K
            khv = e.ctx.lib.ifcbk_conv2d_wgrad_group_member_kh(C.byref(dbw))
            if khv <= 0:
                continue
            key = n.name.split('.')[0] if self.net.name == 'inception_v3' else n.name.rsplit('.', 1)[0]
            buckets.setdefault((key, khv), []).append((n, dbw))
        for (key, khv), mem in buckets.items():
            for c0 in range(0, len(mem), 6):
                part = mem[c0:c0 + 6]
                if len(part) < 2:
                    continue
                members, descs = [m for m, _d in part], [d for _m, d in part]
                need = e.ctx.lib.ifcbk_conv2d_wgrad_group_workspace(len(part), (ConvDesc * len(part))(*descs))
                if need == 0:
                    continue                      # the library keeps such layers on their single launches
                groups.append(WgradGroup(members, descs, need, khv, key))
                self.wg_of.update((m, groups[-1]) for m in members)
        if groups:
            # (a growth here moves the arenas under the graphs of the plans built so far: _grow_workspace drops them)
            e._grow_workspace(e.ctx, max(gq.ws for gq in groups))
            for gq in groups:
                for m in gq.members:
                    e.own_draw(m)
        return groups

    # ------------------------------------------------------------------ backward emitters, one per node kind
    def _bwd_head(self, k, n):
        e = self.e
        wkey, bkey = n.key + '.weight', n.key + '.bias'
        assert n.x.is_full
        acc = self._acc(n.x.buf)
        assert acc == 0, 'head must be the first writer of its input gradient'
        self.bwd.add(_lib.OP_HEAD_BWD, n.name, p=(_vp(n.dlogits), _vp(n.feat), _vp(n.mask) if n.dropout else None, e._pptr(wkey) if n.fc else None,
                        e._pptr(wkey, 'G') if n.fc else None, e._pptr(bkey, 'G') if n.fc else None, self._a(n.x, True)),
                     i=(n.x.buf.C,), head=self._head_desc(n), lane=self.lane_of[n], reads=[('hd', id(n), 0, 1)], writes=[rg(n.x)])

    def _bwd_cb(self, k, n):
        e, bwd, L = self.e, self.bwd, self.lane_of[n]
        d = e._conv_desc(n, self.N)
        dy, ldy = self._a(n.y, True), n.y.buf.C
        if n.relu or n.bias:
            # dz = dy * (y > 0) in place, dbias = column sums of dz
            bnd = BnDesc(self.N * n.P * n.Q, n.K, ldy, ldy, 1 if n.relu else 0, e.cdtype, 0.0, 0.0)
            bwd.add(_lib.OP_BIAS_RELU_BWD, n.name, p=(self._a(n.y), dy, dy if n.relu else None, e._pptr(n.key + '.bias', 'G') if n.bias else None),
                    i=(ldy,), bn=bnd, lane=L, reads=[ra(n.y), rg(n.y)], writes=[rg(n.y)])
        bwd.add(_lib.OP_CONV_WGRAD, n.name, p=(self._a(n.x), dy, e._pptr(n.key + '.weight', 'G')), conv=d, lane=L,
                reads=[ra(n.x), rg(n.y)], writes=[])
        if not n.x.buf.is_input:
            assert n.x.is_full
            bwd.add(_lib.OP_CONV_DGRAD, n.name, p=(dy, self._wT(n), self._a(n.x, True)), flags=self._acc(n.x.buf), conv=d, lane=L,
                    reads=[rg(n.y)], writes=[rg(n.x)])

    def _bwd_drop(self, k, n):
        self.bwd.add(_lib.OP_DROPOUT, n.name, p=(self._a(n.y, True), _vp(n.mask), self._a(n.x, True)),
                     i=(self.N * n.x.H * n.x.W * n.x.C, self.e.cdtype), f=(1.0 / (1.0 - n.p),), flags=self._acc(n.x.buf),
                     lane=self.lane_of[n], reads=[rg(n.y), ('dm', id(n), 0, 1)], writes=[rg(n.x)])

    def _bwd_flat(self, k, n):
        assert n.x.is_full
        self.bwd.add(_lib.OP_FLATTEN_CHW, n.name, p=(self._a(n.x, True), self._a(n.y, True)), i=self._flat_i(n),
                     flags=self._acc(n.x.buf), lane=self.lane_of[n], reads=[rg(n.y)], writes=[rg(n.x)])

    def _bwd_bnr(self, k, n):
        e, bkey = self.e, n.bn_key
        # the slice's gradient: the FIRST backward op that touches the concatenation must cover all of it (densenet: the
        # transition / norm5 that reads the whole block output); later (= earlier-in-forward) layers accumulate
        if n.x.buf.id not in self.written:
            assert n.x.is_full, 'the first gradient written into a concatenation must cover all of it: ' + n.name
        acc = self._acc(n.x.buf)
        self.bwd.add(_lib.OP_BN_BWD, n.name, p=(self._a(n.x), self._a(n.y), self._a(n.y, True), e._pptr(bkey + '.weight'),
                        e._stat(n, 0), e._stat(n, 1), self._a(n.x, True), None, e._pptr(bkey + '.weight', 'G'),
                        e._pptr(bkey + '.bias', 'G'), e._stat(n, 2), e._stat(n, 3)),
                     i=(n.K, n.x.buf.C, 0), flags=ops.FLAG_DX_ACC if acc else 0, bn=self._bnr_desc(n), lane=self.lane_of[n],
                     reads=[ra(n.x), ra(n.y), rg(n.y), rst(n)], writes=[rg(n.x)])

    def _bwd_pool(self, k, n):
        assert n.x.is_full
        if n in self.fused_pool_nodes:
            return                        # gathered inside the producer's bn_bwd_maxpool
        if n in self.e.absorbed_pools:
            return                        # its gradient reaches x through the sibling GEMM's input gradient
        acc, pd, L = self._acc(n.x.buf), self._pool_desc(n), self.lane_of[n]
        if n.kind == 'max':
            self.bwd.add(_lib.OP_MAXPOOL_BWD, n.name, p=(self._a(n.y, True), _vp(self.e.argmax[k]), self._a(n.x, True)), flags=acc,
                         pool=pd, lane=L, reads=[rg(n.y), ram(k)], writes=[rg(n.x)])
        else:
            self.bwd.add(_lib.OP_AVGPOOL_BWD, n.name, p=(self._a(n.y, True), self._a(n.x, True)), flags=acc, pool=pd,
                         lane=L, reads=[rg(n.y)], writes=[rg(n.x)])

    def _bwd_conv(self, k, n):
        """BatchNorm backward into d(raw), then the conv's weight and input gradients (a sibling GEMM's: behind its first member)"""
        e, grp = self.e, n.group
        # d(raw): in a buffer of the node's own until the (grouped / lane's) weight gradient has read it, else the sibling group's merged
        # tensor, else the lane's scratch
        own = n in self.wg_of or (e.wgrad_lane and (grp is None or n.cpool is not None))
        if own:
            draw, rdraw = _vp(e.own_draw(n)), [('drawn', id(n), 0, 1)]
        elif grp is not None and n.cpool is None:
            draw, rdraw = _vp(e.group_draw(grp), e.esize * n.koff), [rdg(n)]
        else:
            draw, rdraw = _vp(e.draw[self.lane_of[n]]), [('draw', self.lane_of[n], 0, 1)]
        LW = self.lane_of[n] if grp is None else 0        # lane of this node's weight gradient: its own (a sibling GEMM's: 0), or ...
        if e.wgrad_lane:
            LW = self.WLs[self.wl_next % len(self.WLs)]       # ... round-robin over the weight-gradient lanes, per NODE
            self.wl_next += 1
        self._bn_bwd(n, draw, rdraw)
        if n.cpool is not None:
            # d(pooled conv output) -> d(conv output): the average pool is its own transpose; into the branch's slice of
            # the merged d(raw) scratch, from where the sibling GEMM's weight / input gradients pick it up
            pn = n.cpool
            ppd = PoolDesc(self.N, pn.x.H, pn.x.W, n.K, grp.Ktot, 3, 3, 1, 1, 1, 1, pn.P, pn.Q, n.K, e.cdtype)
            self.bwd.add(_lib.OP_AVGPOOL_BWD, pn.name + '(' + n.name + ')', p=(draw, _vp(e.group_draw(grp), e.esize * n.koff)),
                         flags=0, pool=ppd, lane=self.lane_of[n], reads=rdraw, writes=[rdg(n)])
        if grp is not None:
            if grp.members[0] is n:
                self._siblings_bwd(grp, LW)
            return
        dbw = e._conv_desc(n, self.N)
        dbw.ldy = n.K                       # dy of the conv = the dense d(raw) scratch
        self._wgrad(n, dbw, draw, rdraw, LW)
        if not n.x.buf.is_input:
            self._dgrad(n, dbw, draw, rdraw)

    def _bn_bwd(self, n, draw, rdraw):
        """BatchNorm (+ReLU) backward into d(raw): through the fused max pool, from its consumer's partial sums, or plain (+ residual)"""
        e, L, grp, bkey = self.e, self.lane_of[n], n.group, n.bn_key
        res, dres_acc = n.residual, 0
        if res is not None:
            assert res.is_full
            dres_acc = self._acc(res.buf)
        ld = n.K if (grp is None or n.cpool is not None) else grp.Ktot
        rawp, ldraw = e._raw_ptr(n)
        w, dw, db = e._pptr(bkey + '.weight'), e._pptr(bkey + '.weight', 'G'), e._pptr(bkey + '.bias', 'G')
        st = [e._stat(n, j) for j in range(4)]
        if n in self.fused_pool:
            pn, pk = self.fused_pool[n]
            ppd = PoolDesc(self.N, pn.x.H, pn.x.W, pn.x.C, ldraw, 3, 3, 2, 2, pn.ph, pn.pw, pn.P, pn.Q, pn.y.buf.C, e.cdtype)
            self.bwd.add(_lib.OP_BN_BWD_MAXPOOL, n.name + '+' + pn.name, p=[rawp, self._a(pn.y, True), _vp(e.argmax[pk]), w] + st + [draw, dw, db],
                         i=(1, n.K), pool=ppd, lane=L, reads=[rraw(n), rg(pn.y), ram(pk), rst(n)], writes=rdraw)
        elif n in self.bnstat_done:
            bs = self.bnstat_done[n]
            self.bwd.add(_lib.OP_BN_BWD_PARTIALS, n.name, p=[rawp, self._a(n.y, True), w] + st + [bs['part'], draw, dw, db],
                         i=(n.y.buf.C, bs['rows'], ld, 0), bn=self._bn_desc(n), lane=L, reads=[rraw(n), rg(n.y), rst(n), bs['res']], writes=rdraw)
        else:
            self.bwd.add(_lib.OP_BN_BWD, n.name, p=[rawp, self._a(n.y), self._a(n.y, True), w, st[0], st[1], draw,
                            self._a(res, True) if res is not None else None, dw, db, st[2], st[3]],
                         i=(n.y.buf.C, ld, res.buf.C if res is not None else 0), flags=dres_acc, bn=self._bn_desc(n), lane=L,
                         reads=[rraw(n), ra(n.y), rg(n.y), rst(n)], writes=rdraw + ([rg(res)] if res is not None else []))

    def _siblings_bwd(self, grp, LW):
        """fused siblings: every member's d(raw) lies in its slice of the merged tensor; the member that comes FIRST in forward order
        is the last one in backward and launches the single weight gradient (per-member segments of G) and input gradient"""
        e = self.e
        gd, gdraw = e._group_desc(grp, self.N), _vp(e.group_draw(grp))
        tag, gres = '+'.join(m.name for m in grp.members), ('dg', id(grp), 0, grp.Ktot)
        self.bwd.add(_lib.OP_CONV_WGRAD_SEG, tag, p=[self._a(grp.x), gdraw] + [e._pptr(m.conv_key + '.weight', 'G') for m in grp.members],
                     i=[m.K for m in grp.members], conv=gd, lane=LW, reads=[ra(grp.x), gres], writes=[])
        self.bwd.add(_lib.OP_CONV_DGRAD, tag, p=(gdraw, _vp(e.Wsh, e.esize * grp.wT_off), self._a(grp.x, True)),
                     flags=self._acc(grp.x.buf), conv=gd, lane=0, reads=[gres], writes=[rg(grp.x)])

    def _wgrad(self, n, dbw, draw, rdraw, LW):
        """weight gradient of a conv outside a sibling GEMM: with its WgradGroup (behind its last member), from the u8 plane, or alone"""
        e, wgq, dw = self.e, self.wg_of.get(n), self.e._pptr(n.conv_key + '.weight', 'G')
        if wgq is not None:
            wgq.seen += 1
            if wgq.seen < len(wgq.members):
                return
            mem = wgq.members                      # every member's d(raw) exists now
            items = (_lib.WgradItem * len(mem))()
            for it, m, dq in zip(items, mem, wgq.descs):
                it.d, it.x, it.dy = dq, self._a(m.x).value, e.draw_own[m].data_ptr()
                it.dw = e._pptr(m.conv_key + '.weight', 'G').value
            self.keep.append(items)
            self.bwd.add(_lib.OP_CONV_WGRAD_GROUP, '+'.join(m.name for m in mem), p=[C.addressof(items)] + [it.dw for it in items],
                         i=(len(mem),), lane=LW, reads=[ra(m.x) for m in mem] + [('drawn', id(m), 0, 1) for m in mem], writes=[])
        elif self.u8 is n:
            self.bwd.add(_lib.OP_STEM_U8_WGRAD, n.name, p=(_vp(e.in_u8[e.in_slot]), draw, _vp(e.in_ab[e.in_slot]), dw), conv=dbw,
                         lane=LW, reads=[ra(n.x)] + rdraw, writes=[])
        else:
            self.bwd.add(_lib.OP_CONV_WGRAD, n.name, p=(self._a(n.x), draw, dw), conv=dbw, lane=LW, reads=[ra(n.x)] + rdraw, writes=[])

    def _dgrad(self, n, dbw, draw, rdraw):
        """input gradient of a conv outside a sibling GEMM; as first writer of a bnstat_of producer's activation gradient it also leaves
        that producer's BatchNorm backward sums (bnstat_done, which the producer's _bn_bwd is reached after)"""
        e, L = self.e, self.lane_of[n]
        assert n.x.is_full
        acc = self._acc(n.x.buf)
        if n in self.bnstat_of and acc == 0:
            pn = self.bnstat_of[n]
            prow, pld = e._raw_ptr(pn)
            part = _vp(e.bn_part[L])
            self.bwd.add(_lib.OP_CONV_DGRAD_BNSTAT, n.name,
                         p=[draw, self._wT(n), self._a(n.x, True), prow] + [e._stat(pn, j) for j in range(4)] + [part], i=(pld,),
                         conv=dbw, lane=L, reads=rdraw + [rraw(pn), rst(pn)], writes=[rg(n.x), rbp(L)])
            self.bnstat_done[pn] = dict(part=part, rows=e.ctx.lib.ifcbk_conv2d_dgrad_bnstat_mblocks(C.byref(dbw)), res=rbp(L))
        else:
            self.bwd.add(_lib.OP_CONV_DGRAD, n.name, p=(draw, self._wT(n), self._a(n.x, True)), flags=acc, conv=dbw, lane=L,
                         reads=rdraw, writes=[rg(n.x)])

    # ------------------------------------------------------------------ programs
    def _loss_ops(self):
        """-> (train loss ops CE(main) + 0.4*CE(aux), neuston_models.py:70-78; the validation loss op; the main head).  No lane
        annotation: loss ops are full barriers on lane 0, so their read-only operands need no resource entry"""
        e, N, NC = self.e, self.N, self.net.NC
        main = [h for h in e.heads if not h.aux][0]
        # an option adds its operands to the ops by name; which kernel a set of operands selects is the header's (IFCBK_OP_SOFTMAX_XENT)
        xent, p, f = _lib.OP_SOFTMAX_XENT, dict(target=_vp(e.target), loss=_vp(e.loss)), {}
        if e.class_weight is not None:                   # TRAIN --class-norm
            xent, p['class_weight'] = _lib.OP_SOFTMAX_XENT_W, _vp(e.class_weight)
        if e.label_smoothing > 0:                        # TRAIN --label-smoothing
            f['smoothing'] = e.label_smoothing
        if e.focal_gamma > 0:                            # TRAIN --focal-gamma (the engine refuses it together with smoothing)
            f['gamma'] = e.focal_gamma
        # the validation loss stays the one-target hard loss; both heads of inception_v3 distil from the teacher's one set of logits
        tp, tf = dict(p), dict(f)
        if e.mix:                                        # TRAIN --mixup / --cutmix
            tp['lam'] = _vp(e.mix_lam[e.in_slot])
        if e.distill is not None:                        # TRAIN --distill
            tp['teacher'] = _vp(e.teacher_logits)
            tf['alpha'], tf['temperature'] = e.distill
        lossl, evl = OpList(), OpList()
        for h in [main] + [h for h in e.heads if h.aux]:
            lossl.add(xent, 'loss_aux' if h.aux else 'loss', p=dict(tp, logits=_vp(h.logits), dlogits=_vp(h.dlogits)), i=(N, NC),
                      f=dict(tf, weight=0.4 if h.aux else 1.0), flags=ops.FLAG_ACC if h.aux else 0)
        evl.add(xent, 'val_loss', p=dict(p, logits=_vp(main.logits)), i=(N, NC), f=dict(f, weight=1.0))
        return lossl, evl, main

    def _optimizer_op(self, grad=None):
        e, opt = self.e, OpList()
        # step, grad_scale and ema_w are stamped per step (Engine._set_update), and with a schedule lr.  grad: the buffer the op reads
        # its gradient (and, clipping, takes its norm) from -- G, or the accumulator of TRAIN --accumulate
        p, f = dict(P=_vp(e.P), G=_vp(e.G if grad is None else grad)), dict(lr=e.lr, weight_decay=e.weight_decay, grad_scale=1.0)
        if e.ema_decay is not None:                      # TRAIN --ema: E at the offset of P (every bucket's op carries its slice)
            p['E'] = _vp(e.E)
        if e.clip_grad is not None:                      # TRAIN --clip-grad: the op takes the norm of the whole of G ahead of its update
            p['clip_state'], f['max_norm'] = _vp(e.clip_state), e.clip_grad
        if e.optimizer == 'sgd':
            # additive option (north_star "SGD/Adam step"; upstream only has Adam): torch.optim.SGD's update, momentum buffer = M
            opt.add(_lib.OP_SGD, 'sgd', p=dict(p, M=_vp(e.M) if e.momentum else None), i=dict(n=e.nparam_padded, step=1),
                    f=dict(f, momentum=e.momentum))
        else:
            # additive option (TRAIN --optimizer AdamW): the same op with its `decoupled` operand set -- weight_decay is then torch.optim.AdamW's
            i = dict(n=e.nparam_padded, step=1, **({'decoupled': 1} if e.optimizer == 'adamw' else {}))
            opt.add(_lib.OP_ADAM, e.optimizer, p=dict(p, M=_vp(e.M), V=_vp(e.V)), i=i,
                    f=dict(f, beta1=e.betas[0], beta2=e.betas[1], eps=e.eps))
        return opt

    def _assemble(self):
        e, fwd_t, bwd = self.e, self.fwd_t, self.bwd
        pl = Plan(self.N)
        pl.fwd_train, pl.fwd_eval, pl.bwd = Program(fwd_t), Program(self.fwd_e), Program(bwd)
        pack = e._pack_multi(self.pack)           # (self.pack: one OP_WEIGHT_PACK per conv -- the bucketed update cuts that list)
        pl.pack, pl.evalprep = Program(pack), Program(self.evalprep)
        lossl, evl, main = self._loss_ops()
        pl.loss, pl.eval_loss = Program(lossl), Program(evl)
        sm = OpList()
        sm.add(_lib.OP_SOFTMAX, 'softmax', p=(_vp(main.logits), _vp(e.probs)), i=(self.N, self.net.NC))
        pl.softmax = Program(sm)
        opt = self._optimizer_op()
        pl.adam = Program(opt)
        # the step's bookkeeping in the step's own op table: num_batches_tracked += 1 of every BatchNorm, loss_sum += loss
        cnt = OpList()
        cnt.add(_lib.OP_STEP_COUNTERS, 'step_counters', p=(_vp(e.nbt), _vp(e.loss_sum), _vp(e.loss)), i=(e.nbt.numel(),))
        # fused train step = fwd + loss + bwd + adam + pack (+ counters); round 5: the optimizer and the repack run PER BUCKET of the
        # flat gradient buffer, on the weight-gradient lane, as soon as backward has finished the bucket (_bucketed_update)
        pl.step = _program(fwd_t, lossl, *self._bucketed_update(bwd, opt, self.pack), cnt)
        pl.step_adam_idxs = pl.step.find(_lib.OP_SGD if e.optimizer == 'sgd' else _lib.OP_ADAM)
        pl.step_adam_idx = pl.step_adam_idxs[-1]
        # data-parallel variant: fwd+loss | backward segments (all-reduce launched after each) | adam+pack
        pl.fwd_loss = _program(fwd_t, lossl)
        pl.fwd_bwd = _program(fwd_t, lossl, bwd)   # the part of a train step whose launch arguments never change: hipGraph-capturable
        pl.adam_pack = _program(opt, pack, cnt)
        if e.accumulate > 1:
            # TRAIN --accumulate: every batch runs fwd_loss + bwd (or the fwd_bwd graph), the engine's ifcbk_grad_accum_flat call and the
            # counters alone; the window's one update reads the accumulator and is followed by the whole repack
            pl.acc_update = _program(self._optimizer_op(e.A), pack)
            pl.acc_count = Program(cnt)
        pl.bwd_list = bwd
        pl.keep = self.keep
        return pl

    def _bucket_opt(self, lst, opt, lo, hi, **sched):
        """the optimizer op over [lo, hi) of the flat buffers: the whole-buffer op with its slices of them (P, G, M, V, E) moved to lo and
        n = hi - lo.  Any other pointer (the clip state: a clipped plan takes the single update) has no per-bucket form"""
        o0 = opt.ops[0]
        row = ops.OPERANDS[o0.kind]
        p = {name: v + 4 * lo for name, v in zip(row['p'], o0.p) if v}
        assert set(p) <= set('PGMVE'), 'optimizer op with a pointer that is no slice of a flat buffer: %s' % sorted(set(p) - set('PGMVE'))
        lst.add(o0.kind, opt.tags[0] + '[%d:%d]' % (lo, hi), p=p, i=dict(zip(row['i'], o0.i), n=hi - lo), f=dict(zip(row['f'], o0.f)), **sched)

    def _packs_in(self, pack_ops, lo, hi):
        """the multi-tensor repack of the pack ops whose fp32 master lies in [lo, hi) of the flat buffer (an empty list: none does)"""
        pbase, sub = self.e.P.data_ptr(), OpList()
        for o, tg, mt in zip(pack_ops.ops, pack_ops.tags, pack_ops.meta):
            if lo <= (o.p[_PACK_MASTER] - pbase) // 4 < hi:
                sub.ops.append(o); sub.tags.append(tg); sub.meta.append(mt)
        return self.e._pack_multi(sub, key=(lo, hi)) if sub.ops else OpList()

    def _shadow_readers(self, bwd, pack_ops):
        """-> (parameter offset -> index of the last backward op that reads its shadow, backward op index -> its 'SH' reads): an input
        gradient reads its filter's shadow (a sibling group's: every member's).  None: a filter this plan cannot attribute"""
        e = self.e
        pbase, sbase = e.P.data_ptr(), e.Wsh.data_ptr()
        regions = [(g.wT_off, g.wT_off + g.Ktot * g.x.C) for g in e.groups]
        skey = lambda off: next((r0 for r0, r1 in regions if r0 <= off < r1), off)
        owners = {}
        for o in pack_ops.ops:
            if o.p[_PACK_WT]:
                owners.setdefault(skey((o.p[_PACK_WT] - sbase) // e.esize), []).append((o.p[_PACK_MASTER] - pbase) // 4)
        last_reader, shreads = {}, {}
        for k, o in enumerate(bwd.ops):
            if o.kind in _DGRAD_WT:
                own = owners.get(skey((o.p[_DGRAD_WT[o.kind]] - sbase) // e.esize))
                if own is None:
                    return None
                shreads[k] = [('SH', off, off + e.palloc[off]) for off in own]
                for off in own:
                    last_reader[off] = k
        return last_reader, shreads

    def _bucketed_update(self, bwd, opt, pack_ops):
        """-> (backward ops with the optimizer + repack of every finished gradient bucket inserted, the last bucket's optimizer, its
        repack).  Backward finishes the flat gradient buffer from its tail (dp.segment_plan: the cuts of the data-parallel exchange);
        a bucket's optimizer op and the repack of its conv weights go onto the weight-gradient lane right behind the ops that
        complete it -- and behind the last input-gradient op that reads a bf16 shadow of the bucket (the shadow is rewritten by the
        repack) -- so that only the last bucket (the stem: 4 % of the parameters) is updated behind the end of backward.  Same
        arithmetic per element as one launch over the whole buffer (Adam / SGD are element-wise; the step count is a launch
        argument of every bucket's op).  One launch at the end (IFCBK_OPT_BUCKETS <= 1, or no cut to be had): the three lists as given.
        With clipping (TRAIN --clip-grad) it is the one launch at the end as well: the coefficient of every element's update is a
        function of the norm of ALL of G, which exists only behind the last backward op, so no bucket can be updated beside backward
        (a per-bucket sum of squares beside backward, with only the update at the end, would win the norm's pass back: not done)"""
        e = self.e
        whole = (bwd, opt, e._pack_multi(pack_ops))
        if self.opt_buckets <= 1 or e.clip_grad is not None:
            return whole
        from .dp import segment_plan
        offs = [e._op_param_offsets(o) for o in bwd.ops]
        try:
            segs = segment_plan(offs, e.palloc, e.nparam_padded, self.opt_buckets)
        except RuntimeError:
            return whole
        shadows = self._shadow_readers(bwd, pack_ops) if len(segs) >= 2 else None
        if shadows is None:
            return whole
        last_reader, shreads = shadows
        LW = e.NL - 1 if e.wgrad_lane else 0
        inserts = {}                           # op index -> OpList to emit BEFORE that op (i.e. behind op index - 1)
        prev_ins = 0
        for (b0, b1, lo, hi) in segs[:-1]:
            prev_ins = ins = max([b1, prev_ins] + [1 + k for off, k in last_reader.items() if lo <= off < hi])
            ol = inserts.setdefault(ins, OpList())
            self._bucket_opt(ol, opt, lo, hi, lane=LW, reads=[('G', lo, hi)],
                             writes=[('P', lo, hi)] + ([('E', lo, hi)] if e.ema_decay is not None else []))
            pm = self._packs_in(pack_ops, lo, hi)
            if pm.ops:
                pm.meta[0] = (LW, [('P', lo, hi)], [('SH', lo, hi)])
                ol.extend(pm)
        out = OpList()
        for k, (o, tg, mt) in enumerate(zip(bwd.ops, bwd.tags, bwd.meta)):
            if k in inserts:
                out.extend(inserts[k])
            lane, reads, writes = mt
            if not (reads is None and writes is None):
                extra_w = [('G', off, off + e.palloc[off]) for off in offs[k]]
                mt = (lane, list(reads or ()) + shreads.get(k, []), list(writes or ()) + extra_w)
            out.ops.append(o); out.tags.append(tg); out.meta.append(mt)
        for k in sorted(inserts):
            if k >= len(bwd.ops):
                out.extend(inserts[k])
        # the last bucket: behind the end of backward, as full barriers (as the single update was)
        lo, hi = segs[-1][2], segs[-1][3]
        last_opt = OpList()
        self._bucket_opt(last_opt, opt, lo, hi)
        return (out, last_opt, self._packs_in(pack_ops, lo, hi))
