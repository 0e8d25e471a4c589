"""Declared resources against the pointers in the op tables (tests/program_footprints.py): in every frozen program of every family's
plan, two ops that touch common bytes -- at least one writing -- are ordered by the lane / wait bits that ctx.hip::run_lanes will
execute.  The footprints come from the op table (pointers + descriptors), not from the (lane, reads, writes) annotation, so an
annotation that forgets a pointer, names the wrong channel range or uses another key than its counterpart shows up as an
unordered pair.  Needs no GPU: Engine(plan_only=True)."""
import contextlib
import os
import random
from unittest import mock

import pytest

import program_footprints as pf
from ifcb_classifier_amd import _lib

PROGRAMS = ('fwd_train', 'fwd_eval', 'bwd', 'step', 'fwd_loss', 'fwd_bwd', 'pack', 'evalprep', 'loss', 'eval_loss', 'softmax', 'adam',
            'adam_pack')

# name -> (model, batch, environment, input kind)
CONFIGS = {
    'inception_v3-b2': ('inception_v3', 2, {}, 'nhwc'),
    'inception_v3-b2-u8': ('inception_v3', 2, {}, 'u8'),                     # the stem reads the resized u8 plane and the fp32 master filter
    'inception_v3-b64': ('inception_v3', 64, {}, 'nhwc'),                    # grouped weight gradients exist from this batch on
    'resnet18-b2': ('resnet18', 2, {}, 'nhwc'),
    'resnet50-b2': ('resnet50', 2, {}, 'nhwc'),
    'densenet121-b2': ('densenet121', 2, {}, 'nhwc'),
    'squeezenet1_1-b2': ('squeezenet', 2, {}, 'nhwc'),
    'vgg11_bn-b2': ('vgg11_bn', 2, {}, 'nhwc'),
    'alexnet-b2': ('alexnet', 2, {}, 'nhwc'),
    'inception_v3-b2-lanes2': ('inception_v3', 2, {'IFCBK_LANES': '2'}, 'nhwc'),
    'inception_v3-b2-opt_buckets1': ('inception_v3', 2, {'IFCBK_OPT_BUCKETS': '1'}, 'nhwc'),
}
_PLANS = {}


def _plan(cfg):
    if cfg not in _PLANS:
        import torch
        from ifcb_classifier_amd import graph
        from ifcb_classifier_amd.engine import Engine
        model, B, env, kind = CONFIGS[cfg]
        keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
        # batch 64 only: planning reads no tensor contents, and empty() keeps its ~5 GB of host buffers from being touched (as
        # tests/golden/make_plan_fingerprints.py does for batch 256).  The item tables the audit reads are not built from such
        # buffers: the pack table is a copy of a ctypes array, the weight-gradient items are a ctypes array
        cheap = [mock.patch.object(torch, 'zeros', torch.empty), mock.patch.object(torch, 'zeros_like', torch.empty_like)] if B >= 64 else []
        with mock.patch.dict(os.environ, dict(keep, **env), clear=True), contextlib.ExitStack() as stack:
            for c in cheap:
                stack.enter_context(c)
            eng = Engine(graph.build(model, 7), max_batch=B, plan_only=True)
            if kind == 'u8':
                assert eng.stem_u8 is not None
                eng.in_kind[eng.in_slot] = 'u8'
            _PLANS[cfg] = (eng, eng.plan(B))
    return _PLANS[cfg]


@pytest.mark.parametrize('cfg', sorted(CONFIGS))
def test_every_conflicting_pair_of_every_frozen_program_is_ordered(cfg):
    eng, pl = _plan(cfg)
    nfp = 0
    for prog in PROGRAMS:
        p = getattr(pl, prog)
        bad = pf.unordered_conflicts(eng, p.arr, p.n, p.tags)          # (raises for a kind without a row, a pointer outside every tensor)
        assert not bad, (cfg, prog, len(bad), bad[:6])
        nfp += sum(len(pf.op_footprints(pf.allocations(eng), p.arr[k], p.tags[k])) for k in range(p.n))
    assert nfp > 8 * pl.step.n > 300, (cfg, nfp)
    if cfg == 'inception_v3-b64':
        assert pl.step.find(_lib.OP_CONV_WGRAD_GROUP)
    if cfg == 'inception_v3-b2-u8':
        assert pl.step.find(_lib.OP_STEM_U8_FWD) and pl.step.find(_lib.OP_STEM_U8_WGRAD)
    if cfg.startswith(('inception', 'resnet', 'densenet', 'squeezenet')) and 'lanes2' not in cfg:
        # the audit is vacuous on a one-lane program: these plans really spread over lanes
        assert len({(pl.step.arr[k].flags >> 8) & 7 for k in range(pl.step.n)}) >= 3, cfg
        assert len({(pl.fwd_eval.arr[k].flags >> 8) & 7 for k in range(pl.fwd_eval.n)}) == 2, cfg


def test_every_kind_run_one_dispatches_has_a_row_and_a_kind_without_one_fails():
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(pf.__file__))), 'ifcb_classifier_amd', 'csrc', 'ctx.hip')).read()
    body = src[src.index('static int run_one('):src.index('// ---------------------------------------------------------------- program runner')]
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(pf.__file__))), 'include', 'ifcbk.h')).read()
    enum = re.sub(r'/\*.*?\*/', '', hdr[hdr.index('IFCBK_OP_CONV_FWD = 1'):hdr.index('typedef struct {\n    ifcbk_conv_desc d;')], flags=re.S)
    number = {name: k + 1 for k, name in enumerate(re.findall(r'IFCBK_OP_\w+', enum))}
    dispatched = {number[name] for name in re.findall(r'case (IFCBK_OP_\w+)\s*:', body)}
    assert len(dispatched) >= 38 and number['IFCBK_OP_SOFTMAX_XENT_W'] == _lib.OP_SOFTMAX_XENT_W
    assert dispatched == set(pf.ROLES), (sorted(dispatched - set(pf.ROLES)), sorted(set(pf.ROLES) - dispatched))
    eng, pl = _plan('resnet18-b2')
    o = _lib.Op.from_buffer_copy(pl.step.arr[0])
    o.kind = _lib.OP_RETIRED_31
    with pytest.raises(AssertionError, match='no row'):
        pf.op_footprints(pf.allocations(eng), o, 'x')
    o = _lib.Op.from_buffer_copy(pl.step.arr[0])
    o.p[0] = 4096                                    # no tensor of the engine lives there
    with pytest.raises(AssertionError, match='outside every tensor'):
        pf.op_footprints(pf.allocations(eng), o, 'x')


def test_overlap_geometry_is_exact_for_equal_pitch_and_conservative_otherwise():
    def cells(f):
        s, w, p, n = f
        return {s + r * p + c for r in range(n) for c in range(w)}
    rng = random.Random(7)
    nhit = nmiss = 0
    for _ in range(4000):
        pa = rng.choice([8, 12, 16])
        pb = pa if rng.random() < 0.7 else rng.choice([8, 12, 16])
        a = (rng.randrange(40), rng.randrange(1, pa + 1), pa, rng.randrange(1, 5))
        b = (rng.randrange(40), rng.randrange(1, pb + 1), pb, rng.randrange(1, 5))
        truth = bool(cells(a) & cells(b))
        got = pf._touch(a, b)
        if pa == pb:
            assert got == truth, (a, b)
            nhit += truth
            nmiss += not truth
        else:
            assert got or not truth, (a, b)
    assert nhit > 300 and nmiss > 300
    # two channel slices of one concatenation never touch; a slice and the whole buffer do
    assert not pf._touch((0, 64, 256, 10), (64, 192, 256, 10))
    assert pf._touch((0, 256 * 10, 256 * 10, 1), (64, 192, 256, 10))


# ---------------------------------------------------------------- negative controls: mutate the annotation, reschedule, audit
def _copy_meta(meta):
    return [(l, None if r is None else list(r), None if w is None else list(w)) for l, r, w in meta]


def _bwd():
    eng, pl = _plan('inception_v3-b2')
    return eng, pl.bwd_list


def test_control_a_removed_read_is_named():
    """a single-layer weight gradient (weight-gradient lane) loses the d(raw) entry of its reads: nothing orders it behind the
    BatchNorm backward that writes that d(raw) on the chain's lane"""
    from ifcb_classifier_amd.engine import schedule_lanes
    eng, bwd = _bwd()
    base = schedule_lanes(bwd.meta)
    j = next(k for k, o in enumerate(bwd.ops) if o.kind == _lib.OP_CONV_WGRAD and bwd.tags[k] == 'Mixed_6b.branch7x7_2.conv')
    i = next(k for k, o in enumerate(bwd.ops) if o.kind in (_lib.OP_BN_BWD, _lib.OP_BN_BWD_PARTIALS) and bwd.tags[k] == bwd.tags[j])
    assert i < j and base[i][0] != base[j][0] and base[j][1] >> base[i][0] & 1
    meta = _copy_meta(bwd.meta)
    drawn = [r for r in meta[j][1] if r[0] == 'drawn']
    assert len(drawn) == 1
    meta[j][1].remove(drawn[0])
    bad = pf.audit_oplist(eng, bwd, meta)
    pairs = {(a[:2], b[:2]) for a, b, _alloc in bad}
    assert pairs == {((bwd.tags[i], _lib.OP_NAMES[bwd.ops[i].kind]), (bwd.tags[j], 'conv_wgrad'))}, bad


def test_control_b_narrowed_channel_range_is_named():
    """the segmented weight gradient of a sibling GEMM (weight-gradient lane) declares the merged d(raw) one member short,
    [K_first, Ktot): the BatchNorm backward of the group's first member, which writes channels [0, K_first) on the caller's lane right
    in front of it, is no longer ordered before it.

    Narrowing by ONE 8-channel chunk cannot unorder anything in this plan: every slice of the inception backward faces an op that
    declares the whole tensor (the group's gradients read all of 'dg', the next block writes all of a concatenation's gradient), so the
    ranges still overlap and the scheduler keeps the wait (test_no_one_chunk_narrowing_can_unorder_the_inception_backward proves it
    for every declared pair; shown here for this entry).  The control narrows by the smallest unit that detaches a pair, one member."""
    from ifcb_classifier_amd.engine import schedule_lanes
    eng, bwd = _bwd()
    base = schedule_lanes(bwd.meta)
    j = next(k for k, o in enumerate(bwd.ops) if o.kind == _lib.OP_CONV_WGRAD_SEG and bwd.tags[k].startswith('Mixed_6b.'))
    meta = _copy_meta(bwd.meta)
    k, whole = next((k, r) for k, r in enumerate(meta[j][1]) if r[0] == 'dg')
    first = [(i, w) for i in range(j) for w in (bwd.meta[i][2] or ()) if w[:2] == whole[:2] and w[-2] == 0]
    assert len(first) == 1
    i, wfirst = first[0]
    assert base[i][0] != base[j][0] and wfirst[-1] < whole[-1] and bwd.tags[i] == bwd.tags[j].split('+')[0]
    # first an 8-channel narrowing: same schedule for this op, nothing to report
    meta[j][1][k] = whole[:-2] + (8, whole[-1])
    assert schedule_lanes(meta)[j] == base[j] and not pf.audit_oplist(eng, bwd, meta)
    meta[j][1][k] = whole[:-2] + (wfirst[-1], whole[-1])
    bad = pf.audit_oplist(eng, bwd, meta)
    pairs = {(a[:2], b[:2]) for a, b, _alloc in bad}
    assert pairs == {((bwd.tags[i], _lib.OP_NAMES[bwd.ops[i].kind]), (bwd.tags[j], 'conv_wgrad'))}, bad


def test_control_c_swapped_member_offsets():
    """two members of a sibling GEMM swap the koff of their ('dg', group, koff, koff + K) entries.  In this plan a member's slice is
    only ever read through the group's whole-range gradients, so the swap alone leaves every pair overlapping and ordered -- the audit
    stays silent, rightly (test_no_swap_of_member_offsets_can_unorder_the_inception_backward proves that for every group).  It bites as soon as a counterpart names a slice: with the segmented weight gradient reading only the
    FIRST member's (true) slice, the member that now claims another slice is still ordered, and the one whose true bytes nobody
    claims any more is named."""
    from ifcb_classifier_amd.engine import schedule_lanes
    eng, bwd = _bwd()
    base = schedule_lanes(bwd.meta)
    j = next(k for k, o in enumerate(bwd.ops) if o.kind == _lib.OP_CONV_WGRAD_SEG and bwd.tags[k].startswith('Mixed_6b.'))
    whole = next(r for r in bwd.meta[j][1] if r[0] == 'dg')
    writers = sorted(((w, i) for i in range(j) for w in (bwd.meta[i][2] or ()) if w[:2] == whole[:2]), key=lambda t: t[0][2])
    assert len(writers) >= 3
    (wa, ia), (wb, ib) = writers[0], writers[1]          # the members at koff 0 and behind it
    assert wa[2] == 0 and base[ia][0] != base[j][0] and base[ib][0] != base[j][0]

    def swapped():
        meta = _copy_meta(bwd.meta)
        for i, w, new in ((ia, wa, (wb[2], wb[2] + wa[3] - wa[2])), (ib, wb, (wa[2], wa[2] + wb[3] - wb[2]))):
            meta[i][2][meta[i][2].index(w)] = w[:2] + new
        return meta
    meta = swapped()
    assert not pf.audit_oplist(eng, bwd, meta)
    # the reader names member a's true slice only: b (claiming a's offset) is ordered; if b's K is smaller than a's, the tail of a's
    # true bytes has no declared writer left in front of the reader -- or, with equal K, a itself is what the reader misses
    meta = swapped()
    kk = meta[j][1].index(whole)
    meta[j][1][kk] = whole[:2] + (wa[3] - 8, wa[3])          # the last chunk of member a's true slice
    bad = pf.audit_oplist(eng, bwd, meta)
    pairs = {(a[:2], b[:2]) for a, b, _alloc in bad}
    seg = (bwd.tags[j], 'conv_wgrad')
    assert ((bwd.tags[ia], _lib.OP_NAMES[bwd.ops[ia].kind]), seg) in pairs, bad
    assert all(b == seg for _a, b in pairs)
    # the same narrowed reader WITHOUT the swap keeps member a ordered (it may rightly lose the others): the swap is what the audit saw
    meta = _copy_meta(bwd.meta)
    meta[j][1][kk] = whole[:2] + (wa[3] - 8, wa[3])
    pairs0 = {(a[:2], b[:2]) for a, b, _alloc in pf.audit_oplist(eng, bwd, meta)}
    assert ((bwd.tags[ia], _lib.OP_NAMES[bwd.ops[ia].kind]), seg) not in pairs0


def _declared(bwd):
    """[(op index, 'r' | 'w', resource)] of every annotated op"""
    return [(j, rw, res) for j, (_l, rd, wr) in enumerate(bwd.meta) if not (rd is None and wr is None)
            for rw, lst in (('r', rd), ('w', wr)) for res in (lst or ())]


def test_no_one_chunk_narrowing_can_unorder_the_inception_backward():
    """why control b narrows by a member: the scheduler drops a wait only when two declared ranges stop overlapping.  Narrowing one
    entry by an 8-channel chunk at either end shrinks each of its overlaps by at most 8 channels, so it can detach a pair only where
    two ranges of one tensor, declared by different ops and at least one a write, overlap by 8 channels or less.  The inception
    backward has no such pair: the narrowest conflicting overlap is a whole member."""
    from ifcb_classifier_amd.engine import _overlap
    eng, bwd = _bwd()
    ent = _declared(bwd)
    by_key = {}
    for e in ent:
        if e[2][-1] - e[2][-2] > 1:                          # channel ranges; (key, 0, 1) marks a whole buffer
            by_key.setdefault(e[2][:-2], []).append(e)
    narrowest, npairs = None, 0
    for lst in by_key.values():
        for a in lst:
            for b in lst:
                if a[0] < b[0] and 'w' in (a[1], b[1]) and _overlap(a[2], b[2]):
                    ov = min(a[2][-1], b[2][-1]) - max(a[2][-2], b[2][-2])
                    npairs += 1
                    narrowest = ov if narrowest is None else min(narrowest, ov)
    assert npairs > 150 and narrowest >= 32, (npairs, narrowest)


def test_no_swap_of_member_offsets_can_unorder_the_inception_backward():
    """why control c needs a counterpart that names a slice: in the inception backward every op that conflicts with a member's slice
    of a sibling GEMM's merged tensor ('dg' / 'gr' keys) declares the WHOLE tensor [0, Ktot).  Two members that swap their koff
    still lie inside (or at least overlap) that range, so every declared conflict -- and with it every wait -- survives the swap."""
    from ifcb_classifier_amd.engine import _overlap
    eng, bwd = _bwd()
    groups = {}
    for e in _declared(bwd):
        if e[2][0] in ('dg', 'gr'):
            groups.setdefault(e[2][:2], []).append(e)
    assert len(groups) >= 11
    nslices = 0
    for key, lst in groups.items():
        ktot = max(e[2][-1] for e in lst)
        for a in lst:
            if (a[2][-2], a[2][-1]) == (0, ktot):
                continue
            nslices += 1
            for b in lst:
                if b[0] != a[0] and 'w' in (a[1], b[1]) and _overlap(a[2], b[2]):
                    assert (b[2][-2], b[2][-1]) == (0, ktot), (bwd.tags[a[0]], a[2], bwd.tags[b[0]], b[2])
                    assert a[2][-1] - a[2][-2] < ktot
    assert nslices >= 30


def test_roles_agree_with_the_constness_of_the_typed_entry_points():
    """ROLES is written by hand; its read / write column is checked here against the sources: for every case of ctx.hip::run_one that
    is one call of a typed entry point, the argument that carries p[k] is matched with the parameter at that position in
    include/ifcbk.h -- a `const` pointer must be R, any other W or RW."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(pf.__file__)))
    src = open(os.path.join(root, 'ifcb_classifier_amd', 'csrc', 'ctx.hip')).read()
    body = src[src.index('static int run_one('):src.index('// ---------------------------------------------------------------- program runner')]
    # the kinds with optional operands index p[] by the slot names of the enums at the top of the file: an enumerator without a value is
    # one more than the one before it, the first of a row 0
    slot = {}
    for row in (ln.split('//')[0] for ln in src.splitlines() if ln.rstrip().endswith('// p[]')):
        slot.update((name.split(' = ')[0], k) for k, name in enumerate(w.strip() for w in row.split(',') if w.strip()))
    assert len(slot) == 7 + 6 + 5 and slot['LOSS_TEACHER'] == 6 and slot['ADAM_CLIP_STATE'] == 5 and slot['SGD_CLIP_STATE'] == 4
    numbered = lambda text: re.sub(r'\bp\[([A-Z][A-Z0-9_]*)\]', lambda m: 'p[%d]' % slot[m.group(1)], text)
    body = numbered(body)
    # the two loss kinds share run_loss, which names its pointers once: its two calls without an option, as the cases they were
    loss = numbered(src[src.index('static int run_loss('):src.index('static int run_one(')])
    var = dict(re.findall(r'\*?(\w+) = [^;,]*?(p\[\d+\])', loss))
    assert set(var) == {'logits', 'target', 'loss', 'dlogits', 'class_weight', 'lam', 'teacher'}
    for kind_name, fn in (('IFCBK_OP_SOFTMAX_XENT_W', 'ifcbk_softmax_xent_w'), ('IFCBK_OP_SOFTMAX_XENT', 'ifcbk_softmax_xent')):
        (args,) = re.findall(r'return %s\((.*?)\);' % fn, loss)
        body += 'case %s: return %s(%s);\n' % (kind_name, fn, ', '.join(var.get(a.strip(), a) for a in args.split(',')))
    # the operands an option adds have no row in ROLES (the audit refuses an op that sets one: tests/test_ema_cpu.py)
    optional = {('IFCBK_OP_ADAM', 4), ('IFCBK_OP_ADAM', 5), ('IFCBK_OP_SGD', 3), ('IFCBK_OP_SGD', 4)}
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'ifcbk.h')).read(), flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(',')] for m in re.finditer(r'IFCBK_API\s+int\s+(ifcbk_\w+)\s*\(([^;]*?)\)\s*;', hdr)}

    def split_args(text):
        out, depth, cur = [], 0, ''
        for ch in text:
            if ch == ',' and depth == 0:
                out.append(cur)
                cur = ''
                continue
            depth += ch in '([' 
            depth -= ch in ')]'
            cur += ch
        return out + [cur]
    # built from loops over segments / item tables, or a HIP runtime call: no single typed call to parse
    indirect = {'IFCBK_OP_CONV_WGRAD_SEG', 'IFCBK_OP_CONV_FWD_AFFINE_SEG', 'IFCBK_OP_CONV_WGRAD_GROUP', 'IFCBK_OP_WEIGHT_PACK_MULTI',
                'IFCBK_OP_MEMSET', 'IFCBK_OP_COPY2D'}
    # void* x is read or written by direction (flags bit 2): both directions are in the row
    by_direction = {('IFCBK_OP_FLATTEN_CHW', 0), ('IFCBK_OP_FLATTEN_CHW', 1)}
    checked = 0
    for m in re.finditer(r'case (IFCBK_OP_\w+):\s*(?:\{)?\s*return (ifcbk_\w+)\((.*?)\);', body, flags=re.S):
        kind_name, fn, args = m.group(1), m.group(2), split_args(m.group(3))
        if kind_name in indirect:
            continue
        kind = getattr(_lib, kind_name[len('IFCBK_'):])
        params = protos[fn]
        assert len(params) == len(args), (kind_name, fn, len(params), len(args))
        probe = _lib.Op()
        for pos, a in enumerate(args):
            for k in re.findall(r'\bp\[(\d+)\]', a):
                k = int(k)
                if (kind_name, k) in optional:
                    assert k not in pf.ROLES[kind]
                    continue
                assert k in pf.ROLES[kind], (kind_name, k)
                role = pf.ROLES[kind][k][0]
                role = role(probe) if callable(role) else role
                if (kind_name, k) in by_direction:
                    continue
                is_const = params[pos].startswith('const ')
                assert (role == pf.R) == is_const, (kind_name, fn, 'p[%d]' % k, params[pos], role)
                checked += 1
    assert checked >= 150, checked
