"""Fingerprints of the op tables that Engine(plan_only=True) builds (no GPU needed): one sha256 per configuration.

  python tests/golden/make_plan_fingerprints.py          # rewrites plan_fingerprints.json

plan_fingerprints.json : configuration name -> sha256 of the canonical text of every program of its plan.

Per op the text holds the kind, the full flags word (lane and wait bits included), the tag, i[], f[], the raw bytes of the
descriptor union, the kernel name ifcbk_op_kernel resolves and every pointer of p[] as a symbolic (owner, byte offset).  The
owners are the tensors the engine and its plan hold, named by where they are reachable from (engine attributes, node and group
attributes, pl.keep); the host tables behind OP_CONV_WGRAD_GROUP (WgradItem) and OP_WEIGHT_PACK_MULTI (PackItem) are expanded
item by item with their pointers mapped the same way.  No raw address, id() or allocation order enters the text.
Regenerate only for a change that is meant to alter the op tables, and say so in its description.
"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(HERE, 'plan_fingerprints.json')

PROGRAMS = ('fwd_train', 'fwd_eval', 'bwd', 'pack', 'evalprep', 'loss', 'eval_loss', 'softmax', 'adam', 'step', 'fwd_loss',
            'fwd_bwd', 'adam_pack')

_CW = [1.0, 0.5, 2.0, 1.5, 0.25, 3.0, 1.0]

# name -> (model, dtype, batch, extra Engine kwargs, environment)
CONFIGS = {
    'inception_v3-bf16-b2': ('inception_v3', 'bf16', 2, {}, {}),
    'inception_v3-bf16-b256': ('inception_v3', 'bf16', 256, {}, {}),
    'inception_v3-fp32-b2': ('inception_v3', 'fp32', 2, {}, {}),
    'resnet50-bf16-b4': ('resnet50', 'bf16', 4, {}, {}),
    'densenet121-bf16-b2': ('densenet121', 'bf16', 2, {}, {}),
    'vgg11_bn-bf16-b2': ('vgg11_bn', 'bf16', 2, {}, {}),
    'squeezenet-bf16-b4': ('squeezenet', 'bf16', 4, {}, {}),
    'alexnet-bf16-b4': ('alexnet', 'bf16', 4, {}, {}),
    'inception_v3-bf16-b2-lanes2': ('inception_v3', 'bf16', 2, {}, {'IFCBK_LANES': '2'}),
    'inception_v3-bf16-b2-dp2': ('inception_v3', 'bf16', 2, {'dp_world': 2}, {}),
    'inception_v3-bf16-b2-fuse_bnstat0': ('inception_v3', 'bf16', 2, {}, {'IFCBK_FUSE_BNSTAT': '0'}),
    'inception_v3-bf16-b2-wgrad_lane0': ('inception_v3', 'bf16', 2, {}, {'IFCBK_WGRAD_LANE': '0'}),
    'inception_v3-bf16-b64-wgrad_group0': ('inception_v3', 'bf16', 64, {}, {'IFCBK_WGRAD_GROUP': '0'}),      # (no groups at b2)
    'inception_v3-bf16-b2-opt_buckets1': ('inception_v3', 'bf16', 2, {}, {'IFCBK_OPT_BUCKETS': '1'}),
    'inception_v3-bf16-b2-fuse_pool0': ('inception_v3', 'bf16', 2, {}, {'IFCBK_FUSE_POOL': '0'}),
    'inception_v3-bf16-b2-u8': ('inception_v3', 'bf16', 2, {}, {}),                                          # (IN_KIND below)
    'inception_v3-bf16-b64': ('inception_v3', 'bf16', 64, {}, {}),             # grouped weight gradients: the workspace grows
    'resnet18-fp32-b2': ('resnet18', 'fp32', 2, {}, {}),
    'inception_v3-bf16-b2-sgd': ('inception_v3', 'bf16', 2, {'optimizer': 'sgd', 'momentum': 0.9}, {}),
    'inception_v3-bf16-b2-ema': ('inception_v3', 'bf16', 2, {'ema_decay': 0.999}, {}),
    'inception_v3-bf16-b2-class_weights-ls': ('inception_v3', 'bf16', 2, {'class_weights': [1.0, 0.5, 2.0, 1.5, 0.25, 3.0, 1.0],
                                                                          'label_smoothing': 0.1}, {}),
    'inception_v3-bf16-b2-focal': ('inception_v3', 'bf16', 2, {'focal_gamma': 2.0}, {}),
    'inception_v3-bf16-b2-mix': ('inception_v3', 'bf16', 2, {'mix': True}, {}),
    'inception_v3-bf16-b2-distill': ('inception_v3', 'bf16', 2, {'distill': (0.5, 2.0)}, {}),
    'inception_v3-bf16-b2-fuse_pool_eval0': ('inception_v3', 'bf16', 2, {}, {'IFCBK_FUSE_POOL_EVAL': '0'}),
    'inception_v3-bf16-b2-fuse_siblings0': ('inception_v3', 'bf16', 2, {}, {'IFCBK_FUSE_SIBLINGS': '0'}),
    # optional operands of the loss and optimizer ops, alone and together (a clipped plan takes the single update)
    'inception_v3-bf16-b2-clip': ('inception_v3', 'bf16', 2, {'clip_grad': 1.0}, {}),
    'inception_v3-bf16-b2-ema-clip': ('inception_v3', 'bf16', 2, {'ema_decay': 0.999, 'clip_grad': 1.0}, {}),
    'inception_v3-bf16-b2-sgd-ema-clip': ('inception_v3', 'bf16', 2, {'optimizer': 'sgd', 'momentum': 0.9, 'ema_decay': 0.999,
                                                                      'clip_grad': 1.0}, {}),
    'inception_v3-bf16-b2-sgd0-clip': ('inception_v3', 'bf16', 2, {'optimizer': 'sgd', 'momentum': 0.0, 'clip_grad': 1.0}, {}),
    'inception_v3-bf16-b2-class_weights-ls-mix': ('inception_v3', 'bf16', 2, {'class_weights': _CW, 'label_smoothing': 0.1,
                                                                              'mix': True}, {}),
    'inception_v3-bf16-b2-class_weights-ls-distill': ('inception_v3', 'bf16', 2, {'class_weights': _CW, 'label_smoothing': 0.1,
                                                                                  'distill': (0.5, 2.0)}, {}),
    'inception_v3-bf16-b2-ema-dp2': ('inception_v3', 'bf16', 2, {'ema_decay': 0.999, 'dp_world': 2}, {}),
}

# configurations planned on the resized u8 plane of the input slot (eng.in_kind) instead of the dense tensor
IN_KIND = {'inception_v3-bf16-b2-u8': 'u8'}


class Owners:
    """storage -> symbolic name, from a walk over everything the engine and the plan hold"""

    def __init__(self, eng, pl):
        import torch
        self.spans = []                      # (start, end, name)
        seen = {}

        def add(name, t):
            st = t.untyped_storage()
            start, nbytes = st.data_ptr(), st.nbytes()
            whole = t.data_ptr() == start and t.numel() * t.element_size() == nbytes
            rank = (0 if whole else 1, name)
            if start not in seen or rank < seen[start][0]:
                seen[start] = (rank, start + nbytes, name)

        def walk(name, v, depth=0):
            if isinstance(v, torch.Tensor):
                add(name, v)
            elif depth > 3:
                return
            elif isinstance(v, (list, tuple)):
                for k, x in enumerate(v):
                    walk('%s[%d]' % (name, k), x, depth + 1)
            elif isinstance(v, dict):
                for k, x in v.items():
                    walk('%s[%s]' % (name, getattr(k, 'name', k)), x, depth + 1)

        for a in sorted(vars(eng)):
            walk(a, vars(eng)[a])
        for k, n in enumerate(eng.net.nodes):
            for a in sorted(vars(n)):
                walk('node[%d:%s].%s' % (k, n.name, a), vars(n)[a])
        for k, g in enumerate(eng.groups):
            for a in sorted(vars(g)):
                walk('group[%d].%s' % (k, a), vars(g)[a])
        walk('keep', pl.keep)
        self.spans = sorted((s, e, name) for s, (_r, e, name) in seen.items())

    def sym(self, ptr):
        if not ptr:
            return None
        for s, e, name in self.spans:
            if s <= ptr < e:
                return '%s+%d' % (name, ptr - s)
        raise KeyError('pointer outside every tensor of the engine and its plan')


def _struct_text(owners, item, ptr_fields):
    raw = bytearray(bytes(item))
    syms = []
    for f in ptr_fields:
        off = getattr(type(item), f).offset
        syms.append('%s=%s' % (f, owners.sym(getattr(item, f))))
        raw[off:off + 8] = bytes(8)          # the address itself is replaced by its symbol
    return raw.hex() + ' ' + ' '.join(syms)


def _host_items(eng, pl, owners, o):
    """the item tables a grouped op points into, expanded"""
    from ifcb_classifier_amd import _lib
    import numpy as np
    if o.kind == _lib.OP_CONV_WGRAD_GROUP:
        n = int(o.i[0])
        items = (_lib.WgradItem * n).from_address(o.p[0])
        return [_struct_text(owners, it, ('x', 'dy', 'dw')) for it in items]
    if o.kind == _lib.OP_WEIGHT_PACK_MULTI:
        tabs = [v[0] for v in eng._pack_tables.values() if v[0].data_ptr() == o.p[0]]
        assert len(tabs) == 1
        raw = tabs[0].cpu().numpy().astype(np.uint8).tobytes()
        items = (_lib.PackItem * int(o.i[0])).from_buffer_copy(raw)
        return [_struct_text(owners, it, ('w_master', 'w', 'wT')) for it in items]
    return []


def plan_text(eng, pl):
    from ifcb_classifier_amd import _lib
    owners = Owners(eng, pl)
    lib = eng.ctx.lib
    buf = C.create_string_buffer(256)
    lines = []
    for prog in PROGRAMS:
        p = getattr(pl, prog)
        lines.append('== %s %d' % (prog, p.n))
        for k in range(p.n):
            o = p.arr[k]
            rc = lib.ifcbk_op_kernel(C.byref(o), buf, 256)
            host = o.kind == _lib.OP_CONV_WGRAD_GROUP              # p[0]: the WgradItem array, expanded below
            ptrs = ['host' if (j == 0 and host) else owners.sym(o.p[j]) for j in range(12)]
            lines.append('%d %d %d %s | i=%s | f=%s | u=%s | k=%d:%s | p=%s' % (
                k, o.kind, o.flags, p.tags[k], list(o.i), [repr(x) for x in o.f], bytes(o.u).hex(), rc, buf.value.decode(),
                ptrs))
            lines.extend('   item ' + t for t in _host_items(eng, pl, owners, o))
    return '\n'.join(lines) + '\n'


def build_plan(cfg, plan_only=True):
    """-> (engine, plan) of one configuration, with the environment it names (and nothing else of the switches) in force;
    plan_only=False: on an engine with a device (tests/test_gpu_plan_fingerprint.py)"""
    from unittest import mock
    import torch
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    model, dtype, B, kw, env = CONFIGS[cfg]
    # every switch is unset for a configuration unless it names one (IFCBK_LIB: which library, read at import)
    keep = {k: v for k, v in os.environ.items() if not ((k.startswith('IFCBK_') and k != 'IFCBK_LIB') or k == 'WORLD_SIZE')}
    # planning reads no tensor contents: empty() instead of zeros() keeps the ~20 GB of host buffers of a batch-256 plan
    # from being touched (committed)
    with mock.patch.dict(os.environ, dict(keep, **env), clear=True), mock.patch.object(torch, 'zeros', torch.empty), \
            mock.patch.object(torch, 'zeros_like', torch.empty_like):
        eng = Engine(graph.build(model, 7), max_batch=B, dtype=dtype, plan_only=plan_only, **kw)
        if cfg in IN_KIND:
            assert eng.stem_u8 is not None
            eng.in_kind[eng.in_slot] = IN_KIND[cfg]
        return eng, eng.plan(B)


def fingerprint(cfg, plan_only=True):
    eng, pl = build_plan(cfg, plan_only)
    return hashlib.sha256(plan_text(eng, pl).encode()).hexdigest()


if __name__ == '__main__':
    import torch
    torch.manual_seed(0)
    out = {cfg: fingerprint(cfg) for cfg in CONFIGS}
    with open(GOLDEN, 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write('\n')
    print('\n'.join('%s %s' % kv for kv in sorted(out.items())))
