"""The operand layout of ``ifcbk_op`` (include/ifcbk.h) for every op kind the plans emit or read: one row per kind with the names of
its p[], i[] and f[] slots, in slot order.  The names are the parameter names of the kind's typed entry point; the four kinds with
optional operands (the two losses, Adam, SGD) carry the names of their layout blocks in the header.  A slot nobody sets keeps the zero
of a fresh op, which every optional operand reads as "off".

A counted tail is written ``name*n`` and names the slots ``name0 .. name<n-1>`` (the destinations and widths of a segmented GEMM, the
members' gradients of a grouped weight gradient); ``tail(kind, name)`` gives its slots in order.

``slot(kind, name)`` resolves a name to its index in whichever of p / i / f holds it (a name occurs once per kind): resolve once, at
import or at plan time, then index with the result.  ``PARAM_GRADS`` lists, per kind, the p slots that point into the flat gradient
buffer."""
from . import _lib as L

# ifcbk_op.flags, bits 0-7 (bits 8-10 and 12-19 are the lane and the wait mask, written by OpList.freeze)
FLAG_ACC, FLAG_PARAM_ACC, FLAG_RELU, FLAG_DX_ACC, FLAG_TIMED = 1, 2, 4, 8, 0x80
FLAG_TO_CHW = 4                 # OP_FLATTEN_CHW's reading of bit 2
NP, NI, NF = 12, 4, 8           # slots of ifcbk_op.p / .i / .f


def _row(p='', i='', f='', grads=''):
    def names(s):
        out = []
        for w in s.split():
            base, star, n = w.partition('*')
            out += [base + str(k) for k in range(int(n))] if star else [w]
        return tuple(out)
    return dict(p=names(p), i=names(i), f=names(f), grads=names(grads))


_LOSS = _row('logits target loss dlogits class_weight lam teacher', 'N NC', 'weight smoothing gamma alpha temperature')
_BN_STATS4 = 'mean invstd scale shift'

OPERANDS = {
    L.OP_CONV_FWD: _row('x w y bn_part'),
    L.OP_CONV_FWD_AFFINE: _row('x w y scale shift residual', 'ldr'),
    L.OP_CONV_FWD_AFFINE_MAXPOOL: _row('x w y_pooled scale shift', 'ldp'),
    L.OP_CONV_FWD_AFFINE_SEG: _row('x w y*4 scale shift', 'seg*4'),        # seg: channels | ld << 20 | affine << 40, 0 = unused
    L.OP_CONV_DGRAD: _row('dy wT dx'),
    L.OP_CONV_DGRAD_BNSTAT: _row('dy wT dx prev_raw prev_mean prev_invstd prev_scale prev_shift part', 'prev_ld'),
    L.OP_CONV_WGRAD: _row('x dy dw', grads='dw'),
    L.OP_CONV_WGRAD_SEG: _row('x dy dw*4', 'kseg*4', grads='dw*4'),        # kseg: channels of the segment, 0 = unused
    L.OP_CONV_WGRAD_GROUP: _row('items dw*8', 'n', grads='dw*8'),          # items: HOST array of n WgradItem; dw0..dw<n-1> again
    L.OP_STEM_U8_FWD: _row('g w_master ab y bn_part scale shift'),
    L.OP_STEM_U8_WGRAD: _row('g dy ab dw', grads='dw'),
    L.OP_WEIGHT_PACK: _row('w_master w wT', 'wT_ld'),
    L.OP_WEIGHT_PACK_MULTI: _row('items_dev', 'n_items total_blocks dtype'),
    L.OP_BN_FINALIZE: _row('part gamma beta running_mean running_var ' + _BN_STATS4, 'mblocks part_ld'),
    L.OP_BN_STATS: _row('x part'),
    L.OP_BN_APPLY: _row('x scale shift residual y', 'ldr'),
    L.OP_BN_APPLY_MAXPOOL: _row('x scale shift y argmax', 'relu'),
    L.OP_BN_BWD: _row('x y dy gamma mean invstd dx dres dgamma dbeta scale shift', 'lddy lddx lddres', grads='dgamma dbeta'),
    L.OP_BN_BWD_MAXPOOL: _row('x dpool argmax gamma ' + _BN_STATS4 + ' dx dgamma dbeta', 'relu lddx', grads='dgamma dbeta'),
    L.OP_BN_BWD_PARTIALS: _row('x dy gamma ' + _BN_STATS4 + ' part dx dgamma dbeta', 'lddy ntiles lddx part_ld', grads='dgamma dbeta'),
    L.OP_BIAS_RELU_BWD: _row('y dy dz dbias', 'lddz', grads='dbias'),
    L.OP_MAXPOOL_FWD: _row('x y argmax'),
    L.OP_MAXPOOL_BWD: _row('dy argmax dx'),
    L.OP_AVGPOOL_FWD: _row('x y'),
    L.OP_AVGPOOL_BWD: _row('dy dx'),
    L.OP_AVGPOOL_AFFINE: _row('x scale shift y'),
    L.OP_HEAD_FWD: _row('x mask W b feat logits'),
    L.OP_HEAD_BWD: _row('dlogits feat mask W dW db dx', 'lddx', grads='dW db'),
    L.OP_DROPOUT: _row('x mask y', 'n dtype', 'scale'),
    L.OP_FLATTEN_CHW: _row('x flat', 'N HW C ldx_dtype'),                  # ldx_dtype: ldx | dtype << 32
    L.OP_SOFTMAX: _row('logits probs', 'N NC'),
    L.OP_SOFTMAX_XENT: _LOSS,                                              # (class_weight stays NULL: the plain kind does not read it)
    L.OP_SOFTMAX_XENT_W: _LOSS,
    L.OP_ADAM: _row('P G M V E clip_state', 'n step decoupled', 'lr beta1 beta2 eps weight_decay grad_scale ema_w max_norm'),
    L.OP_SGD: _row('P G M E clip_state', 'n step', 'lr momentum weight_decay grad_scale ema_w max_norm'),
    L.OP_STEP_COUNTERS: _row('num_batches_tracked loss_sum loss', 'n'),
}

for _kind, _r in OPERANDS.items():
    _all = _r['p'] + _r['i'] + _r['f']
    assert len(_r['p']) <= NP and len(_r['i']) <= NI and len(_r['f']) <= NF and len(set(_all)) == len(_all), L.OP_NAMES[_kind]
    assert set(_r['grads']) <= set(_r['p']), L.OP_NAMES[_kind]


def slot(kind, name):
    """index of operand `name` of `kind` in the array (p, i or f) that holds it"""
    for names in (OPERANDS[kind][a] for a in 'pif'):
        if name in names:
            return names.index(name)
    raise KeyError('%s op has no operand %r' % (L.OP_NAMES[kind], name))


def tail(kind, name):
    """the slots name0, name1, ... of a counted tail, in order"""
    r = OPERANDS[kind]
    return [slot(kind, w) for w in r['p'] + r['i'] + r['f'] if w[:len(name)] == name and w[len(name):].isdigit()]


def fill(kind, which, arr, vals, conv):
    """write operands into arr (= op.p / .i / .f, `which` = 'p' / 'i' / 'f'): a tuple in slot order, or a dict keyed by slot name.  None
    (pointers only) or an absent name leaves the zero of a fresh op"""
    names = OPERANDS[kind][which]
    if isinstance(vals, dict):
        unknown = set(vals) - set(names)
        if unknown:
            raise KeyError('%s op has no %s operand %s (it has %s)' % (L.OP_NAMES[kind], which, sorted(unknown), ', '.join(names)))
        vals = [vals.get(n) for n in names]
    elif len(vals) > len(names):
        raise ValueError('%s op: %d %s operands given, the kind has %d (%s)' % (L.OP_NAMES[kind], len(vals), which, len(names), ', '.join(names)))
    for k, v in enumerate(vals):
        if v is not None:
            arr[k] = conv(v)


PARAM_GRADS = {kind: tuple(slot(kind, n) for n in r['grads']) for kind, r in OPERANDS.items() if r['grads']}
