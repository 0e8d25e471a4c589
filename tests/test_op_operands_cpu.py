"""ifcb_classifier_amd/ops.py, the planner's table of operand names per op kind, and OpList.add's use of it (CPU, nothing is planned
or launched).  For the four kinds with optional operands the table meets tests/option_matrix.py's decoder tables, which are written
from include/ifcbk.h on their own: this is the one place where the two copies are compared."""
import ctypes as C

import pytest

import option_matrix as om
from ifcb_classifier_amd import _lib, ops
from ifcb_classifier_amd.plan import OpList


def test_the_optional_operand_kinds_name_their_slots_as_the_header_decoders_do():
    for kind in (_lib.OP_SOFTMAX_XENT, _lib.OP_SOFTMAX_XENT_W):
        assert ops.OPERANDS[kind]['p'] == om.LOSS_P and ops.OPERANDS[kind]['f'] == om.LOSS_F
    assert ops.OPERANDS[_lib.OP_ADAM]['p'] == om.ADAM_P and ops.OPERANDS[_lib.OP_ADAM]['f'] == om.ADAM_F
    assert ops.OPERANDS[_lib.OP_SGD]['p'] == om.SGD_P and ops.OPERANDS[_lib.OP_SGD]['f'] == om.SGD_F
    assert [ops.slot(_lib.OP_ADAM, n) for n in ('V', 'step', 'max_norm')] == [3, 1, 7]
    assert [ops.slot(_lib.OP_SGD, n) for n in ('E', 'step', 'max_norm')] == [3, 1, 5]


def test_no_kind_names_more_slots_than_an_op_has():
    o = _lib.Op()
    assert (len(o.p), len(o.i), len(o.f)) == (12, 4, 8) == (ops.NP, ops.NI, ops.NF)
    for kind, row in ops.OPERANDS.items():
        assert len(row['p']) <= 12 and len(row['i']) <= 4 and len(row['f']) <= 8, _lib.OP_NAMES[kind]
        assert kind in _lib.OP_NAMES


def test_a_counted_tail_is_named_by_index():
    k = _lib.OP_CONV_WGRAD_SEG
    assert ops.OPERANDS[k]['p'] == ('x', 'dy', 'dw0', 'dw1', 'dw2', 'dw3') and ops.tail(k, 'dw') == [2, 3, 4, 5]
    assert ops.tail(k, 'kseg') == [0, 1, 2, 3] and ops.PARAM_GRADS[k] == (2, 3, 4, 5)
    assert ops.PARAM_GRADS[_lib.OP_CONV_WGRAD_GROUP] == tuple(range(1, 9))


def test_add_refuses_an_unknown_name_and_an_over_long_tuple():
    ol = OpList()
    with pytest.raises(KeyError, match='adam op has no p operand'):
        ol.add(_lib.OP_ADAM, 't', p=dict(P=16, momentum_buffer=32))
    with pytest.raises(KeyError, match='sgd op has no f operand'):
        ol.add(_lib.OP_SGD, 't', f=dict(beta1=0.9))                      # Adam's name on the SGD kind
    with pytest.raises(KeyError, match='softmax_xent op has no i operand'):
        ol.add(_lib.OP_SOFTMAX_XENT, 't', i=dict(N=2, C=7))
    with pytest.raises(ValueError, match='6 f operands given, the kind has 5'):
        ol.add(_lib.OP_SOFTMAX_XENT_W, 't', f=(1.0, 0.0, 0.0, 0.3, 4.0, 1.0))
    with pytest.raises(ValueError, match='avgpool_fwd op: 3 p operands given, the kind has 2'):
        ol.add(_lib.OP_AVGPOOL_FWD, 't', p=(16, 32, 48))
    with pytest.raises(ValueError, match='1 i operands given, the kind has 0'):
        ol.add(_lib.OP_CONV_FWD, 't', i=(1,))
    with pytest.raises(KeyError):
        ops.slot(_lib.OP_SGD, 'V')
    assert not ol.ops and not ol.tags and not ol.meta                    # a refused op is not half added


def test_a_dict_and_its_padded_tuple_give_the_same_bytes():
    vp = C.c_void_p
    pairs = [
        (_lib.OP_SOFTMAX_XENT_W,
         dict(p=dict(logits=vp(16), target=vp(32), loss=vp(48), dlogits=None, teacher=vp(96)), i=dict(N=2, NC=7),
              f=dict(weight=0.4, alpha=0.3, temperature=4.0), flags=ops.FLAG_ACC),
         dict(p=(vp(16), vp(32), vp(48), None, None, None, vp(96)), i=(2, 7), f=(0.4, 0.0, 0.0, 0.3, 4.0), flags=1)),
        (_lib.OP_SGD,
         dict(p=dict(P=vp(16), G=vp(32), clip_state=vp(64)), i=dict(n=1024, step=1), f=dict(lr=0.1, grad_scale=1.0, max_norm=0.75)),
         dict(p=(vp(16), vp(32), None, None, vp(64)), i=(1024, 1), f=(0.1, 0.0, 0.0, 1.0, 0.0, 0.75))),
        (_lib.OP_ADAM,
         dict(p=dict(G=32, P=16, M=48, V=64, E=80), i=dict(step=1, n=8), f=dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0)),
         dict(p=(16, 32, 48, 64, 80), i=(8, 1), f=(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0))),
    ]
    ol = OpList()
    for kind, named, padded in pairs:
        a, b = ol.add(kind, 't', **named), ol.add(kind, 't', **padded)
        assert bytes(a) == bytes(b) and any(a.p) and a.kind == kind
