"""ONNX files of the backbones ``graph.build`` describes, written and read without the ``onnx`` package.

An ONNX model is a protocol-buffer message of a small fixed schema (onnx/onnx.proto, public).  ``export`` walks the layer
graph and encodes an NCHW inference graph of the eval-mode network: input ``input`` [batch, 3, S, S], output ``output``
[batch, nclasses] raw logits (no softmax, no aux head), BatchNorm kept unfolded so that every initializer is exactly one
``state_dict`` tensor under its torchvision key.  Concat-free buffers (Inception blocks, Fire modules, densenet's growing
block buffer) become explicit ``Concat`` nodes in channel order.

``read`` is the inverse for the files ``export`` writes: initializers, metadata and I/O shapes.  It is not an ONNX importer.
"""
import struct

import numpy as np
import torch

from . import graph

FORMAT_VERSION = '1'
TRANSFORM_SCALE = (0.229 / 0.5, 0.224 / 0.5, 0.225 / 0.5)     # torchvision Inception3._transform_input
TRANSFORM_SHIFT = ((0.485 - 0.5) / 0.5, (0.456 - 0.5) / 0.5, (0.406 - 0.5) / 0.5)
MAX_BYTES = 2 ** 31 - 1                                        # protobuf's limit on one serialised message
OPSETS = range(10, 22)                                         # MaxPool / AveragePool ceil_mode needs opset 10
_ADAPTIVE = {'alexnet': 6, 'vgg': 7}                           # AdaptiveAvgPool2d output size in front of the classifier

# onnx.proto field numbers
FLOAT, INT64, FLOAT16 = 1, 7, 10                               # TensorProto.DataType
_ATTR_FLOAT, _ATTR_INT, _ATTR_INTS = 1, 2, 7                   # AttributeProto.AttributeType


def _ir_version(opset):
    """IR version of the ONNX release that introduced ``opset`` (onnx/docs/Versioning.md)"""
    return {10: 5, 11: 6, 12: 7, 13: 7, 14: 7, 15: 8, 16: 8, 17: 8, 18: 8, 19: 9, 20: 9, 21: 10}[opset]


# ------------------------------------------------------------------------------------------ protobuf encoding
def _varint(v):
    v &= (1 << 64) - 1                                         # negative int64 -> two's complement, 10 bytes
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _int(field, v):
    return _varint(field << 3) + _varint(int(v))


def _bytes(field, b):
    if isinstance(b, str):
        b = b.encode('utf-8')
    return _varint(field << 3 | 2) + _varint(len(b)) + b


def _f32(field, v):
    return _varint(field << 3 | 5) + struct.pack('<f', v)


def _attr(name, v):
    """AttributeProto: name 1, f 2, i 3, ints 8, type 20"""
    if isinstance(v, float):
        return _bytes(1, name) + _f32(2, v) + _int(20, _ATTR_FLOAT)
    if isinstance(v, int):
        return _bytes(1, name) + _int(3, v) + _int(20, _ATTR_INT)
    return _bytes(1, name) + b''.join(_int(8, i) for i in v) + _int(20, _ATTR_INTS)


def _node(op, inputs, outputs, name, **attrs):
    """NodeProto: input 1, output 2, name 3, op_type 4, attribute 5"""
    return (b''.join(_bytes(1, i) for i in inputs) + b''.join(_bytes(2, o) for o in outputs) + _bytes(3, name)
            + _bytes(4, op) + b''.join(_bytes(5, _attr(k, v)) for k, v in attrs.items()))


def _tensor(name, arr, dtype):
    """TensorProto: dims 1, data_type 2, name 8, raw_data 9 (little endian)"""
    return (b''.join(_int(1, d) for d in arr.shape) + _int(2, dtype) + _bytes(8, name)
            + _bytes(9, np.ascontiguousarray(arr).tobytes()))


def _value_info(name, elem_type, dims):
    """ValueInfoProto{name 1, type 2: TypeProto{tensor_type 1: {elem_type 1, shape 2: TensorShapeProto{dim 1:
    {dim_value 1 | dim_param 2}}}}}"""
    shape = b''.join(_bytes(1, _bytes(2, d) if isinstance(d, str) else _int(1, d)) for d in dims)
    return _bytes(1, name) + _bytes(2, _bytes(1, _int(1, elem_type) + _bytes(2, shape)))


# ------------------------------------------------------------------------------------------ graph -> nodes
class _Emitter:
    def __init__(self, sd, np_dtype):
        self.sd, self.np_dtype = sd, np_dtype
        self.nodes, self.inits, self.used = [], [], set()
        self.segments = {}         # buf id -> [(coff, C, tensor name)] channel slices written so far
        self.flat = set()          # tensor names that are [N, features] (after Flatten)
        self.concats = {}
        self.n = 0

    def tmp(self, hint):
        self.n += 1
        return '%s:%d' % (hint, self.n)

    def node(self, op, inputs, hint, out=None, **attrs):
        out = out or self.tmp(hint)
        self.nodes.append(_node(op, inputs, [out], '%s_%d' % (op, len(self.nodes)), **attrs))
        return out

    def param(self, key):
        if key not in self.used:
            if key not in self.sd:
                raise KeyError('state_dict has no tensor %r' % key)
            t = self.sd[key].detach().to('cpu', torch.float32).numpy()
            self.inits.append(_tensor(key, t.astype(self.np_dtype), FLOAT16 if self.np_dtype == np.float16 else FLOAT))
            self.used.add(key)
        return key

    def const(self, name, values, shape):
        a = np.asarray(values, np.float32).astype(self.np_dtype).reshape(shape)
        self.inits.append(_tensor(name, a, FLOAT16 if self.np_dtype == np.float16 else FLOAT))
        return name

    def write(self, view, name):
        self.segments.setdefault(view.buf.id, []).append((view.coff, view.C, name))

    def read(self, view):
        """the tensor holding channels [coff, coff + C) of a buffer: one writer's output, or a Concat of several"""
        segs = sorted(self.segments.get(view.buf.id, []))
        lo, hi = view.coff, view.coff + view.C
        picked = [s for s in segs if s[0] >= lo and s[0] + s[1] <= hi]
        if sum(s[1] for s in picked) != view.C or any(s[0] < hi and s[0] + s[1] > lo and s not in picked for s in segs):
            raise ValueError('%s[%d:%d] is not a union of whole written slices %s' % (view.buf.name, lo, hi, segs))
        if len(picked) == 1:
            return picked[0][2]
        key = tuple(s[2] for s in picked)
        if key not in self.concats:
            self.concats[key] = self.node('Concat', list(key), view.buf.name + ':cat', axis=1)
        return self.concats[key]


def _pool_attrs(n, kind):
    a = dict(kernel_shape=[n.R, n.S], strides=[n.sh, n.sw], pads=[n.ph, n.pw, n.ph, n.pw])
    if (n.P, n.Q) != (graph._out(n.x.H, n.R, n.sh, n.ph), graph._out(n.x.W, n.S, n.sw, n.pw)):
        a['ceil_mode'] = 1
    if kind == 'avg':
        a['count_include_pad'] = 1               # torch's AvgPool2d / F.avg_pool2d default
    return a


def _emit(net, em, x_in):
    em.segments[net.input.id] = [(0, net.input.C, x_in)]
    out_name = None
    for n in net.nodes:
        if getattr(n, 'aux', False):
            continue                              # AuxLogits: train-mode only
        kind = getattr(n, 'kind', None)
        if isinstance(n, graph.PoolNode):
            op = 'MaxPool' if n.kind == 'max' else 'AveragePool'
            em.write(n.y, em.node(op, [em.read(n.x)], n.name, **_pool_attrs(n, n.kind)))
        elif kind == 'conv':
            ins = [em.read(n.x), em.param(n.conv_key + '.weight')] + ([em.param(n.conv_key + '.bias')] if n.conv_bias else [])
            y = em.node('Conv', ins, n.conv_key, kernel_shape=[n.R, n.S], strides=[n.sh, n.sw], pads=[n.ph, n.pw, n.ph, n.pw])
            y = em.node('BatchNormalization', [y] + [em.param(n.bn_key + s) for s in
                        ('.weight', '.bias', '.running_mean', '.running_var')], n.bn_key, epsilon=float(n.eps))
            if n.residual is not None:
                y = em.node('Add', [y, em.read(n.residual)], n.name + ':add')
            if n.relu:
                y = em.node('Relu', [y], n.name + ':relu')
            em.write(n.y, y)
        elif kind == 'cb':
            x = em.read(n.x)
            ins = [x, em.param(n.key + '.weight')] + ([em.param(n.key + '.bias')] if n.bias else [])
            if n.linear:
                assert x in em.flat, n.key
                y = em.node('Gemm', ins, n.key, transB=1)
                em.flat.add(y)
            else:
                y = em.node('Conv', ins, n.key, kernel_shape=[n.R, n.S], strides=[n.sh, n.sw], pads=[n.ph, n.pw, n.ph, n.pw])
            if n.relu:
                y = em.node('Relu', [y], n.key + ':relu')
                if n.linear:
                    em.flat.add(y)
            em.write(n.y, y)
        elif kind == 'bnr':
            y = em.node('BatchNormalization', [em.read(n.x)] + [em.param(n.bn_key + s) for s in
                        ('.weight', '.bias', '.running_mean', '.running_var')], n.bn_key, epsilon=float(n.eps))
            if n.relu:
                y = em.node('Relu', [y], n.bn_key + ':relu')
            em.write(n.y, y)
        elif kind == 'drop':
            em.write(n.y, em.read(n.x))           # eval: identity
        elif kind == 'flat':
            fam = 'vgg' if net.name.startswith('vgg') else net.name
            if fam in _ADAPTIVE and (n.x.H, n.x.W) != (_ADAPTIVE[fam],) * 2:
                raise ValueError('%s: AdaptiveAvgPool2d((%d, %d)) on a %dx%d map is not the identity; not exportable'
                                 % (net.name, _ADAPTIVE[fam], _ADAPTIVE[fam], n.x.H, n.x.W))
            y = em.node('Flatten', [em.read(n.x)], n.name, axis=1)
            em.flat.add(y)
            em.write(n.y, y)
        elif kind == 'head':
            x = em.read(n.x)
            if x not in em.flat:                  # [N, C, H, W] -> adaptive_avg_pool2d(1) -> flatten
                x = em.node('GlobalAveragePool', [x], n.name + ':gap')
                x = em.node('Flatten', [x], n.name + ':flat', axis=1, out=None if n.fc else 'output')
            if n.fc:
                x = em.node('Gemm', [x, em.param(n.key + '.weight'), em.param(n.key + '.bias')], n.key, out='output', transB=1)
            out_name = x
        else:
            raise TypeError('no ONNX mapping for graph node %r' % n)
    if out_name != 'output':
        raise ValueError('%s: the graph has no classifier head' % net.name)


def export(state_dict, model_name, classes, pretrained, path, half=False, opset=12, batch_size=0, pad=None):
    """Write the eval-mode ``model_name`` with the tensors of ``state_dict`` (torchvision keys; a checkpoint's ``model.``
    prefix is dropped) to ``path``.  ``batch_size=0``: dynamic batch dim ``batch_size``.  ``pad`` (the model's TRAIN --pad setting) is recorded as ``ifcbk.pad`` when
    set; ``read_pad`` decodes it.  Returns the number of bytes written."""
    if opset not in OPSETS:
        raise ValueError('opset %d: this writer emits opsets %d..%d' % (opset, OPSETS[0], OPSETS[-1]))
    sd = {(k[len('model.'):] if k.startswith('model.') else k): v for k, v in state_dict.items()}
    classes = list(classes)
    net = graph.build(model_name, len(classes), pretrained)
    dt = np.float16 if half else np.float32
    elem = FLOAT16 if half else FLOAT
    em = _Emitter(sd, dt)
    x = 'input'
    if net.transform_input:
        scale = em.const('transform_input.scale', TRANSFORM_SCALE, (1, 3, 1, 1))
        shift = em.const('transform_input.shift', TRANSFORM_SHIFT, (1, 3, 1, 1))
        x = em.node('Add', [em.node('Mul', [x, scale], 'transform_input'), shift], 'transform_input')
    _emit(net, em, x)

    size = sum(len(t) for t in em.inits)
    if size > MAX_BYTES:
        raise ValueError('%s: %.2f GB of weights; an ONNX file without external data holds at most 2 GB'
                         % (model_name, size / 1e9))
    b = int(batch_size) if batch_size else 'batch_size'
    g = (b''.join(_bytes(1, nd) for nd in em.nodes) + _bytes(2, 'ifcb_classifier_amd.' + model_name)
         + b''.join(_bytes(5, t) for t in em.inits)
         + _bytes(11, _value_info('input', elem, [b, 3, net.S, net.S])) + _bytes(12, _value_info('output', elem, [b, net.NC])))
    meta = dict(model=model_name, num_classes=str(net.NC), pretrained=str(int(bool(pretrained))), resize=str(net.S),
                version=FORMAT_VERSION)
    if pad is not None:
        from .neuston_data import parse_pad
        meta['pad'] = str(parse_pad(pad))
    from . import __version__
    m = (_int(1, _ir_version(opset)) + _bytes(2, 'ifcb_classifier_amd') + _bytes(3, __version__) + _bytes(7, g)
         + _bytes(8, _bytes(1, '') + _int(2, opset))
         + b''.join(_bytes(14, _bytes(1, 'ifcbk.' + k) + _bytes(2, v)) for k, v in meta.items()))
    if len(m) > MAX_BYTES:
        raise ValueError('%s: the ONNX message is %d bytes; protobuf holds at most 2 GB' % (model_name, len(m)))
    with open(path, 'wb') as f:
        f.write(m)
    return len(m)


def read_pad(metadata):
    """the ``pad`` setting of a file's ``metadata`` dict (``read(path)['metadata']``): None without ``ifcbk.pad``"""
    from .neuston_data import parse_pad
    return parse_pad(metadata.get('ifcbk.pad'))


def write_classes(path, classes):
    """the ``.classes`` file next to an export: one label per line, no trailing newline (upstream's ``'\\n'.join``)"""
    with open(path, 'w') as f:
        f.write('\n'.join(classes))


# ------------------------------------------------------------------------------------------ reading
def _fields(buf):
    """(field number, wire type, value) of one message; value = int for varint / fixed, memoryview for length-delimited"""
    i, n = 0, len(buf)
    while i < n:
        key, i = _read_varint(buf, i)
        f, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _read_varint(buf, i)
        elif wt == 2:
            ln, i = _read_varint(buf, i)
            v, i = buf[i:i + ln], i + ln
        elif wt == 5:
            v, i = bytes(buf[i:i + 4]), i + 4
        elif wt == 1:
            v, i = bytes(buf[i:i + 8]), i + 8
        else:
            raise ValueError('protobuf wire type %d' % wt)
        yield f, wt, v


def _read_varint(buf, i):
    v, s = 0, 0
    while True:
        b = buf[i]
        i += 1
        v |= (b & 0x7F) << s
        s += 7
        if not b & 0x80:
            return v, i


_NP = {FLOAT: np.float32, FLOAT16: np.float16}


def _read_tensor(buf):
    dims, dtype, name, raw = [], None, None, None
    for f, wt, v in _fields(buf):
        if f == 1:
            dims.extend([v] if wt == 0 else [x for _, _, x in _fields_packed(v)])
        elif f == 2:
            dtype = v
        elif f == 8:
            name = bytes(v).decode()
        elif f == 9:
            raw = v
    if dtype not in _NP or raw is None:
        raise ValueError('initializer %s: only raw FLOAT / FLOAT16 tensors are read (data_type %s)' % (name, dtype))
    return name, np.frombuffer(raw, dtype=np.dtype(_NP[dtype]).newbyteorder('<')).reshape(dims)


def _fields_packed(buf):
    i = 0
    while i < len(buf):
        v, i = _read_varint(buf, i)
        yield None, 0, v


def _read_value_info(buf):
    name, elem, dims = None, None, []
    for f, _, v in _fields(buf):
        if f == 1:
            name = bytes(v).decode()
        elif f == 2:
            for f2, _, tt in _fields(v):
                if f2 != 1:
                    continue
                for f3, _, v3 in _fields(tt):
                    if f3 == 1:
                        elem = v3
                    elif f3 == 2:
                        for _, _, dim in _fields(v3):
                            for f4, _, v4 in _fields(dim):
                                if f4 == 1:
                                    dims.append(v4)
                                elif f4 == 2:
                                    dims.append(bytes(v4).decode())
    return dict(name=name, elem_type=elem, dims=dims)


def read(path):
    """{'ir_version', 'opset', 'metadata': {key: value}, 'inputs' / 'outputs': [{name, elem_type, dims}],
    'initializers': {name: ndarray}} of an ONNX file (node list not decoded)"""
    with open(path, 'rb') as f:
        buf = memoryview(f.read())
    out = dict(ir_version=None, opset=None, metadata={}, inputs=[], outputs=[], initializers={})
    for f, _, v in _fields(buf):
        if f == 1:
            out['ir_version'] = v
        elif f == 8:
            d = dict((f2, v2) for f2, _, v2 in _fields(v))
            if not bytes(d.get(1, b'')):
                out['opset'] = d.get(2)
        elif f == 14:
            d = dict((f2, bytes(v2).decode()) for f2, _, v2 in _fields(v))
            out['metadata'][d.get(1, '')] = d.get(2, '')
        elif f == 7:
            inits = set()
            for f2, _, v2 in _fields(v):
                if f2 == 5:
                    name, arr = _read_tensor(v2)
                    out['initializers'][name] = arr
                    inits.add(name)
                elif f2 == 11:
                    out['inputs'].append(_read_value_info(v2))
                elif f2 == 12:
                    out['outputs'].append(_read_value_info(v2))
            out['inputs'] = [i for i in out['inputs'] if i['name'] not in inits]   # (IR < 4 lists initializers as inputs)
    return out
