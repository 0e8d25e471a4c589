"""Test helper: an independent ONNX protobuf decoder and a torch-CPU evaluator for the op set of the exported backbones.

Written against the public onnx.proto schema only -- it does not import the package's writer or reader -- so a file that this
decoder reads and this evaluator reproduces is checked from outside.  The same code reads the files torch's own serializer
writes (tests/test_onnx_cpu.py), which pins the field numbers used here.
"""
import struct

import numpy as np
import torch
import torch.nn.functional as F

_DTYPES = {1: np.float32, 6: np.int32, 7: np.int64, 10: np.float16, 11: np.float64, 9: np.bool_}


def _varint(buf, i):
    v = s = 0
    while True:
        b = buf[i]
        i += 1
        v |= (b & 0x7F) << s
        s += 7
        if b < 0x80:
            return v, i


def _signed(v):
    return v - (1 << 64) if v >= 1 << 63 else v


def fields(buf):
    """[(field number, wire type, value)]: varint -> int, 64-bit / 32-bit -> bytes, length-delimited -> bytes"""
    out, i = [], 0
    while i < len(buf):
        key, i = _varint(buf, i)
        num, wt = key >> 3, key & 7
        if wt == 0:
            v, i = _varint(buf, i)
        elif wt == 1:
            v, i = bytes(buf[i:i + 8]), i + 8
        elif wt == 2:
            n, i = _varint(buf, i)
            v, i = bytes(buf[i:i + n]), i + n
        elif wt == 5:
            v, i = bytes(buf[i:i + 4]), i + 4
        else:
            raise ValueError('wire type %d' % wt)
        out.append((num, wt, v))
    return out


def _ints(wt, v):
    """a repeated int64 field entry: one varint, or a packed run of them"""
    if wt == 0:
        return [_signed(v)]
    res, i = [], 0
    while i < len(v):
        x, i = _varint(v, i)
        res.append(_signed(x))
    return res


def decode_tensor(buf):
    dims, dtype, name, raw, floats, int64s, int32s = [], 1, '', None, [], [], []
    for num, wt, v in fields(buf):
        if num == 1:
            dims += _ints(wt, v)
        elif num == 2:
            dtype = v
        elif num == 8:
            name = v.decode()
        elif num == 9:
            raw = v
        elif num == 4:
            floats += [struct.unpack('<f', v)[0]] if wt == 5 else list(struct.unpack('<%df' % (len(v) // 4), v))
        elif num == 7:
            int64s += _ints(wt, v)
        elif num == 5:
            int32s += _ints(wt, v)
    np_t = _DTYPES[dtype]
    if raw is not None:
        a = np.frombuffer(raw, dtype=np.dtype(np_t).newbyteorder('<')).astype(np_t)
    elif floats:
        a = np.array(floats, np_t)
    elif int64s:
        a = np.array(int64s, np_t)
    else:
        a = np.array(int32s, np.int32).view(np.uint16).reshape(-1, 2)[:, 0].view(np.float16) if dtype == 10 else np.array(int32s, np_t)
    return name, dtype, a.reshape(dims)


def decode_attr(buf):
    d = {'ints': [], 'floats': []}
    for num, wt, v in fields(buf):
        if num == 1:
            d['name'] = v.decode()
        elif num == 2:
            d['f'] = struct.unpack('<f', v)[0]
        elif num == 3:
            d['i'] = _signed(v)
        elif num == 4:
            d['s'] = v
        elif num == 5:
            d['t'] = decode_tensor(v)
        elif num == 7:
            d['floats'] += [struct.unpack('<f', v)[0]] if wt == 5 else list(struct.unpack('<%df' % (len(v) // 4), v))
        elif num == 8:
            d['ints'] += _ints(wt, v)
        elif num == 20:
            d['type'] = v
    t = d.get('type')
    value = {1: d.get('f'), 2: d.get('i'), 3: d.get('s'), 4: d.get('t'), 6: d['floats'], 7: d['ints']}.get(t)
    return d['name'], value


def decode_value_info(buf):
    name, elem, dims = '', None, []
    for num, _, v in fields(buf):
        if num == 1:
            name = v.decode()
        elif num == 2:                                   # TypeProto.tensor_type
            for n2, _, tt in fields(v):
                if n2 != 1:
                    continue
                for n3, _, v3 in fields(tt):
                    if n3 == 1:
                        elem = v3
                    elif n3 == 2:                        # TensorShapeProto.dim
                        for _, _, dim in fields(v3):
                            for n4, _, v4 in fields(dim):
                                dims.append(_signed(v4) if n4 == 1 else v4.decode())
    return dict(name=name, elem_type=elem, dims=dims)


def decode_model(data):
    """ModelProto -> plain dict: ir_version, opset_import {domain: version}, producer, metadata, graph{nodes, initializers,
    inputs, outputs}"""
    m = dict(ir_version=None, opset_import={}, metadata={}, producer=None)
    for num, wt, v in fields(data):
        if num == 1:
            m['ir_version'] = v
        elif num == 2:
            m['producer'] = v.decode()
        elif num == 8:
            d = dict((n, x) for n, _, x in fields(v))
            m['opset_import'][d.get(1, b'').decode()] = d.get(2)
        elif num == 14:
            d = dict((n, x.decode()) for n, _, x in fields(v))
            m['metadata'][d.get(1, '')] = d.get(2, '')
        elif num == 7:
            g = dict(nodes=[], initializers={}, init_types={}, inputs=[], outputs=[])
            for n2, _, v2 in fields(v):
                if n2 == 1:
                    nd = dict(inputs=[], outputs=[], attrs={}, op=None)
                    for n3, _, v3 in fields(v2):
                        if n3 == 1:
                            nd['inputs'].append(v3.decode())
                        elif n3 == 2:
                            nd['outputs'].append(v3.decode())
                        elif n3 == 4:
                            nd['op'] = v3.decode()
                        elif n3 == 5:
                            k, val = decode_attr(v3)
                            nd['attrs'][k] = val
                    g['nodes'].append(nd)
                elif n2 == 5:
                    name, dt, arr = decode_tensor(v2)
                    g['initializers'][name] = arr
                    g['init_types'][name] = dt
                elif n2 == 11:
                    g['inputs'].append(decode_value_info(v2))
                elif n2 == 12:
                    g['outputs'].append(decode_value_info(v2))
            g['inputs'] = [i for i in g['inputs'] if i['name'] not in g['initializers']]
            m['graph'] = g
    return m


def load(path):
    with open(path, 'rb') as f:
        return decode_model(f.read())


def _pads(a, k):
    p = a.get('pads') or [0] * (2 * k)
    assert p[:k] == p[k:], 'asymmetric pads %s' % p
    return p[:k]


def evaluate(model, x, half_storage=None):
    """run the decoded graph on torch CPU in float32 (``x`` rounded to the graph input's type first).  half_storage (default: the
    graph's input is FLOAT16) rounds every node output to float16, as a runtime storing fp16 activations would."""
    g = model['graph']
    half_input = g['inputs'][0]['elem_type'] == 10
    if half_storage is None:
        half_storage = half_input
    env = {k: torch.from_numpy(np.array(v)) for k, v in g['initializers'].items()}
    env = {k: (v.float() if v.is_floating_point() else v) for k, v in env.items()}
    xin = torch.as_tensor(x)
    env[g['inputs'][0]['name']] = (xin.half() if half_input else xin).float()
    for nd in g['nodes']:
        op, a, i = nd['op'], nd['attrs'], [env.get(n) if n else None for n in nd['inputs']]
        if op == 'Conv':
            k = len(a.get('kernel_shape') or i[1].shape[2:])
            y = F.conv2d(i[0], i[1], i[2] if len(i) > 2 else None, stride=a.get('strides') or 1, padding=_pads(a, k),
                         dilation=a.get('dilations') or 1, groups=a.get('group') or 1)
        elif op == 'BatchNormalization':
            y = F.batch_norm(i[0], i[3], i[4], i[1], i[2], False, 0.0, a.get('epsilon', 1e-5))
        elif op == 'Relu':
            y = F.relu(i[0])
        elif op in ('MaxPool', 'AveragePool'):
            ks = a['kernel_shape']
            kw = dict(kernel_size=ks, stride=a.get('strides') or 1, padding=_pads(a, len(ks)), ceil_mode=bool(a.get('ceil_mode', 0)))
            if op == 'MaxPool':
                y = F.max_pool2d(i[0], **kw)
            else:
                y = F.avg_pool2d(i[0], count_include_pad=bool(a.get('count_include_pad', 0)), **kw)
        elif op == 'GlobalAveragePool':
            y = i[0].mean(dim=(2, 3), keepdim=True)
        elif op == 'Flatten':
            ax = a.get('axis', 1)
            y = i[0].reshape(int(np.prod(i[0].shape[:ax])), -1)
        elif op == 'Gemm':
            A = i[0].t() if a.get('transA') else i[0]
            B = i[1].t() if a.get('transB') else i[1]
            y = a.get('alpha', 1.0) * (A @ B)
            if len(i) > 2 and i[2] is not None:
                y = y + a.get('beta', 1.0) * i[2]
        elif op == 'Concat':
            y = torch.cat(i, dim=a['axis'])
        elif op in ('Add', 'Mul', 'Sub', 'Div'):
            y = {'Add': torch.add, 'Mul': torch.mul, 'Sub': torch.sub, 'Div': torch.div}[op](i[0], i[1])
        elif op in ('Identity', 'Dropout'):
            y = i[0]
        elif op == 'Constant':
            y = torch.from_numpy(np.array(a['value'][2]))
            y = y.float() if y.is_floating_point() else y
        elif op == 'Gather':
            y = torch.index_select(i[0], a.get('axis', 0), i[1].reshape(-1).long())
            if i[1].dim() == 0:
                y = y.squeeze(a.get('axis', 0))
        elif op == 'Unsqueeze':
            y = i[0]
            for ax in sorted(a['axes'] if 'axes' in a else i[1].tolist()):
                y = y.unsqueeze(ax)
        elif op == 'Slice':
            y = i[0]
            starts, ends = i[1].tolist(), i[2].tolist()
            axes = i[3].tolist() if len(i) > 3 and i[3] is not None else list(range(len(starts)))
            steps = i[4].tolist() if len(i) > 4 and i[4] is not None else [1] * len(starts)
            for s, e, ax, st in zip(starts, ends, axes, steps):
                n = y.shape[ax]
                y = y.narrow(ax, 0, n)[(slice(None),) * ax + (slice(max(-n, min(s, n)), max(-n - 1, min(e, n)), st),)]
        elif op == 'Reshape':
            shape = [d if d != 0 else i[0].shape[j] for j, d in enumerate(i[1].tolist())]
            y = i[0].reshape(shape)
        else:
            raise NotImplementedError('evaluator: op %s' % op)
        if half_storage and y.is_floating_point():
            y = y.half().float()
        env[nd['outputs'][0]] = y
    return env[g['outputs'][0]['name']]
