"""Walk the HIP plan node by node after one forward+backward and check every node against the node-level
CPU oracle (oracle/ops.py) on the HIP path's OWN inputs (teacher forcing).  Returns a dict of worst errors.

fp64 mode (check_plan(..., fp64=Snapshot(hip))): the same walk after one fused ``eng.train_step(N)``.  Every quantity is evaluated
three ways -- what the HIP step stored, oracle/ops.py at fp32 storage, the same oracle/ops.py call on .double() inputs -- and
recorded in ``fp64.rows`` as (node, kernel, quantity, e_hip, e_ora): the relative L2 distances of the first two to the third.  The
gradients are read from the engine's flat buffer, the parameters from the snapshot made BEFORE the step (the optimizer has moved the
live ones), and two quantities join that only the fused step has: the loss kernel's dlogits and the optimizer update of every tensor
(from the HIP gradient).  The d(raw) of a BatchNorm backward lives in a per-lane scratch that the next layer overwrites, so dW and
the input gradient are held as BatchNorm-backward-then-conv composites on the stored upstream gradient, as in the fp32 walk."""
import ctypes as C

import torch

from oracle import ops as O


def rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _nchw(t, view, N):
    return t[:N, :, :, view.coff:view.coff + view.C].float().cpu().permute(0, 3, 1, 2).contiguous()


def _flat_view(eng, flat, key):
    """a tensor of one of the engine's flat buffers (P, G, M, V) in the layout of the module's parameter"""
    o, n, shape, kind, node = eng.poff[key]
    if kind == 'conv':
        K, Cw, R, S = shape
        return flat[o:o + n].view(K, R, S, Cw).permute(0, 3, 1, 2)
    return flat[o:o + n].view(shape)


class Snapshot:
    """the state the fp64 walk needs from BEFORE the fused step: parameters and optimizer state (host copies)"""

    def __init__(self, hip, target=None, hook=None):
        eng = hip.engine
        self.keys = [k for k, _ in hip.named_parameters()]
        self.P = {k: p.detach().cpu().clone() for k, p in hip.named_parameters()}
        self.M = {k: _flat_view(eng, eng.M, k).cpu().clone() for k in self.keys}
        self.V = {k: _flat_view(eng, eng.V, k).cpu().clone() for k in self.keys}
        self.step = eng.step_count
        self.target = target            # the labels of the step (host), for the loss kernel's dlogits
        self.hook = hook                # hook(quantity, node name, kernel, **tensors): per-element checks of the caller
        self.rows = []                  # (node, kernel, quantity, e_hip, e_ora)


def op_kernels(eng, N):
    """node tag -> {op kind: kernel name} over the fused step's op table (ifcbk_op_kernel; the op's name where it resolves none)"""
    from ifcb_classifier_amd import _lib
    p = eng.plan(N).step
    buf = C.create_string_buffer(256)
    out = {}
    for k in range(p.n):
        o = p.arr[k]
        eng.ctx.lib.ifcbk_op_kernel(C.byref(o), buf, 256)
        name = buf.value.decode() or _lib.OP_NAMES.get(o.kind, str(o.kind))
        out.setdefault(p.tags[k].split('[')[0], {}).setdefault(_lib.OP_NAMES.get(o.kind, str(o.kind)), name)
    return out


def _dbl(t):
    return None if t is None else t.double()


def optimizer_update(eng, p, g, m, v, step, dtype):
    """torch.optim's step of the engine's optimizer on (p, g) from state (m, v) after `step` steps, evaluated in `dtype` -> p - p0"""
    p0 = p.to(dtype)
    q = p0.clone().requires_grad_(True)
    if eng.optimizer == 'sgd':
        opt = torch.optim.SGD([q], lr=eng.lr, momentum=eng.momentum, weight_decay=eng.weight_decay)
        if step > 0 and eng.momentum:
            opt.state[q] = dict(momentum_buffer=m.to(dtype).clone())
    else:
        opt = torch.optim.Adam([q], lr=eng.lr, betas=tuple(eng.betas), eps=eng.eps, weight_decay=eng.weight_decay)
        if step > 0:
            opt.state[q] = dict(step=torch.tensor(float(step)), exp_avg=m.to(dtype).clone(), exp_avg_sq=v.to(dtype).clone())
    q.grad = g.to(dtype).clone()
    opt.step()
    return q.detach() - p0


def check_plan(hip, N, mask=None, verbose=False, fp64=None):
    eng = hip.engine
    net = eng.net
    act = lambda v: _nchw(eng.act[v.buf.id], v, N)
    grd = lambda v: _nchw(eng.grad[v.buf.id], v, N)
    kern = None        # (fp64 mode only, as are kn, row and add_expected64 below)
    if fp64 is None:
        P = {k: p.detach().cpu() for k, p in hip.named_parameters()}
        G = {k: p.grad.detach().cpu() for k, p in hip.named_parameters()}
    else:
        assert O.STORAGE == 'fp32', 'the fp64-arbitrated walk is stated for the fp32 parity mode'
        P = fp64.P
        G = {k: _flat_view(eng, eng.G, k).detach().cpu().clone() for k in fp64.keys}
        kern = op_kernels(eng, N)
    expected64 = {}    # buf id -> the same in fp64 (fp64 mode)
    contrib = {}       # buf id -> kernels that wrote into its gradient
    chains = {}

    def kn(name, *kinds):
        assert fp64 is not None
        ks = {}
        for tag, d in kern.items():
            if name in tag.split('+'):              # (a fused op carries both nodes' names: 'conv1+maxpool')
                ks.update(d)
        return ' + '.join(dict.fromkeys(ks[k] for k in kinds if k in ks)) or '-'

    def row(q, name, kernel, got, ora32, ref64, **hook):
        """fp64 mode: one quantity three ways"""
        assert fp64 is not None
        e_h, e_o = rel(got, ref64), rel(ora32, ref64)
        fp64.rows.append((name, kernel, q, e_h, e_o))
        if verbose:
            print('fp64 %-8s %-28s %-44s hip %.3e  oracle %.3e' % (q, name, kernel, e_h, e_o))
        if fp64.hook is not None:
            fp64.hook(q, name, kernel, got=got, ref64=ref64, **hook)

    def add_expected64(view, g, kernel, chain=1):
        b = view.buf
        if b.id not in expected64:
            expected64[b.id] = torch.zeros(N, b.C, b.H, b.W, dtype=torch.float64)
        expected64[b.id][:, view.coff:view.coff + view.C] += g
        contrib.setdefault(b.id, []).append(kernel)
        chains[b.id] = max(chains.get(b.id, 1), chain)      # the longest fp32 summation chain behind an element
    expected = {}      # buf id -> expected total gradient (NCHW fp32)
    worst = dict(raw=0.0, raw_cp=0.0, y=0.0, dW=0.0, dW_cp=0.0, dgamma=0.0, dbeta=0.0, pool=0.0, head=0.0, dx=0.0, stats=0.0)

    relu_out = {}      # buf id -> [(coff, C, activation)]: conv(+bias)+ReLU outputs whose stored gradient is already masked in place

    def add_expected(view, g):
        b = view.buf
        if b.id not in expected:
            expected[b.id] = torch.zeros(N, b.C, b.H, b.W)
        expected[b.id][:, view.coff:view.coff + view.C] += g

    def upd(k, e, name):
        if verbose:
            print('%-8s %-34s %.3e' % (k, name, e))
        worst[k] = max(worst[k], e)

    def upd_dgamma(name, g_hip, dg32, args, gy, y_h):
        """dgamma = sum(dz * xhat) can cancel to 1e-5 of its terms (a deep random-init network's first BatchNorm): the fp32 oracle's own
        summation order then shows at the 1e-2 level.  Where the two disagree by more than 1e-4 in fp32 storage, an fp64 evaluation of the
        SAME node arbitrates: 'dgamma64' = distance of the HIP result from the fp64 value, 'dgamma64_oracle' = of the fp32 oracle's."""
        e = rel(g_hip, dg32)
        upd('dgamma', e, name)
        if O.STORAGE == 'fp32' and e > 1e-4:
            raw, gamma, beta, eps, relu, res = args
            _, dg64, _, _ = O.bn_act_bwd(raw.double(), gamma.double(), beta.double(), eps, relu, None if res is None else res.double(),
                                         gy.double(), y_for_mask=y_h.double())
            worst['dgamma64'] = max(worst.get('dgamma64', 0.0), rel(g_hip.double(), dg64))
            worst['dgamma64_oracle'] = max(worst.get('dgamma64_oracle', 0.0), rel(dg32.double(), dg64))
            if verbose:
                print('dgamma64 %-34s hip %.3e  fp32 oracle %.3e' % (name, rel(g_hip.double(), dg64), rel(dg32.double(), dg64)))

    fused = getattr(eng, 'fused_pool', {})            # conv node -> (max-pool node, index): activation never materialised
    fused_y = {}                                      # pool node -> the oracle's activation of the HIP raw output
    absorbed = getattr(eng, 'absorbed_pools', set())    # avg pools that run BEHIND their 1x1 conv in training (engine.__init__)
    for k, n in enumerate(net.nodes):
        if fp64 is not None and (n.kind in ('cb', 'drop', 'bnr') or (n.kind == 'head' and not n.fc)):
            raise NotImplementedError('the fp64 walk covers conv+BatchNorm, pool, flatten and fc-head nodes: %s is a %s' % (n.name, n.kind))
        if n.kind == 'conv':
            cp = getattr(n, 'cpool', None)
            if cp is not None:
                # the engine computed avgpool(conv1x1(x)); the reference order conv1x1(avgpool(x)) is the same linear map:
                # the oracle takes the reference order on the block input the HIP path read
                x0 = act(cp.x)
                x = O.pool_fwd('avg', x0, (cp.R, cp.S), (cp.sh, cp.sw), (cp.ph, cp.pw))
            else:
                x = act(n.x)
            if n.x.buf.is_input:
                x = x[:, :3]
            w = P[n.conv_key + '.weight']
            gamma, beta = P[n.bn_key + '.weight'], P[n.bn_key + '.bias']
            stride, pad = (n.sh, n.sw), (n.ph, n.pw)
            raw_h = eng.act[n.raw.id][:N].float().cpu().permute(0, 3, 1, 2).contiguous()
            # a commuted pool branch rounds to the storage type at a different place than the reference order (after the conv
            # and after the pool, instead of after the pool and after the conv): same count of roundings, not the same bits
            upd('raw_cp' if cp is not None else 'raw', rel(raw_h, O.conv_raw(x, w, stride, pad)), n.name)
            res = act(n.residual) if n.residual is not None else None
            y_ref, mean, var = O.bn_act_fwd(raw_h, gamma, beta, n.eps, n.relu, res)
            if n in fused:
                pn = fused[n][0]
                fused_y[pn] = y_ref
                y_h = y_ref
                gy = O.pool_bwd('max', y_ref, (pn.R, pn.S), (pn.sh, pn.sw), (pn.ph, pn.pw), grd(pn.y))
            else:
                y_h = act(n.y)
                gy = grd(n.y)
                upd('y', rel(y_h, y_ref), n.name)
            st_mean = eng.stats[n.st_off:n.st_off + n.K].cpu()
            st_is = eng.stats[n.st_off + n.st_ld:n.st_off + n.st_ld + n.K].cpu()
            upd('stats', max(rel(st_mean, mean), rel(st_is, 1.0 / torch.sqrt(var + n.eps))), n.name)
            d_raw, dg, db, dres = O.bn_act_bwd(raw_h, gamma, beta, n.eps, n.relu, res, gy, y_for_mask=y_h)
            upd_dgamma(n.name, G[n.bn_key + '.weight'], dg, (raw_h, gamma, beta, n.eps, n.relu, res), gy, y_h)
            upd('dbeta', rel(G[n.bn_key + '.bias'], db), n.name)
            need_dx = not n.x.buf.is_input
            dw, dx = O.conv_bwd(x, w, d_raw, stride, pad, need_dx)
            upd('dW_cp' if cp is not None else 'dW', rel(G[n.conv_key + '.weight'], dw), n.name)      # (same remark as raw_cp)
            if fp64 is not None:
                assert cp is None, 'the fp64 walk does not cover commuted pool branches'
                k_fwd, k_bn = kn(n.name, 'conv_fwd'), kn(n.name, 'bn_bwd', 'bn_bwd_maxpool')
                row('raw', n.name, k_fwd, raw_h, O.conv_raw(x, w, stride, pad), O.conv_raw(x.double(), w.double(), stride, pad),
                    x=x, w=w, stride=stride, pad=pad)
                y64, mean64, var64 = O.bn_act_fwd(raw_h.double(), gamma.double(), beta.double(), n.eps, n.relu, _dbl(res))
                row('mean', n.name, k_fwd + ' + ' + kn(n.name, 'bn_finalize'), st_mean, mean, mean64, raw=raw_h, eps=n.eps)
                row('invstd', n.name, k_fwd + ' + ' + kn(n.name, 'bn_finalize'), st_is, 1.0 / torch.sqrt(var + n.eps),
                    1.0 / torch.sqrt(var64 + n.eps), raw=raw_h, eps=n.eps)
                sc = eng.stats[n.st_off + 2 * n.st_ld:n.st_off + 2 * n.st_ld + n.K].cpu()
                sh = eng.stats[n.st_off + 3 * n.st_ld:n.st_off + 3 * n.st_ld + n.K].cpu()
                if n in fused:
                    fused_y[(pn, 64)] = y64
                    fused_y[(pn, 'affine')] = dict(raw=raw_h, scale=sc, shift=sh, relu=n.relu)
                    gy64 = O.pool_bwd('max', y64, (pn.R, pn.S), (pn.sh, pn.sw), (pn.ph, pn.pw), grd(pn.y).double())
                    ymask64 = y64
                else:
                    gy64, ymask64 = gy.double(), y_h.double()
                    row('y', n.name, kn(n.name, 'bn_apply'), y_h, y_ref, y64, raw=raw_h, scale=sc, shift=sh, res=res, relu=n.relu)
                d_raw64, dg64, db64, dres64 = O.bn_act_bwd(raw_h.double(), gamma.double(), beta.double(), n.eps, n.relu, _dbl(res), gy64,
                                                           y_for_mask=ymask64)
                bnb = dict(raw=raw_h, gy=gy64, ymask=ymask64, mean=st_mean, invstd=st_is, gamma=gamma, relu=n.relu, scale=sc, shift=sh,
                           pooled=n in fused)
                row('dgamma', n.name, k_bn, G[n.bn_key + '.weight'], dg, dg64, **bnb)
                row('dbeta', n.name, k_bn, G[n.bn_key + '.bias'], db, db64, **bnb)
                dw64, dx64 = O.conv_bwd(x.double(), w.double(), d_raw64, stride, pad, need_dx)
                row('dW', n.name, k_bn + ' + ' + kn(n.name, 'conv_wgrad'), G[n.conv_key + '.weight'], dw, dw64, x=x, d_raw64=d_raw64, w=w,
                    stride=stride, pad=pad, desc=eng._conv_desc(n, N), bn=bnb, xbuf=n.x.buf.name if need_dx else None,
                    resbuf=None if n.residual is None else n.residual.buf.name)
                if need_dx:
                    add_expected64(n.x, dx64, k_bn + ' + ' + kn(n.name, 'conv_dgrad'), n.R * n.S * n.K)
                if dres64 is not None:
                    add_expected64(n.residual, dres64, k_bn)
            if need_dx and cp is not None:
                add_expected(cp.x, O.pool_bwd('avg', x0, (cp.R, cp.S), (cp.sh, cp.sw), (cp.ph, cp.pw), dx))
            elif need_dx:
                add_expected(n.x, dx)
            if dres is not None:
                add_expected(n.residual, dres)
        elif n.kind in ('max', 'avg'):
            if n in absorbed:
                continue                          # checked together with its conv above
            x = fused_y[n] if n in fused_y else act(n.x)
            upd('pool', rel(act(n.y), O.pool_fwd(n.kind, x, (n.R, n.S), (n.sh, n.sw), (n.ph, n.pw))), n.name)
            if n not in fused_y:
                add_expected(n.x, O.pool_bwd(n.kind, x, (n.R, n.S), (n.sh, n.sw), (n.ph, n.pw), grd(n.y)))
            if fp64 is not None:
                geo = ((n.R, n.S), (n.sh, n.sw), (n.ph, n.pw))
                x64 = fused_y[(n, 64)] if n in fused_y else x.double()
                k_pool = kn(n.name, 'maxpool_fwd', 'avgpool_fwd', 'bn_apply_maxpool')
                row('pool', n.name, k_pool, act(n.y), O.pool_fwd(n.kind, x, *geo), O.pool_fwd(n.kind, x64, *geo), exact=n.kind == 'max',
                    x=x, geo=geo, kind=n.kind, fused=fused_y.get((n, 'affine')))
                if n not in fused_y:
                    add_expected64(n.x, O.pool_bwd(n.kind, x64, *geo, grd(n.y).double()), kn(n.name, 'maxpool_bwd', 'avgpool_bwd'), 4)
        elif n.kind == 'cb':
            # conv (+bias) (+ReLU) without BatchNorm, nn.Linear as a 1x1 conv: ONE stored tensor; its gradient buffer holds
            # dz = dy * (y > 0) (masked in place by ifcbk_bias_relu_bwd)
            x = act(n.x)
            if n.x.buf.is_input:
                x = x[:, :3]
            w = P[n.key + '.weight']
            if w.dim() == 2:
                w = w[:, :, None, None]
            kr = n.K_real
            bias = P[n.key + '.bias'] if n.bias else None
            stride, pad = (n.sh, n.sw), (n.ph, n.pw)
            y_h = act(n.y)
            y_ref = torch.nn.functional.conv2d(x, O.bf16_round(w), bias, stride, pad)
            y_ref = O.bf16_round(torch.relu(y_ref) if n.relu else y_ref)
            upd('y', rel(y_h[:, :kr], y_ref), n.name)
            if kr != n.K:
                assert float(y_h[:, kr:].abs().max()) == 0.0, n.name       # padded output channels stay zero
            dz = grd(n.y)
            if n.relu:
                assert float((dz * (y_h <= 0)).abs().max()) == 0.0, n.name + ': gradient not masked'
                relu_out.setdefault(n.y.buf.id, []).append((n.y.coff, n.y.C, y_h))
            if bias is not None:
                upd('dbeta', rel(G[n.key + '.bias'], dz[:, :kr].sum((0, 2, 3))), n.name)
            need_dx = not n.x.buf.is_input
            dw, dx = O.conv_bwd(x, w, dz[:, :kr], stride, pad, need_dx)
            upd('dW', rel(G[n.key + '.weight'].reshape(dw.shape), dw), n.name)
            if need_dx:
                add_expected(n.x, dx)
        elif n.kind == 'drop':
            x = act(n.x)
            m = n.mask[:N].reshape(N, n.x.H, n.x.W, n.x.C).permute(0, 3, 1, 2).float().cpu() * (1.0 / (1.0 - n.p))
            upd('pool', rel(act(n.y), O.bf16_round(x * m)), n.name)
            add_expected(n.x, grd(n.y) * m)
        elif n.kind == 'flat':
            x = act(n.x)
            upd('pool', rel(act(n.y).reshape(N, -1), torch.flatten(x, 1)), n.name)
            add_expected(n.x, grd(n.y).reshape(x.shape))
            if fp64 is not None:
                row('pool', n.name, kn(n.name, 'flatten_chw'), act(n.y).reshape(N, -1), torch.flatten(x, 1), torch.flatten(x, 1).double(),
                    exact=True)
                add_expected64(n.x, grd(n.y).reshape(x.shape).double(), kn(n.name, 'flatten_chw'))
        elif n.kind == 'bnr':
            # BatchNorm -> ReLU in front of a conv (densenet), on a channel slice of the block's concatenation
            x = act(n.x)
            gamma, beta = P[n.bn_key + '.weight'], P[n.bn_key + '.bias']
            y_ref, mean, var = O.bn_act_fwd(x, gamma, beta, n.eps, n.relu)
            y_h = act(n.y)
            upd('y', rel(y_h, y_ref), n.name)
            st_mean = eng.stats[n.st_off:n.st_off + n.K].cpu()
            st_is = eng.stats[n.st_off + n.st_ld:n.st_off + n.st_ld + n.K].cpu()
            upd('stats', max(rel(st_mean, mean), rel(st_is, 1.0 / torch.sqrt(var + n.eps))), n.name)
            d_x, dg, db, _ = O.bn_act_bwd(x, gamma, beta, n.eps, n.relu, None, grd(n.y), y_for_mask=y_h)
            upd_dgamma(n.name, G[n.bn_key + '.weight'], dg, (x, gamma, beta, n.eps, n.relu, None), grd(n.y), y_h)
            upd('dbeta', rel(G[n.bn_key + '.bias'], db), n.name)
            add_expected(n.x, d_x)
        elif n.kind == 'head' and not n.fc:
            # squeezenet: the pooled channels of the classifier conv ARE the logits
            x = act(n.x)
            logits = x.mean((2, 3))[:, :n.NC]
            upd('head', rel(n.logits[:N].cpu(), logits), n.name + ':logits')
            dl = n.dlogits[:N].cpu()
            dx = torch.zeros_like(x)
            dx[:, :n.NC] = (dl / float(n.HW))[:, :, None, None]
            add_expected(n.x, O.bf16_round(dx))
        elif n.kind == 'head':
            x = act(n.x)
            W, b = P[n.key + '.weight'], P[n.key + '.bias']
            m = mask[:N] if (n.dropout and mask is not None) else None
            feat, logits = O.head_fwd(x, W, b, m)
            upd('head', rel(n.logits[:N].cpu(), logits), n.name + ':logits')
            dl = n.dlogits[:N].cpu()
            dx, dW, db = O.head_bwd(x, W, b, m, dl)
            upd('head', rel(G[n.key + '.weight'], dW), n.name + ':dW')
            upd('head', rel(G[n.key + '.bias'], db), n.name + ':db')
            add_expected(n.x, dx)
            if fp64 is not None:
                k_f, k_b = kn(n.name, 'head_fwd'), kn(n.name, 'head_bwd')
                _, logits64 = O.head_fwd(x.double(), W.double(), b.double(), m)
                lg_h = n.logits[:N].cpu()
                row('logits', n.name, k_f, lg_h, logits, logits64, x=x, W=W, b=b)
                dx64, dW64, db64 = O.head_bwd(x.double(), W.double(), b.double(), m, dl.double())
                row('head dW', n.name, k_b, G[n.key + '.weight'], dW, dW64, x=x, dl=dl, W=W, xbuf=n.x.buf.name)
                row('head db', n.name, k_b, G[n.key + '.bias'], db, db64, dl=dl)
                add_expected64(n.x, dx64, k_b, n.NC + 3)
                if fp64.target is not None:
                    wgt = 0.4 if n.aux else 1.0
                    _, dl32 = O.xent(lg_h, fp64.target[:N], wgt)
                    _, dl64 = O.xent(lg_h.double(), fp64.target[:N], wgt)
                    row('dlogits', 'loss_aux' if n.aux else 'loss', kn('loss_aux' if n.aux else 'loss', 'softmax_xent', 'softmax_xent_w'),
                        dl, dl32, dl64, logits=lg_h, target=fp64.target[:N], weight=wgt)
    for bid, g in expected.items():
        b = net.bufs[bid]
        for coff, Cc, y_h in relu_out.get(bid, ()):
            g[:, coff:coff + Cc] *= (y_h > 0).to(g.dtype)
        dx_h = _nchw(eng.grad[bid], b.full(), N)
        upd('dx', rel(dx_h, g), b.name)
        if fp64 is not None:
            row('dx', b.name, ' | '.join(dict.fromkeys(contrib[bid])), dx_h, g, expected64[bid], chain=chains[bid])
    if fp64 is not None:
        # the optimizer update of every tensor, from the HIP gradient and the state before the step
        tag = [t for t in kern if t in ('sgd', 'adam')][0]
        for key in fp64.keys:
            p_new = _flat_view(eng, eng.P, key).detach().cpu()
            st = (eng, fp64.P[key], G[key], fp64.M[key], fp64.V[key], fp64.step)
            row('update', key, kn(tag, 'sgd', 'adam'), p_new - fp64.P[key], optimizer_update(*st, torch.float32),
                optimizer_update(*st, torch.float64), p=fp64.P[key], g=G[key], m=fp64.M[key], v=fp64.V[key], step=fp64.step, p_new=p_new)
    return worst
