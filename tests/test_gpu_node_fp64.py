"""Every quantity of every node of ONE fused fp32 train step of resnet18 (nc 2, 224 x 224, SGD(0.005, 0.9), the seeds of
test_gpu_trained_weights._trajectories), at batch 8 and at batch 16, arbitrated by float64: local_parity.check_plan in its fp64 mode
evaluates each node on the HIP step's own stored inputs three ways (HIP, oracle/ops.py in fp32, the same call in float64).

Two conditions per quantity:

1. the a-priori per-element bound of conv_bounds.py / op_bounds.py for that kernel's arithmetic, on the node's real inputs and real
   reduction lengths.  No new constants; where a kernel's operand lives only in the step's scratch, the bound of the kernel that
   wrote it is carried through (the composites below):
     raw            conv_bounds.check on the stored input and the snapshot filter
     mean, invstd   op_bounds.finalize on the float64 128-pixel partial rows of the stored raw output, plus the rows' own fp32 error
                    gamma_(128 + 2) * sum |terms| (conv_bounds.check_sums' rule for one row), carried through finalize's formulas
     y, pool-fused stem activation   op_bounds.affine with the step's stored scale / shift (the max over a window is 1-Lipschitz)
     dgamma, dbeta  op_bounds.BnBwd.check_params (mask from the stored y; the pool-fused stem: mask recomputed, ambiguity allowed)
     dW             conv_bounds.wgrad on d(raw) = BnBwd.dx's float64 value, plus BnBwd.dx's e carried through sum |x| e
     dx per buffer  the sum of its writers: conv_bounds.dgrad on the same d(raw) plus its e through sum |w| e; the residual branch's
                    dz (a copy); op_bounds.head_dx; one rounding per accumulating writer.  A buffer with ONE writer that copies
                    (the downsample branches' outputs) is bit-equal
     logits, head dW, head db   op_bounds.gap / fc_fwd / fc_wgrad / fc_bgrad, the pooled features' e carried through |W| and |dl|
     dlogits        op_bounds.xent;   update   op_bounds.sgd / adam;   max pool, flatten: bit-equal to the float64 value rounded once

2. e_hip <= F * e_ora + 2^-24 in relative L2 norm to the float64 value.  2^-24: one correct rounding of the exact value to fp32 is at
   most that far away, below it a ratio compares noise.  F comes from the summation model of conv_bounds.py: a fp32 sum of n terms
   in one chain carries gamma_n, a pairwise sum gamma_ceil(log2 n); errors of random sign grow like the square root of the count, so
   the expected ratio is sqrt(gamma_n / gamma_ceil(log2 n)), times 2 for the spread of one draw.  n is the longest fp32 chain of the
   HIP kernel: R S C of the MFMA k-loop (raw), the 128-row tile of the conv epilogue's statistics, the 1024-row tile of the
   BatchNorm-backward sums, split_len + nsplit of conv_wgrad_f32's split-K (dW: wgrad_f32_split mirrors make_plan and is held to the
   library's workspace query), R S K (input gradient), C + 2 (logits), N + 2 (head gradients), NC (dlogits); 1 for elementwise
   kernels (F = 2).  Measured worst ratios per kind: DESIGN.md 4a.  No kind is out of line at batch 8 against batch 16."""
import ctypes as C
import math

import pytest
import torch

import conv_bounds as cb
import local_parity as LP
import op_bounds as ob
from test_gpu_conv_f32_bounds import pick_tile

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -24
U = cb.U


def F_of(n):
    """2 x the model's expected error of one fp32 chain of n terms over that of a pairwise sum of n terms"""
    if n < 2:
        return 2.0
    return 2.0 * math.sqrt(cb.gamma(n) / cb.gamma(math.ceil(math.log2(n))))


def wgrad_f32_split(M, K, RSC):
    """conv_wgrad.hip make_plan for fp32 (32-pixel steps, 128-column tiles, 512 resident blocks) -> (nsplit, split_len)"""
    cdiv = lambda a, b: -(-a // b)
    tiles = cdiv(K, 32 * pick_tile(K)) * cdiv(RSC, 128)
    steps = cdiv(M, 32)
    ns = max(1, min(512 // tiles, max(steps // 8, 1)))
    ln = cdiv(steps, ns) * 32
    return cdiv(M, ln), ln


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _rows(t):
    """NCHW -> [M, C]"""
    return _nhwc(t).reshape(-1, t.shape[1])


def _chain(eng, q, kw):
    if q == 'raw':
        return kw['w'][0].numel()
    if q in ('mean', 'invstd'):
        return 128
    if q in ('dgamma', 'dbeta'):
        r = kw['raw']
        return min(1024, r.numel() // r.shape[1])
    if q == 'dW':
        d = kw['desc']
        ns, ln = wgrad_f32_split(d.N * d.P * d.Q, d.K, d.R * d.S * d.C)
        assert eng.ctx.lib.ifcbk_conv2d_wgrad_workspace(C.byref(d)) == ns * d.K * d.R * d.S * d.C * 4, 'wgrad_f32_split is not make_plan'
        return min(ln, d.N * d.P * d.Q) + ns
    if q == 'dx':
        return kw['chain']
    if q == 'logits':
        return kw['W'].shape[1] + 2
    if q in ('head dW', 'head db'):
        return kw['dl'].shape[0] + 2
    if q == 'dlogits':
        return kw['logits'].shape[1]
    return 1          # y, pool, update: elementwise


class Bounds:
    """condition 1, quantity by quantity in the order of the walk; the writers of every gradient buffer are collected on the way"""

    def __init__(self, eng):
        self.eng = eng
        self.bad, self.checked = [], {}
        self.writers = {}          # buffer name -> [(want NHWC float64, e, copies)]
        self.bn = {}               # node name -> its BnBwd (dgamma, dbeta and dW share it)

    def _bnbwd(self, name, b):
        if name not in self.bn:
            self.bn.clear()        # (one node at a time: the float64 tensors of the stem are large)
            pooled = b['pooled']
            self.bn[name] = ob.BnBwd(_rows(b['raw']), _rows(b['gy']), b['gamma'], b['mean'], b['invstd'],
                                     mask=(2 if pooled else 1) if b['relu'] else 0, y=None if pooled else _rows(b['ymask']),
                                     scale=b['scale'], shift=b['shift'], dz_ops=3 if pooled else 0)
        return self.bn[name]

    def _stats(self, raw, eps):
        """op_bounds.finalize on exact partial rows, plus the fp32 error of the rows themselves"""
        y = _rows(raw).double()
        M, K = y.shape
        part = torch.stack([torch.stack([c.sum(0), (c * c).sum(0)]) for c in y.split(128)])
        one, zero = torch.ones(K), torch.zeros(K)
        w = ob.finalize(part, M, eps, 0.1, one, zero, zero, one)
        g = cb.gamma(128 + 2)
        eS1, eS2 = g * y.abs().sum(0), g * (y * y).sum(0)
        mean, e_mean = w['mean']
        var, e_var = w['var']
        e_mean = e_mean + eS1 / M
        e_var = e_var + eS2 / M + 2 * mean.abs() * eS1 / M
        invstd = w['invstd'][0]
        return {'mean': (mean, e_mean), 'invstd': (invstd, (2 * U + e_var / (2 * (var + ob.f32(eps)))) * invstd)}

    def __call__(self, q, name, kernel, got, ref64, **kw):
        self.checked[q] = self.checked.get(q, 0) + 1
        tag = '%s %s' % (q, name)
        try:
            r = self._one(q, name, tag, got, ref64, kw)
        except AssertionError as ex:
            self.bad.append(str(ex))
            return
        assert r is not None, 'no per-element bound for %s' % tag
        for x in (r if isinstance(r, (list, tuple)) else (r,)):
            if x.nbad:
                self.bad.append(x.msg)

    def _exact(self, tag, got, want):
        ob.exact(tag, got, cb.rne(want.double(), 'f32'))
        return ()

    def _one(self, q, name, tag, got, ref64, kw):
        eng = self.eng
        if q == 'raw':
            return cb.check(tag, _nhwc(got), *cb.fwd(kw['x'], kw['w'], kw['stride'], kw['pad']), out='f32', raise_=False)
        if q in ('mean', 'invstd'):
            want, e = self._stats(kw['raw'], kw['eps'])[q]
            return ob.elem(tag, got, want, e, 'f32', dims=('channel',), raise_=False)
        if q == 'y':
            want, e = ob.affine(_nhwc(kw['raw']), kw['scale'], kw['shift'], None if kw['res'] is None else _nhwc(kw['res']), kw['relu'])
            return ob.elem(tag, _nhwc(got), want, e, 'f32', raise_=False)
        if q == 'pool' and kw.get('fused') is not None:
            f = kw['fused']
            want, e = ob.affine(_nhwc(f['raw']), f['scale'], f['shift'], None, f['relu'])
            pool = lambda t: torch.nn.functional.max_pool2d(t.permute(0, 3, 1, 2), *kw['geo'])
            return ob.elem(tag, got, pool(want), pool(e), 'f32', raise_=False)          # |max a - max b| <= max |a - b|
        if q == 'pool':
            assert kw.get('exact'), 'only the exact pools are covered'
            return self._exact(tag, got, ref64)
        if q in ('dgamma', 'dbeta'):
            bb = self._bnbwd(name, kw)
            assert bb.amb_frac <= ob.AMBIGUOUS_MAX, '%s: %.2e of the elements have an ambiguous ReLU mask' % (tag, bb.amb_frac)
            terms, mags = (bb.dz, bb.m1) if q == 'dbeta' else (bb.dz * bb.xhat, bb.m2)
            return ob.sums(tag, got, terms, mags, n=bb.tile, ops=3 + bb.dz_ops, raise_=False)
        if q == 'dW':
            bb = self._bnbwd(name, kw['bn'])
            x, w, stride, pad = kw['x'], kw['w'], kw['stride'], kw['pad']
            N, K, P, Q = kw['d_raw64'].shape
            d, e_d = bb.dx(bb.dz)
            if bool(bb.amb.any()):                                               # either side of an ambiguous mask
                e_d = e_d + (bb.dx(torch.where(bb.amb, bb.dy - bb.dz, bb.dz))[0] - d).abs()
            back = lambda t: t.reshape(N, P, Q, K).permute(0, 3, 1, 2)
            d, e_d = back(d), back(e_d)
            ref, A, n = cb.wgrad(x, d, w.shape, stride, pad)
            extra = torch.nn.grad.conv2d_weight(x.double().abs(), w.shape, e_d, stride, pad).permute(0, 2, 3, 1)
            e = 2.0 * cb.gamma(n + 1) * (A + extra) + extra
            out = [cb.check_e(tag, _nhwc(got), ref, e, 'fp32', dims=('k', 'r', 's', 'c'), raise_=False)]
            if kw['xbuf'] is not None:
                gr, gA, gn = cb.dgrad(d, w, x.shape, stride, pad)
                gx = torch.nn.grad.conv2d_input(x.shape, w.double().abs(), e_d, stride, pad).permute(0, 2, 3, 1)
                self.writers.setdefault(kw['xbuf'], []).append((gr, 2.0 * cb.gamma(gn + 1) * (gA + gx) + gx, False))
            if kw['resbuf'] is not None:
                self.writers.setdefault(kw['resbuf'], []).append((bb.dz.reshape(N, P, Q, K), torch.zeros(N, P, Q, K, dtype=torch.float64), True))
            return out
        if q in ('logits', 'head dW', 'head db'):
            dl = kw.get('dl')
            if q == 'head db':
                ref, A, n = ob.fc_bgrad(dl)
                return ob.elem(tag, got, ref, cb.gamma(n) * A, 'f32', raise_=False)
            x = kw['x']
            N, Cc, H, W_ = x.shape
            feat, fA, fn = ob.gap(_nhwc(x).reshape(N, H * W_, Cc), None, 1.0)
            e_f = cb.gamma(fn) * fA
            Wt = kw['W'].double()
            if q == 'logits':
                ref, A, n = ob.fc_fwd(feat, kw['W'], kw['b'])
                e_in = e_f @ Wt.abs().t()
                return ob.elem(tag, got, ref, cb.gamma(n) * (A + e_in) + e_in, 'f32', raise_=False)
            ref, A, n = ob.fc_wgrad(dl, feat)
            e_in = dl.double().abs().t() @ e_f
            hr, hA, hn = ob.head_dx(dl, kw['W'], None, 1.0, H * W_, Cc)
            full = lambda t: t[:, None, None, :].expand(N, H, W_, Cc)
            self.writers.setdefault(kw['xbuf'], []).append((full(hr), full(cb.gamma(hn) * hA), False))
            return ob.elem(tag, got, ref, cb.gamma(n) * (A + e_in) + e_in, 'f32', raise_=False)
        if q == 'dx':
            ws = self.writers.pop(name)
            if len(ws) == 1 and ws[0][2]:
                return self._exact(tag, _nhwc(got), ws[0][0])                     # a first-writer copy
            want = sum(w[0] for w in ws)
            mag = sum(w[0].abs() + w[1] for w in ws)
            e = sum(w[1] for w in ws) + (len(ws) - 1) * U * mag                   # one rounding per accumulating writer
            return ob.elem(tag, _nhwc(got), want, e, 'f32', dims=('n', 'h', 'w', 'c'), raise_=False)
        if q == 'dlogits':
            want, e = ob.xent(kw['logits'], kw['target'], kw['weight'])['dlogits']
            return ob.elem(tag, got, want, e, 'f32', raise_=False)
        if q == 'update':
            if eng.optimizer == 'sgd':
                w = ob.sgd(kw['p'], kw['g'], kw['m'] if eng.momentum else None, eng.lr, eng.momentum, eng.weight_decay, 1.0)['p']
            else:
                w = ob.adam(kw['p'], kw['g'], kw['m'], kw['v'], eng.lr, eng.betas[0], eng.betas[1], eng.eps, eng.weight_decay,
                            kw['step'] + 1, 1.0)['p']
            return ob.elem(tag, kw['p_new'], w[0], w[1], 'f32', raise_=False)
        return None


_WALKS = {}


def _walk(B):
    """one fused step and its walk, shared by the two tests of a batch size -> (rows, chain lengths, Bounds); the engine is dropped"""
    if B in _WALKS:
        return _WALKS[B]
    from ifcb_classifier_amd.neuston_models import get_namebrand_model
    from oracle import ops as O
    seed, nc, S = 0, 2, 224
    torch.manual_seed(seed)
    hip = get_namebrand_model('resnet18', nc, max_batch=B, dtype='fp32', optimizer='sgd', lr=0.005, momentum=0.9)
    eng = hip.engine
    g = torch.Generator().manual_seed(100 + seed)
    x = torch.rand(B, 3, S, S, generator=g)
    y = torch.randint(0, nc, (B,), generator=g)
    chains, bounds = {}, Bounds(eng)

    def hook(q, name, kernel, got, ref64, **kw):
        chains[(q, name)] = _chain(eng, q, kw)
        bounds(q, name, kernel, got, ref64, **kw)

    before = O.STORAGE
    O.set_storage('fp32')
    try:
        hip.train()
        snap = LP.Snapshot(hip, target=y, hook=hook)
        N = eng.load_input_nchw(x.cuda())
        eng.target[:N].copy_(y.cuda())
        eng.train_step(N)
        torch.cuda.synchronize()
        LP.check_plan(hip, N, fp64=snap)
    finally:
        O.set_storage(before)
    bounds.eng = None
    bounds.bn.clear()
    snap.hook = None
    _WALKS[B] = (snap.rows, chains, bounds)
    return _WALKS[B]


KINDS = {'raw', 'mean', 'invstd', 'y', 'dgamma', 'dbeta', 'dW', 'pool', 'logits', 'head dW', 'head db', 'dlogits', 'dx', 'update'}


@pytest.mark.parametrize('B', [8, 16])
def test_every_node_of_the_fused_step_meets_its_fp64_bound(B):
    rows, chains, bounds = _walk(B)
    assert set(bounds.checked) == KINDS and sum(bounds.checked.values()) == len(rows)       # every row went through a bound
    assert not bounds.writers, 'gradient writers without a buffer row: %s' % sorted(bounds.writers)
    assert not bounds.bad, '\n'.join(bounds.bad)


@pytest.mark.parametrize('B', [8, 16])
def test_every_node_of_the_fused_step_is_as_close_to_fp64_as_the_reference(B):
    import conftest
    rows, chains, bounds = _walk(B)
    assert len(rows) > 200 and {r[2] for r in rows} == KINDS
    worst, over = {}, []
    for name, kernel, q, e_h, e_o in rows:
        F = F_of(chains[(q, name)])
        ratio = e_h / max(e_o, FLOOR)
        if ratio > worst.get(q, (0.0,))[0]:
            worst[q] = (ratio, name, kernel, F)
        if not e_h <= F * e_o + FLOOR:
            over.append('%s %s [%s]: e_hip %.3e > %.2f x e_ora %.3e + 2^-24' % (q, name, kernel, e_h, F, e_o))
    ln = 'node walk fp64, resnet18 fp32 batch %d: worst e_hip / e_ora per kind: %s' % (
        B, '; '.join('%s %.2f (%s, F %.1f)' % (q, w[0], w[1], w[3]) for q, w in worst.items()))
    print(ln)
    conftest.MEASURED.append(ln)
    assert not over, '\n'.join(over)
