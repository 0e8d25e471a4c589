"""Per-element error bounds for the convolution kernels, against a float64 reference of the same operation.

A plain helper module imported by the tests (like local_parity.py).  Everything here runs on the CPU in float64.

The reference is computed from the operands the kernel read (bf16- or fp32-representable values), so it carries no error of its own
that matters: every product of two bf16 or fp32 values and every sum below is exact to about 2^-53.

Bound of one output element y whose exact value is y64 = sum of n products p_i, with A64 = sum |p_i| (the same convolution of the
absolute values) and u = 2^-24 (fp32 unit roundoff):

    |y - y64| <= 1/2 ulp_out(|y64| + e) + e,        e = 2 * gamma_n * A64,        gamma_n = n u / (1 - n u)

* gamma_n * A64 bounds a fp32 sum of n terms in ANY order, split-K partial sums and their combine included: a summation tree of n
  leaves is at most n - 1 adds deep, and one more rounding covers the products of fp32 operands (bf16 x bf16 products are exact
  in fp32).  The factor 2 is a margin: the guides of this project document the fp32 MFMA as an fma chain, but not how the bf16
  MFMA orders its internal additions.
* n is the reduction length of that element: R*S*Cw for the forward, the taps that actually hit times K for the input gradient,
  N*P*Q for the weight gradient.
* 1/2 ulp_out is the final rounding to the output type, taken at |y64| + e so that a result just across a binade edge is covered.
* Accumulating forms (dx += ..., dw += ...): the reference is old + y64, the old value joins the sum as one more term.  The kernels'
  shared epilogue (conv_common.h) rounds the fresh contribution to the storage type before it adds the old value (the C tile is
  staged in LDS in that type): one rounding for each operation, so a bf16 accumulate also allows 1/2 ulp_bf16 of the contribution.
* Eval affine epilogue act(scale * acc + shift [+ res]): the conv result is rounded to the storage type first (the same staging),
  then the multiply-add and the residual add are one fp32 rounding each, the ReLU is 1-Lipschitz, the store rounds once more.
  In fp32 storage (check_affine(out='f32')) the same terms hold with 1/2 ulp_f32 for the staged conv value and for the store (the
  staging does not round an fp32 accumulator; the term stays as a margin) and there is no mismatch fraction, as in check().

Bf16 outputs also get a sensitivity check, which the worst-case bound is too loose to replace: the fraction of elements where
y != rne_bf16(y64) must be at most 1 %.  One fp32 accumulation rounded once lands near 1e-3; a bf16-rounded partial sum pushes it to
tens of percent.  Where the epilogue rounds an intermediate by design (accumulate, affine), either rounding model is accepted
(the single rounding of the exact value, or the designed rounding of the rounded conv value).

The u8 stem (conv_stem_u8.hip) has bounds of its own, counted from its source: see stem_u8_fwd / stem_u8_wgrad below.

Detection limit: 2 * gamma_n * A64 grows like n^1.5 for unit-variance operands, one term like n^-0.5 (filters scaled by
1/sqrt(fan-in)) or like 1 (weight gradients).  A single dropped term stays visible for forward / input-gradient reductions up to
several thousand terms and for weight gradients up to N*P*Q of about 2000; test_conv_bounds_cpu.py shows where.
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
MISMATCH_MAX = 0.01


def gamma(n):
    nu = n * U
    return nu / (1.0 - nu)


def _ulp(a, mant_bits, min_exp):
    e = torch.floor(torch.log2(a.double().abs().clamp_min(2.0 ** min_exp)))
    return torch.exp2(e - mant_bits)


def ulp_bf16(a):
    return _ulp(a, 7, -126)


def ulp_f32(a):
    return _ulp(a, 23, -126)


def ulp(a, out):
    return ulp_bf16(a) if out == 'bf16' else ulp_f32(a)


def rne(t, out):
    """round a float64 tensor to the output type (round to nearest even), back to float64"""
    return t.to(torch.bfloat16 if out == 'bf16' else torch.float32).double()


# ------------------------------------------------------------------------------------------------------ float64 references
# x NCHW, w KCRS, dy NKPQ (any float dtype holding the kernel's operand values).  Results are in the kernels' layouts:
# forward [N][P][Q][K], input gradient [N][H][W][C], weight gradient [K][R][S][C].  Each returns (ref, A, n).

def fwd(x, w, stride=1, pad=0):
    x, w = x.double(), w.double()
    y = F.conv2d(x, w, None, stride, pad).permute(0, 2, 3, 1)
    a = F.conv2d(x.abs(), w.abs(), None, stride, pad).permute(0, 2, 3, 1)
    K, Cw, R, S = w.shape
    return y, a, R * S * Cw


def dgrad(dy, w, xshape, stride=1, pad=0):
    dy, w = dy.double(), w.double()
    g = torch.nn.grad.conv2d_input(xshape, w, dy, stride, pad).permute(0, 2, 3, 1)
    a = torch.nn.grad.conv2d_input(xshape, w.abs(), dy.abs(), stride, pad).permute(0, 2, 3, 1)
    N, C, H, W = xshape
    K, _, R, S = w.shape
    taps = torch.nn.grad.conv2d_input((N, 1, H, W), torch.ones(1, 1, R, S, dtype=torch.float64),
                                      torch.ones(N, 1, dy.shape[2], dy.shape[3], dtype=torch.float64), stride, pad)
    return g, a, (taps.permute(0, 2, 3, 1) * K).round()


def wgrad(x, dy, wshape, stride=1, pad=0):
    x, dy = x.double(), dy.double()
    g = torch.nn.grad.conv2d_weight(x, wshape, dy, stride, pad).permute(0, 2, 3, 1)
    a = torch.nn.grad.conv2d_weight(x.abs(), wshape, dy.abs(), stride, pad).permute(0, 2, 3, 1)
    return g, a, dy.shape[0] * dy.shape[2] * dy.shape[3]


# ------------------------------------------------------------------------------------------------------ reporting
_FAMILY = {}          # family -> [worst ratio, worst mismatch fraction, checks, index into conftest.MEASURED]


def _record(family, ratio, frac, prefix='conv bound'):
    """prefix: how the family's line in the measured section starts (tests/op_bounds.py records under 'op bound')"""
    try:
        import conftest
    except ImportError:         # (imported outside pytest)
        return
    row = _FAMILY.get((prefix, family))
    if row is None:
        row = _FAMILY[(prefix, family)] = [0.0, None, 0, len(conftest.MEASURED)]
        conftest.MEASURED.append('')
    row[0] = max(row[0], ratio)
    if frac is not None:
        row[1] = frac if row[1] is None else max(row[1], frac)
    row[2] += 1
    conftest.MEASURED[row[3]] = '%s %-44s worst err/bound %.3f  bf16 mismatch %s  (%d checks)' % (
        prefix, family, row[0], '-' if row[1] is None else '%.2e' % row[1], row[2])


class Result:
    def __init__(self, ratio, frac, nbad, msg):
        self.ratio, self.frac, self.nbad, self.msg = ratio, frac, nbad, msg

    def __repr__(self):
        return self.msg


def _finish(name, family, got, want, err, bound, frac, dims, raise_=True, prefix='conv bound'):
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    r = err / bound
    bad = ~(err <= bound)
    nbad = int(bad.sum())
    i = int(torch.argmax(r.flatten()))
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), got.shape))
    ratio = float(r.flatten()[i])
    msg = '%s: %d of %d elements over the bound; worst at %s = %s: got %.8g want %.8g bound %.3g (err/bound %.3g)' % (
        name, nbad, got.numel(), '(%s)' % ', '.join(dims), idx, float(got[idx]), float(want[idx]), float(bound[idx]), ratio)
    if frac is not None:
        msg += '; bf16 mismatch fraction %.3e (limit %.0e)' % (frac, MISMATCH_MAX)
    res = Result(ratio, frac, nbad, msg)
    if family is not None:
        _record(family, ratio, frac, prefix)
    if raise_:
        assert nbad == 0 and (frac is None or frac <= MISMATCH_MAX), msg
    return res


def check(name, got, ref, A, n, out='bf16', old=None, dims=('n', 'p', 'q', 'k'), family=None, raise_=True):
    """got: the kernel's output (any dtype, the reference's layout); ref, A, n: from fwd / dgrad / wgrad.  old: the destination's
    value before an accumulating call (then the reference is old + ref)."""
    got = got.detach().double().cpu()
    ref, A = ref.double(), A.double()
    n = torch.as_tensor(n, dtype=torch.float64)
    e = 2.0 * gamma(n + 1) * A
    if old is None:
        want = ref
        bound = 0.5 * ulp(want.abs() + e, out) + e
        frac = float((got != rne(want, out)).double().mean()) if out == 'bf16' else None
    else:
        old = old.detach().double().cpu()
        want = old + ref
        e = 2.0 * gamma(n + 1) * (A + old.abs())
        inter = 0.5 * ulp(ref.abs() + e, out) if out == 'bf16' else 0.0      # the contribution rounded before the add
        bound = 0.5 * ulp(want.abs() + e + inter, out) + e + inter
        frac = float(((got != rne(want, out)) & (got != rne(old + rne(ref, out), out))).double().mean()) if out == 'bf16' else None
    return _finish(name, family, got, want, (got - want).abs(), bound, frac, dims, raise_)


def check_e(name, got, want, e, out='bf16', alts=(), dims=('n', 'p', 'q', 'k'), family=None, raise_=True):
    """|got - want| <= 1/2 ulp_out(|want| + e) + e per element, for an e counted elsewhere (the u8 stem); bf16: the fraction of
    elements that differ from rne(want) (or from a designed rounding model in alts) is held to MISMATCH_MAX like check()"""
    got, want = got.detach().double().cpu(), want.double()
    e = torch.as_tensor(e, dtype=torch.float64).expand_as(want)
    bound = 0.5 * ulp(want.abs() + e, out) + e + 1e-300
    frac = None
    if out == 'bf16':
        match = got == rne(want, out)
        for a in alts:
            match = match | (got == rne(a.double(), out))
        frac = float((~match).double().mean())
    return _finish(name, family, got, want, (got - want).abs(), bound, frac, dims, raise_)


def check_affine(name, got, ref, A, n, scale, shift, res=None, relu=False, dims=('n', 'p', 'q', 'k'), family=None, raise_=True,
                 out='bf16'):
    """y = act(scale[k] * conv + shift[k] (+ res)) stored as `out` ('bf16' | 'f32'), scale / shift fp32 per output channel (last axis),
    res the residual in the storage type"""
    got = got.detach().double().cpu()
    ref, A = ref.double(), A.double()
    s, b = scale.detach().double().cpu(), shift.detach().double().cpu()
    r = torch.zeros(()) if res is None else res.detach().double().cpu()
    e = 2.0 * gamma(torch.as_tensor(n, dtype=torch.float64) + 1) * A
    e_raw = e + 0.5 * ulp(ref.abs() + e, out)                         # the conv value as staged in the storage type
    lin = s * ref + b + r
    mag = s.abs() * (ref.abs() + e_raw) + b.abs() + r.abs()
    e_lin = s.abs() * e_raw + 2.0 * U * mag                           # multiply-add and residual add: one rounding each
    act = (lambda t: t.clamp_min(0)) if relu else (lambda t: t)
    want = act(lin)
    bound = 0.5 * ulp(want.abs() + e_lin, out) + e_lin
    frac = None
    if out == 'bf16':
        alt = act(s * rne(ref, 'bf16') + b + r)
        frac = float(((got != rne(want, 'bf16')) & (got != rne(alt, 'bf16'))).double().mean())
    return _finish(name, family, got, want, (got - want).abs(), bound, frac, dims, raise_)


def check_sums(name, got, terms, mags=None, ops=2, family=None, raise_=True, n=None, prefix='conv bound'):
    """per-channel sums (the BatchNorm partial rows of an epilogue, summed over rows in float64) against float64 sums of the terms
    [rows, channels] built from the kernel's own rounded outputs; bound gamma_(M + ops) * sum |term| (ops: roundings inside one term).
    mags: magnitudes of the terms' operands when a term's own roundings act on larger values than the term (default |terms|).
    n: the longest fp32 summation chain when it is shorter than the number of rows (fp32 row tiles combined in double)"""
    got = got.detach().double().cpu()
    terms = terms.double()
    want = terms.sum(0)
    M = terms.shape[0] if n is None else n
    mags = terms.abs() if mags is None else mags.double()
    bound = gamma(M + ops) * mags.sum(0) + 1e-30
    return _finish(name, family, got, want, (got - want).abs(), bound, None, ('channel',), raise_, prefix)


def check_bn_fwd_sums(name, part, yh, family=None):
    """forward statistics: part [rows][2][K] fp32, yh [..., K] the kernel's rounded outputs"""
    y = yh.detach().double().cpu().reshape(-1, yh.shape[-1])
    p = part.detach().double().cpu().sum(0)
    check_sums(name + ' sum', p[0], y, family=family)
    check_sums(name + ' sumsq', p[1], y * y, family=family)


def check_bn_bwd_sums(name, part, dx, raw, mean, invstd, bsc, bsh, family=None):
    """MODE 3 sums of one producer: sum dz, sum dz * (raw - mean) * invstd with dz = dx where raw * bsc + bsh > 0.  dx: the kernel's
    rounded input gradient; the activation test is evaluated in fp32 by the kernel: elements whose pre-activation is within a few
    fp32 roundings of 0 may fall on either side, and their terms join the bound"""
    C_ = dx.shape[-1]
    d = dx.detach().double().cpu().reshape(-1, C_)
    rw = raw.detach().double().cpu().reshape(-1, C_)
    mu, ist, sc, sh = (t.detach().double().cpu() for t in (mean, invstd, bsc, bsh))
    pre = rw * sc + sh
    amb = pre.abs() <= 4 * U * ((rw * sc).abs() + sh.abs())
    dz = torch.where(pre > 0, d, torch.zeros(()))
    xh = (rw - mu) * ist
    p = part.detach().double().cpu().sum(0)
    m1 = dz.abs() + amb * d.abs() / (gamma(dz.shape[0] + 3))
    m2 = dz.abs() * (rw.abs() + mu.abs()) * ist + amb * (d * xh).abs() / (gamma(dz.shape[0] + 3))
    check_sums(name + ' sum dz', p[0], dz, m1, ops=3, family=family)
    check_sums(name + ' sum dz*xhat', p[1], dz * xh, m2, ops=3, family=family)


# ------------------------------------------------------------------------------------------------------ the u8 stem
# conv_stem_u8.hip: y[k] = sum_t g_t We[k,t] + B[k],  We[k,t] = sum_c a_c w[k,t,c],  B[k] = sum_{t,c} b_c w[k,t,c]  (g: u8 pixels, exact;
# w: the fp32 master filter [K][R][S][C]; a_c, b_c: the fp32 input affine).  Counted from the source, u = 2^-24:
#   taps and bias in fp32 (both kernels):  We = w0 a0 + w1 a1 + w2 a2: at most 3 roundings on a term (3 fmas / 3 products and 2 adds);
#       B: the same expression per tap, then 9 adds `b += ...`: at most 3 + 9 = 12.  Relative to the sums of MAGNITUDES, because both
#       cancel in fp32:   e_w = gamma_3 T + gamma_12 Bb,   T = sum_t g_t sum_c |a_c w|,   Bb = sum_{t,c} |b_c w|.
#   the accumulation acts on the computed taps and bias:  mag = G + |B| + e_w,   G = sum_t g_t |We|.
#   stem_u8_fwd_kernel (fp32 storage, or Q < 32):  v = bias; 9 x v = fmaf(g_t, we_t, v): gamma_9 mag.
#   stem_u8_fwd_mfma_kernel (bf16, Q >= 32):  split3 writes a tap as hi + mid + lo, three bf16 values rounded to nearest (unit roundoff
#       2^-8), the two remainders exact in fp32: |w - hi| <= 2^-8 |w|, |r1 - mid| <= 2^-16 |w|, |r2 - lo| <= 2^-24 |w|: the pieces
#       represent the tap to u |w| (two pieces: 2^-16 |w|, which this bound must reject -- test_conv_bounds_cpu.py).  Then 27 + 3 exact
#       bf16 x bf16 products in two chained MFMAs of 16 slots: 32 terms in an order the guides do not document, so gamma_33 in any
#       order with the factor 2 of check(); the pieces' magnitudes add up to at most (1 + 2^-7) |w|:
#           e = e_w + u mag + 2 gamma_33 (1 + 2^-7) mag.
#   eval epilogue (both): act(fmaf(v, scale, shift)) on the fp32 v: e_lin = |scale| e + u (|scale ref| + |scale| e + |shift|).
#   weight gradient dw[k,t,c] = a_c A[k,t] + b_c S[k],  A = sum dy g_t,  S = sum dy  (products exact: dy bf16 / fp32 times an integer
#       <= 255 inside an fma, or bf16 x bf16 in the MFMA).  fp32 chain of one block partial: stem_u8_wgrad_kernel 32 fmas per thread
#       (PIXB / 64 trips) + 4 shuffle adds + 2 adds across the waves = 38; stem_u8_wgrad_mfma_kernel: a wave runs 2 gpr MFMAs of 32
#       terms (RB gpr / 4 items, gpr = ceil(Q / 32)) + 2 adds: 64 gpr + 2 terms, any order, factor 2.  stem_u8_wgrad_reduce_kernel adds
#       the block partials and forms a_c A + b_c S in double (d = 2^-53 per operation) and rounds once to fp32:
#           e = c gamma_n mag + (blocks + 3) d mag,   mag = |a_c| sum |dy| g_t + |b_c| sum |dy|   (a_c g and b_c cancel inside x_c:
#           relative to |a| g + |b|, not to |x_c|), then the store (1/2 ulp_fp32); accumulating: the rounded value joins old in one add.
STEM_K, STEM_PIXB, STEM_RB = 32, 2048, 8


def stem_mfma(dtype, Q):
    """conv_stem_u8.hip: stem_mfma"""
    return dtype == 'bf16' and Q >= 32


def stem_rows(N, P, Q, dtype):
    """ifcbk_stem_u8_rows: the grid of both passes"""
    return (N * P + STEM_RB - 1) // STEM_RB if stem_mfma(dtype, Q) else (N * P * Q + STEM_PIXB - 1) // STEM_PIXB


def stem_u8_fwd(g, w, ab, mfma, pieces=3):
    """g [N][H][W] u8, w [K][3][3][3] fp32 master, ab the six fp32 affine values -> (ref, e), [N][P][Q][K] float64.
    pieces: bf16 pieces per tap in the MFMA kernel (3 in the source)"""
    g = g.detach().double().cpu()[:, None]
    w = w.detach().double().cpu()
    ab = ab.detach().double().cpu()
    wa, wb = w * ab[:3], w * ab[3:]
    we, B, Bb = wa.sum(-1), wb.sum((1, 2, 3)), wb.abs().sum((1, 2, 3))
    conv = lambda k: F.conv2d(g, k[:, None], None, 2).permute(0, 2, 3, 1)
    ref, G, T = conv(we) + B, conv(we.abs()), conv(wa.abs().sum(-1))
    e_w = gamma(3) * T + gamma(12) * Bb
    mag = G + B.abs() + e_w
    if mfma:
        e = e_w + 2.0 ** (-8 * pieces) * mag + 2.0 * gamma(33) * (1 + 2.0 ** -7) * mag
    else:
        e = e_w + gamma(9) * mag
    return ref, e


def stem_affine(ref, e, scale, shift, relu):
    """(want, e_lin) of act(fmaf(v, scale, shift))"""
    s, b = scale.detach().double().cpu(), shift.detach().double().cpu()
    lin = s * ref + b
    e_lin = s.abs() * e + U * ((s * ref).abs() + s.abs() * e + b.abs())
    return (lin.clamp_min(0) if relu else lin), e_lin


def stem_u8_wgrad(g, dy, ab, mfma):
    """g [N][H][W] u8, dy [N][P][Q][K] (the values the kernel read) -> (ref, e), [K][3][3][3] float64"""
    g = g.detach().double().cpu()[:, None]
    d = dy.detach().double().cpu().permute(0, 3, 1, 2).contiguous()
    ab = ab.detach().double().cpu()
    N, K, P, Q = d.shape
    A = torch.nn.grad.conv2d_weight(g, (K, 1, 3, 3), d, 2)[:, 0]                      # [K][3][3]
    Aa = torch.nn.grad.conv2d_weight(g, (K, 1, 3, 3), d.abs(), 2)[:, 0]
    S, Sa = d.sum((0, 2, 3)), d.abs().sum((0, 2, 3))
    ref = A[..., None] * ab[:3] + S[:, None, None, None] * ab[3:]
    mag = Aa[..., None] * ab[:3].abs() + Sa[:, None, None, None] * ab[3:].abs()
    gpr = (Q + 31) // 32
    c, n = (2.0, 64 * gpr + 2) if mfma else (1.0, STEM_PIXB // 64 + 6)
    blocks = (N * P + STEM_RB - 1) // STEM_RB if mfma else (N * P * Q + STEM_PIXB - 1) // STEM_PIXB
    e = c * gamma(n) * mag + (blocks + 3) * 2.0 ** -53 * mag
    return ref, e


def check_stem_wgrad(name, got, ref, e, old=None, family=None, raise_=True):
    """dw fp32 [K][3][3][3]; old: the destination before an accumulating call (the fresh value is rounded to fp32, then added)"""
    if old is None:
        return check_e(name, got, ref, e, 'fp32', dims=('k', 'r', 's', 'c'), family=family, raise_=raise_)
    old = old.detach().double().cpu()
    e2 = e + 0.5 * ulp_f32(ref.abs() + e)
    return check_e(name, got, old + ref, e2, 'fp32', dims=('k', 'r', 's', 'c'), family=family, raise_=raise_)


def family_of(kname, role):
    """'conv_pp2<3, 10, 4, 0>' -> 'conv_pp2 fwd' (mode suffix kept where the template's last argument is the epilogue mode)"""
    base = kname.split('<')[0]
    return '%s %s' % (base, role)


def kname(ctx, d, kind, flags=0, residual=False):
    """the kernel ifcbk_op_kernel names for one conv op of descriptor d"""
    import ctypes as C
    from ifcb_classifier_amd import _lib
    op = _lib.Op()
    op.kind = kind
    op.flags = flags
    op.u.conv = d
    if residual:
        op.p[5] = 1
    buf = C.create_string_buffer(128)
    ctx.lib.ifcbk_op_kernel(C.byref(op), buf, 128)
    return buf.value.decode()
