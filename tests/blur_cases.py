"""TRAIN --blur: the float64 twin, the case table and the bound the tests hold ifcbk_batch_blur to.  Helpers only.

Twin (`twin`): the weights w[j] = exp(-0.5 ((j - r) / sigma)^2) / sum and torch's 'reflect' index map in float64, from the float32
sigma the kernel is handed, then the 2-D sum with w (x) w.  tests/test_blur_cpu.py holds it to F.pad(mode='reflect') + conv2d in float64.

What the kernel does (csrc/batch_blur.hip), with u = 2^-24 and gamma(n) = n u / (1 - n u):
  * e[j] = expf(-0.5f * (q * q)), q = (j - r) / sigma in fp32: the division and the square round (the product with 0.5 is exact), so
    the argument t has a relative error of at most gamma(3) and exp(t) one of gamma(3) |t|; expf is good to 1 ulp = 2 u:
        d[j] = gamma(3) |t[j]| + 2 u      (relative, per unnormalised weight)
    An e[j] below the fp32 normal range may be flushed: an absolute 2^-126, k times, against a sum >= 1 -- carried as K_FLUSH.
  * the sum s of the e[j] in ascending j: k - 1 roundings, all terms positive: relative error at most sum_j w[j] d[j] + gamma(k - 1);
    the division w[j] = e[j] / s rounds once.  The l1 error of the weights is therefore at most
        W0 = 2 sum_j w[j] d[j] + gamma(k - 1) + u + K_FLUSH,        W = W0 / (1 - W0)  (second order)
  * one pass is a chain acc = fmaf(w[j], v[j], acc) from 0 in ascending j: the term j goes through k - j roundings, so with |v| <= M
        |pass - sum_j w[j] v[j]|  <=  M (W + C + W gamma(k)),        C = sum_j w[j] gamma(k - j)
    (W for the weights, C for the chain under the exact weights, W gamma(k) for the chain under their error).
  * the second pass takes inputs that are off by the first pass's E1 and are at most M + E1 in size:
        E1 = M (W + C + W gamma(k)),        E2 = E1 (1 + W) + (M + E1) (W + C + W gamma(k))
  `fp32_bound(sigma, r, M)` = E2, with M the largest magnitude of the plane.  The chain's last fmaf already rounds to fp32, so the fp32
  form adds nothing; bf16 (8 significand bits: unit roundoff 2^-8) adds half an ulp of the stored value, at most 2^-8 (|twin| + E2); the u8 form stores rint of the fp32 value:
  the byte equals rint(twin) unless twin lies within E2 of a half (`near_tie`), where it may be either neighbour.
Every constant above comes from counting roundings; none is read off the kernel's results.

The u8 cap: near-tie pixels may be at most 0.1 % of any test image (`TIE_CAP`).  E2 grows with M and with k, so the random u8 images of
a case are drawn from 0..amp-1 with `amp` small enough for the case's radius (a blurred random image spreads its fractions evenly:
the share is about 2 E2); tests/test_blur_cpu.py asserts the cap on the twin alone, for every image of every case."""
import functools
import math

import numpy as np

U = 2.0 ** -24
K_FLUSH = 25 * 2.0 ** -126
TIE_CAP = 1e-3
SIGMA_MIN = 0.1


def gamma(n):
    return n * U / (1.0 - n * U)


def weights64(sigma, r):
    """the 2 r + 1 normalised weights in float64 from the float32 value of sigma, and t[j] = -0.5 ((j - r) / sigma)^2"""
    s = float(np.float32(sigma))
    with np.errstate(over='ignore', under='ignore'):
        t = -0.5 * (np.arange(-r, r + 1, dtype=np.float64) / s) ** 2
        e = np.exp(t)
    return e / e.sum(), t


def reflect_map(S, r):
    """the source index of padded position p = 0 .. S + 2 r - 1 under torch's 'reflect' (-1 -> 1, S -> S - 2); needs r < S"""
    assert 0 < r < S
    i = np.abs(np.arange(-r, S + r))
    return np.where(i >= S, 2 * (S - 1) - i, i)


def twin(img, sigma, r):
    """float64 [S, S] -> its 2-D convolution with w (x) w under the reflected border; a sigma that is not > 0 (or not finite) returns
    the image itself"""
    img = np.asarray(img, np.float64)
    s = float(np.float32(sigma))
    if not (s > 0 and math.isfinite(s)):
        return img.copy()
    S = img.shape[0]
    assert img.shape == (S, S)
    w, _ = weights64(s, r)
    idx = reflect_map(S, r)
    h = np.zeros_like(img)
    for j in range(2 * r + 1):
        h += w[j] * img[:, idx[j:j + S]]
    out = np.zeros_like(img)
    for j in range(2 * r + 1):
        out += w[j] * h[idx[j:j + S], :]
    return out


def pass_coef(sigma, r):
    """W + C + W gamma(k) of the module docstring, and W"""
    k = 2 * r + 1
    w, t = weights64(sigma, r)
    with np.errstate(invalid='ignore', over='ignore'):
        d = np.where(w > 0, gamma(3) * np.abs(t), 0.0) + 2 * U      # (a weight that is exactly 0 in float64 carries no relative term)
    W0 = 2.0 * float((w * d).sum()) + gamma(k - 1) + U + K_FLUSH
    W = W0 / (1.0 - W0)
    C = float((w * np.array([gamma(k - j) for j in range(k)])).sum())
    return W + C + W * gamma(k), W


def fp32_bound(sigma, r, M):
    """E2: |kernel's fp32 value - twin| may be at most this on a plane whose magnitudes are at most M"""
    s = float(np.float32(sigma))
    if not (s > 0 and math.isfinite(s)):
        return 0.0
    c, W = pass_coef(s, r)
    E1 = M * c
    return E1 * (1.0 + W) + (M + E1) * c


def stored_bound(form, sigma, r, M, ref):
    """per-element bound of the dense forms: `ref` = the twin's values"""
    b = fp32_bound(sigma, r, M)
    if b == 0.0:
        return np.zeros_like(ref)                                   # not drawn: the bits stay
    return b + (2.0 ** -8 * (np.abs(ref) + b) if form == 'bf16' else 0.0)


def near_tie(ref, bound):
    """pixels of the twin within `bound` of a half: the u8 result may be either neighbour there"""
    return np.abs(ref - np.floor(ref) - 0.5) <= bound


def u8_verdict(got, ref, bound):
    """got: the kernel's bytes, ref: the twin -> (wrong, share): `wrong` marks bytes that are not rint(ref) off the near-ties and not one
    of the two neighbours on them; share = near-tie pixels / pixels"""
    got = np.asarray(got, np.float64)
    tie = near_tie(ref, bound)
    want = np.clip(np.rint(ref), 0, 255)
    wrong = np.where(tie, np.abs(got - ref) > 0.5 + bound, got != want)
    return wrong, float(tie.mean())


# ---- the case table.  (name, S, r, sigmas of the N images, amp of the random u8 images)
# sigma runs over the run's whole range [0.1, r / 3] (r = ceil(3 SIGMA_MAX)); 0 = not drawn.
def _amp(r):
    """the largest power of two <= 256 for which 2 E2 at sigma = r / 3 and M = amp - 1 stays under TIE_CAP with a margin of 2"""
    a = 256
    while a > 2 and 2.0 * fp32_bound(r / 3.0, r, a - 1) > TIE_CAP / 2.0:
        a //= 2
    return a


CASES = [
    # S = r + 1: every tap but the centre's is reflected, and the reflection reaches the far edge
    ('S=r+1 r=1', 2, 1, (0.1, 1.0 / 3.0), _amp(1)),
    ('S=r+1 r=12', 13, 12, (4.0, 0.0, 2.7183), _amp(12)),
    # S = 2 r + 1: the ring holds the whole image
    ('S=2r+1 r=1', 3, 1, (0.25, 0.3333), _amp(1)),
    ('S=2r+1 r=12', 25, 12, (3.9, 0.1, 1.4142), _amp(12)),
    # odd S: the u8 images start at odd byte addresses; a batch mixing sigma = 0 and sigma > 0; a band that ends short (33 = 8 * 4 + 1)
    ('S=33 r=6', 33, 6, (0.0, 2.0, 0.0, 0.7071, 1.5), _amp(6)),
    ('S=33 r=1 full range', 33, 1, (0.3, 0.1731), 256),
    # N = 1
    ('N=1 S=33 r=3', 33, 3, (0.9,), _amp(3)),
    # the training shape: more rows than the ring, more than one band, unaligned images (299 * 299 is odd)
    ('S=299 r=12', 299, 12, (4.0, 0.0, 1.7321), _amp(12)),
    ('S=299 r=6', 299, 6, (2.0, 0.1, 1.0), _amp(6)),
    # high magnitudes at the longest chain: a bright patch (levels 200..255, 255 among them) on a dark field.  At M = 255 and r = 12 the
    # bound is wide enough for about 0.27 % of RANDOM pixels to be near-ties, so the patch is kept small: the flat field around it blurs
    # to exact zeros, which are no ties, and the share over the whole image stays under the cap
    ('S=97 r=12 bright patch', 97, 12, (4.0, 2.0), 256),
]
PATCH = 20                                                         # side of the bright patch of the 'bright patch' case
CASE_IDS = [c[0] for c in CASES]
# an image of 33 x 33 pixels may hold ONE near-tie under the cap: these cases take the first seed whose twin has at most that
SEED_SALT = {'S=33 r=6': 1, 'S=33 r=1 full range': 1}
FORMS = ('u8', 'bf16', 'f32')


@functools.lru_cache(maxsize=None)
def case_input(name, form):
    """the case's input, fixed seed: u8 -> uint8 [N, S, S] in 0..amp-1; dense -> float32 [N, S, S, 8] of normalised-image magnitudes
    (about -2.2 .. 2.7, what Normalize makes of a byte) in channels 0..2 and a NONZERO pattern in the pad channels, which must keep
    their bits.  bf16 inputs are returned already rounded to bf16 (as float32), so the twin sees what the kernel reads."""
    _, S, r, sigmas, amp = CASES[CASE_IDS.index(name)]
    N = len(sigmas)
    rng = np.random.default_rng([0x626c7572, CASE_IDS.index(name), SEED_SALT.get(name, 0)])
    if form == 'u8' and name.endswith('bright patch'):
        x = np.zeros((N, S, S), np.uint8)
        lo = (S - PATCH) // 2
        x[:, lo:lo + PATCH, lo:lo + PATCH] = rng.integers(200, 256, (N, PATCH, PATCH))
        x[:, lo + 3:lo + 6, lo + 3:lo + 6] = 255
    elif form == 'u8':
        x = rng.integers(0, amp, (N, S, S)).astype(np.uint8)
    else:
        x = rng.uniform(-2.2, 2.7, (N, S, S, 8)).astype(np.float32)
        if form == 'bf16':
            x = (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)      # (truncated: exactly representable in bf16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def case_twin(name, form):
    """-> (ref, bound): float64 arrays shaped like the input; for u8 the bound is E2 per image, for the dense forms `stored_bound` per
    element (0 in the pad channels and in the images that are not drawn: their bits stay)"""
    _, S, r, sigmas, _ = CASES[CASE_IDS.index(name)]
    x = case_input(name, form)
    ref = x.astype(np.float64)
    bound = np.zeros_like(ref)
    for n, s in enumerate(sigmas):
        if form == 'u8':
            ref[n] = twin(x[n], s, r)
            bound[n] = fp32_bound(s, r, float(x[n].max()))
        else:
            for c in range(3):
                ref[n, :, :, c] = twin(x[n, :, :, c], s, r)
                bound[n, :, :, c] = stored_bound(form, s, r, float(np.abs(x[n, :, :, c]).max()), ref[n, :, :, c])
    ref.setflags(write=False)
    bound.setflags(write=False)
    return ref, bound
