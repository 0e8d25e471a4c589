"""TRAIN --clip-grad: the reference and the bound the tests hold ifcbk_grad_norm and the clipped optimizer steps to.  Helpers only.

Reference: torch.nn.utils.clip_grad_norm_ on the CPU (`torch_clip`), on float64 copies where a norm is compared (torch's own fp32 sum
has an error of its own, which is not the kernel's), on the fp32 tensors where the clipped gradient feeds torch.optim.

What the kernel does (csrc/grad_clip.hip; include/ifcbk.h documents the geometry): B = (ifcbk_grad_clip_state_floats() - 4) / 2 blocks of
256 threads, one float4 per thread and pass, so one pass of the grid covers B * 1024 elements and thread t of block b owns the float4s
b * 256 + t + k * B * 256.  A thread squares each element in fp32 and adds it to one of four fp32 accumulators (one per float4
component), the first thread also adds the n % 4 tail elements to its first accumulator, the four are added as (a0 + a1) + (a2 + a3),
and everything behind that is float64: wave, block, partials, the sum of the partials, the square root, the product with grad_scale;
one rounding to fp32 gives the norm.

The bound, with u = 2^-24 and L = ceil((n // 4) / (B * 256)) the float4s of the busiest thread:
  * every g[i]^2 reaches the thread's sum through at most 1 rounding of the square (none when the compiler contracts a + g * g into a
    fused multiply-add), L additions of its accumulator's chain, 3 additions of the tail and 2 of the final tree: all terms are
    non-negative, so the thread's sum, and with it the whole sum S, has a relative error of at most (1 + u)^(L + 6) - 1 =
    (L + 6) u + O((L u)^2);
  * the float64 tree behind it (at most 6 + 2 + 16 + 6 additions, the square root and one product, 2^-53 each) adds less than 2^-47;
  * sqrt halves a relative error: (L + 6) u / 2; the rounding of the norm to fp32 adds u;
  * second-order terms and the float64 part: L <= 2^10 here (n < 2^30), so ((L + 6) u)^2 < 2^-27 < u / 8; together with the 2^-47 of the
    float64 part that is covered by one more u.
  relative: ((L + 6) / 2 + 2) u.
  * absolute: a square below the fp32 normal range (|g| < 2^-63) is rounded to a multiple of 2^-149, an error of at most 2^-150 per
    element whatever its size, and sums of subnormals are exact; sqrt(S + e) <= sqrt(S) + sqrt(e): grad_scale * sqrt(n * 2^-150), plus
    2^-149 for a norm that is itself subnormal.
None of this is read off the kernel's results."""
import math

import numpy as np
import torch

U = 2.0 ** -24
THREADS = 256


def geometry(lib):
    """-> (blocks, elements one pass of the whole grid covers), from what the library reports"""
    blocks = (int(lib.ifcbk_grad_clip_state_floats()) - 4) // 2
    return blocks, blocks * THREADS * 4


def chain(n, blocks):
    """float4s of the busiest thread"""
    return -(-(n // 4) // (blocks * THREADS))


def norm_bound(n, blocks, ref, grad_scale=1.0):
    """|device norm - ref| may be at most this (ref: the float64 norm)"""
    rel = ((chain(n, blocks) + 6) / 2.0 + 2.0) * U
    return rel * abs(ref) + grad_scale * math.sqrt(n * 2.0 ** -150) + 2.0 ** -149


def ref_norm(g, grad_scale=1.0):
    """float64: grad_scale * sqrt(sum g^2) of the fp32 values of g"""
    return float(np.float32(grad_scale)) * math.sqrt(float((g.double() * g.double()).sum()))


def host_coef(norm, max_norm):
    """torch's clip_coef = max_norm / (total_norm + 1e-6) clamped to 1, in fp32 as on fp32 tensors, from an fp32 norm.  A python scalar
    divided by a tensor is reciprocal(tensor) * scalar (Tensor.__rtruediv__): two roundings, which is what the kernel does as well
    (tests/test_clip_grad_cpu.py holds this function to clip_grad_norm_'s bits)"""
    with np.errstate(all='ignore'):
        c = (np.float32(1.0) / (np.float32(norm) + np.float32(1e-6))) * np.float32(max_norm)
    return np.float32(1.0) if c > np.float32(1.0) else c          # (a NaN is not > 1: it stays, as torch.clamp keeps it)


def f32_bits(x):
    return int(np.float32(x).view(np.int32))


def torch_clip(grads, max_norm, dtype=None):
    """torch.nn.utils.clip_grad_norm_ on copies of `grads` (a list of tensors) -> (total norm as a float, the clipped copies)"""
    ps = []
    for g in grads:
        g = g.detach().cpu().clone().contiguous()
        if dtype is not None:
            g = g.to(dtype)
        p = torch.nn.Parameter(torch.zeros_like(g))
        p.grad = g
        ps.append(p)
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    return float(total), [p.grad for p in ps]
