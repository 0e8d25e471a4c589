"""RUN --tta: the float64 mean of float64 softmaxes and its per-element fp32 error bound, for ifcbk_softmax_acc (csrc/loss.hip) called
once per view.  A plain helper module in the conventions of op_bounds.py (U = 2^-24, gamma_n = n U / (1 - n U)), derived from its
``softmax`` and not tuned:

    the device computes   acc = fl(... fl(fl(p_1 + p_2) + p_3) ... + p_V),   out = fl(acc * scale),   scale = 1 / V
    p_v is ifcbk_softmax's value for view v: within e_p,v of the float64 softmax (op_bounds.softmax, which already ends with the
      rounding of its product);
    the V - 1 additions and the product are V roundings of partial sums that are at most sum_v p_v (all terms are non-negative):
      gamma_(V + 1) * sum_v p_v covers them with one to spare (the conversion of scale, exact for a power of two);
    the store is the product's rounding; U * |mean| restates it at the result's magnitude, as every bound of op_bounds ends.

    e = scale * (sum_v e_p,v + gamma_(V + 1) * sum_v p_v) + U * |mean|
"""
import op_bounds as ob


def mean_softmax(logit_views):
    """(want, e): float64 mean over the views of softmax(dim=1) of each fp32 logits tensor [N, NC], and the bound above"""
    V = len(logit_views)
    scale = 1.0 / V
    sum_p = sum_e = 0.0
    for l in logit_views:
        p, e_p, _ = ob.softmax(l)
        sum_p = sum_p + p
        sum_e = sum_e + e_p
    want = sum_p * scale
    return want, scale * (sum_e + ob.gamma(V + 1) * sum_p) + ob.U * want.abs()
