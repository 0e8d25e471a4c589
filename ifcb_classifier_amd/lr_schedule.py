"""The learning rate of every optimizer step as a pure function of the step's index (TRAIN --lr-schedule / --warmup / --lr-min).

``LrSchedule(kind, base, total_steps, warmup_steps, lr_min).at(t)`` is the rate of the t-th update, t counted from 0, evaluated in
double.  W = warmup_steps, T = total_steps:

    t < W  (only when W >= 2)   base * (t + 1) / W                          torch's LinearLR(start_factor=1/W, end_factor=1, total_iters=W-1)
    t >= W, u = (t - W) / max(1, T - W)
        'constant'              base
        'cosine'                lr_min + (base - lr_min) * (1 + cos(pi u)) / 2   CosineAnnealingLR(T_max=T-W, eta_min=lr_min), closed form
        'linear'                base + (lr_min - base) * u
    t >= T                      the rate of step T - 1 (TRAIN never gets there)

No state: the engine asks for ``at(step_count - 1)`` ahead of every optimizer launch, so whatever moves the step count (a loaded
optimizer state, another batch size's plan) moves the rate with it."""
import math

KINDS = ('constant', 'cosine', 'linear')


class LrSchedule:
    def __init__(self, kind, base, total_steps, warmup_steps=0, lr_min=0.0):
        if kind not in KINDS:
            raise ValueError('lr schedule kind must be one of %s, got %r' % (', '.join(KINDS), kind))
        self.kind, self.base, self.lr_min = kind, float(base), float(lr_min)
        self.total_steps, self.warmup_steps = int(total_steps), int(warmup_steps)
        if self.total_steps != total_steps or self.warmup_steps != warmup_steps:
            raise ValueError('lr schedule: total_steps and warmup_steps are whole numbers of steps')
        if not (math.isfinite(self.base) and self.base >= 0):
            raise ValueError('lr schedule: the base rate must be finite and >= 0')
        if self.total_steps < 1:
            raise ValueError('lr schedule: total_steps must be >= 1')
        if not 0 <= self.warmup_steps < self.total_steps:
            raise ValueError('lr schedule: warmup_steps must be in [0, total_steps)')
        if not 0.0 <= self.lr_min <= self.base:                   # (a NaN fails both comparisons)
            raise ValueError('lr schedule: lr_min must be in [0, base]')

    def at(self, t):
        """the rate of update t (0-based), a python float"""
        W, T = self.warmup_steps, self.total_steps
        t = min(int(t), T - 1)
        if t < 0:
            raise ValueError('lr schedule: step index %d' % t)
        if t < W and W >= 2:
            # (the last warm-up step is the base rate's own bits, which base * W / W need not be)
            return self.base if t == W - 1 else self.base * (t + 1) / W
        if self.kind == 'constant':
            return self.base
        u = (t - W) / max(1, T - W) if t >= W else 0.0            # (W == 1: its one warm-up step is the base rate itself)
        if self.kind == 'cosine':
            return self.lr_min + (self.base - self.lr_min) * 0.5 * (1.0 + math.cos(math.pi * u))
        return self.base + (self.lr_min - self.base) * u

    def __repr__(self):
        return 'LrSchedule(%r, base=%g, total_steps=%d, warmup_steps=%d, lr_min=%g)' % (
            self.kind, self.base, self.total_steps, self.warmup_steps, self.lr_min)


def schedule_steps(emax, warmup_epochs, steps_per_epoch):
    """-> (T, W) of a TRAIN run: T = emax * steps_per_epoch updates, W = round(warmup_epochs * steps_per_epoch) of them warming up"""
    return int(emax) * int(steps_per_epoch), int(round(float(warmup_epochs) * int(steps_per_epoch)))
