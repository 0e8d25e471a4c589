"""Plan/executor for one backbone on one GPU: owns the flat parameter / gradient / optimizer-state buffers,
the NHWC activation and gradient buffers, and the op tables that ``ifcbk_run_program`` launches.

No autograd, no tracing: the graph is static (``graph.py``), so forward, backward and update are three
pre-built op tables; one FFI crossing launches a whole step.  PyTorch is used only for device memory and
streams.  The HIP library is mandatory -- there is no CPU fallback in this module.
"""
import contextlib
import ctypes as C
import math
import os

import torch

from . import _lib, ops
from ._lib import Op, ConvDesc, BnDesc, PoolDesc, HeadDesc
from .plan import OpList, Program, PlanBuilder, schedule_lanes, _overlap, _vp       # noqa: F401  (re-exported: tests import them from here)

# operand slots the engine reads back from ops of a plan
_PACK_W_MASTER, _PACK_W, _PACK_WT, _PACK_WT_LD = (ops.slot(_lib.OP_WEIGHT_PACK, name) for name in ('w_master', 'w', 'wT', 'wT_ld'))
_GROUP_N, _SEG_K = ops.slot(_lib.OP_CONV_WGRAD_GROUP, 'n'), ops.tail(_lib.OP_CONV_WGRAD_SEG, 'kseg')


# environment switches the library reads at launch time that change a workspace size or a partial-row count (csrc/conv_*.hip,
# bn.hip), plus the engine's weight-gradient switches; tests/test_switches_cpu.py checks the list against the library sources
_DISPATCH_SWITCHES = ('IFCBK_CONV_PP3', 'IFCBK_CONV_PP3_GRID', 'IFCBK_WGRAD_LANE', 'IFCBK_WGRAD_GROUP', 'IFCBK_WGRAD_GROUP_MINKH', 'IFCBK_CONV_BIG', 'IFCBK_CONV_SLAB', 'IFCBK_CONV_BIG_MT', 'IFCBK_CONV_BIG_TN', 'IFCBK_CONV_FLAT', 'IFCBK_CONV_NT',
                      'IFCBK_CONV_WM', 'IFCBK_CONV_WS', 'IFCBK_CONV_WS_TILES', 'IFCBK_CONV_ROWS', 'IFCBK_WGRAD_PP',
                      'IFCBK_WGRAD_PP_KH', 'IFCBK_WGRAD_COLS', 'IFCBK_WGRAD_STEM', 'IFCBK_WGRAD_ROUNDS', 'IFCBK_WGRAD_FLAT',
                      'IFCBK_BN_BWD_ROWS')


def _dispatch_env():
    return tuple(os.environ.get(k) for k in _DISPATCH_SWITCHES)


def dtype_is_bf16(eng):
    return eng.dtype == 'bf16'


def ema_decay_at(decay, t, warmup=True):
    """decay of the t-th update (t = 1, 2, ...) of a weight average since it was initialised: min(decay, (1 + t) / (10 + t)), the
    warm-up of TensorFlow's ExponentialMovingAverage(num_updates) -- a short training is not held to its initial weights for
    1 / (1 - decay) steps; warmup=False: decay itself"""
    return min(float(decay), (1.0 + t) / (10.0 + t)) if warmup else float(decay)


def ema_weight(decay, t, warmup=True):
    """the w of e <- e + w (p - e) for that update: 1 - d_t in double, rounded ONCE to fp32 (what the kernels are given)"""
    return C.c_float(1.0 - ema_decay_at(decay, t, warmup)).value


# The largest activation an engine may hold: that of the largest batch an eval program was verified on, bit for bit against its
# 256-image parts over every activation (scripts/big_batch_bisect.py: 4,096 inception_v3 images, 147 x 147 x 64 bf16 each).
VERIFIED_ACTIVATION_BYTES = 4096 * 147 * 147 * 64 * 2


def _index_bytes():
    # development switch (scripts/big_batch_bisect.py): another cap, to look beyond the verified one
    e = os.environ.get('IFCBK_DEV_INDEX_GIB')
    return int(float(e) * (1 << 30)) if e else VERIFIED_ACTIVATION_BYTES


def check_distill(distill, focal_gamma=0.0, mix=False):
    """the ``distill`` argument of Engine: None, or (alpha, T) with alpha in [0, 1] and T finite and > 0 -> None or a tuple of two floats.
    Distillation combines with neither focal loss nor a mixed batch (the library refuses such an op as well)."""
    if distill is None:
        return None
    try:
        alpha, T = (float(v) for v in distill)
    except (TypeError, ValueError):
        raise ValueError('distill must be None or (alpha, temperature), got %r' % (distill,)) from None
    if not 0.0 <= alpha <= 1.0:                                   # (a NaN fails both comparisons)
        raise ValueError('distill: alpha must be in [0, 1]')
    if not 0.0 < T < math.inf:
        raise ValueError('distill: the temperature must be finite and > 0')
    if focal_gamma and focal_gamma > 0:
        raise ValueError('distill and focal_gamma do not combine: give one of them')
    if mix:
        raise ValueError('distill and mix do not combine: give one of them')
    return alpha, T


def _per_roi_f32(t, n, device, message):
    """refuse (ValueError ``message`` % (n, device)) what is not a contiguous float32 tensor of one value per ROI on the ROIs' device"""
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.device == device and t.numel() == n and t.is_contiguous()):
        raise ValueError(message % (n, device))


class Engine:
    """Device state of one model replica."""

    @staticmethod
    def capacity_limit(net, dtype='bf16'):
        """the largest batch one engine serves (see __init__: largest activation <= VERIFIED_ACTIVATION_BYTES)"""
        per_img = max(b.H * b.W * b.C for b in net.bufs) * (2 if dtype == 'bf16' else 4)
        return max(1, _index_bytes() // per_img)

    def __init__(self, net, device=0, max_batch=32, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, dtype='bf16', optimizer='adam',
                 momentum=0.0, plan_only=False, train_batch=None, dp_world=None, class_weights=None, weight_decay=0.0,
                 label_smoothing=0.0, focal_gamma=0.0, mix=False, ema_decay=None, ema_warmup=True, distill=None, clip_grad=None,
                 blur_radius=None, lr_schedule=None, accumulate=1):
        # dp_world: world size of the data-parallel job this replica belongs to (None: WORLD_SIZE of the launcher, else an
        # initialised torch.distributed group, else 1) -- it picks the program-lane default, and train_step_ddp checks it
        self._dp_world_arg = None if dp_world is None else int(dp_world)
        # plan_only: build buffers on the host and the op tables only (no HIP context, nothing can run) -- the CPU tests
        # of the data-parallel bucket plan read the REAL backward list of a network this way
        self.plan_only = bool(plan_only)
        if not self.plan_only and not torch.cuda.is_available():
            raise RuntimeError('ifcb_classifier_amd needs a HIP device (MI355X); none is visible and there is no CPU path')
        if str(optimizer).lower() not in ('adam', 'sgd', 'adamw'):
            raise ValueError("optimizer must be 'adam' (the reference's only behaviour, neuston_models.py:63-64), 'sgd' or 'adamw'")
        # 'adamw' (additive, TRAIN --optimizer AdamW): Adam's op, buffers, step count and bias correction with the op's `decoupled` operand
        # set, so that weight_decay is torch.optim.AdamW's p *= 1 - lr * wd instead of the L2 term
        self.optimizer, self.momentum = str(optimizer).lower(), float(momentum)
        # the slots _set_update stamps on every step, resolved once
        opt_kind = _lib.OP_SGD if self.optimizer == 'sgd' else _lib.OP_ADAM
        self._upd_step, self._upd_scale, self._upd_ema_w, self._upd_lr = (ops.slot(opt_kind, name)
                                                                          for name in ('step', 'grad_scale', 'ema_w', 'lr'))
        # additive (TRAIN --lr-schedule / --warmup): an lr_schedule.LrSchedule (anything with .at(t)); the optimizer ops of step t + 1 then
        # carry fp32(at(t)) in their lr operand.  None: the ops keep the lr written at plan time
        if lr_schedule is not None and not callable(getattr(lr_schedule, 'at', None)):
            raise ValueError('lr_schedule must be None or an object with .at(step index) -> rate (lr_schedule.LrSchedule)')
        self.lr_schedule = lr_schedule
        # additive options (TRAIN --weight-decay / --class-norm; upstream has neither): torch's L2 form g + wd * p in the fused
        # Adam / SGD kernels, and per-class weights of the loss (nn.CrossEntropyLoss(weight=...)); None / 0.0: upstream's behaviour
        self.weight_decay = float(weight_decay or 0.0)
        if self.weight_decay < 0:
            raise ValueError('weight_decay must be >= 0')
        if class_weights is not None:
            class_weights = [float(w) for w in (class_weights.tolist() if hasattr(class_weights, 'tolist') else class_weights)]
            if len(class_weights) != net.NC:
                raise ValueError('class_weights: %d values for %d classes' % (len(class_weights), net.NC))
            if not all(math.isfinite(w) and w >= 0 for w in class_weights) or not any(class_weights):
                raise ValueError('class_weights must be finite, non-negative and not all zero')
        self._class_weights_arg = class_weights
        # additive (TRAIN --label-smoothing): nn.CrossEntropyLoss(label_smoothing=eps) in the fused loss ops; None / 0.0: the hard loss
        self.label_smoothing = float(label_smoothing or 0.0)
        if not 0.0 <= self.label_smoothing <= 1.0:                # (a NaN fails both comparisons)
            raise ValueError('label_smoothing must be in [0, 1]')
        # additive (TRAIN --focal-gamma): focal loss u^gamma * CE in the fused loss ops, u = 1 - p[target]; None / 0.0: the plain loss
        self.focal_gamma = float(focal_gamma or 0.0)
        if not 0.0 <= self.focal_gamma < math.inf:                # (a NaN fails both comparisons)
            raise ValueError('focal_gamma must be finite and not negative')
        if self.focal_gamma > 0 and self.label_smoothing > 0:
            raise ValueError('focal_gamma and label_smoothing do not combine: give one of them')
        # additive (TRAIN --mixup / --cutmix): the train loss ops read per-image mix factors from a device array (mix_lam) and run the
        # two-target kernel; mix_batch() mixes a loaded batch with its reverse.  False: buffers, plans and launches are what they were
        self.mix = bool(mix)
        # additive (TRAIN --blur): the radius of the run's Gaussian window, 1..12; load_rois(blur=sigmas) then blurs the resized batch in
        # place (ifcbk_batch_blur).  None: load_rois refuses sigmas.  No buffer, plan or op depends on it
        self.blur_radius = None if blur_radius is None else int(blur_radius)
        if self.blur_radius is not None and not (1 <= self.blur_radius <= 12 and self.blur_radius == blur_radius):
            raise ValueError('blur_radius must be an integer 1..12, or None for an engine that never blurs')
        if self.blur_radius is not None and self.blur_radius >= net.S:
            raise ValueError('blur_radius %d >= the input side %d: the reflected border needs r < S' % (self.blur_radius, net.S))
        if self.mix and self.focal_gamma > 0:
            raise ValueError('mix and focal_gamma do not combine: give one of them')
        # additive (TRAIN --distill): (alpha, T) -- the train loss ops run Hinton's loss (ifcbk_softmax_xent_distill) against the logits in
        # ``teacher_logits``, a fp32 [max_batch][NC] buffer THIS engine owns for its whole life, so plans and captured graphs hold one
        # address; whoever runs the teacher copies its logits there ahead of a train step, on the step's stream.  None: no buffer, and
        # plans, op tables and launches are what they were
        self.distill = check_distill(distill, self.focal_gamma, self.mix)
        # additive (TRAIN --ema): an exponential moving average E / ERB of the parameters P and the BatchNorm running statistics RB, taken
        # inside the optimizer ops (their operand E) and by one ifcbk_ema_flat call per step; ema_weights() evaluates and exports it.
        # None: no shadow buffers, and plans, op tables and launches are what they were
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        if self.ema_decay is not None and not 0.0 < self.ema_decay < 1.0:      # (a NaN fails both comparisons)
            raise ValueError('ema_decay must be in (0, 1), or None for no weight average')
        self.ema_warmup = bool(ema_warmup)
        self.ema_stale = True             # P was set from outside the optimizer (params_changed): the next train step starts E = P, ERB = RB
        self.ema_updates = 0              # t of the decay schedule: updates since E was last initialised
        self._ema_w = 0.0
        self._ema_view = None             # (P, RB, stale flag) saved by ema_weights() while the averaged model stands in P / RB
        # additive (TRAIN --clip-grad): torch.nn.utils.clip_grad_norm_(parameters, clip_grad) ahead of every optimizer step, on the device:
        # the step's one optimizer op takes the norm of the whole of G (ifcbk_grad_norm) into ``clip_state`` and its update reads the
        # coefficient from there (its p[5] / p[4]); nothing is waited for.  None: no state, and plans, op tables and launches are what
        # they were
        self.clip_grad = None if clip_grad is None else float(clip_grad)
        if self.clip_grad is not None and not 0.0 < self.clip_grad < math.inf:      # (a NaN fails both comparisons)
            raise ValueError('clip_grad must be a finite number > 0, or None for no gradient clipping')
        if self.clip_grad is not None and not 0.0 < C.c_float(self.clip_grad).value < math.inf:
            raise ValueError('clip_grad %r is not a finite fp32 number > 0' % self.clip_grad)
        # additive (TRAIN --accumulate K): Lightning's accumulate_grad_batches -- the gradients of K consecutive batches are summed into
        # ``A`` (ifcbk_grad_accum_flat behind every backward) and ONE optimizer step is taken from the sum times 1 / K; BatchNorm and the
        # step's counters move with every batch.  1: no buffer, and plans, op tables and launches are what they were
        if isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1:
            raise ValueError('accumulate must be an integer >= 1 (batches per optimizer step), got %r' % (accumulate,))
        self.accumulate = accumulate
        self.acc_pending = 0              # batches in the open window (0: closed)
        self._acc_plan = None             # the plan of the window's last batch: its optimizer program applies the window
        self.net = net
        if dtype not in ('bf16', 'fp32'):
            raise ValueError("dtype must be 'bf16' (performance) or 'fp32' (parity mode)")
        self.dtype = dtype
        self.tdtype = torch.bfloat16 if dtype == 'bf16' else torch.float32
        self.esize = 2 if dtype == 'bf16' else 4
        self.cdtype = _lib.BF16 if dtype == 'bf16' else _lib.F32
        if self.plan_only:
            self.dev = torch.device('cpu')
            self.ctx = _lib.PlanOnlyContext()
        else:
            self.dev = torch.device('cuda', device)
            torch.cuda.set_device(self.dev)
            self.ctx = _lib.Context(device)
        # The conv kernels address every tensor through a 32-bit buffer descriptor (2 GiB window): the largest per-image tensor
        # (inception_v3: 147x147x64 bf16 = 2.77 MB) bounds the images ONE LAUNCH can take (776 in bf16, 388 in fp32).  Programs
        # without batch statistics (the eval forward) go beyond it: the library cuts such a convolution into launches over image
        # groups (csrc/conv_igemm.hip conv_fwd_impl), so the engine's capacity is what was asked for; a TRAINING step beyond the
        # window is refused (BatchNorm statistics and the split-K weight gradient are per launch).
        self.requested_batch = int(max_batch)
        per_img = max(b.H * b.W * b.C for b in net.bufs) * (2 if dtype == 'bf16' else 4)
        self.window_batch = max(1, ((1 << 31) - 1) // per_img)
        # ... and an eval batch beyond that window is verified bit for bit against its parts up to 4,096 inception images, every
        # activation compared (scripts/big_batch_bisect.py; tests/test_gpu_model.py at 1024 and across the 2 GiB offset of the stem
        # output).  Round 4 had capped this at 3 GiB after batch 1536 faulted and batch 2048 returned wrong probabilities: the u8
        # stem kernel sign-extended the low half of its 64-bit row offset (readfirstlane returns int), so the rows of images
        # >= 1,511 were written 4 GiB in front of the tensor -- fixed in csrc/conv_stem_u8.hip.  The engine still refuses a
        # capacity beyond what was verified instead of finding out on the device; RUN chunks a larger --batch itself.
        self.index_batch = max(1, _index_bytes() // per_img)
        if int(max_batch) > self.index_batch:
            raise RuntimeError('max_batch %d: the largest activation of %s would exceed the verified %.1f GiB; batches beyond %d '
                               'images are not supported in one program (run them in chunks)'
                               % (int(max_batch), net.name, _index_bytes() / (1 << 30), self.index_batch))
        self.max_batch = int(max_batch)
        # capacity of the TRAINING-side buffers (activation gradients, d(raw) scratch, pool arg-max, split-K workspace): a training
        # step beyond the window is refused anyway, so they never need more than it; an inference-only engine (neuston_net RUN:
        # train_batch=1) keeps to activations -- 'RUN --batch 2048' must not allocate gradients for 2048 images
        self.train_batch = max(1, min(self.max_batch, self.window_batch if train_batch is None else int(train_batch)))
        self.lr, self.betas, self.eps = lr, betas, eps
        self.step_count = 0
        self.packed = False
        self.eval_stats_ready = False
        self.dropout_seed = 0x1234
        self.fuse_siblings = os.environ.get('IFCBK_FUSE_SIBLINGS', '1') != '0'
        self.dropout_calls = 0
        self.external_mask = None
        self._plans = {}
        self._alloc_params()
        self._alloc_acts()

    # ------------------------------------------------------------------ parameters
    def _alloc_params(self):
        net, dev = self.net, self.dev
        off = 0
        self.poff = {}
        self.palloc = {}          # flat offset -> padded element count of the tensor stored there
        for key, shape, kind, node in net.params:
            n = na = int(math.prod(shape))
            if getattr(node, 'kind', '') == 'cb' and node.K != node.K_real:
                na = n // shape[0] * node.K       # output channels padded to a whole 16-byte chunk: the extra rows stay zero
            self.poff[key] = (off, n, shape, kind, node)
            self.palloc[off] = (na + 3) // 4 * 4
            off += (na + 3) // 4 * 4          # keep every tensor 16-byte aligned
        self.nparam_padded = off
        self.cbias_after = {}
        for key, (o, n, shape, kind, node) in self.poff.items():
            if kind == 'bn_cbias':
                self.cbias_after[self.poff[node.bn_key + '.weight'][0]] = [o]
        self.P = torch.zeros(off, dtype=torch.float32, device=dev)
        self.G = torch.zeros(off, dtype=torch.float32, device=dev)
        self.M = torch.zeros(off, dtype=torch.float32, device=dev)
        self.V = torch.zeros(off, dtype=torch.float32, device=dev)
        self.E = torch.zeros(off, dtype=torch.float32, device=dev) if self.ema_decay is not None else None      # layout of P
        # the accumulator (layout of G): never zeroed, the first batch of a window overwrites it
        self.A = torch.empty(off, dtype=torch.float32, device=dev) if self.accumulate > 1 else None
        assert self.A is None or self.A.data_ptr() % 16 == 0
        # the clip state: norm, coefficient, the epoch's two running figures, and the norm kernel's per-block partial sums
        self.clip_state = None
        if self.clip_grad is not None:
            self.clip_state = torch.zeros(int(self.ctx.lib.ifcbk_grad_clip_state_floats()), dtype=torch.float32, device=dev)
            assert self.clip_state.data_ptr() % 16 == 0
        self.pviews, self.gviews = {}, {}
        for key, (o, n, shape, kind, node) in self.poff.items():
            if kind == 'conv':
                K, Cw, R, S = shape
                self.pviews[key] = self.P[o:o + n].view(K, R, S, Cw).permute(0, 3, 1, 2)   # OIHW view of KRSC memory
                self.gviews[key] = self.G[o:o + n].view(K, R, S, Cw).permute(0, 3, 1, 2)
            else:
                self.pviews[key] = self.P[o:o + n].view(shape)
                self.gviews[key] = self.G[o:o + n].view(shape)
        # BN running statistics
        boff = 0
        self.boff = {}
        for key, shape, node in net.buffers:
            self.boff[key] = (boff, shape[0])
            boff += shape[0]
        self.RB = torch.zeros(boff, dtype=torch.float32, device=dev)
        self.ERB = torch.zeros(boff, dtype=torch.float32, device=dev) if self.ema_decay is not None else None   # layout of RB
        self.bviews = {k: self.RB[o:o + n] for k, (o, n) in self.boff.items()}
        for k, v in self.bviews.items():
            if k.endswith('running_var'):
                v.fill_(1.0)
        convs = [n for n in net.nodes if getattr(n, 'kind', '') == 'conv']
        self.convs = convs
        self.plains = [n for n in net.nodes if n.kind == 'cb']       # conv (+bias) (+ReLU) without BatchNorm, nn.Linear layers
        self.bnrs = [n for n in net.nodes if n.kind == 'bnr']        # BatchNorm -> ReLU in front of a conv (densenet)
        self.bn_nodes = [n for n in net.nodes if n.kind in ('conv', 'bnr')]
        self.bn_index = {n: k for k, n in enumerate(self.bn_nodes)}
        self.nbt = torch.zeros(len(self.bn_nodes), dtype=torch.int64, device=dev)        # num_batches_tracked (all BNs)
        self.ones = torch.ones(max([n.K for n in self.plains] + [8]), dtype=torch.float32, device=dev)
        # bf16 shadows + per-BN statistics
        # horizontal fusion: sibling 1x1 convs that read the same tensor become ONE GEMM (filters concatenated along K)
        # in the training forward / dgrad / wgrad; their BatchNorms stay per branch on channel slices.
        class Group:
            pass
        self.groups = []
        bykey = {}
        # An Inception block's pool branch is avgpool3x3(s1,p1) -> 1x1 conv -> BN -> ReLU.  Both operators are linear and the
        # conv has no bias, so conv1x1(avgpool(x)) == avgpool(conv1x1(x)) (zero padding included: count_include_pad averages
        # zeros, and conv1x1(0) = 0).  In TRAINING the engine runs the conv first -- as one more member of the block's
        # sibling GEMM on x -- and pools its pf = 32..192 output channels instead of the block's 192..2048 input channels:
        # the pool's traffic shrinks 4-10x in both directions and the branch needs no conv launches of its own.  BatchNorm
        # then normalises the pooled tensor, whose batch statistics come from ifcbk_bn_stats; in eval mode the pool applies the
        # folded BatchNorm affine + ReLU in its epilogue (ifcbk_avgpool3x3_affine).
        self.commute_pool = os.environ.get('IFCBK_COMMUTE_POOL', '1') != '0' and self.fuse_siblings
        self.eval_groups = os.environ.get('IFCBK_EVAL_GROUPS', '1') != '0'      # eval forward: sibling 1x1 convs as one GEMM
        nread = {}
        for m in net.nodes:
            for v in ((m.x, getattr(m, 'residual', None)) if m.kind == 'conv' else (m.x,)):
                if v is not None:
                    nread[v.buf.id] = nread.get(v.buf.id, 0) + 1
        for n in convs:
            n.cpool = None
            if (self.commute_pool and n.R == 1 and n.S == 1 and n.sh == 1 and n.sw == 1 and n.ph == 0 and n.pw == 0
                    and n.x.is_full and n.residual is None and n.relu and not n.aux and nread.get(n.x.buf.id, 0) == 1):
                prod = [m for m in net.nodes if m.kind == 'avg' and m.y.buf.id == n.x.buf.id]
                if (len(prod) == 1 and (prod[0].R, prod[0].S, prod[0].sh, prod[0].sw, prod[0].ph, prod[0].pw) == (3, 3, 1, 1, 1, 1)
                        and prod[0].x.is_full and prod[0].y.is_full and not prod[0].x.buf.is_input and not prod[0].aux):
                    n.cpool = prod[0]
        if self.fuse_siblings:
            for n in convs:
                n.group = None
                src = n.cpool.x if n.cpool is not None else n.x
                if (n.R == 1 and n.S == 1 and n.sh == 1 and n.sw == 1 and n.ph == 0 and n.pw == 0 and src.is_full
                        and not src.buf.is_input and n.residual is None and n.relu):
                    bykey.setdefault(src.buf.id, []).append(n)
        for members in bykey.values():
            plain = [m for m in members if m.cpool is None]
            if not (2 <= len(members) <= 4) or not plain:
                for m in members:
                    m.cpool = None                      # no sibling GEMM to join: keep the reference order
                members = plain
            members = plain + [m for m in members if m.cpool is not None]      # the first member launches the group's GEMMs
            if 2 <= len(members) <= 4:
                g = Group()
                g.members, g.x = members, members[0].x
                g.Ktot = sum(m.K for m in members)
                off = 0
                for m in members:
                    m.group, m.koff = g, off
                    off += m.K
                self.groups.append(g)
        for n in convs:
            if not hasattr(n, 'group'):
                n.group = None
            if n.group is None:
                n.cpool = None
        self.absorbed_pools = {n.cpool for n in convs if n.cpool is not None}
        soff = 0
        stoff = 0
        done = set()
        for n in convs:
            g = n.group
            if g is None:
                n.w_off = soff
                soff += n.K * n.R * n.S * n.x.C
                n.wT_off = soff
                soff += n.K * n.R * n.S * n.x.C
                n.wT_ld = 0
                n.st_off, n.st_ld = stoff, n.K
                stoff += 6 * n.K          # mean, invstd, scale, shift, eval_scale, eval_shift
            elif id(g) not in done:
                done.add(id(g))
                Cin = g.x.C
                g.w_off = soff                      # [Ktot][Cin]: member rows are contiguous
                soff += g.Ktot * Cin
                g.wT_off = soff                     # [Cin][Ktot]: members own column slices
                soff += g.Ktot * Cin
                g.st_off = stoff                    # 6 arrays of Ktot
                stoff += 6 * g.Ktot
                for m in g.members:
                    m.w_off = g.w_off + m.koff * Cin
                    m.wT_off = g.wT_off + m.koff
                    m.wT_ld = g.Ktot
                    m.st_off, m.st_ld = g.st_off + m.koff, g.Ktot
        for n in self.plains:
            n.group = None
            n.w_off = soff
            soff += n.K * n.R * n.S * n.x.C
            n.wT_off = soff
            soff += n.K * n.R * n.S * n.x.C
            n.wT_ld = 0
        for n in self.bnrs:
            n.group = None
            n.st_off, n.st_ld = stoff, n.K
            stoff += 6 * n.K
        self.Wsh = torch.zeros(soff, dtype=self.tdtype, device=dev)
        self.stats = torch.zeros(stoff, dtype=torch.float32, device=dev)

    def init_weights(self, seed=None):
        """[TV] initialisation: truncated normal (inception) / kaiming fan_out (resnet); the replaced
        ``fc`` heads use ``nn.Linear``'s default init (neuston_models.py:25-26,39)."""
        g = torch.Generator(device='cpu')
        if seed is None:        # draw from torch's global RNG so that seed_everything(--seed) makes the init reproducible
            seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        g.manual_seed(int(seed))
        incep = self.net.name == 'inception_v3'
        for key, (o, n, shape, kind, node) in self.poff.items():
            v = self.pviews[key]
            how = getattr(node, 'init', None)
            if kind in ('conv', 'lin_w') and how is not None:
                # [TV] alexnet: torch defaults; vgg: kaiming_normal(fan_out) convs, N(0, 0.01) Linears, zero biases; squeezenet:
                # kaiming_uniform convs, zero biases; densenet: kaiming_normal (fan_in) convs; the layers the reference replaces
                # (neuston_models.py:27-42) keep torch's default init
                rf = shape[2] * shape[3] if len(shape) == 4 else 1
                fan_in, fan_out = shape[1] * rf, shape[0] * rf
                w = torch.empty(shape)
                if how == 'default':
                    w.uniform_(-1.0 / math.sqrt(fan_in), 1.0 / math.sqrt(fan_in), generator=g)
                elif how == 'kaiming_uniform':
                    w.uniform_(-math.sqrt(6.0 / fan_in), math.sqrt(6.0 / fan_in), generator=g)
                elif how == 'kaiming_out':
                    w.normal_(0, math.sqrt(2.0 / fan_out), generator=g)
                elif how == 'kaiming_in':
                    w.normal_(0, math.sqrt(2.0 / fan_in), generator=g)
                elif how == 'normal01':
                    w.normal_(0, 0.01, generator=g)
                else:
                    raise ValueError(how)
                v.copy_(w.to(self.dev))
            elif kind == 'cbias':
                wshape = self.poff[key[:-4] + 'weight'][2]
                fan_in = int(math.prod(wshape[1:]))
                if node.init == 'default':
                    v.copy_(((torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)).to(self.dev))
                else:
                    v.zero_()
            elif kind == 'bn_cbias':
                v.zero_()
            elif kind == 'conv':
                w = torch.empty(shape)
                if incep:
                    std = 0.01 if key.startswith('AuxLogits.conv1') else 0.1
                    torch.nn.init.trunc_normal_(w, 0.0, std, -2 * std, 2 * std, generator=g)
                else:
                    fan_out = shape[0] * shape[2] * shape[3]
                    w.normal_(0, math.sqrt(2.0 / fan_out), generator=g)
                v.copy_(w.to(self.dev))
            elif kind == 'bn_w':
                v.fill_(1.0)
            elif kind == 'bn_b':
                v.zero_()
            elif kind == 'fc_w':
                bound = 1.0 / math.sqrt(shape[1])
                v.copy_(((torch.rand(shape, generator=g) * 2 - 1) * bound).to(self.dev))
            elif kind == 'fc_b':
                fan_in = self.poff[key[:-4] + 'weight'][2][1]
                bound = 1.0 / math.sqrt(fan_in)
                v.copy_(((torch.rand(shape, generator=g) * 2 - 1) * bound).to(self.dev))
        self.params_changed()
        self.accumulate_discard()

    def params_changed(self):
        self.packed = False
        self.eval_stats_ready = False
        self.ema_stale = True             # (the optimizer paths do not come through here: only writes from outside restart the average)

    # ------------------------------------------------------------------ gradient clipping (TRAIN --clip-grad)
    def grad_clip_stats(self):
        """-> (norm of the last step's gradient before clipping, its coefficient, the largest norm and the number of clipped steps since
        reset_grad_clip_stats).  One 16-byte device-to-host read on the engine's stream: it waits for the steps queued there"""
        if self.clip_state is None:
            raise RuntimeError('grad_clip_stats: this engine was built without clip_grad')
        norm, coef, top, clipped = self.clip_state[:4].tolist()
        return norm, coef, top, int(clipped)

    def reset_grad_clip_stats(self):
        """zero the two running figures (largest norm, clipped steps): the start of an epoch's report"""
        if self.clip_state is None:
            raise RuntimeError('reset_grad_clip_stats: this engine was built without clip_grad')
        self.clip_state[2:4].zero_()

    # ------------------------------------------------------------------ weight average (TRAIN --ema)
    def _ema_begin_step(self, update=True):
        """at the start of a train step (update=False: of a training forward that an adam_step will follow): initialise the average if P
        was set from outside since the last step -- E = P, ERB = RB as they stand BEFORE this step's forward, whichever way the step is
        launched -- then count the update and round its weight once"""
        if self.ema_decay is None:
            return
        if self._ema_view is not None:
            raise RuntimeError('a train step inside ema_weights(): P holds the averaged weights there')
        if self.ema_stale:
            self.E.copy_(self.P)
            self.ERB.copy_(self.RB)
            self.ema_updates = 0
            self.ema_stale = False
        if update:
            self.ema_updates += 1
            self._ema_w = ema_weight(self.ema_decay, self.ema_updates, self.ema_warmup)

    def _ema_end_step(self):
        """behind the step program, on its stream: the running statistics are final, ERB takes the update E took inside the optimizer ops"""
        if self.ema_decay is not None and self.RB.numel():
            self.ctx.call('ifcbk_ema_flat', _vp(self.ERB), _vp(self.RB), self.RB.numel(), self._ema_w, self.stream())

    @contextlib.contextmanager
    def ema_weights(self):
        """inside: forward_eval, the eval loss and every view of P / RB (the module's state_dict) see the averaged model E / ERB;
        num_batches_tracked stays the live count.  On leaving, P and RB hold their own bits again (M, V and the step count were never
        touched) and the next train step repacks from P.  Once per epoch: plain copies, no kernel of its own."""
        if self.ema_decay is None:
            raise RuntimeError('ema_weights: this engine was built without ema_decay')
        if self._ema_view is not None:
            raise RuntimeError('ema_weights: already inside')
        if self.ema_stale:
            # nothing was averaged since P was last set: the average of that model is the model
            self.E.copy_(self.P)
            self.ERB.copy_(self.RB)
            self.ema_updates = 0
            self.ema_stale = False
        self._ema_view = (self.P.clone(), self.RB.clone())
        self.P.copy_(self.E)
        self.RB.copy_(self.ERB)
        self.packed = self.eval_stats_ready = False
        try:
            yield self
        finally:
            p, rb = self._ema_view
            self.P.copy_(p)
            self.RB.copy_(rb)
            self._ema_view = None
            self.packed = self.eval_stats_ready = False
            self.ema_stale = False        # (an eval forward of the module inside calls params_changed(): nothing was written)

    # ------------------------------------------------------------------ activations
    def _alloc_acts(self):
        net, dev, N = self.net, self.dev, self.max_batch
        Nt = self.train_batch
        bf = self.tdtype
        self.act = {}
        self.grad = {}
        grouped_raw = {m.raw.id: m for g in self.groups for m in g.members if m.cpool is None}
        for b in net.bufs:
            if b.id in grouped_raw:
                continue                              # lives inside the group's merged raw tensor
            self.act[b.id] = torch.zeros(N, b.H, b.W, b.C, dtype=bf, device=dev)
        for g in self.groups:
            g.raw = torch.zeros(N, g.x.H, g.x.W, g.Ktot, dtype=bf, device=dev)
            for m in g.members:
                if m.cpool is None:
                    self.act[m.raw.id] = g.raw[..., m.koff:m.koff + m.K]        # strided view (tests / debugging)
                # a commuted pool branch: its slice of g.raw is the UNPOOLED conv output, m.raw (own buffer) the pooled one
        need_grad = set()
        for n in net.nodes:
            if getattr(n, 'kind', '') == 'conv':
                need_grad.add(n.y.buf.id)
                if n.residual is not None:
                    need_grad.add(n.residual.buf.id)
            elif n.kind in ('max', 'avg', 'cb', 'drop', 'flat', 'bnr'):
                need_grad.add(n.y.buf.id)
        need_grad.discard(net.input.id)
        for bid in need_grad:
            b = net.bufs[bid]
            if b.name.endswith(':raw'):
                continue
            self.grad[bid] = torch.zeros(Nt, b.H, b.W, b.C, dtype=bf, device=dev)
        # program lanes (branch-parallel streams) of the training programs: 4 on a single GPU, 2 in a data-parallel job (world > 1)
        # until a run with one process per GPU on >= 2 GPUs shows 4 is no slower THERE.  Round 1 saw 1.3-6.5 s per step with 3-4
        # lanes on a 2-rank rehearsal (two processes' 5 streams each on ONE device's hardware queues); round 3 measured the DP step
        # on ProcessGroupNCCL at world 1 (scripts/dp_lanes.py: 2 / 3 / 4 lanes = 25.57 / 24.15 / 23.98 ms, no stall) -- but a
        # world-1 all-reduce launches no RCCL ring kernels, so that run cannot show the lanes competing with them for CUs and
        # hardware queues (main + 4 lanes + RCCL = 6 streams on 4 queues).  No multi-GPU node was available to this build: the
        # conservative count ships, IFCBK_LANES overrides it, bench.py prints the count in `config.program_lanes`.
        # world size: the explicit argument, else the launcher's WORLD_SIZE (set before any rank builds its engine, so every rank
        # agrees whether or not init_process_group has run yet), else an initialised process group
        dp_world = self._dp_world_arg
        if dp_world is None:
            try:
                dp_world = int(os.environ.get('WORLD_SIZE', '0')) or None
            except ValueError:
                dp_world = None
        if dp_world is None:
            dp_world = 1
            try:
                import torch.distributed as _d
                if _d.is_available() and _d.is_initialized():
                    dp_world = _d.get_world_size()
            except Exception:
                dp_world = 1
        self.dp_world = max(1, int(dp_world))
        dp_world = self.dp_world
        self.NL = max(1, min(8, int(os.environ.get('IFCBK_LANES', '2' if dp_world > 1 else '4'))))
        self.NL_eval = max(1, min(self.NL, int(os.environ.get('IFCBK_LANES_EVAL', '2'))))     # ... of the eval forward (measured best)
        # hipGraph replay of the static programs.  Measured on MI355X (B=256): the eval forward replays 1.8 % faster than its
        # launch list (6.73 vs 6.85 ms); the train fwd+bwd graph is 4 % SLOWER (28.7 vs 27.6 ms per step: the graph's own
        # branch scheduling loses to the lane assignment below) -- so the default is 'eval'.  IFCBK_GRAPH=0 | eval | all
        gm = os.environ.get('IFCBK_GRAPH', 'eval')
        # (any lane count can be captured: ctx.hip records lane-to-lane edges through the origin stream, see run_lanes)
        self.graph_eval = gm not in ('0', 'off', 'none')
        self.graph_train = gm in ('1', 'all', 'train')
        # IFCBK_WGRAD_LANE=1 (round 4): EVERY weight gradient on the last lane, the branch chains on the others, and every layer keeps
        # its d(raw) in a buffer of its own (4.6 GB at batch 256) -- the backward critical path is then BN-backward -> input gradient
        # -> BN-backward ..., and the MFMA-bound weight gradients (6.7 ms of a step when each runs alone) fill in beside the
        # HBM-bound BatchNorm / pool kernels instead of standing in front of every input gradient on its lane
        # default: ONE weight-gradient lane (the last) when there are at least 3 lanes.  Measured at batch 256, same box, ms/step:
        # 4 chain lanes 22.67 | 3 chains + 1 weight-gradient lane 21.72 | the same with that lane's stream at low priority 21.60 (off, below) |
        # 2 + 1 lanes 22.34 | FIVE streams (4 + 1, 3 + 2) 27.7, six 31.8: this runtime has four hardware queues per process.
        # Two lanes (the data-parallel default): 2 chains 22.90 | 1 chain + 1 weight-gradient lane 22.52.
        self.wgrad_lane = int(os.environ.get('IFCBK_WGRAD_LANE', '1' if self.NL >= 2 else '0'))       # number of weight-gradient lanes
        if self.NL - self.wgrad_lane < 1:
            self.wgrad_lane = 0
        # (round 4's least-priority stream for that lane -- 0.0-0.1 ms per step -- is gone: round 5)
        if not self.plan_only:
            self.ctx.call('ifcbk_ctx_set_lanes', self.NL)     # one workspace arena per lane in use (was: always 8)
        max_raw = max([n.P * n.Q * n.K for n in self.convs] + [8])
        # d(raw) scratch: per lane
        self.draw = [torch.zeros(Nt * max_raw, dtype=bf, device=dev) for _ in range(self.NL)]
        gmax = max([g.x.H * g.x.W * g.Ktot for g in self.groups] + [0])
        self.draw_group = torch.zeros(max(1, Nt * gmax), dtype=bf, device=dev)
        # ... and the d(raw) tensors that outlive their layer's backward (own_draw / group_draw), out of one pool (_carve)
        self.draw_own, self._draw_pool, self._draw_used = {}, None, 0
        for g in self.groups:
            g.draw_own = None
        # partial BatchNorm sums, per lane: rows x 2 x channels of the largest layer -- over EVERY batch a plan can be built for, not
        # the capacity alone.  The row count follows the kernel the library picks for a batch, so it is not monotonic: resnet18 takes
        # 125,440 floats at batch 5 and 100,352 at batch 8, and the partial last batch of an epoch runs on these buffers
        # (tests/test_engine_life_cpu.py)
        mb = max(self._bn_part_floats(b) for b in self._plan_batches())
        self.bn_part = [torch.zeros(mb, dtype=torch.float32, device=dev) for _ in range(self.NL)]
        self.argmax = {}
        for k, n in enumerate(net.nodes):
            if n.kind == 'max':
                self.argmax[k] = torch.zeros(Nt, n.P, n.Q, n.x.C, dtype=torch.uint8, device=dev)
        self.heads = [n for n in net.nodes if n.kind == 'head']
        for h in self.heads:
            h.feat = torch.zeros(N, h.C, dtype=torch.float32, device=dev)
            h.logits = torch.zeros(N, h.NC, dtype=torch.float32, device=dev)
            h.dlogits = torch.zeros(N, h.NC, dtype=torch.float32, device=dev)
            h.mask = torch.ones(N, h.C, dtype=torch.uint8, device=dev) if h.dropout else None
        self.drops = [n for n in net.nodes if n.kind == 'drop']
        for n in self.drops:
            n.mask = torch.ones(N, n.x.H * n.x.W * n.x.C, dtype=torch.uint8, device=dev)
        self.probs = torch.zeros(N, net.NC, dtype=torch.float32, device=dev)
        # Two input slots (network input tensor + labels): while a step runs on slot s, the next batch is uploaded and
        # preprocessed into slot 1-s on a side stream (prefetch_begin / prefetch_end / use_prefetched).  Programs are built per
        # slot (only the pointers of the first conv, its weight gradient and the loss ops differ).
        self.tgt_bufs = [torch.zeros(N, dtype=torch.int64, device=dev) for _ in range(2)]
        self.in_bufs = [self.act[net.input.id], torch.zeros_like(self.act[net.input.id])]
        self.in_slot = 0
        # Grey ROIs into inception's Conv2d_1a: the resize writes only the u8 plane and the stem conv reads it directly
        # (csrc/conv_stem_u8.hip) -- the [N,S,S,8] tensor of the slot is then not written at all.  in_kind[slot]: 'nhwc' (the dense
        # tensor is current: load_input_nchw, RGB images) or 'u8' (the plane is current); programs are built per (slot, kind).
        self.stem_u8 = None
        first = [n for n in self.convs if n.x.buf.is_input]
        if (os.environ.get('IFCBK_STEM_U8', '1') != '0' and len(first) == 1 and first[0].group is None
                and self.ctx.lib.ifcbk_stem_u8_rows(C.byref(self._conv_desc(first[0], N))) > 0):
            self.stem_u8 = first[0]
            self.in_u8 = [torch.zeros(N, net.S, net.S, dtype=torch.uint8, device=dev) for _ in range(2)]
            self.in_ab = [torch.zeros(6, dtype=torch.float32, device=dev) for _ in range(2)]
            self._in_ab_host = [None, None]
        self.in_kind = ['nhwc', 'nhwc']
        self.pre_stream = self.pre_ctx = None
        self.ev_ready, self.ev_free, self.prefetched = [None, None], [None, None], None
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_sum = torch.zeros(1, dtype=torch.float32, device=dev)
        # per-class loss weights: one fp32 [NC] tensor, read by the loss ops only (never written by a program)
        self.class_weight = None if self._class_weights_arg is None else torch.tensor(self._class_weights_arg, dtype=torch.float32, device=dev)
        if self.mix:
            # one factor per image and input slot, 1 = unmixed; the loss ops of a slot's plans (and the graphs captured from them) hold
            # the array's address, which is why the factors live on the device and not in the ops' f[]
            self.mix_lam = [torch.ones(N, dtype=torch.float32, device=dev) for _ in range(2)]
        if self.distill is not None:
            # one buffer for both input slots: the teacher runs on the step's stream just ahead of the step, not in the prefetch
            self.teacher_logits = torch.zeros(N, net.NC, dtype=torch.float32, device=dev)
        # workspace: wgrad split-K slabs / bn_bwd partials -- again over every trainable batch: the split-K depth follows the batch, and
        # resnet18's weight gradients take 12,544,000 bytes at batch 7 and 12,142,592 at batch 8 (a step at 7 on an engine of capacity
        # 8 was refused with IFCBK_ENOMEM)
        self.ctx.reserve(max([1 << 20] + [self._train_workspace(b) for b in range(1, Nt + 1)]))

    def _carve(self, nelem):
        """a d(raw) buffer out of ONE pooled allocation per engine (78 tensors of an inception plan: one hipMalloc instead of 78,
        not zero-filled -- BatchNorm backward writes every element before anything reads it)"""
        if not self.wgrad_lane:
            # (without a weight-gradient lane only the members of grouped launches keep a buffer of their own: a handful of
            # tensors -- a pool sized for EVERY conv, 4.6 GB at batch 256, would be mostly unused)
            return torch.empty(nelem, dtype=self.tdtype, device=self.dev)
        if self._draw_pool is None:
            own = [m.P * m.Q * m.K for m in self.convs if m.group is None or m.cpool is not None]
            tot = sum((self.train_batch * per_img + 127) // 128 * 128 for per_img in own + [g.x.H * g.x.W * g.Ktot for g in self.groups])
            self._draw_pool = torch.empty(max(tot, 128), dtype=self.tdtype, device=self.dev)
        n = (nelem + 127) // 128 * 128
        if self._draw_used + n > self._draw_pool.numel():
            return torch.empty(nelem, dtype=self.tdtype, device=self.dev)
        v = self._draw_pool[self._draw_used:self._draw_used + nelem]
        self._draw_used += n
        return v

    def own_draw(self, m):
        """conv m's d(raw) in a buffer of its own, kept for the engine's life (carved on first use: the order is the plan builder's)"""
        if m not in self.draw_own:
            self.draw_own[m] = self._carve(self.train_batch * m.P * m.Q * m.K)
        return self.draw_own[m]

    def group_draw(self, g):
        """the merged d(raw) tensor of a sibling GEMM: the shared scratch, or the group's own when weight gradients have a lane"""
        if not self.wgrad_lane:
            return self.draw_group
        if g.draw_own is None:
            g.draw_own = self._carve(self.train_batch * g.x.H * g.x.W * g.Ktot)
        return g.draw_own

    def _plan_batches(self):
        """every batch whose plan touches the training-side scratch (1 .. train_batch), and the capacity"""
        return list(range(1, self.train_batch + 1)) + ([self.max_batch] if self.max_batch > self.train_batch else [])

    def _bn_part_floats(self, N):
        """floats one lane's partial-sum buffer must hold for a plan at batch N (every producer of partial rows in plan.PlanBuilder)"""
        lib = self.ctx.lib
        need = [16]
        for n in self.convs:
            d = self._conv_desc(n, N)
            need.append(lib.ifcbk_conv2d_fwd_mblocks(C.byref(d)) * 2 * n.K)
            need.append(max(0, lib.ifcbk_conv2d_dgrad_bnstat_mblocks(C.byref(d))) * 2 * n.x.C)       # its producer's sums, in its dgrad
            if n.x.buf.is_input:
                need.append(max(0, lib.ifcbk_stem_u8_rows(C.byref(d))) * 2 * n.K)
        for g in self.groups:
            need.append(lib.ifcbk_conv2d_fwd_mblocks(C.byref(self._group_desc(g, N))) * 2 * g.Ktot)
        for n in self.bnrs:
            need.append(lib.ifcbk_bn_stats_rows(N * n.x.H * n.x.W) * 2 * n.K)
        return max(need)

    def _train_workspace(self, Nt):
        """bytes of ctx workspace (per lane) the backward ops of a plan at batch Nt ask for"""
        lib = self.ctx.lib
        ws = 0
        for n in self.convs:
            ws = max(ws, lib.ifcbk_conv2d_wgrad_workspace(C.byref(self._conv_desc(n, Nt))))
            M = Nt * n.P * n.Q
            ws = max(ws, (((M + 255) // 256) * 2 * n.K + 2 * n.K) * 4)
        for g in self.groups:
            ws = max(ws, lib.ifcbk_conv2d_wgrad_workspace(C.byref(self._group_desc(g, Nt))))
        for n in self.plains:
            ws = max(ws, lib.ifcbk_conv2d_wgrad_workspace(C.byref(self._conv_desc(n, Nt))),
                     lib.ifcbk_bias_relu_bwd_workspace(Nt * n.P * n.Q, n.K))
        for n in self.bnrs:
            M = Nt * n.x.H * n.x.W
            ws = max(ws, (((M + 255) // 256) * 2 * n.K + 2 * n.K) * 4)
        if self.stem_u8 is not None:
            ws = max(ws, lib.ifcbk_stem_u8_wgrad_workspace(C.byref(self._conv_desc(self.stem_u8, Nt))))
        return ws

    def _grow_workspace(self, ctx, need):
        """reserve `need` bytes per lane if the ctx holds less.  A growth of the engine's own ctx moves its arenas: the graphs captured
        so far hold stale pointers (ifcbk_graph_launch would refuse them), so they are destroyed and captured again on next use"""
        if self.plan_only or need <= ctx.lib.ifcbk_ctx_workspace_bytes(ctx.h):
            return
        ctx.reserve(need)
        if ctx is self.ctx:
            for pl in self._plans.values():
                for g in pl.graphs.values():
                    ctx.lib.ifcbk_graph_destroy(ctx.h, g)
                pl.graphs.clear()

    @property
    def target(self):
        return self.tgt_bufs[self.in_slot]

    # ------------------------------------------------------------------ input pipelining
    def _select_slot(self, slot):
        self.in_slot = slot
        self.act[self.net.input.id] = self.in_bufs[slot]

    def prefetch_stream(self):
        """the side stream of the input pipeline (created on first use, with its own library context / workspace arena)"""
        if self.plan_only:
            raise RuntimeError('prefetch: this engine was built with plan_only=True')
        if self.pre_stream is None:
            self.pre_stream = torch.cuda.Stream(self.dev)
            self.pre_ctx = _lib.Context(self.dev.index)          # its own workspace arena: the resize tables of the prefetch
        return self.pre_stream

    def prefetch_begin(self):
        """-> (slot, stream): everything the caller enqueues on `stream` until prefetch_end() -- host-to-device copies of the
        next batch, load_rois(..., slot=slot), the label copy into tgt_bufs[slot] -- runs beside the step in flight.  The side
        stream first waits until the last step that read this slot has finished."""
        self.prefetch_stream()
        slot = 1 - self.in_slot
        if self.ev_free[slot] is not None:
            self.pre_stream.wait_event(self.ev_free[slot])
        return slot, self.pre_stream

    def prefetch_end(self, slot):
        ev = torch.cuda.Event()
        ev.record(self.pre_stream)
        self.ev_ready[slot] = ev
        self.prefetched = slot

    def use_prefetched(self):
        """make the prefetched slot the current one: the caller's stream waits for its preprocessing; the slot just left is
        marked busy until everything enqueued so far (the step that read it) has finished."""
        slot = self.prefetched
        if slot is None:
            raise RuntimeError('use_prefetched: nothing was prefetched')
        cur = torch.cuda.current_stream(self.dev)
        ev = torch.cuda.Event()
        ev.record(cur)
        self.ev_free[self.in_slot] = ev
        cur.wait_event(self.ev_ready[slot])
        self._select_slot(slot)
        self.prefetched = None
        return slot

    def activation_bytes(self):
        tot = sum(t.numel() * t.element_size() for t in self.act.values())
        tot += sum(t.numel() * t.element_size() for t in self.grad.values())
        return tot + sum(t.numel() for t in self.draw) * self.esize

    # ------------------------------------------------------------------ descriptors
    def _conv_desc(self, n, N):
        if (n.R * n.S > 1 and n.R == n.x.H and n.S == n.x.W and n.ph == 0 and n.pw == 0 and n.P == 1 and n.Q == 1
                and n.x.is_full and n.Cw == n.x.C):
            # the filter covers the whole input (inception AuxLogits.conv1, 5x5 on 5x5): a plain GEMM.  Lower it as a
            # 1x1 conv over the flattened pixel -- KRSC weights and NHWC activations already have that layout -- so
            # dgrad does not walk 25 taps of which one is valid per pixel
            CC = n.R * n.S * n.x.C
            return ConvDesc(N, 1, 1, CC, CC, n.K, 1, 1, 1, 1, 0, 0, 1, 1, n.y.buf.C, CC, self.cdtype)
        return ConvDesc(N, n.x.H, n.x.W, n.x.C, n.x.buf.C, n.K, n.R, n.S, n.sh, n.sw, n.ph, n.pw, n.P, n.Q,
                        n.y.buf.C, n.Cw, self.cdtype)

    def zeros_k(self, K):
        z = getattr(self, '_zeros_k', None)
        if z is None or z.numel() < K:
            z = self._zeros_k = torch.zeros(max(K, 4096), dtype=torch.float32, device=self.dev)
        return z

    def _pack_desc(self, n, d):
        """weight_pack of a layer whose output channels were padded (squeezenet's classifier conv): only the true rows exist in
        the fp32 master; the shadow rows behind them stay zero"""
        if n.K_real == n.K:
            return d
        dp = ConvDesc.from_buffer_copy(d)
        dp.K = n.K_real
        return dp

    def _group_desc(self, g, N):
        x = g.x
        return ConvDesc(N, x.H, x.W, x.C, x.buf.C, g.Ktot, 1, 1, 1, 1, 0, 0, x.H, x.W, g.Ktot, x.C, self.cdtype)

    def _aptr(self, view, grad=False):
        t = (self.grad if grad else self.act)[view.buf.id]
        return _vp(t, self.esize * view.coff)

    def _pptr(self, key, which='P'):
        o = self.poff[key][0]
        return _vp(getattr(self, which), 4 * o)

    def _stat(self, n, k):
        return _vp(self.stats, 4 * (n.st_off + k * n.st_ld))

    def _raw_ptr(self, n):
        """(pointer, pixel stride) of a conv's raw output -- a channel slice of the merged tensor for fused siblings"""
        if n.group is not None and n.cpool is None:
            return _vp(n.group.raw, self.esize * n.koff), n.group.Ktot
        return _vp(self.act[n.raw.id]), n.K

    def _pre_ptr(self, n):
        """a commuted pool branch's unpooled 1x1-conv output: its channel slice of the sibling GEMM's merged tensor"""
        return _vp(n.group.raw, self.esize * n.koff), n.group.Ktot

    # ------------------------------------------------------------------ programs
    def plan(self, N):
        if N > self.max_batch:
            raise RuntimeError('batch %d exceeds the engine capacity %d' % (N, self.max_batch))
        key = (N, self.in_slot, self.in_kind[self.in_slot])
        if key not in self._plans:
            self._plans[key] = PlanBuilder(self, N).build()
            self._plans[key].dispatch_env = _dispatch_env()
        pl = self._plans[key]
        if pl.dispatch_env != _dispatch_env():
            # the library picks its conv kernels per launch from these switches, while the rows of the BatchNorm partial sums (and
            # the workspace) were sized when the plan was built: a change in between would make bn_finalize sum the wrong rows
            raise RuntimeError('a kernel-dispatch switch (%s) changed after the plan for batch %d was built: build a new model/engine '
                               'instead' % (', '.join(k for k, v in zip(_DISPATCH_SWITCHES, pl.dispatch_env) if os.environ.get(k) != v), N))
        return pl

    def _pack_multi(self, pack, key=None):
        """fold the per-conv weight_pack ops into ONE multi-tensor launch (device-side item table, built once per ``key``:
        None = every conv of the network, (lo, hi) = the convs of one optimizer bucket)."""
        import numpy as np
        cache = self.__dict__.setdefault('_pack_tables', {})
        if key not in cache:
            items = (_lib.PackItem * len(pack.ops))()
            blk = 0
            for k, o in enumerate(pack.ops):
                d = o.u.conv
                it = items[k]
                it.w_master, it.w, it.wT = o.p[_PACK_W_MASTER], o.p[_PACK_W], o.p[_PACK_WT]
                it.K, it.RS, it.C, it.Cw = d.K, d.R * d.S, d.C, d.Cw
                it.wT_ld = int(o.i[_PACK_WT_LD])
                it.first_block = blk
                blk += ((d.K + 31) // 32) * d.R * d.S * ((d.C + 31) // 32)      # 32x32 (k, c) tiles per filter tap
            raw = np.frombuffer(bytes(items), dtype=np.uint8).copy()
            cache[key] = (torch.from_numpy(raw).to(self.dev), len(pack.ops), blk)
        tab, n, blocks = cache[key]
        if key is None:
            self._pack_items, self._pack_n, self._pack_blocks = tab, n, blocks
        out = OpList()
        out.add(_lib.OP_WEIGHT_PACK_MULTI, 'weight_pack' + ('' if key is None else '[%d:%d]' % key), p=(_vp(tab),),
                i=(n, blocks, self.cdtype))
        return out

    def _op_param_offsets(self, o):
        """element offsets (into the flat gradient buffer) of the parameter tensors a backward op writes."""
        base, slots = self.G.data_ptr(), ops.PARAM_GRADS.get(o.kind, ())
        # the counted kinds: as many gradients as the group has members, one per segment in use
        if o.kind == _lib.OP_CONV_WGRAD_GROUP:
            slots = slots[:int(o.i[_GROUP_N])]
        elif o.kind == _lib.OP_CONV_WGRAD_SEG:
            slots = [s for s, k in zip(slots, _SEG_K) if o.i[k] > 0]
        offs = [(o.p[s] - base) // 4 for s in slots if o.p[s]]
        # (a vgg*_bn conv's bias rides with its BatchNorm's gradients, the first of which cbias_after is keyed by: nothing writes it -- the
        # batch mean absorbs the bias, its gradient is identically zero -- but the bucket plan must see the whole flat buffer covered)
        return offs + self.cbias_after.get(offs[0], []) if offs else offs

    def ddp_segments(self, pl, nseg=8):
        """split the backward list into <= nseg runs whose finished gradients form a contiguous tail
        [lo, prev_lo) of the flat buffer, so each run's all-reduce can start while later runs compute."""
        if pl.ddp_segs is not None:
            return pl.ddp_segs
        from .dp import segment_plan
        padded = self.palloc
        ops = pl.bwd_list.ops
        segs = []
        for (b0, b1, lo, hi) in segment_plan([self._op_param_offsets(o) for o in ops], padded, self.nparam_padded, nseg):
            segs.append((Program(pl.bwd_list.slice(b0, b1)), b1, lo, hi))
        pl.ddp_segs = segs
        return segs

    def train_step_ddp(self, N, world, all_reduce, mark=None):
        """data-parallel step: gradient all-reduce (sum) of each finished tail bucket is launched right after
        the backward segment that completes it and overlaps the remaining backward; Adam divides by world."""
        self._check_train_batch(N)
        if int(world) != self.dp_world and 'IFCBK_LANES' not in os.environ:
            raise RuntimeError('train_step_ddp(world=%d): this engine chose its program lanes for world %d (built before the process '
                               'group existed and without WORLD_SIZE?); pass dp_world=%d to Engine or set IFCBK_LANES'
                               % (int(world), self.dp_world, int(world)))
        if self.accumulate > 1:
            return self._acc_step(N, int(world), all_reduce, mark, ddp=True)
        pl = self.plan(N)
        self.ensure_packed(pl)
        self.make_dropout_mask(N)
        self._ema_begin_step()
        self.run(pl.fwd_loss)
        from .dp import run_overlapped
        run_overlapped(self.ddp_segments(pl), lambda seg: self.run(seg[0]), self.G, all_reduce, mark)
        self.step_count += 1
        # with clipping the op takes its norm over the REDUCED buffer with this grad_scale, i.e. the norm of the averaged gradient: every
        # rank holds the same bits of G behind the all-reduce, so every rank computes the same coefficient and no collective is needed
        self._set_update(pl.adam_pack.arr[0], 1.0 / world)
        self.run(pl.adam_pack)                    # (Adam, repack, and the step's counters: nbt += 1, loss_sum += loss)
        self._ema_end_step()
        self.eval_stats_ready = False
        return pl

    # ------------------------------------------------------------------ lifetime
    def close(self):
        """destroy every captured graph of this engine, then its library context (arenas, lane streams, events).  The library
        enforces the same order by itself (a ctx owns its graphs); doing it here keeps the handles in ``pl.graphs`` from dangling."""
        ctx = getattr(self, 'ctx', None)
        if ctx is None or getattr(ctx, 'h', None) is None:
            return
        for pl in getattr(self, '_plans', {}).values():
            for g in pl.graphs.values():
                ctx.lib.ifcbk_graph_destroy(ctx.h, g)
            pl.graphs.clear()
        for c in (getattr(self, 'pre_ctx', None), ctx):
            if c is not None:
                c.close()

    def plan_graph_handles(self):
        return [g for pl in self._plans.values() for g in pl.graphs.values()]

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ execution
    def stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)

    def run(self, prog, op_ms=None):
        self.ctx.run_program(prog.arr, prog.n, self.stream(), op_ms)

    def replay(self, pl, name):
        """run program ``name`` of plan ``pl`` as a hipGraph (captured on first use: all lanes, with their fork / wait /
        join edges); buffers are static per plan, so the baked pointers stay valid."""
        g = pl.graphs.get(name)
        if g is None:
            prog = getattr(pl, name)
            g = pl.graphs[name] = self.ctx.capture(prog.arr, prog.n)
        self.ctx.graph_launch(g, self.stream())

    def ensure_packed(self, pl):
        if not self.packed:
            self.run(pl.pack)
            self.packed = True

    def load_input_nchw(self, x):
        """fp32 NCHW [N,3,S,S] (device) -> the plan's NHWC bf16 input buffer (+ [TV] transform_input)."""
        N, Cc, H, W = x.shape
        S = self.net.S
        if Cc != 3 or H != S or W != S:
            raise RuntimeError('expected input [N,3,%d,%d], got %s' % (S, S, tuple(x.shape)))
        x = x.to(device=self.dev, dtype=torch.float32).contiguous()
        sc = sh = None
        if self.net.transform_input:
            sc = (C.c_float * 3)(0.229 / 0.5, 0.224 / 0.5, 0.225 / 0.5)
            sh = (C.c_float * 3)((0.485 - 0.5) / 0.5, (0.456 - 0.5) / 0.5, (0.406 - 0.5) / 0.5)
        self.ctx.call('ifcbk_nchw_to_nhwc', _vp(x), N, 3, S, S, 8, self.cdtype, sc, sh, _vp(self.act[self.net.input.id]),
                      self.stream())
        self.in_kind[self.in_slot] = 'nhwc'
        return N

    def load_rois(self, pixels, offs, hs, ws, max_h, max_w, in_channels=1, flips=None, mean=None, std=None, slot=None, turn=False, pad=None,
                  jitter=None, blur=None):
        """ragged u8 ROIs (device tensors) -> input buffer via the PIL-exact resize kernel.  slot: the input slot of a
        prefetch (runs on the prefetch stream with the prefetch context's workspace); None = the current slot, current stream.
        turn: the codes in ``flips`` may hold bit 2 = transpose (TRAIN --rot90; neuston_data.fold_turns).
        pad: None = squash to S x S (ifcbk_roi_preprocess); 'border' or a level 0..255 = keep the aspect ratio and fill the rest
        (TRAIN --pad; ifcbk_roi_preprocess_fit).
        jitter: None, or (brightness, contrast): float32 device tensors of one factor per ROI, either may be None (TRAIN --jitter).
        ifcbk_roi_jitter then maps the ROIs IN PLACE ahead of the resize, on the same ctx and stream: ``pixels`` is overwritten
        with the jittered ROIs.
        blur: None, or a float32 device tensor of one sigma per ROI, 0 = leave the image alone (TRAIN --blur).  ifcbk_batch_blur then
        blurs the RESIZED batch in place with the engine's ``blur_radius``, behind the resize on the same ctx and stream, on whichever
        buffer the resize wrote (the u8 plane or the dense tensor), so plans and captured graphs keep their addresses; a ``mix_batch``
        of the slot comes after it.  Without ``blur`` nothing more is launched."""
        n = hs.numel()
        if blur is not None:
            if self.blur_radius is None:
                raise RuntimeError('load_rois(blur=): this engine was built without blur_radius')
            _per_roi_f32(blur, n, pixels.device, 'blur: a float32 tensor of %d sigmas on %s, or None')
        target = self._slot_target(slot)
        ctx, stream, _, s, _ = target
        self._load_rois_into(target, pixels, offs, hs, ws, max_h=max_h, max_w=max_w, in_channels=in_channels, flips=flips, mean=mean,
                             std=std, turn=turn, pad=pad, jitter=jitter)
        if blur is not None:
            buf, kind = self._slot_image(s)
            ctx.call('ifcbk_batch_blur', _vp(buf), kind, n, self.net.S, _vp(blur), self.blur_radius, stream)
        return n

    def _slot_target(self, slot):
        """where a call on an input slot runs -> (ctx, stream handle, torch stream, slot, main).  slot None: the current slot, on the
        engine's own context and the current stream (main = True); else a prefetch slot, on the prefetch context and stream"""
        if slot is not None:
            return self.pre_ctx, C.c_void_p(self.pre_stream.cuda_stream), self.pre_stream, slot, False
        cur = torch.cuda.current_stream(self.dev)
        return self.ctx, C.c_void_p(cur.cuda_stream), cur, self.in_slot, True

    def _slot_image(self, s):
        """(buf, kind) of the batch in input slot ``s`` for the in-place batch kernels: whichever buffer the slot's load wrote, the u8
        plane or the dense tensor"""
        if self.in_kind[s] == 'u8':
            return self.in_u8[s], _lib.MIX_U8
        return self.in_bufs[s], self.cdtype

    def _load_rois_into(self, target, pixels, offs, hs, ws, *, max_h, max_w, in_channels, flips, mean, std, turn, pad, jitter):
        """the body of ``load_rois`` on a ``_slot_target``: workspace growth, the in-place jitter, the resize"""
        ctx, stream, tstream, slot, main = target
        n = hs.numel()
        d, fn, fill = _lib.roi_resize(n, self.net.S, in_channels, self.cdtype, flips, turn, mean, std, self.net.transform_input, pad)
        need = getattr(ctx.lib, fn + '_workspace')(C.byref(d), int(max_h), int(max_w))
        if jitter is not None and jitter[0] is None and jitter[1] is None:
            jitter = None
        if jitter is not None:
            for f in jitter:
                if f is not None:
                    _per_roi_f32(f, n, pixels.device, 'jitter: (brightness, contrast) are float32 tensors of %d factors on %s, or None')
            need = max(need, ctx.lib.ifcbk_roi_jitter_workspace(n))
        if need > ctx.lib.ifcbk_ctx_workspace_bytes(ctx.h):
            if not main:
                self.pre_stream.synchronize()        # an earlier prefetch may still read the arena that is about to move
            self._grow_workspace(ctx, need)              # (the engine's own ctx: graphs captured so far hold stale pointers and go)
        if jitter is not None:
            # in place on the uploaded blob, stream-ordered in front of the resize (its sums lie where the resize puts its tables)
            ctx.call('ifcbk_roi_jitter', _vp(pixels), _vp(offs), _vp(hs), _vp(ws), n, int(in_channels), int(max_h), int(max_w),
                     _vp(jitter[0]), _vp(jitter[1]), _vp(pixels), stream)
        u8 = self.stem_u8 is not None and in_channels == 1
        if u8:
            # grey ROIs: only the resized u8 plane is written; x_c = a_c * g + b_c (ToTensor, Normalize, transform_input) goes to the
            # stem conv as six floats
            ab = tuple(d.tin_scale[k] / (255.0 * d.std[k]) for k in range(3)) + \
                tuple(d.tin_shift[k] - d.tin_scale[k] * d.mean[k] / d.std[k] for k in range(3))
            if self._in_ab_host[slot] != ab:
                with torch.cuda.stream(tstream):
                    self.in_ab[slot].copy_(torch.tensor(ab, dtype=torch.float32), non_blocking=False)
                self._in_ab_host[slot] = ab
        ctx.call(fn, C.byref(d), _vp(pixels), _vp(offs), _vp(hs), _vp(ws), _vp(flips), int(max_h), int(max_w), *fill,
                 None if u8 else _vp(self.in_bufs[slot]), _vp(self.in_u8[slot]) if u8 else None, stream)
        self.in_kind[slot] = 'u8' if u8 else 'nhwc'

    def mix_batch(self, n, lam, box=None, slot=None):
        """mix the ``n`` loaded images of an input slot with their reverse, in place (TRAIN --mixup / --cutmix; timm's Mixup, batch mode):
        image i becomes lam[i] x[i] + (1 - lam[i]) x[n - 1 - i] outside ``box`` and x[n - 1 - i] inside it, and the factors go to the
        slot's ``mix_lam``, which the train loss ops read.  lam: a float32 device tensor of n factors in [0, 1], or a python float for
        all n.  box: None (no cut) or (y0, y1, x0, x1) in pixels of the S x S input.  slot: as ``load_rois`` -- None is the current
        slot on the current stream, a prefetch slot runs on the prefetch stream and context, right behind its resize."""
        if not self.mix:
            raise RuntimeError('mix_batch: this engine was built without mix=True')
        n = int(n)
        if not 1 <= n <= self.max_batch:
            raise ValueError('mix_batch: n %d outside 1..%d' % (n, self.max_batch))
        ctx, stream, tstream, s, _ = self._slot_target(slot)
        y0, y1, x0, x1 = (0, 0, 0, 0) if box is None else (int(v) for v in box)
        with torch.cuda.stream(tstream):
            if torch.is_tensor(lam):
                if not (lam.dtype == torch.float32 and lam.device == self.dev and lam.numel() == n):
                    raise ValueError('mix_batch: lam is a float32 tensor of %d factors on %s, or a python float' % (n, self.dev))
                self.mix_lam[s][:n].copy_(lam.reshape(n), non_blocking=True)
            else:
                self.mix_lam[s][:n].fill_(float(lam))
        buf, kind = self._slot_image(s)
        ctx.call('ifcbk_batch_mix', _vp(buf), kind, n, self.net.S, _vp(self.mix_lam[s]), y0, y1, x0, x1, stream)
        return n

    # the views of test-time augmentation (RUN --tta) as walks over ifcbk_batch_sym's ops: every step turns the batch into a view not seen
    # before.  'flips': e, H, VH, V (one more V restores the batch); 'all': with T the transpose, H after T is a quarter turn, so the
    # alternating walk passes through all eight symmetries of the square (one more H restores)
    TTA_WALKS = {'flips': (_lib.SYM_HFLIP, _lib.SYM_VFLIP, _lib.SYM_HFLIP),
                 'all': (_lib.SYM_TRANSPOSE, _lib.SYM_HFLIP) * 3 + (_lib.SYM_TRANSPOSE,)}

    def sym_batch(self, n, op, slot=None):
        """apply one symmetry (``_lib.SYM_HFLIP`` / ``SYM_VFLIP`` / ``SYM_TRANSPOSE``) to the ``n`` loaded images of an input slot, in
        place on whichever buffer the slot's load wrote (the u8 plane or the dense tensor): the plans of the slot, and the graphs
        captured from them, go on reading the same pointers.  slot: as ``mix_batch`` -- None is the current slot on the current
        stream, a prefetch slot runs on the prefetch stream and context."""
        n = int(n)
        if not 1 <= n <= self.max_batch:
            raise ValueError('sym_batch: n %d outside 1..%d' % (n, self.max_batch))
        ctx, stream, _, s, _ = self._slot_target(slot)
        buf, kind = self._slot_image(s)
        ctx.call('ifcbk_batch_sym', _vp(buf), kind, n, self.net.S, int(op), stream)
        return n

    def softmax_acc(self, N, first, scale=1.0):
        """softmax of the main head's logits of the last forward at batch ``N``, added into ``probs`` (``first``: stored instead) and
        the sum scaled by ``scale`` (ifcbk_softmax_acc), on the current stream.  No op kind, no program: a direct call."""
        main = [h for h in self.heads if not h.aux][0]
        self.ctx.call('ifcbk_softmax_acc', _vp(main.logits), int(N), self.net.NC, _vp(self.probs), 0 if first else 1, float(scale),
                      self.stream())

    def make_dropout_mask(self, N):
        ext = self.external_mask
        for h in self.heads:
            if h.dropout:
                if ext is not None and not isinstance(ext, dict):
                    h.mask[:N].copy_(ext[:N].to(torch.uint8))
                elif isinstance(ext, dict) and h.name in ext:
                    h.mask[:N].copy_(ext[h.name][:N].to(torch.uint8))
                else:
                    self.ctx.call('ifcbk_dropout_mask', _vp(h.mask), N * h.C, 0.5, self.dropout_seed,
                                  self.dropout_calls * (1 << 24), self.stream())
        for k, n in enumerate(self.drops):
            # nn.Dropout layers of a classifier stack (alexnet / vgg / squeezenet): one keep-mask per layer and step; a parity
            # test hands masks over as {node name: [B, H*W*C] in NHWC element order}
            if isinstance(ext, dict) and n.name in ext:
                n.mask[:N].copy_(ext[n.name][:N].reshape(N, -1).to(torch.uint8))
            else:
                self.ctx.call('ifcbk_dropout_mask', _vp(n.mask), N * n.mask.shape[1], float(n.p),
                              self.dropout_seed + 0x9E3779B1 * (k + 1), self.dropout_calls * (1 << 26), self.stream())
        self.dropout_calls += 1

    def _check_train_batch(self, N):
        if N > self.train_batch and N <= self.window_batch:
            raise RuntimeError('batch %d > %d: this engine was built for inference (train_batch=%d): its gradient buffers hold %d image(s)'
                               % (N, self.train_batch, self.train_batch, self.train_batch))
        if N > self.window_batch:
            raise RuntimeError('batch %d > %d: the 2 GiB buffer-descriptor window holds %d images of this network per launch, and '
                               'BatchNorm batch statistics cannot be taken over chunks: use a smaller --batch per GPU (more GPUs), or '
                               'a larger effective batch on the same GPUs with accumulate=K (TRAIN --accumulate K)'
                               % (N, self.window_batch, self.window_batch))

    def forward_train(self, N):
        self._check_train_batch(N)
        pl = self.plan(N)
        self.ensure_packed(pl)
        self.make_dropout_mask(N)
        self._ema_begin_step(update=False)
        self.run(pl.fwd_train)
        self.nbt += 1
        self.eval_stats_ready = False
        return pl

    def forward_eval(self, N):
        pl = self.plan(N)
        self.ensure_packed(pl)
        if not self.eval_stats_ready:
            self.run(pl.evalprep)
            self.eval_stats_ready = True
        if self.graph_eval:
            self.replay(pl, 'fwd_eval')
        else:
            self.run(pl.fwd_eval)
        return pl

    def backward(self, N):
        self._check_train_batch(N)
        self.run(self.plan(N).bwd)

    def _set_update(self, op, grad_scale=1.0):
        """per-step scalars of the optimizer op: the step count (Adam's bias correction), the gradient scale (1/world), with a weight
        average the weight of this step's update (_ema_begin_step), and with a schedule this step's learning rate: a function of the
        step count alone, so every way of launching a step, at any batch size and after any load, carries the same rate"""
        op.i[self._upd_step] = self.step_count
        op.f[self._upd_scale] = grad_scale
        if self.lr_schedule is not None:
            op.f[self._upd_lr] = self.lr_schedule.at(self.step_count - 1)
        if self.ema_decay is not None:
            op.f[self._upd_ema_w] = self._ema_w

    @property
    def lr_now(self):
        """the learning rate of the last optimizer step as the op carried it (ahead of the first: of the first); ``lr`` stays the base"""
        if self.lr_schedule is None:
            return self.lr
        return C.c_float(self.lr_schedule.at(max(self.step_count, 1) - 1)).value

    def adam_step(self, N):
        pl = self.plan(N)
        self.step_count += 1
        self._ema_begin_step()
        self._set_update(pl.adam.arr[0])
        self.run(pl.adam)
        self._ema_end_step()
        self.packed = False
        self.eval_stats_ready = False

    def train_step(self, N, op_ms=None, ev_slot=None, ev_arr=None):
        """one fused launch list: fwd + CE(+0.4 aux) + bwd + Adam + weight repack; loss stays on device."""
        self._check_train_batch(N)
        if self.accumulate > 1:
            if op_ms is not None or ev_slot is not None or ev_arr is not None:
                raise RuntimeError('train_step: per-op timing (op_ms / ev_slot) of an accumulating engine (accumulate=%d) is not supported: '
                                   'the step is several launch lists; time an engine built with accumulate=1' % self.accumulate)
            return self._acc_step(N)
        pl = self.plan(N)
        self.ensure_packed(pl)
        self.make_dropout_mask(N)
        self.step_count += 1
        self._ema_begin_step()
        for j in pl.step_adam_idxs:
            self._set_update(pl.step.arr[j])
        if ev_slot is not None:
            # ev_arr: pl.step.timed(...) -- which ops to bracket with HIP events (default: all)
            if ev_arr is None:
                if getattr(pl, 'step_timed_all', None) is None:
                    pl.step_timed_all = pl.step.timed()
                ev_arr = pl.step_timed_all
            for j in pl.step_adam_idxs:
                self._set_update(ev_arr[j])
            self.ctx.call('ifcbk_run_program_ev', ev_arr, pl.step.n, self.stream(), int(ev_slot))
        elif self.graph_train and op_ms is None:
            # fwd + loss + bwd replayed as one hipGraph; Adam (its step count is a launch argument) + repack stay plain launches
            self.replay(pl, 'fwd_bwd')
            self._set_update(pl.adam_pack.arr[0])
            self.run(pl.adam_pack)
        else:
            self.ctx.run_program(pl.step.arr, pl.step.n, self.stream(), op_ms)
        self._ema_end_step()
        # (nbt += 1 and loss_sum += loss are the step's last op: no framework kernel between load_rois and the end of a step)
        self.eval_stats_ready = False
        return pl

    # ------------------------------------------------------------------ gradient accumulation (TRAIN --accumulate)
    def accumulate_discard(self):
        """drop an open window without applying it (init_weights, load_state_dict): the next batch opens a new one and overwrites A"""
        self.acc_pending = 0
        self._acc_plan = None

    def _acc_add(self, lo, hi, first):
        """A[lo:hi] = G[lo:hi] (first) or A[lo:hi] + G[lo:hi], behind the backward ops that finished that slice, on their stream; lo is
        the offset of a parameter tensor, a multiple of 4 elements"""
        self.ctx.call('ifcbk_grad_accum_flat', _vp(self.A, 4 * lo), _vp(self.G, 4 * lo), hi - lo, 1 if first else 0, self.stream())

    def _acc_step(self, N, world=1, all_reduce=None, mark=None, ddp=False):
        """one batch of an accumulating engine (train_step; ddp: train_step_ddp): forward, loss and backward at batch N -- the batches of
        a window may differ in N --, G summed into A, the batch's counters (nbt += 1, loss_sum += loss), and behind the K-th batch of the
        window its one update.  Data parallel: no collective until the window's last batch, whose backward runs in the bucket segments;
        each finished slice is accumulated and A's slice exchanged beside the rest of backward"""
        K = self.accumulate
        pl = self.plan(N)
        self.ensure_packed(pl)
        self.make_dropout_mask(N)
        self._ema_begin_step(update=False)            # (E = P, ERB = RB as they stand ahead of the window's first forward)
        first, last = self.acc_pending == 0, self.acc_pending + 1 == K
        if ddp and last:
            from .dp import run_overlapped

            def segment(seg):
                self.run(seg[0])
                self._acc_add(seg[2], seg[3], first)
            self.run(pl.fwd_loss)
            run_overlapped(self.ddp_segments(pl), segment, self.A, all_reduce, mark)
        else:
            if self.graph_train and not ddp:
                self.replay(pl, 'fwd_bwd')
            else:
                self.run(pl.fwd_loss)
                self.run(pl.bwd)
            self._acc_add(0, self.nparam_padded, first)
        self.run(pl.acc_count)
        self.acc_pending += 1
        self._acc_plan = pl
        if last:
            self._acc_apply(1.0 / (K * world))
        self.eval_stats_ready = False
        return pl

    def _acc_apply(self, grad_scale):
        """the window's optimizer step, from A times grad_scale: the step count, the schedule's rate, the weight average, the clip norm
        (taken over A) and its figures count optimizer steps"""
        pl = self._acc_plan
        self.step_count += 1
        self._ema_begin_step()
        self._set_update(pl.acc_update.arr[0], grad_scale)
        self.run(pl.acc_update)                       # (the optimizer over A, then the whole repack)
        self._ema_end_step()
        self.accumulate_discard()

    def accumulate_flush(self, world=1, all_reduce=None):
        """apply an open window that holds fewer than K batches (the end of an epoch), still scaled by 1 / K as Lightning does; nothing
        on a closed window.  Data parallel (all_reduce given): the whole of A is exchanged in one call ahead of the update.  -> whether
        an optimizer step was taken"""
        if self.acc_pending == 0:
            return False
        if all_reduce is not None:
            work = all_reduce(self.A)
            if work is not None:
                work.wait()
        self._acc_apply(1.0 / (self.accumulate * world))
        self.eval_stats_ready = False
        return True
