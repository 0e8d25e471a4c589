"""Parity of the HIP backbone with the CPU oracle on identical weights, inputs and dropout mask.

Train mode: random-init BatchNorm networks are chaotic (the fp32 oracle itself moves its logits by 1.6e-4
for a 1e-6 input perturbation, and by 0.14 rel under bf16 storage), so every node of the plan is checked
locally against oracle/ops.py on the HIP path's own inputs -- forward, backward, all parameter gradients --
and the end-to-end distance is bounded by the oracle's own bf16-vs-fp32 distance.  Eval mode (fixed
statistics) is not chaotic and is compared end to end."""
import pytest
import torch
import torch.nn.functional as F

from local_parity import check_plan, rel

pytestmark = pytest.mark.gpu


def _pair(name, nc, B, storage='bf16', seed=0):
    from ifcb_classifier_amd.neuston_models import get_namebrand_model
    from oracle import tv_models
    torch.manual_seed(seed)
    hip = get_namebrand_model(name, nc, max_batch=B)
    sd = {k: v.detach().cpu().clone() for k, v in hip.state_dict().items()}
    ora = tv_models.get_namebrand_model(name, nc, storage=storage)
    ora.load_state_dict(sd, strict=True)
    return hip, ora


def _loss(out, y):
    if isinstance(out, tuple):
        return F.cross_entropy(out[0], y) + 0.4 * F.cross_entropy(out[1], y)
    return F.cross_entropy(out, y)


# last column: IFCBK_FUSE_BNSTAT -- BatchNorm-backward sums in dgrad epilogues off (0); None = the default (1, layers with one
# producer and one consumer)
@pytest.mark.parametrize('name,nc,B,S,fuse', [('inception_v3', 10, 4, 299, None), ('resnet18', 2, 6, 224, None),
                                              ('resnet50', 3, 4, 224, None), ('resnet34', 5, 3, 224, None),
                                              ('inception_v3', 10, 4, 299, '0')])
def test_train_step_local_parity(name, nc, B, S, fuse, monkeypatch):
    if fuse is not None:
        monkeypatch.setenv('IFCBK_FUSE_BNSTAT', fuse)
    hip, ora = _pair(name, nc, B)
    if name == 'inception_v3':
        from ifcb_classifier_amd import _lib
        prog = hip.engine.plan(B).step
        kinds = [prog.arr[k].kind for k in range(prog.n)]
        one, retired = kinds.count(_lib.OP_CONV_DGRAD_BNSTAT), kinds.count(_lib.OP_RETIRED_31)
        print('IFCBK_FUSE_BNSTAT', fuse, 'one-producer fusions', one)
        assert retired == 0 and (one == 0 if fuse == '0' else one > 0)      # (31: the retired table fusion, never planned)
    x = torch.rand(B, 3, S, S)
    y = torch.randint(0, nc, (B,))
    mask = None
    if name == 'inception_v3':
        mask = torch.rand(B, 2048) > 0.5
        hip.set_dropout_mask(mask.cuda())
        ora.dropout_mask = mask
    hip.train()
    out_h = hip(x.cuda())
    loss_h = _loss(out_h, y.cuda())
    loss_h.backward()
    worst = check_plan(hip, B, mask)
    print(name, 'node-local worst rel errors:', {k: '%.2e' % v for k, v in worst.items()})
    assert worst['raw'] < 3e-3 and worst['y'] < 3e-3 and worst['pool'] < 3e-3
    # pool branch run as avgpool(conv1x1(x)): the two bf16 roundings sit at other places than in the oracle's reference order
    assert worst['raw_cp'] < 6e-3 and worst['dW_cp'] < 2e-2
    assert worst['stats'] < 1e-4
    assert worst['head'] < 1e-4
    assert worst['dW'] < 1e-2 and worst['dgamma'] < 1e-2 and worst['dbeta'] < 1e-2
    assert worst['dx'] < 1.5e-2
    # global: same loss within the oracle's own bf16-vs-fp32 sensitivity
    ora.train()
    loss_o = _loss(ora(x), y)
    print('loss hip %.5f oracle(bf16 storage) %.5f' % (loss_h.item(), loss_o.item()))
    assert abs(loss_h.item() - loss_o.item()) < 0.1 * abs(loss_o.item())
    # BN bookkeeping
    for k, b in hip.named_buffers():
        if k.endswith('num_batches_tracked'):
            assert int(b.item()) == 1


@pytest.mark.parametrize('name,nc,B,S', [('inception_v3', 10, 4, 299), ('resnet18', 2, 6, 224), ('resnet50', 3, 4, 224)])
def test_eval_forward_end_to_end(name, nc, B, S):
    hip, ora = _pair(name, nc, B)
    x = torch.rand(B, 3, S, S)
    # calibrate running statistics to this batch (momentum 1) so eval activations stay O(1)
    for m in ora.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = 1.0
    ora.train()
    with torch.no_grad():
        ora(x)
    hip.load_state_dict(ora.state_dict())
    hip.eval(); ora.eval()
    with torch.no_grad():
        eo = ora(x)
        eh = hip(x.cuda()).cpu()
    ob = {k: v for k, v in ora.state_dict().items()}
    from oracle import tv_models
    o32 = tv_models.get_namebrand_model(name, nc, storage='fp32')
    o32.load_state_dict(ob)
    o32.eval()
    with torch.no_grad():
        e32 = o32(x)
    r, r32 = rel(eh, eo), rel(eh, e32)
    print(name, 'eval logits rel vs bf16-storage oracle %.3e, vs fp32 oracle %.3e (oracle bf16 vs fp32 %.3e)'
          % (r, r32, rel(eo, e32)))
    # random-init logits are ill-conditioned under ANY bf16 storage (oracle bf16 vs fp32: 0.28 inception,
    # 0.04 resnet18); the HIP path must sit well inside that envelope and next to the bf16-storage oracle
    # (0.5: the Inception pool branches run as avgpool(conv1x1(x)) -- the same linear map as the oracle's conv1x1(avgpool(x)) with
    # two of the bf16 roundings at other places; every placement of the roundings is one draw from the same envelope.  The
    # fp32 parity mode below pins the arithmetic itself to 1e-3.)
    assert r < 0.5 * rel(eo, e32) + 2e-3
    assert r32 < 1.25 * rel(eo, e32) + 2e-3


def test_fused_step_equals_autograd_surface_and_adam_oracle():
    """fit_batch (one fused HIP program) == reference-style training_step + torch Adam on the same model."""
    from ifcb_classifier_amd.neuston_models import NeustonModel
    from oracle import ops as O
    import argparse
    B, nc = 4, 5
    hp = argparse.Namespace(MODEL='resnet18', classes=list('abcde'), pretrained=False, batch_size=B)
    torch.manual_seed(3)
    m = NeustonModel(hp)
    x = torch.rand(B, 3, 224, 224).cuda()
    y = torch.randint(0, nc, (B,)).cuda()
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    # reference-style: forward, loss, backward -> grads
    m.train()
    out = m.training_step((x, y, ['a'] * B), 0)
    out['loss'].backward()
    eng = m.model.engine
    g_ref = eng.G.clone()
    p0 = eng.P.clone()
    loss_ref = out['loss'].item()
    # restore, then fused step
    m.load_state_dict(sd0)
    eng.nbt.zero_(); eng.M.zero_(); eng.V.zero_(); eng.step_count = 0
    m.fit_batch(x, y)
    torch.cuda.synchronize()
    assert abs(eng.loss.item() - loss_ref) < 1e-5 * max(1, abs(loss_ref))
    # same forward bits; dlogits come from torch's CE backward on one side and the fused kernel on the other
    assert rel(eng.G, g_ref) < 1e-2
    g_ref = eng.G.clone()
    pn, mn, vn = O.adam_step(p0.cpu(), g_ref.cpu(), torch.zeros_like(p0).cpu(), torch.zeros_like(p0).cpu(), 1)
    assert rel(eng.P.cpu(), pn) < 1e-6
    assert (eng.P.cpu() - pn).abs().max().item() < 1e-6
    assert rel(eng.M.cpu(), mn) < 1e-6 and rel(eng.V.cpu(), vn) < 5e-5    # fma contraction vs addcmul_
    assert abs(m.epoch_train_loss() - loss_ref) < 1e-5 * max(1, abs(loss_ref))


def test_state_dict_keys_match_oracle():
    from ifcb_classifier_amd.neuston_models import get_namebrand_model
    from oracle import tv_models
    for name, nc in (('inception_v3', 100), ('resnet18', 2), ('resnet50', 5)):
        hip = get_namebrand_model(name, nc, max_batch=1)
        ora = tv_models.get_namebrand_model(name, nc)
        sh, so = hip.state_dict(), ora.state_dict()
        assert list(sh.keys()) == list(so.keys())
        for k in sh:
            assert tuple(sh[k].shape) == tuple(so[k].shape), k
        assert [k for k, _ in hip.named_parameters()] == [k for k, _ in ora.named_parameters()]
        del hip


def test_unknown_model_raises_keyerror():
    from ifcb_classifier_amd.neuston_models import get_namebrand_model
    with pytest.raises(KeyError, match='model unknown'):
        get_namebrand_model('efficientnet_b4', 10)


# ------------------------------------------------------------------------------------------------ fp32 parity mode
def _pair32(name, nc, B, seed=0):
    from ifcb_classifier_amd.neuston_models import get_namebrand_model
    from oracle import tv_models
    torch.manual_seed(seed)
    hip = get_namebrand_model(name, nc, max_batch=B, dtype='fp32')
    sd = {k: v.detach().cpu().clone() for k, v in hip.state_dict().items()}
    ora = tv_models.get_namebrand_model(name, nc, storage='fp32')
    ora.load_state_dict(sd, strict=True)
    return hip, ora


@pytest.mark.parametrize('name,nc,B,S', [('inception_v3', 10, 4, 299), ('resnet18', 2, 6, 224), ('resnet50', 3, 4, 224)])
def test_fp32_mode_meets_the_north_star_tolerance(name, nc, B, S):
    """fp32 storage + v_mfma_f32_16x16x4_f32: class logits within 1e-3 rel of the reference's fp32 CPU arithmetic
    (BASELINE.json north_star) in train AND eval mode and every plan node within 2e-5.  Two train steps, each
    started from the oracle's weights: Adam's first steps move a parameter by +-lr whatever the gradient's size, so
    a parameter whose gradient sits at rounding-noise level may legitimately step the other way and a chaotic
    random-init BatchNorm network then amplifies it -- trajectories are therefore re-synchronised per step; the
    Adam arithmetic itself is pinned bit-tight by test_gpu_ops / test_fused_step_*."""
    from oracle import ops as O
    hip, ora = _pair32(name, nc, B)
    incep = name == 'inception_v3'
    opt_o = torch.optim.Adam(ora.parameters(), lr=1e-3)
    opt_h = torch.optim.Adam(hip.parameters(), lr=1e-3)
    O.set_storage('fp32')
    g = torch.Generator().manual_seed(11)
    try:
        for step in range(2):
            x = torch.rand(B, 3, S, S, generator=g)
            y = torch.randint(0, nc, (B,), generator=g)
            mask = None
            if incep:
                mask = torch.rand(B, 2048, generator=g) > 0.5
                hip.set_dropout_mask(mask.cuda())
                ora.dropout_mask = mask
            ora.train(); hip.train()
            out_o = ora(x)
            out_h = hip(x.cuda())
            lo = out_o.logits if incep else out_o
            lh = out_h.logits if incep else out_h
            r = rel(lh.detach().cpu(), lo.detach())
            print(name, 'step', step, 'train logits rel vs fp32 oracle %.2e' % r)
            assert r < 1e-3
            if incep:
                assert rel(out_h.aux_logits.detach().cpu(), out_o.aux_logits.detach()) < 1e-3
            loss_o, loss_h = _loss(out_o, y), _loss(out_h, y.cuda())
            assert abs(loss_h.item() - loss_o.item()) < 1e-4 * abs(loss_o.item())
            opt_o.zero_grad(); opt_h.zero_grad()
            loss_o.backward(); loss_h.backward()
            worst = check_plan(hip, B, mask)
            print(name, 'fp32 node-local worst:', {k: '%.1e' % v for k, v in worst.items()})
            assert max(worst.values()) < 2e-5
            # end-to-end gradients (backward re-amplifies the 4e-5 forward distance through 47 BatchNorm layers)
            op = dict(ora.named_parameters())
            gr = max(rel(p.grad.cpu(), op[k].grad) for k, p in hip.named_parameters())
            print(name, 'end-to-end parameter gradients: worst tensor rel %.2e' % gr)
            assert gr < 5e-2
            opt_o.step(); opt_h.step()
            ob = dict(ora.named_buffers())
            for k, b in hip.named_buffers():
                if not k.endswith('num_batches_tracked'):
                    assert rel(b.cpu(), ob[k]) < 1e-4, k
            hip.load_state_dict(ora.state_dict())                 # re-synchronise weights for the next step / eval
            for po, ph in zip(ora.parameters(), hip.parameters()):
                st_o, st_h = opt_o.state[po], opt_h.state[ph]
                st_h['exp_avg'].copy_(st_o['exp_avg']); st_h['exp_avg_sq'].copy_(st_o['exp_avg_sq'])
        hip.eval(); ora.eval()
        with torch.no_grad():
            r = rel(hip(x.cuda()).cpu(), ora(x))
        print(name, 'eval logits rel vs fp32 oracle %.2e' % r)
        assert r < 1e-3
    finally:
        O.set_storage('bf16')


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,S', [('inception_v3', 6, 299), ('resnet18', 8, 224)])
def test_train_steps_are_bitwise_reproducible(name, B, S):
    """Two replicas from the same seed, fed the same batches, stay bit-identical over several fused steps: every reduction
    has a fixed order (no float atomics) and the program lanes are ordered by the static data flow.  (At this batch the lanes hardly
    overlap, so this run cannot be relied on to expose a missing dependency between lanes: tests/test_gpu_lane_order.py forces the
    timing, tests/test_program_footprints_cpu.py audits the schedule against the pointers of the op tables.)"""
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    engs = []
    for _ in range(2):
        eng = Engine(graph.build(name, 7, pretrained=False), device=0, max_batch=B)
        eng.init_weights(seed=4321)
        engs.append(eng)
    g = torch.Generator().manual_seed(5)
    for step in range(3):
        x = torch.rand(B, 3, S, S, generator=g)
        y = torch.randint(0, 7, (B,), generator=g)
        for eng in engs:
            eng.load_input_nchw(x.cuda())
            eng.target[:B].copy_(y)
            if eng.heads[0].dropout or any(h.dropout for h in eng.heads):
                eng.dropout_seed = 99          # same mask stream on both replicas
            eng.train_step(B)
        torch.cuda.synchronize()
        assert torch.equal(engs[0].loss, engs[1].loss), step
        assert torch.equal(engs[0].G, engs[1].G), step
        assert torch.equal(engs[0].P, engs[1].P), step
    assert torch.equal(engs[0].RB, engs[1].RB)


@pytest.mark.gpu
@pytest.mark.parametrize('name,B,S,lanes', [('inception_v3', 6, 299, '2'), ('resnet18', 8, 224, '2'), ('inception_v3', 6, 299, '4'),
                                             ('inception_v3', 6, 299, '3')])
def test_hipgraph_replay_equals_plain_launches(name, B, S, lanes, monkeypatch):
    """BASELINE config 4 asks for hipGraph-captured batches: the captured programs (eval forward; train forward + loss +
    backward, all lanes with their fork / wait / join edges) must replay to the same bits as the plain launch lists."""
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    # 3 and 4 lanes: round 1's captures of such programs died in the ROCm runtime (unbounded recursion of the stream's
    # EndCapture over a cycle of "parallel capture streams", made by event waits between two forked streams); ctx.hip now
    # records a lane-to-lane edge as two edges through the origin stream
    monkeypatch.setenv('IFCBK_LANES', lanes)
    monkeypatch.setenv('IFCBK_LANES_EVAL', lanes)
    engs = []
    for use_graph in (False, True):
        eng = Engine(graph.build(name, 5, pretrained=False), device=0, max_batch=B)
        eng.graph_eval = eng.graph_train = use_graph
        eng.init_weights(seed=77)
        eng.dropout_seed = 3
        engs.append(eng)
    g = torch.Generator().manual_seed(6)
    for step in range(3):
        x = torch.rand(B, 3, S, S, generator=g)
        y = torch.randint(0, 5, (B,), generator=g)
        for eng in engs:
            eng.load_input_nchw(x.cuda())
            eng.target[:B].copy_(y)
            eng.train_step(B)
        torch.cuda.synchronize()
        assert torch.equal(engs[0].loss, engs[1].loss), step
        assert torch.equal(engs[0].G, engs[1].G), step
        assert torch.equal(engs[0].P, engs[1].P), step
    assert len(engs[1].plan(B).graphs) == 1 and not engs[0].plan(B).graphs
    outs = []
    for eng in engs:
        for _ in range(2):                       # second pass replays the captured eval graph
            eng.load_input_nchw(x.cuda())
            pl = eng.forward_eval(B)
        torch.cuda.synchronize()
        outs.append([h for h in eng.heads if not h.aux][0].logits[:B].clone())
    assert torch.equal(outs[0], outs[1])
    assert 'fwd_eval' in engs[1].plan(B).graphs


@pytest.mark.gpu
def test_a_graph_belongs_to_its_ctx_and_dies_with_it():
    """The lifetime rule behind round 4's hipGraphLaunch SIGSEGV audit: every captured graph is owned by the ctx it was
    captured through.  (a) it is counted there; (b) another ctx can neither launch nor destroy it; (c) Engine.close() -- and
    ifcbk_ctx_destroy by itself -- destroys the graphs BEFORE the arenas / streams / events they refer to, so that no
    hipGraphExec outlives an engine (before round 5 every dropped handle leaked its exec for the life of the process: 135
    engines into the GPU suite is where the crash hit); (d) a destroyed handle is refused, not dereferenced."""
    import ctypes as C
    from ifcb_classifier_amd import graph, _lib
    from ifcb_classifier_amd.engine import Engine
    eng = Engine(graph.build('resnet18', 3, pretrained=False), device=0, max_batch=4)
    eng.graph_eval = eng.graph_train = True
    eng.init_weights(seed=1)
    other = _lib.Context(0)
    assert eng.ctx.live_graphs() == 0
    eng.load_input_nchw(torch.rand(4, 3, 224, 224).cuda())
    eng.target[:4].copy_(torch.tensor([0, 1, 2, 1]))
    eng.train_step(4)
    eng.forward_eval(4)
    torch.cuda.synchronize()
    assert eng.ctx.live_graphs() == 2
    g = eng.plan(4).graphs['fwd_eval']
    assert other.lib.ifcbk_graph_launch(other.h, g, eng.stream()) == _lib.EINVAL          # (b)
    assert b'not a live graph of this ctx' in other.lib.ifcbk_last_error(other.h)
    assert other.lib.ifcbk_graph_destroy(other.h, g) == _lib.EINVAL
    assert eng.ctx.live_graphs() == 2
    eng.forward_eval(4)                                                                   # still launchable through its owner
    torch.cuda.synchronize()
    lib, h = eng.ctx.lib, eng.ctx.h
    eng.close()                                                                           # (c)
    assert eng.ctx.h is None and not eng.plan_graph_handles()
    # (c) without the engine's help: the ctx destroys what the caller left
    ctx2 = _lib.Context(0)
    ops = (_lib.Op * 1)()                                                                 # (a kernel node: a memset is not captured, ifcbk.h)
    ops[0].kind = _lib.OP_SOFTMAX
    buf, out = torch.zeros(8, 8, device='cuda'), torch.zeros(8, 8, device='cuda')
    ops[0].p[0], ops[0].p[1] = buf.data_ptr(), out.data_ptr()
    ops[0].i[0], ops[0].i[1] = 8, 8
    g2 = ctx2.capture(ops, 1)
    assert ctx2.live_graphs() == 1
    ctx2.graph_launch(g2, _lib.cur_stream())
    torch.cuda.synchronize()
    assert torch.equal(out, torch.full_like(out, 0.125))
    assert lib.ifcbk_graph_destroy(ctx2.h, g2) == 0 and ctx2.live_graphs() == 0
    g3 = ctx2.capture(ops, 1)
    assert ctx2.live_graphs() == 1 and g3
    ctx2.close()                                                                          # g3 goes with it: no leak, no dangling exec
    other.close()


@pytest.mark.gpu
def test_batch_beyond_the_descriptor_window_is_one_eval_program_and_refused_in_training():
    """The conv kernels address a tensor through a 32-bit buffer descriptor: 776 inception_v3 images (bf16) fit the 2 GiB window of
    ONE launch.  An eval batch beyond it (SURVEY 8(d) config 4 sweeps batch 1024) is still one program / one hipGraph: the library
    cuts each convolution into launches over image groups, and the logits equal those of the same images run 256 at a time, bit
    for bit (samples are independent: neuston_models.py:152-157).  A training batch beyond the window is refused (BatchNorm batch
    statistics are per step)."""
    from ifcb_classifier_amd.neuston_models import get_namebrand_model
    B = 1024
    torch.manual_seed(11)
    m = get_namebrand_model('inception_v3', 12, max_batch=B)
    eng = m.engine
    assert eng.window_batch == ((1 << 31) - 1) // (147 * 147 * 64 * 2) == 776 and eng.max_batch == B
    g = torch.Generator().manual_seed(12)
    x = torch.rand(B, 3, 299, 299, generator=g).cuda()
    m.eval()
    with torch.no_grad():
        m(x)                                   # captures the batch-1024 graph
        whole = m(x)                           # replays it
        parts = torch.cat([m(x[i:i + 256]) for i in range(0, B, 256)], 0)
    assert 'fwd_eval' in eng.plan(B).graphs
    assert whole.shape == (B, 12) and torch.isfinite(whole).all() and torch.equal(whole, parts)
    m.train()
    with pytest.raises(RuntimeError, match='BatchNorm batch statistics'):
        m(x)
    with pytest.raises(RuntimeError, match='BatchNorm batch statistics'):
        eng.train_step(B)
    with pytest.raises(RuntimeError, match='larger max_batch'):
        m.eval()
        m(torch.rand(B + 1, 3, 299, 299).cuda())


@pytest.mark.gpu
def test_roi_batch_whose_stem_output_passes_2_gib_equals_its_parts():
    """RUN path (ragged u8 ROIs -> resized plane -> u8 stem kernel -> hipGraph-replayed eval forward -> softmax) at 1,536 images:
    Conv2d_1a's output is 2.18 GB, Conv2d_4a's runs as two image groups.  Probabilities equal those of the same ROIs run 256 at
    a time, bit for bit (round 4: this batch size faulted -- csrc/conv_stem_u8.hip, the sign-extended row offset)."""
    import bench
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    B = 1536
    eng = Engine(graph.build('inception_v3', 20, pretrained=False), device=0, max_batch=B, train_batch=1)
    eng.init_weights(seed=4)
    rois, _ = bench.synth_rois(B, 31, eng.dev)

    def run(i0, n):
        eng.load_rois(rois['pixels'], rois['offs'][i0:i0 + n], rois['hs'][i0:i0 + n], rois['ws'][i0:i0 + n], rois['max_h'], rois['max_w'])
        p = eng.forward_eval(n)
        eng.run(p.softmax)
        torch.cuda.synchronize()
        return eng.probs[:n].clone()
    run(0, B)
    whole = run(0, B)
    parts = torch.cat([run(i, 256) for i in range(0, B, 256)], 0)
    assert torch.isfinite(whole).all() and torch.equal(whole, parts)
    del eng
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_lane_count_does_not_change_the_result(monkeypatch):
    """The lane count only decides which stream a kernel is launched on (data-parallel jobs use 2 lanes, a single GPU 4, one
    lane is plain stream order): every reduction has a fixed order and the per-lane scratch buffers carry no state, so
    1, 2 and 4 lanes must produce the same bits.  (A dependency the 2- or 4-lane schedule misses changes the result only when the
    timing goes wrong, which this batch rarely provokes: tests/test_gpu_lane_order.py slows each lane in turn on poisoned buffers to
    force it, and tests/test_program_footprints_cpu.py audits the schedule against the pointers of the op tables.)"""
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    B, S = 6, 299
    g = torch.Generator().manual_seed(9)
    xs = [torch.rand(B, 3, S, S, generator=g) for _ in range(2)]
    ys = [torch.randint(0, 7, (B,), generator=g) for _ in range(2)]
    results = []
    for lanes in ('1', '2', '4'):
        monkeypatch.setenv('IFCBK_LANES', lanes)
        eng = Engine(graph.build('inception_v3', 7, pretrained=False), device=0, max_batch=B)
        assert eng.NL == int(lanes)
        eng.init_weights(seed=4321)
        eng.dropout_seed = 5
        for x, y in zip(xs, ys):
            eng.load_input_nchw(x.cuda())
            eng.target[:B].copy_(y)
            eng.train_step(B)
        torch.cuda.synchronize()
        results.append((eng.loss.clone(), eng.P.clone(), eng.RB.clone()))
        del eng
    for r in results[1:]:
        assert torch.equal(results[0][0], r[0]) and torch.equal(results[0][1], r[1]) and torch.equal(results[0][2], r[2])


@pytest.mark.gpu
@pytest.mark.parametrize('name,B', [('resnet18', 6), ('inception_v3', 3)])
def test_prefetched_input_slots_equal_sequential_steps(name, B):
    """input pipelining (Engine.prefetch_begin / prefetch_end / use_prefetched, two input slots, preprocess of batch k+1 on a side
    stream beside step k): four training steps and an eval forward give bitwise the parameters, running statistics, loss and
    probabilities of the one-stream preprocess-then-step loop (reference: the DataLoader / Trainer loop, neuston_net.py:101-115)."""
    import numpy as np
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    NCLS = 4            # (inception_v3: grey ROIs take the u8-plane stem -- plane, affine and plan are per input slot)
    rng = np.random.default_rng(7)
    batches = []
    for _ in range(5):
        hs = rng.integers(20, 150, B).astype(np.int32)
        ws = rng.integers(20, 150, B).astype(np.int32)
        sizes = hs.astype(np.int64) * ws
        offs = np.zeros(B, np.int64)
        offs[1:] = np.cumsum(sizes)[:-1]
        blob = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8)
        kw = dict(pixels=torch.from_numpy(blob).cuda(), offs=torch.from_numpy(offs).cuda(), hs=torch.from_numpy(hs).cuda(),
                  ws=torch.from_numpy(ws).cuda(), max_h=int(hs.max()), max_w=int(ws.max()))
        batches.append((kw, torch.from_numpy(rng.integers(0, NCLS, B)).cuda()))
    engs = []
    for _ in range(2):
        e = Engine(graph.build(name, NCLS), 0, max_batch=B)
        e.init_weights(seed=5)
        if name == 'inception_v3':
            e.external_mask = torch.ones(B, 2048, dtype=torch.uint8, device='cuda')
        engs.append(e)
    seq, pipe = engs
    for kw, y in batches[:4]:
        seq.load_rois(**kw)
        seq.target[:B].copy_(y)
        seq.train_step(B)
    seq.load_rois(**batches[4][0])
    pl = seq.forward_eval(B)
    seq.run(pl.softmax)

    def stage(e, kw, y):
        slot, side = e.prefetch_begin()
        with torch.cuda.stream(side):
            e.load_rois(slot=slot, **kw)
            e.tgt_bufs[slot][:B].copy_(y)
        e.prefetch_end(slot)

    stage(pipe, *batches[0])
    for k in range(4):
        pipe.use_prefetched()
        stage(pipe, *batches[k + 1])
        pipe.train_step(B)
    pipe.use_prefetched()
    pl = pipe.forward_eval(B)
    pipe.run(pl.softmax)
    torch.cuda.synchronize()
    assert {k[1] for k in pipe._plans} == {0, 1}                 # both input slots were used
    assert {k[2] for k in pipe._plans} == ({'u8'} if name == 'inception_v3' else {'nhwc'})
    assert torch.equal(seq.P, pipe.P) and torch.equal(seq.RB, pipe.RB)
    assert torch.equal(seq.loss_sum, pipe.loss_sum)
    assert torch.equal(seq.probs[:B], pipe.probs[:B])
