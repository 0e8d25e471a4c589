"""dev tool: the six fused loss kernels of this tree's libifcbk.so against another build's, bit for bit and in time (one MI355X).

  python scripts/loss_ab.py /abs/path/to/other/libifcbk.so [--rounds 3]

Every loss entry point runs over the case tables of tests/ (loss_smooth_bounds.py for _w and _ls, loss_focal_bounds.py, mix_cases.py,
distill_cases.py, the XENT table of test_gpu_op_bounds.py) and over EXTRA below, with and without loss_accumulate and with dlogits
NULL; the bytes of loss_out and dlogits are hashed per case.  The library is chosen at import (IFCBK_LIB), so each build runs in child
processes, the two alternating over --rounds rounds; every round also times each kernel with events at the benchmark's shape (batch
256, 100 classes).  Prints the cases whose bytes differ and one line of microseconds per kernel; exit status 1 on any difference."""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# slot boundary, second round, inactive slots; around the four-lane split
EXTRA = [(N, NC) for N in (1, 255, 256, 257, 513) for NC in (1, 3, 4, 5)]
OLD = 5.0
FAMILIES = ('xent', 'w', 'ls', 'focal', 'mix', 'distill')


def cases():
    """(family, name, entry point, tensors before N and NC, scalars after them)"""
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    import torch
    import distill_cases as dc
    import loss_focal_bounds as fb
    import loss_smooth_bounds as sb
    import mix_cases as mc
    from test_gpu_op_bounds import XENT
    ones = lambda NC: torch.ones(NC)
    for N, NC, spread, shift, tmode, _, _ in XENT:
        g = torch.Generator().manual_seed(N + NC)
        l = torch.randn(N, NC, generator=g) * spread + shift
        t = {'argmax': l.argmax(1), 'least': l.argmin(1), 'rand': torch.randint(0, NC, (N,), generator=g)}[tmode]
        yield 'xent', 'XENT %s' % ((N, NC, spread, shift, tmode),), 'ifcbk_softmax_xent', (l, t), (0.7,)
    for N, NC in dict.fromkeys(sb.SHAPES + EXTRA):
        for wm in sb.WEIGHTS:
            for off in (False, True):
                l, t, cw = sb.inputs(N, NC, wm, offset_row=off)
                name = '(%d, %d) %s%s' % (N, NC, wm, ' offset' if off else '')
                if wm == 'none':
                    yield 'xent', name, 'ifcbk_softmax_xent', (l, t), (0.4,)
                yield 'w', name, 'ifcbk_softmax_xent_w', (l, t, ones(NC) if cw is None else cw), (0.4,)
                for eps in (0.0, 0.1, 1.0):
                    yield 'ls', '%s eps %g' % (name, eps), 'ifcbk_softmax_xent_ls', (l, t, cw), (0.4, eps)
            for mode in fb.MODES:
                l, t, cw = fb.inputs(N, NC, wm, mode=mode)
                for gam in (0.0,) + fb.GAMMAS:
                    yield 'focal', '(%d, %d) %s %s gamma %g' % (N, NC, wm, mode, gam), 'ifcbk_softmax_xent_focal', (l, t, cw), (0.4, gam)
        for case in dc.CASES:
            alpha, T, eps, scale, wm, off = case[:6]
            l, t, z, cw = dc.inputs(N, NC, wm, off)
            yield 'distill', dc.case_name(N, NC, case), 'ifcbk_softmax_xent_distill', (l, t, z, cw), (scale, eps, alpha, T)
    for N, NC in dict.fromkeys([(N, NC) for N in mc.LOSS_NS for NC in mc.LOSS_NCS] + EXTRA + [(256, 100)]):
        for wm in mc.WEIGHTS:
            for lam in mc.LAMS:
                l, t, lm, cw = mc.loss_inputs(N, NC, wm, lam, spread=30.0 if lam == 'rows' else 4.0)
                for eps in mc.EPSS:
                    yield 'mix', '(%d, %d) %s lam %s eps %g' % (N, NC, wm, lam, eps), 'ifcbk_softmax_xent_mix', (l, t, lm, cw), (0.4, eps)


def child(out, bits):
    sys.path.insert(0, ROOT)
    import torch
    from ifcb_classifier_amd import _lib
    ctx = _lib.Context(0)
    P, st = _lib.ptr, _lib.cur_stream
    res = {'hash': {}, 'us': {}}
    shape = {}
    for fam, name, fn, tens, scal in cases():
        N, NC = tens[0].shape
        timed = (N, NC) == (256, 100) and fam not in shape
        if not (bits or timed):
            continue
        dev = [None if t is None else t.cuda() for t in tens]
        args = [P(t) for t in dev] + [N, NC] + list(scal)
        if timed:
            shape[fam] = (fn, dev, args)
        if not bits:
            continue
        h = hashlib.sha256()
        for acc, with_dl in ((0, 1), (1, 1), (0, 0), (1, 0)):
            loss = torch.full((1,), OLD, device='cuda')
            dl = torch.full((N, NC), -12345.0, device='cuda') if with_dl else None
            ctx.call(fn, *(args + [P(loss), acc, P(dl), st()]))
            torch.cuda.synchronize()
            h.update(loss.cpu().numpy().tobytes())
            if with_dl:
                h.update(dl.cpu().numpy().tobytes())
        key = '%s %s' % (fam, name)
        assert key not in res['hash'], key
        res['hash'][key] = h.hexdigest()
    assert set(shape) == set(FAMILIES), sorted(shape)
    loss = torch.zeros(1, device='cuda')
    dl = torch.empty(256, 100, device='cuda')
    for fam, (fn, dev, args) in sorted(shape.items()):
        full = args + [P(loss), 0, P(dl), st()]
        for _ in range(50):
            ctx.call(fn, *full)
        best = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(500):
                ctx.call(fn, *full)
            b.record()
            torch.cuda.synchronize()
            best.append(a.elapsed_time(b) * 1000.0 / 500)
        res['us'][fam] = sorted(best)[len(best) // 2]              # median of five windows of 500 calls
    json.dump(res, open(out, 'w'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('other', nargs='?')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', help='directory for the child processes\' JSON results (default: a temporary one)')
    ap.add_argument('--child')
    ap.add_argument('--bits', type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.bits)
    other = os.path.abspath(a.other)
    a.out = a.out or tempfile.mkdtemp(prefix='loss_ab_')
    os.makedirs(a.out, exist_ok=True)
    runs = {'other': [], 'this': []}
    for r in range(a.rounds):
        for who in ('other', 'this'):
            env = {k: v for k, v in os.environ.items() if k != 'IFCBK_LIB'}
            if who == 'other':
                env['IFCBK_LIB'] = other
            path = os.path.join(a.out, 'loss_ab_%s_%d.json' % (who, r))
            subprocess.run([sys.executable, os.path.abspath(__file__), '--child', path, '--bits', str(int(r == 0))], env=env, check=True,
                           timeout=600)
            runs[who].append(json.load(open(path)))
    ha, hb = runs['other'][0]['hash'], runs['this'][0]['hash']
    assert set(ha) == set(hb) and ha
    bad = sorted(k for k in ha if ha[k] != hb[k])
    for k in bad:
        print('BYTES DIFFER: %s' % k)
    for fam in FAMILIES:
        n = sum(k.startswith(fam + ' ') for k in ha)
        print('%-8s %5d cases x 4 calls, %d differ' % (fam, n, sum(k.startswith(fam + ' ') for k in bad)))
    print('us per call at (256, 100), dlogits written; one figure per round')
    for fam in FAMILIES:
        o, t = [x['us'][fam] for x in runs['other']], [x['us'][fam] for x in runs['this']]
        inside = min(o) <= sum(t) / len(t) <= max(o)
        print('%-8s other %s | this %s | other spread %.2f - %.2f | mean ratio %.3f | %s' % (
            fam, ' / '.join('%.2f' % v for v in o), ' / '.join('%.2f' % v for v in t), min(o), max(o),
            (sum(t) / len(t)) / (sum(o) / len(o)), 'within' if inside else ('below' if max(t) < min(o) else 'OUTSIDE')))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
