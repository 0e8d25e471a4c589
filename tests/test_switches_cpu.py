"""Every environment switch the library reads is accounted for (CPU): a plan snapshots the switches that change a workspace size or
a partial-row count (engine._DISPATCH_SWITCHES) and refuses to run after one of them changed; every other name the library sources
mention has its reason here.  The scan is over string literals, so names passed through a helper (conv_big.hip's env_int) count."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc')

# name -> why a plan need not snapshot it
EXEMPT = {
    'IFCBK_SEGV_BACKTRACE': 'diagnostic: a SIGSEGV handler installed at context creation',
    'IFCBK_POOL_FAST': 'picks the pool kernel only (no workspace, no partial rows)',
    'IFCBK_POOL_REMAP': 'index order inside the pool kernel only',
    'IFCBK_DEBUG_DROP': 'only under #ifdef IFCBK_EXPERIMENT_DROP / _FLAT (timing-only builds)',
    'IFCBK_STEM_DBG': 'only under #ifdef IFCBK_EXPERIMENT_STEM (timing-only builds)',
    'IFCBK_EXPERIMENT_NOFINALIZE': 'only under #ifdef IFCBK_EXPERIMENT_NOFINALIZE (timing-only builds)',
    'IFCBK_EXPERIMENT_EMPTYFINALIZE': 'only under #ifdef IFCBK_EXPERIMENT_NOFINALIZE (timing-only builds)',
}
EXPERIMENT_ONLY = ('IFCBK_DEBUG_DROP', 'IFCBK_STEM_DBG', 'IFCBK_EXPERIMENT_NOFINALIZE', 'IFCBK_EXPERIMENT_EMPTYFINALIZE')


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, '*.hip')) + glob.glob(os.path.join(CSRC, '*.h')))


def _literals():
    """name -> [(file, line, inside an #ifdef IFCBK_EXPERIMENT_* block)]"""
    found = {}
    for path in _sources():
        stack = []                                       # per open #if: is it an experiment block (and not its #else)
        for k, ln in enumerate(open(path), 1):
            d = ln.strip()
            if d.startswith('#if'):
                stack.append(bool(re.match(r'#ifdef\s+IFCBK_EXPERIMENT_', d)))
            elif d.startswith('#else') or d.startswith('#elif'):
                stack[-1] = False
            elif d.startswith('#endif'):
                stack.pop()
            for name in re.findall(r'"(IFCBK_[A-Z0-9_]+)"', ln):
                found.setdefault(name, []).append((os.path.basename(path), k, any(stack)))
    return found


def test_every_library_switch_is_guarded_or_exempt():
    from ifcb_classifier_amd.engine import _DISPATCH_SWITCHES
    found = _literals()
    assert len(found) >= 25
    unaccounted = sorted(n for n in found if n not in _DISPATCH_SWITCHES and n not in EXEMPT)
    assert not unaccounted, unaccounted
    assert not set(_DISPATCH_SWITCHES) & set(EXEMPT)
    for name in EXPERIMENT_ONLY:
        assert found[name] and all(inside for _f, _k, inside in found[name]), (name, found[name])


def test_every_guarded_switch_is_still_read():
    from ifcb_classifier_amd import engine, plan
    found = _literals()
    src = open(engine.__file__).read() + open(plan.__file__).read()      # (the plan builder reads the weight-gradient group switch)
    for name in engine._DISPATCH_SWITCHES:
        assert name in found or src.count("'%s'" % name) > 1, name       # (> 1: the tuple itself names it once)


def test_the_shipped_library_holds_no_experiment_switch():
    """the timing experiments that give wrong results exist only in builds with make EXTRA=-DIFCBK_EXPERIMENT_..."""
    with open(os.path.join(ROOT, 'ifcb_classifier_amd', 'libifcbk.so'), 'rb') as fh:
        blob = fh.read()
    for name in EXPERIMENT_ONLY:
        assert name.encode() not in blob, name


def test_fuse_bnstat_takes_zero_or_one_only(monkeypatch):
    """IFCBK_FUSE_BNSTAT=2 (the per-chunk-table fusion) was removed; a value the planner does not know is refused, not read as 1"""
    import pytest
    from ifcb_classifier_amd import graph
    from ifcb_classifier_amd.engine import Engine
    monkeypatch.setenv('IFCBK_FUSE_BNSTAT', '2')
    eng = Engine(graph.build('resnet18', 2), max_batch=2, plan_only=True)
    with pytest.raises(ValueError, match='IFCBK_FUSE_BNSTAT'):
        eng.plan(2)
