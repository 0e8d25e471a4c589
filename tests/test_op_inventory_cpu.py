"""Every kernel of bn.hip, pool_head.hip and plain.hip is reached by a case of tests/test_gpu_op_bounds.py, and every entry point of
include/ifcbk.h is called by some test (CPU): a kernel or an entry point added later without a test fails here."""
import glob
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ifcb_classifier_amd', 'csrc')
FILES = ('bn.hip', 'pool_head.hip', 'plain.hip')
EXEMPT_KERNELS = ('experiment_empty_kernel',)          # timing-only builds (#ifdef IFCBK_EXPERIMENT_NOFINALIZE)

# entry point -> why no test calls it by name
EXEMPT_API = {
    'ifcbk_ctx_create': 'reached through _lib.Context(), which the session ctx fixture and every Engine build',
    'ifcbk_ctx_reserve': 'reached through Context.reserve (conftest.py, most GPU tests)',
    'ifcbk_ctx_set_lanes': 'called by Engine.__init__, so by every whole-model test; test_lanes_cpu.py checks the lane plan itself',
    'ifcbk_ctx_live_graphs': 'reached through Context.live_graphs (test_gpu_model.py)',
    'ifcbk_run_program': 'reached through Context.run_program (test_gpu_conv_forced.py, every Engine step)',
    'ifcbk_run_program_ev': 'the event-timed variant of the same runner (the engine\'s per-op timing mode); same launches as ifcbk_run_program',
    'ifcbk_program_times': 'host read-back of the events of ifcbk_run_program_ev; launches nothing',
    'ifcbk_program_capture': 'reached through Context.capture (test_gpu_model.py)',
    'ifcbk_op_cost': 'host-only bookkeeping (flops / bytes of an op) used by the profiling scripts; launches nothing',
}


def _norm(s):
    return re.sub(r'\s+', ' ', s)


def _kernels(fname):
    src = open(os.path.join(CSRC, fname)).read()
    return set(re.findall(r'__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(', src))


def test_every_kernel_has_cases_and_a_quoted_dispatch_condition():
    t = importlib.import_module('test_gpu_op_bounds')
    found = {k: f for f in FILES for k in _kernels(f) if k not in EXEMPT_KERNELS}
    assert len(found) >= 30
    assert sorted(found) == sorted(t.KERNELS), (sorted(set(found) - set(t.KERNELS)), sorted(set(t.KERNELS) - set(found)))
    for name, (fname, table, reaches, cond) in t.KERNELS.items():
        assert found[name] == fname, name
        cases = getattr(t, table)
        assert isinstance(cases, list) and cases, table
        assert any(reaches(c) for c in cases), '%s: no case of %s reaches it (%s)' % (name, table, cond)
        src = _norm(open(os.path.join(CSRC, fname)).read()) + _norm(open(os.path.join(ROOT, 'include', 'ifcbk.h')).read())
        assert _norm(cond) in src, '%s: the dispatch condition %r is no longer in the source' % (name, cond)


def test_every_entry_point_is_called_by_a_test():
    hdr = open(os.path.join(ROOT, 'include', 'ifcbk.h')).read()
    api = re.findall(r'IFCBK_API\s+[\w\s\*]+?\b(ifcbk_\w+)\s*\(', hdr)
    assert len(api) >= 70 and len(set(api)) == len(api)
    text = ''.join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, 'tests', '*.py'))) if os.path.basename(p) != os.path.basename(__file__))
    missing = sorted(n for n in api if not re.search(r'\b%s\b' % n, text) and n not in EXEMPT_API)
    assert not missing, missing
    assert not [n for n in EXEMPT_API if n not in api], 'an exemption names an entry point that is gone'


def test_the_library_is_built_without_flags_that_change_rounding():
    """op_bounds.py counts sqrtf and / as one rounding each and a * b + c as one or two: true under -ffp-contract=on without
    fast-math, reciprocal or denormal flags"""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS\s*=(.*)$', mk, re.M).group(1)
    assert '-ffp-contract=on' in flags
    for bad in ('fast-math', 'ffp-contract=fast', 'unsafe-math', 'reciprocal', 'fhip-fp32-correctly-rounded-divide-sqrt', 'daz', 'ftz', 'Ofast',
                'approx-func', 'finite-math'):
        assert bad not in flags, bad
