"""Every kernel of bn.hip, pool_head.hip and plain.hip is reached by a case of tests/test_gpu_op_bounds.py, every kernel of the input
path (roi.hip, conv_stem_u8.hip, stats.hip) by a case of its own table, and every entry point of include/ifcbk.h is called by some
test (CPU): a kernel or an entry point added later without a test fails here."""
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
    'ifcbk_program_capture': 'reached through Context.capture (test_gpu_model.py)',
    'ifcbk_op_cost': 'host-only bookkeeping (flops / bytes of an op) used by the profiling scripts; launches nothing',
}


def _norm(s):
    return re.sub(r'\s+', ' ', s)


def _kernels(fname):
    src = open(os.path.join(CSRC, fname)).read()
    return set(re.findall(r'__global__\s+(?:__launch_bounds__\(\w+\)\s+)?void\s+(\w+)\s*\(', src))


def _stem(kernel):
    return lambda c: kernel in importlib.import_module('test_gpu_stem_u8').stem_kernels_reached([c])


def _roi(prefix):
    return lambda c: any(p.startswith(prefix) for p in importlib.import_module('roi_bounds').paths(c))


_MFMA = 'static bool stem_mfma(const ifcbk_conv_desc* d) { return d->dtype == IFCBK_BF16 && d->Q >= 32; }'
# the input path: kernel -> (file, module holding the case table, table, reaches(case), dispatch condition quoted from the file).
# roi_resize_kernel's three arithmetic paths have a predicate and a quoted condition each in roi_bounds.PATHS (test_roi_paths_cpu.py).
INPUT_KERNELS = {
    'roi_coeffs_kernel': ('roi.hip', 'roi_bounds', 'ROI', lambda c: True, 'hipLaunchKernelGGL(roi_coeffs_kernel, dim3(cdiv(nco, 256))'),
    'roi_resize3_kernel': ('roi.hip', 'roi_bounds', 'ROI', _roi('roi_resize3_kernel'), 'if (d->in_channels == 1 && kmax == 3 && d->S <= 320)'),
    'roi_resize_kernel': ('roi.hip', 'roi_bounds', 'ROI', _roi('roi_resize_kernel'), 'else hipLaunchKernelGGL(roi_resize_kernel,'),
    'stem_u8_fwd_kernel': ('conv_stem_u8.hip', 'test_gpu_stem_u8', 'STEM', _stem('stem_u8_fwd_kernel'),
                           'else hipLaunchKernelGGL((stem_u8_fwd_kernel<bf16_t, false>), grid, blk, 0, st, a);'),
    'stem_u8_fwd_mfma_kernel': ('conv_stem_u8.hip', 'test_gpu_stem_u8', 'STEM', _stem('stem_u8_fwd_mfma_kernel'), _MFMA),
    'stem_u8_wgrad_kernel': ('conv_stem_u8.hip', 'test_gpu_stem_u8', 'STEM', _stem('stem_u8_wgrad_kernel'),
                             'else hipLaunchKernelGGL(stem_u8_wgrad_kernel<bf16_t>, dim3(nblk), dim3(256), 0, st, a);'),
    'stem_u8_wgrad_mfma_kernel': ('conv_stem_u8.hip', 'test_gpu_stem_u8', 'STEM', _stem('stem_u8_wgrad_mfma_kernel'),
                                  'else if (stem_mfma(d)) hipLaunchKernelGGL(stem_u8_wgrad_mfma_kernel,'),
    'stem_u8_wgrad_reduce_kernel': ('conv_stem_u8.hip', 'test_gpu_stem_u8', 'STEM', _stem('stem_u8_wgrad_reduce_kernel'),
                                    'hipLaunchKernelGGL(stem_u8_wgrad_reduce_kernel, dim3(K1), dim3(640), 0, st, (const float*)ctx->ws, nblk, ab, dw, accumulate);'),
    'u8_moments_kernel': ('stats.hip', 'test_gpu_util', 'MOMENTS', lambda c: 1 <= c[0] <= 4, 'if (channels < 1 || channels > 4)'),
}


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


def test_every_input_path_kernel_has_cases_and_a_quoted_dispatch_condition():
    files = ('roi.hip', 'conv_stem_u8.hip', 'stats.hip')
    found = {k: f for f in files for k in _kernels(f)}
    assert sorted(found) == sorted(INPUT_KERNELS), (sorted(set(found) - set(INPUT_KERNELS)), sorted(set(INPUT_KERNELS) - set(found)))
    for name, (fname, module, table, reaches, cond) in INPUT_KERNELS.items():
        assert found[name] == fname, name
        cases = getattr(importlib.import_module(module), table)
        assert isinstance(cases, list) and cases, table
        assert any(reaches(c) for c in cases), '%s: no case of %s.%s reaches it (%s)' % (name, module, table, cond)
        assert _norm(cond) in _norm(open(os.path.join(CSRC, fname)).read()), '%s: the dispatch condition %r is no longer in the source' % (name, cond)
    # every channel count the moments kernel is instantiated for
    assert {c[0] for c in importlib.import_module('test_gpu_util').MOMENTS} == {1, 2, 3, 4}
    # the conv inventory's exemptions name the same five stem kernels
    counted = importlib.import_module('test_gpu_conv_bounds').COUNTED
    assert {k for k in INPUT_KERNELS if k.startswith('stem_u8')} <= set(counted)
    assert not [v for v in counted.values() if 'norm' in v]


def test_every_entry_point_is_called_by_a_test():
    hdr = open(os.path.join(ROOT, 'include', 'ifcbk.h')).read()
    api = re.findall(r'IFCBK_API\s+[\w\s\*]+?\b(ifcbk_\w+)\s*\(', hdr)
    assert len(api) >= 70 and len(set(api)) == len(api)
    text = ''.join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, 'tests', '*.py'))) if os.path.basename(p) != os.path.basename(__file__))
    missing = sorted(n for n in api if not re.search(r'\b%s\b' % n, text) and n not in EXEMPT_API)
    assert not missing, missing
    assert not [n for n in EXEMPT_API if n not in api], 'an exemption names an entry point that is gone'


def test_the_loss_row_reduction_is_written_once():
    """the quad butterflies and the fixed-order slot sums of the six fused loss kernels stand once, in loss_rows.h: a loss variant that
    pastes a further copy instead of calling the shared pieces fails here"""
    shared = open(os.path.join(CSRC, 'loss_rows.h')).read()
    loss = open(os.path.join(CSRC, 'loss.hip')).read()
    head = open(os.path.join(CSRC, 'pool_head.hip')).read()
    assert len(_kernels('loss.hip')) == 6 and sum(k.startswith('softmax_xent_') for k in _kernels('loss.hip')) == 5
    m = re.search(r'void\s+softmax_xent_kernel\s*\(.*?\n}\n', head, re.S)
    assert m and 'for (int n0 = 0; n0 < N; n0 += 256)' in m.group(0) and 'loss_store(' in m.group(0)
    slot_loop = r'for\s*\(\s*int\s+i\s*=\s*0\s*;\s*i\s*<\s*\w+\s*;\s*\+\+i\s*\)'
    for where, text in (('loss.hip', loss), ('softmax_xent_kernel', m.group(0))):
        assert '__shfl_xor' not in text, where
        assert 'for (int i = 0; i < 256; ++i)' not in text and not re.search(slot_loop, text), where
        assert '#include "loss_rows.h"' in (loss if where == 'loss.hip' else head), where
    # each butterfly (two exchange steps), the slot sum and each of its callers is defined once, and the butterflies only there
    assert len(re.findall(r'__shfl_xor', shared)) == 4 and len(re.findall(slot_loop, shared)) == 1
    assert 'for (int i = 0; i < LOSS_SLOTS; ++i) s += sl[i];' in shared and re.search(r'constexpr int LOSS_SLOTS = 256;', shared)
    for fn in ('quad_max', 'quad_sum', 'row_max', 'row_expsum', 'class_w', 'slot_total', 'slot_sum0', 'slot_sum', 'slot_sum2', 'loss_store'):
        assert len(re.findall(r'__device__ __forceinline__ \w+ %s\(' % fn, shared)) == 1, fn
    rule = re.search(r'^%\.o:(.*)$', open(os.path.join(CSRC, 'Makefile')).read(), re.M).group(1)
    assert 'loss_rows.h' in rule.split()


def test_the_library_is_built_without_flags_that_change_rounding():
    """op_bounds.py counts sqrtf and / as one rounding each and a * b + c as one or two: true under -ffp-contract=on without
    fast-math, reciprocal or denormal flags"""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    flags = re.search(r'^CXXFLAGS\s*=(.*)$', mk, re.M).group(1)
    assert '-ffp-contract=on' in flags
    for bad in ('fast-math', 'ffp-contract=fast', 'unsafe-math', 'reciprocal', 'fhip-fp32-correctly-rounded-divide-sqrt', 'daz', 'ftz', 'Ofast',
                'approx-func', 'finite-math'):
        assert bad not in flags, bad
