"""TRAIN --resident on the GPU: ifcbk_roi_gather (csrc/roi_gather.hip) byte for byte against the numpy model (tests/resident_cases.py).
The destination starts 7 bytes behind a 64-byte guard and ends in front of another; both guards, every byte of the capacity behind the
total and the whole source must come back as they were.  Cases: one ROI, one byte, repeated indices, empty entries, every pair of
source and destination alignments for widths 1..33, sizes around the copy's chunk, one ROI of over a megabyte among tiny ones, the
scan's boundaries up to its limit, three channels, ROIs behind byte 2^32 of the source, a capacity beyond the total, the error returns."""
import numpy as np
import pytest
import torch

import resident_cases as rc

pytestmark = pytest.mark.gpu
GUARD, SHIFT, POISON = 64, 7, 0x5A


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def call(ctx, src, offs, hs, ws, idx, ch, capacity, dst_ptr, n=None):
    """one call on device tensors -> (dst_offs[n + 1], dst_hs, dst_ws) on the device"""
    from ifcb_classifier_amd import _lib
    n = len(idx) if n is None else n
    d_offs = torch.full((len(idx) + 1,), -7, dtype=torch.int64, device='cuda')
    d_hs = torch.full((len(idx),), -7, dtype=torch.int32, device='cuda')
    d_ws = torch.full((len(idx),), -7, dtype=torch.int32, device='cuda')
    ctx.call('ifcbk_roi_gather', _lib.ptr(src), _lib.ptr(offs), _lib.ptr(hs), _lib.ptr(ws), _lib.ptr(idx), n, ch, dst_ptr, capacity,
             _lib.ptr(d_offs), _lib.ptr(d_hs), _lib.ptr(d_ws), _lib.cur_stream())
    return d_offs, d_hs, d_ws


def run(ctx, case, shift=SHIFT):
    import ctypes as C
    blob, offs, hs, ws = rc.layout(case['shapes'], case['ch'], case['leads'])
    want_px, want_offs, want_hs, want_ws = rc.gather(blob, offs, hs, ws, case['idx'], case['ch'])
    total = int(want_offs[-1])
    assert total == want_px.size
    capacity = total + case['extra']
    src, s_offs, s_hs, s_ws = _dev(blob), _dev(offs), _dev(hs), _dev(ws)
    idx = torch.tensor(case['idx'], dtype=torch.int64).cuda()
    buf = torch.full((GUARD + shift + capacity + GUARD,), POISON, dtype=torch.uint8, device='cuda')
    assert buf.data_ptr() % 16 == 0
    d_offs, d_hs, d_ws = call(ctx, src, s_offs, s_hs, s_ws, idx, case['ch'], capacity, C.c_void_p(buf.data_ptr() + GUARD + shift))
    torch.cuda.synchronize()
    name = case['name']
    got = buf.cpu().numpy()
    lo = GUARD + shift
    assert (got[:lo] == POISON).all(), name + ': bytes in front of dst_pixels were written'
    assert (got[lo + total:] == POISON).all(), name + ': bytes at or behind dst_pixels + dst_offs[n] were written'
    assert np.array_equal(d_offs.cpu().numpy(), want_offs), name + ': dst_offs'
    assert np.array_equal(d_hs.cpu().numpy(), want_hs) and np.array_equal(d_ws.cpu().numpy(), want_ws), name + ': dst_hs / dst_ws'
    bad = np.flatnonzero(got[lo:lo + total] != want_px)
    assert bad.size == 0, '%s: %d of %d bytes differ, first at %d: got %d want %d' % (
        name, bad.size, total, bad[0], got[lo + bad[0]], want_px[bad[0]])
    assert np.array_equal(src.cpu().numpy(), blob), name + ': src_pixels was written'
    assert np.array_equal(s_offs.cpu().numpy(), offs) and np.array_equal(s_hs.cpu().numpy(), hs) and np.array_equal(s_ws.cpu().numpy(), ws)
    return total


@pytest.mark.parametrize('case', rc.CASES, ids=[c['name'] for c in rc.CASES])
def test_gather_equals_the_numpy_model_byte_for_byte(ctx, case):
    run(ctx, case)


def test_every_pair_of_source_and_destination_alignments(ctx):
    seen = set()
    for d in range(16):
        case = rc.alignment_case(d)
        _, offs, _, ws = rc.layout(case['shapes'], 1, case['leads'])
        cur = 0
        for k in case['idx']:
            if k >= 16:
                seen.add((int(offs[k]) % 16, cur % 16, int(ws[k])))
            cur += int(ws[k])
        run(ctx, case)
    assert seen == {(s, d, w) for s in range(16) for d in range(16) for w in range(1, 34)}
    # dst_pixels itself at every alignment, with ROIs around a unit
    for shift in range(16):
        run(ctx, rc._case('dst_pixels at base + %d' % shift, [(1, 15), (1, 16), (1, 17), (3, 11), (1, 48)], [4, 0, 1, 2, 3, 4]), shift=shift)


def test_rois_behind_byte_2_to_the_32_of_the_source(ctx):
    """a source of 2^32 + 4096 bytes of which only two ROIs are initialised: offsets are 64-bit from the table to the address"""
    import ctypes as C
    big = torch.empty(2 ** 32 + 4096, dtype=torch.uint8, device='cuda')
    rng = np.random.default_rng(9)
    rois = [rng.integers(0, 256, 37 * 11, dtype=np.uint8), rng.integers(0, 256, 50 * 20, dtype=np.uint8)]
    places = [2 ** 32 + 5, 2 ** 32 + 1003]
    for p, r in zip(places, rois):
        big[p:p + r.size] = _dev(r)
    # entry 0 of the table is a one-byte ROI at the blob's start
    big[:1] = 3
    offs, hs, ws = np.array([0] + places, np.int64), np.array([1, 37, 50], np.int32), np.array([1, 11, 20], np.int32)
    order = [2, 0, 1, 2]
    want = np.concatenate([rois[1], np.array([3], np.uint8), rois[0], rois[1]])
    buf = torch.full((GUARD + SHIFT + want.size + GUARD,), POISON, dtype=torch.uint8, device='cuda')
    d_offs, d_hs, d_ws = call(ctx, big, _dev(offs), _dev(hs), _dev(ws), torch.tensor(order).cuda(), 1, want.size,
                              C.c_void_p(buf.data_ptr() + GUARD + SHIFT))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    lo = GUARD + SHIFT
    assert (got[:lo] == POISON).all() and (got[lo + want.size:] == POISON).all()
    assert np.array_equal(got[lo:lo + want.size], want)
    assert d_offs.cpu().tolist() == [0, 1000, 1001, 1408, 2408] and d_hs.cpu().tolist() == [50, 1, 37, 50] and d_ws.cpu().tolist() == [20, 1, 11, 20]
    for p, r in zip(places, rois):
        assert np.array_equal(big[p:p + r.size].cpu().numpy(), r)
    del big


def test_error_returns_name_the_entry_point(ctx):
    import ctypes as C
    from ifcb_classifier_amd import _lib
    blob, offs, hs, ws = rc.layout([(4, 4), (2, 3)])
    src, s_offs, s_hs, s_ws = _dev(blob), _dev(offs), _dev(hs), _dev(ws)
    idx = torch.tensor([1, 0], dtype=torch.int64).cuda()
    many = torch.zeros(rc.MAX_N + 1, dtype=torch.int64).cuda()
    buf = torch.full((64,), POISON, dtype=torch.uint8, device='cuda')
    P = _lib.ptr
    d_offs = torch.full((rc.MAX_N + 2,), -7, dtype=torch.int64, device='cuda')
    d_hs = torch.full((rc.MAX_N + 1,), -7, dtype=torch.int32, device='cuda')
    d_ws = torch.full((rc.MAX_N + 1,), -7, dtype=torch.int32, device='cuda')
    good = dict(src=P(src), offs=P(s_offs), hs=P(s_hs), ws=P(s_ws), idx=P(idx), n=2, ch=1, dst=P(buf), cap=22, d_offs=P(d_offs), d_hs=P(d_hs),
                d_ws=P(d_ws))

    def go(**kw):
        a = dict(good, **kw)
        ctx.call('ifcbk_roi_gather', a['src'], a['offs'], a['hs'], a['ws'], a['idx'], a['n'], a['ch'], a['dst'], a['cap'], a['d_offs'], a['d_hs'],
                 a['d_ws'], _lib.cur_stream())

    assert (_lib.ROI_GATHER_MAX_N, _lib.ROI_GATHER_CHUNK) == (rc.MAX_N, rc.CHUNK)
    for kw, word in ((dict(n=0), 'n 0'), (dict(n=-2), 'n -2'), (dict(n=rc.MAX_N + 1, idx=P(many)), "scan's limit"), (dict(ch=2), 'in_channels'),
                     (dict(ch=0), 'in_channels'), (dict(ch=4), 'in_channels'), (dict(cap=-1), 'dst_capacity'), (dict(src=None), 'NULL'),
                     (dict(offs=None), 'NULL'), (dict(hs=None), 'NULL'), (dict(ws=None), 'NULL'), (dict(idx=None), 'NULL'),
                     (dict(dst=None), 'NULL'), (dict(d_offs=None), 'NULL'), (dict(d_hs=None), 'NULL'), (dict(d_ws=None), 'NULL')):
        with pytest.raises(RuntimeError, match='ifcbk_roi_gather') as e:
            go(**kw)
        assert word in str(e.value) and '(%d)' % _lib.EINVAL in str(e.value), (kw, str(e.value))
    torch.cuda.synchronize()
    assert bool((buf == POISON).all()) and bool((d_offs == -7).all()) and bool((d_hs == -7).all())      # a refused call writes nothing
    go()
    torch.cuda.synchronize()
    assert d_offs[:3].cpu().tolist() == [0, 6, 22] and bool((buf[22:] == POISON).all())
    assert np.array_equal(buf[:22].cpu().numpy(), np.concatenate([blob[offs[1]:offs[1] + 6], blob[offs[0]:offs[0] + 16]]))
