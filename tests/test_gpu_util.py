"""CALC_IMG_NORM on the GPU: ifcbk_u8_channel_moments exact against numpy integer sums, the RGB u8 plane of ifcbk_roi_preprocess
written without the float tensor (out = NULL) on ragged batches against Pillow, and the whole command on the golden tree against
what the reference's own calc_img_norm produced."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import util_norm_check as unc

pytestmark = pytest.mark.gpu
G = unc.golden()


def _moments(ctx, x_dev, n, ppi, ch, offset=0):
    from ifcb_classifier_amd import _lib
    out = torch.full((max(n, 1), ch, 2), -7, dtype=torch.int64, device='cuda')
    ctx.call('ifcbk_u8_channel_moments', C.c_void_p(x_dev.data_ptr() + offset), n, ppi, ch, _lib.ptr(out), _lib.cur_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def _numpy_moments(planes, ch):
    """[n][pixels * ch] u8 -> [n][ch][2] exact sums (int64 per image)"""
    out = np.zeros((planes.shape[0], ch, 2), np.uint64)
    for i, p in enumerate(planes):
        v = p.reshape(-1, ch)
        out[i, :, 0] = v.sum(0, dtype=np.int64)
        out[i, :, 1] = (v.astype(np.int64) ** 2).sum(0)
    return out


# the cases of u8_moments_kernel (stats.hip), also read by test_op_inventory_cpu.py: (channels, (h, w), images)
MOMENT_CH, MOMENT_HW, MOMENT_N = [1, 3], [(299, 299), (224, 224), (1, 1), (37, 53)], [1, 7, 300]
MOMENT_EXTRA = [(2, (61, 47), 5), (4, (61, 47), 5)]           # test_u8_channel_moments_two_and_four_channels_and_all_255
MOMENTS = [(ch, hw, n) for ch in MOMENT_CH for hw in MOMENT_HW for n in MOMENT_N] + MOMENT_EXTRA


@pytest.mark.parametrize('ch', MOMENT_CH)
@pytest.mark.parametrize('hw', MOMENT_HW)
@pytest.mark.parametrize('n', MOMENT_N)
def test_u8_channel_moments_exact(ctx, ch, hw, n):
    rng = np.random.default_rng(ch * 1000 + hw[0] + n)
    ppi = hw[0] * hw[1]
    planes = rng.integers(0, 256, (n, ppi * ch), dtype=np.uint8)
    if n == 300:
        planes[::3] = 255                                       # all-255 images: the largest sums (> 2^32 at 299^2)
    # offset 0: the plane as allocated; offset 5: a base address off the 16-byte grid (every image takes the head / tail path)
    for offset in (0, 5):
        x = torch.zeros(offset + planes.size, dtype=torch.uint8)
        x[offset:] = torch.from_numpy(planes.reshape(-1))
        got = _moments(ctx, x.cuda(), n, ppi, ch, offset)
        assert np.array_equal(got, _numpy_moments(planes, ch)), (offset, got[:2], _numpy_moments(planes, ch)[:2])


def test_u8_channel_moments_two_and_four_channels_and_all_255(ctx):
    rng = np.random.default_rng(4)
    for ch, (h, w), n in MOMENT_EXTRA:
        planes = rng.integers(0, 256, (n, h * w * ch), dtype=np.uint8)
        assert np.array_equal(_moments(ctx, torch.from_numpy(planes).cuda(), n, h * w, ch), _numpy_moments(planes, ch))
    full = torch.full((300, 299 * 299 * 3), 255, dtype=torch.uint8, device='cuda')
    got = _moments(ctx, full, 300, 299 * 299, 3)
    assert (got[..., 0] == 299 * 299 * 255).all() and (got[..., 1] == 299 * 299 * 255 * 255).all()


def test_u8_channel_moments_empty_batch_and_invalid_arguments(ctx):
    from ifcb_classifier_amd import _lib
    lib, st = ctx.lib, _lib.cur_stream()
    x = torch.zeros(64, dtype=torch.uint8, device='cuda')
    out = torch.full((4, 4, 2), -7, dtype=torch.int64, device='cuda')
    assert lib.ifcbk_u8_channel_moments(ctx.h, _lib.ptr(x), 0, 16, 3, _lib.ptr(out), st) == _lib.OK
    assert lib.ifcbk_u8_channel_moments(ctx.h, None, 0, 16, 3, None, st) == _lib.OK
    torch.cuda.synchronize()
    assert (out.cpu() == -7).all()                               # n_img = 0 writes nothing
    for args, what in (((_lib.ptr(x), 1, 16, 0, _lib.ptr(out)), 'channels'), ((_lib.ptr(x), 1, 16, 5, _lib.ptr(out)), 'channels'),
                       ((_lib.ptr(x), 1, -1, 1, _lib.ptr(out)), 'pixels_per_img'), ((_lib.ptr(x), -1, 16, 1, _lib.ptr(out)), 'n_img'),
                       ((None, 1, 16, 1, _lib.ptr(out)), 'null'), ((_lib.ptr(x), 1, 16, 1, None), 'null')):
        assert lib.ifcbk_u8_channel_moments(ctx.h, *args, st) == _lib.EINVAL, args
        assert what in lib.ifcbk_last_error(ctx.h).decode()
    torch.cuda.synchronize()
    assert (out.cpu() == -7).all()


@pytest.mark.parametrize('S', [224, 299])
def test_roi_preprocess_rgb_plane_without_the_tensor_vs_pillow(ctx, S):
    """the call CALC_IMG_NORM makes: a ragged RGB batch (smaller and larger than S) -> u8 plane only (out = NULL)"""
    from PIL import Image
    from ifcb_classifier_amd import _lib
    rng = np.random.default_rng(S)
    dims = [(9, 400), (400, 9), (57, 131), (350, 320), (S, S), (224, 300), (13, 13)]
    rois = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in dims]
    d = _lib.RoiDesc()
    d.n_img, d.S, d.in_channels, d.out_channels, d.flip_bits_valid, d.dtype = len(rois), S, 3, 8, 0, _lib.BF16
    for k in range(3):
        d.mean[k], d.std[k], d.tin_scale[k], d.tin_shift[k] = 0.0, 1.0, 1.0, 0.0
    offs = np.zeros(len(rois), np.int64)
    offs[1:] = np.cumsum([r.size for r in rois])[:-1]
    pix = torch.from_numpy(np.concatenate([r.reshape(-1) for r in rois])).cuda()
    offs_d = torch.from_numpy(offs).cuda()
    hs = torch.tensor([h for h, _ in dims], dtype=torch.int32).cuda()
    ws = torch.tensor([w for _, w in dims], dtype=torch.int32).cuda()
    mh, mw = max(h for h, _ in dims), max(w for _, w in dims)
    ctx.reserve(max(ctx.lib.ifcbk_ctx_workspace_bytes(ctx.h), ctx.lib.ifcbk_roi_preprocess_workspace(C.byref(d), mh, mw)))
    plane = torch.full((len(rois), S, S, 3), 7, dtype=torch.uint8, device='cuda')
    ctx.call('ifcbk_roi_preprocess', C.byref(d), _lib.ptr(pix), _lib.ptr(offs_d), _lib.ptr(hs), _lib.ptr(ws), None, mh, mw,
             None, _lib.ptr(plane), _lib.cur_stream())
    torch.cuda.synchronize()
    got = plane.cpu().numpy()
    for i, r in enumerate(rois):
        want = np.asarray(Image.fromarray(r, 'RGB').resize((S, S), Image.BILINEAR))
        assert np.array_equal(got[i], want), (i, dims[i])


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('util_tree'))
    unc.build_tree(root)
    return root


@pytest.mark.parametrize('name', [c['name'] for c in G['cases']])
def test_calc_img_norm_end_to_end_vs_reference(tree, capsys, name):
    from ifcb_classifier_amd import neuston_util as nu
    case = next(c for c in G['cases'] if c['name'] == name)
    # loaders=0, as the CLI tests (test_gpu_cli.py) run: starting worker processes from the long-lived suite process costs tens of
    # seconds per DataLoader there; the batches and their order are the same for any worker count (shuffle=False)
    t0 = time.perf_counter()
    seen, out = unc.run_case(nu, case, tree, capsys, loaders=0)
    dt = time.perf_counter() - t0
    unc.check_case(case, seen, out, unc.bound(G))
    import conftest
    conftest.MEASURED.append('CALC_IMG_NORM case %s (%d batches): %.2f s' % (name, len(seen), dt))
