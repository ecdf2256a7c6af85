"""GPU: isa.DpSeamFinder(ctx).find (csrc/seam.hip: host logic behind one staged device round trip) against the numpy / scipy
reference of tests/refimpl_seam_dp.py, byte for byte, over the scenes of test_refimpl_seam_dp_cpu.py; then what only the library
has: device, host, mixed and pitched odd-address buffers, the per-thread pair state and the staging buffers reused over calls of
different sizes, host threads over independent pairs, and the refusals."""
import ctypes as C

import numpy as np
import pytest

from test_refimpl_seam_dp_cpu import NAMES, reference, scene

pytestmark = pytest.mark.gpu

MIS_E_INVALID, MIS_E_UNSUPPORTED = -1, -6


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _pitched(a, device):
    """-> (holder, view, holder as filled): `a` at [1:1+h, 1:1+w] of a larger buffer full of a sentinel pattern, on the device or the
    host.  The holder's width is even, so the row pitch exceeds the row and the view's first byte sits at an odd address."""
    h, w = a.shape[:2]
    shape = (h + 2, w + 2 + w % 2) + a.shape[2:]
    filled = (np.arange(int(np.prod(shape)), dtype=np.int64) % 251 + 1).astype(np.uint8).reshape(shape)
    filled[1:1 + h, 1:1 + w] = a
    holder = _dev(filled) if device else filled.copy()
    view = holder[1:1 + h, 1:1 + w]
    addr = view.data_ptr() if device else view.ctypes.data
    assert addr % 2 == 1
    return holder, view, filled


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _check(got, name, what):
    want = reference(name)[0]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g = _np(g)
        assert np.array_equal(g, w), "%s, %s: mask %d differs in %d pixels, first at %s" % (name, what, k, (g != w).sum(), np.argwhere(g != w)[0])


@pytest.mark.parametrize("name", NAMES + ["seam_scale"])
def test_library_equals_reference(ctx, name):
    """Every scene, once with device tensors and once with host arrays."""
    import image_stitching_amd as isa
    im, c, m = scene(name)
    dm = [_dev(k) for k in m]
    isa.DpSeamFinder(ctx).find([_dev(i) for i in im], c, dm)
    _check(dm, name, "device tensors")
    hm = [k.copy() for k in m]
    isa.DpSeamFinder(ctx).find([i.copy() for i in im], c, hm)
    _check(hm, name, "host arrays")


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("name", ["six", "near_edges", "bytes"])
def test_pitched_views_at_odd_addresses(ctx, name, device):
    """Images and masks that are slices of larger buffers: same masks, nothing outside a mask's view written."""
    import image_stitching_amd as isa
    im, c, m = scene(name)
    pi = [_pitched(i, device) for i in im]
    pm = [_pitched(k, device) for k in m]
    isa.DpSeamFinder(ctx).find([p[1] for p in pi], c, [p[1] for p in pm])
    _check([p[1] for p in pm], name, "pitched views")
    for (holder, _, filled), k in zip(pi + pm, im + m):
        got, want = _np(holder).copy(), filled.copy()
        got[1:1 + k.shape[0], 1:1 + k.shape[1]] = 0
        want[1:1 + k.shape[0], 1:1 + k.shape[1]] = 0
        assert np.array_equal(got, want)
    for (holder, _, filled) in pi:
        assert np.array_equal(_np(holder), filled)               # images are read only


def test_mixed_host_and_device_buffers(ctx):
    """One call whose images and masks alternate between host and device memory, image and mask of a frame on different sides."""
    import image_stitching_amd as isa
    for name in ("six", "five"):
        im, c, m = scene(name)
        images = [_dev(i) if k % 2 else i.copy() for k, i in enumerate(im)]
        masks = [k_.copy() if k % 3 else _dev(k_) for k, k_ in enumerate(m)]
        isa.DpSeamFinder(ctx).find(images, c, masks)
        _check(masks, name, "mixed buffers")


def test_one_context_large_small_large(ctx):
    """Calls of different sizes and image counts on one context, device and host in turn: the pair state that a host thread keeps
    between calls and the staging buffers carry nothing over."""
    import image_stitching_amd as isa
    finder = isa.DpSeamFinder(ctx)
    for k, name in enumerate(["seam_scale", "one_pixel", "six", "seam_scale", "contained", "five", "gap", "seam_scale"]):
        im, c, m = scene(name)
        masks = [_dev(x) for x in m] if k % 2 == 0 else [x.copy() for x in m]
        finder.find([_dev(i) for i in im] if k % 2 == 0 else im, c, masks)
        _check(masks, name, "call %d of the sequence" % k)


def test_six_frames_ten_times(ctx):
    """Independent pairs run on host threads: ten runs give the reference's masks every time."""
    import image_stitching_amd as isa
    im, c, m = scene("six")
    assert reference("six")[1]["independent_pairs"]
    di = [_dev(i) for i in im]
    first = None
    for k in range(10):
        dm = [_dev(x) for x in m]
        isa.DpSeamFinder(ctx).find(di, c, dm)
        got = [_np(x) for x in dm]
        if first is None:
            first = got
        assert all(np.array_equal(a, b) for a, b in zip(got, first)), "run %d differs from run 0" % k
    _check(first, "six", "ten runs")


def _c_call(ctx, images, corners, masks, n, cost_func=0):
    from image_stitching_amd import _capi as capi
    from image_stitching_amd.stitching import as_image
    k = max(1, len(masks))
    cs = (capi.MisPoint * k)(*[capi.MisPoint(int(c[0]), int(c[1])) for c in corners])
    im = (capi.MisImage * k)(*[as_image(i) for i in images])
    mk = (capi.MisImage * k)(*[as_image(m) for m in masks])
    return ctx.lib.mis_seam_dp(ctx.h, cs, im, mk, n, cost_func)


def test_no_image_and_one_image_leave_the_masks(ctx):
    import image_stitching_amd as isa
    im, c, m = scene("bytes")
    dm = _dev(m[0])
    assert _c_call(ctx, [_dev(im[0])], c[:1], [dm], 0) == 0
    assert np.array_equal(_np(dm), m[0])
    isa.DpSeamFinder(ctx).find([_dev(im[0])], c[:1], [dm])
    assert np.array_equal(_np(dm), m[0])
    hm = m[0].copy()
    isa.DpSeamFinder(ctx).find([im[0]], c[:1], [hm])
    assert np.array_equal(hm, m[0])


def test_refusals(ctx):
    """A cost function other than COLOR is MIS_E_UNSUPPORTED, an image / mask size mismatch MIS_E_INVALID; neither touches the
    masks, and the context serves a good call after."""
    import image_stitching_amd as isa
    im, c, m = scene("side_by_side")
    dm = [_dev(x) for x in m]
    di = [_dev(i) for i in im]
    assert _c_call(ctx, di, c, dm, 2, cost_func=1) == MIS_E_UNSUPPORTED
    with pytest.raises(isa.stitching.MisError) as e:
        isa.DpSeamFinder(ctx, 1).find(di, c, dm)
    assert e.value.code == MIS_E_UNSUPPORTED
    assert _c_call(ctx, di, c, [dm[0], dm[1][:-1]], 2) == MIS_E_INVALID
    assert _c_call(ctx, [di[0][:, :-1], di[1]], c, dm, 2) == MIS_E_INVALID
    for g, w in zip(dm, m):
        assert np.array_equal(_np(g), w)
    isa.DpSeamFinder(ctx).find(di, c, dm)
    _check(dm, "side_by_side", "after the refusals")
