"""GPU: DpSeamFinder(COLOR_GRAD) of the library against the numpy reference tests/refimpl_seam_dp_grad.py.
  * isa.seam_gradients (mis_seam_gradients; the kernel of csrc/seam_grad.hip) bit for bit, at the smallest shapes where its tiling,
    halo and border code can go wrong: one-pixel and one-line frames, 2 x 2 and 3 x 3, one below / at / one above the 64 x 16 tile
    in each dimension, several tiles, frames of different sizes in one call (the z-table), more frames than one launch holds;
    device tensors, host arrays, pitched views, mixed.
  * isa.DpSeamFinder(ctx, "COLOR_GRAD").find byte for byte on every scene of refimpl_seam_dp and on the edge scene, where it must
    also differ from the library's own COLOR masks -- the test that fails without the feature.
  * the refusals, and that neither finder leaves state behind for the other."""
import ctypes as C

import numpy as np
import pytest

import refimpl_seam_dp_grad as rg
from test_refimpl_seam_dp_cpu import NAMES, reference, scene
from test_refimpl_seam_dp_gpu import _c_call, _dev, _np, _pitched
from test_refimpl_seam_dp_grad_cpu import edge_reference, grad_reference

pytestmark = pytest.mark.gpu

MIS_E_INVALID, MIS_E_UNSUPPORTED = -1, -6
TW, TH = 64, 16                         # csrc/seam_grad.hip: SG_TW, SG_TH
SG_MAX = 32                             # frames per launch

SMALL = [(1, 1), (7, 1), (1, 7), (2, 2), (3, 3)]                                          # (w, h)
TILE_EDGES = [(w, h) for w in (TW - 1, TW, TW + 1) for h in (TH - 1, TH, TH + 1)]
SEVERAL_TILES = [(2 * TW + 3, 2 * TH + 5), (1, 3 * TH + 1), (3 * TW + 1, 1), (2, TH + 1), (TW + 1, 2)]
SHAPES = SMALL + TILE_EDGES + SEVERAL_TILES


def _image(w, h, seed):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if w * h > 4:
        img.reshape(-1, 3)[:: 5] = rng.integers(0, 2, (len(img.reshape(-1, 3)[:: 5]), 3)) * 255      # full-contrast steps among the noise
    return img


IMAGES = [_image(w, h, 100 + k) for k, (w, h) in enumerate(SHAPES)]
WANT = [rg.gradients(i) for i in IMAGES]                     # computed once, shared, never written
for _a in IMAGES + [p for g in WANT for p in g]:
    _a.setflags(write=False)


def _bits(a):
    return np.ascontiguousarray(_np(a), np.float32).view(np.uint32)


def _check_planes(gx, gy, want, what):
    assert len(gx) == len(gy) == len(want)
    for k, (x, y, (wx, wy)) in enumerate(zip(gx, gy, want)):
        for name, got, ref in (("gradx", x, wx), ("grady", y, wy)):
            g = _np(got)
            assert g.shape == ref.shape and g.dtype == np.float32
            bad = _bits(g) != ref.view(np.uint32)
            assert not bad.any(), "%s: %s of frame %d (%dx%d) differs in %d values, first at %s: %r, reference %r" % (
                what, name, k, ref.shape[1], ref.shape[0], bad.sum(), np.argwhere(bad)[0], g[tuple(np.argwhere(bad)[0])], ref[tuple(np.argwhere(bad)[0])])


def test_gradients_every_shape_in_one_call_device(ctx):
    """Frames of 19 different sizes on the grid's z: blocks outside a smaller frame leave, every frame has its own table entry."""
    import image_stitching_amd as isa
    gx, gy = isa.seam_gradients(ctx, [_dev(i) for i in IMAGES])
    assert all(g.is_cuda for g in gx + gy)
    _check_planes(gx, gy, WANT, "device, one call")


def test_gradients_every_shape_in_one_call_host(ctx):
    import image_stitching_amd as isa
    gx, gy = isa.seam_gradients(ctx, [i.copy() for i in IMAGES])
    assert all(isinstance(g, np.ndarray) for g in gx + gy)
    _check_planes(gx, gy, WANT, "host, one call")


@pytest.mark.parametrize("k", range(len(SMALL) + len(TILE_EDGES)), ids=["%dx%d" % s for s in SMALL + TILE_EDGES])
def test_gradients_one_frame_alone(ctx, k):
    """The grid is sized by the frame itself (in the joint call the largest frame sizes it)."""
    import image_stitching_amd as isa
    gx, gy = isa.seam_gradients(ctx, [_dev(IMAGES[k])])
    _check_planes(gx, gy, [WANT[k]], "alone")


def test_gradients_more_frames_than_one_launch(ctx):
    import image_stitching_amd as isa
    idx = [k % len(SHAPES) for k in range(SG_MAX + 3)]
    gx, gy = isa.seam_gradients(ctx, [_dev(IMAGES[k]) for k in idx])
    _check_planes(gx, gy, [WANT[k] for k in idx], "%d frames" % len(idx))


def _pitched_f32(w, h, device):
    """A float32 plane view at [1:1+h, 1:1+w] of a larger buffer full of a sentinel -> (holder, view, holder as filled)."""
    filled = np.full((h + 2, w + 3), -12345.5, np.float32)
    holder = _dev(filled) if device else filled.copy()
    return holder, holder[1:1 + h, 1:1 + w], filled


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_gradients_pitched_views(ctx, device):
    """Images that are slices of larger buffers at odd addresses, planes that are slices of larger float buffers: the same values,
    nothing outside a plane's view written, the images read only."""
    import image_stitching_amd as isa
    pi = [_pitched(i, device) for i in IMAGES]
    px = [_pitched_f32(w, h, device) for w, h in SHAPES]
    py = [_pitched_f32(w, h, device) for w, h in SHAPES]
    gx, gy = isa.seam_gradients(ctx, [p[1] for p in pi], [p[1] for p in px], [p[1] for p in py])
    _check_planes(gx, gy, WANT, "pitched views")
    for (holder, _, filled), (w, h) in zip(px + py, SHAPES + SHAPES):
        got = _np(holder).copy()
        got[1:1 + h, 1:1 + w] = filled[0, 0]
        assert np.array_equal(got, filled)
    for holder, _, filled in pi:
        assert np.array_equal(_np(holder), filled)


def test_gradients_mixed_host_and_device(ctx):
    """Images and planes alternate between host and device memory, an image and its planes on different sides."""
    import torch
    import image_stitching_amd as isa
    images = [_dev(i) if k % 2 else i.copy() for k, i in enumerate(IMAGES)]
    def planes(r):
        return [torch.empty((h, w), dtype=torch.float32, device="cuda") if k % 3 == r else np.empty((h, w), np.float32) for k, (w, h) in enumerate(SHAPES)]
    gx, gy = isa.seam_gradients(ctx, images, planes(0), planes(1))
    _check_planes(gx, gy, WANT, "mixed")


def _c_grad(ctx, images, gx, gy, n):
    from image_stitching_amd import _capi as capi
    from image_stitching_amd.stitching import as_image
    k = max(1, len(images))
    return ctx.lib.mis_seam_gradients(ctx.h, (capi.MisImage * k)(*[as_image(i) for i in images]), n,
                                      (capi.MisImage * k)(*[as_image(g) for g in gx]), (capi.MisImage * k)(*[as_image(g) for g in gy]))


def test_gradients_no_image_and_refusals(ctx):
    """n = 0 is MIS_OK and writes nothing; a size, type or channel mismatch anywhere in the call is MIS_E_INVALID and writes nothing,
    not even the planes of the good frames before it; the context serves a good call after."""
    import torch
    import image_stitching_amd as isa
    assert isa.seam_gradients(ctx, []) == ([], [])
    im = [_dev(IMAGES[5]), _dev(IMAGES[6])]
    def fresh():
        return [torch.full(tuple(i.shape[:2]), 7.0, dtype=torch.float32, device="cuda") for i in im]
    gx, gy = fresh(), fresh()
    assert _c_grad(ctx, im, gx, gy, 0) == 0
    bad_calls = [
        (im, [gx[0], gx[1][:-1]], gy),                                               # a plane one row short
        (im, gx, [gy[0], gy[1][:, :-1]]),                                            # a plane one column short
        ([im[0], im[1][:, :-1]], gx, gy),                                            # an image one column short
        (im, [gx[0], gx[1].to(torch.int16)], gy),                                    # a plane of another type
        ([im[0], im[1][:, :, 0].contiguous()], gx, gy),                                          # a one-channel image
        ([im[0], im[1].to(torch.float32)], gx, gy),                                  # a float image
    ]
    for a in bad_calls:
        assert _c_grad(ctx, *a, 2) == MIS_E_INVALID
        for g in gx + gy:
            assert bool((g == 7.0).all())
    assert ctx.lib.mis_seam_gradients(ctx.h, None, -1, None, None) == MIS_E_INVALID
    gx, gy = isa.seam_gradients(ctx, im)
    _check_planes(gx, gy, WANT[5:7], "after the refusals")


# ------------------------------------------------------------------------------------------------ the finder
def _check_masks(got, want, name, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g = _np(g)
        assert np.array_equal(g, w), "%s, %s: mask %d differs in %d pixels, first at %s" % (name, what, k, (g != w).sum(), np.argwhere(g != w)[0])


@pytest.mark.parametrize("name", NAMES + ["seam_scale"])
def test_colorgrad_masks_equal_reference(ctx, name):
    """Every scene, once with device tensors and once with host arrays (uploaded for the gradient kernel)."""
    import image_stitching_amd as isa
    im, c, m = scene(name)
    want = grad_reference(name)
    dm = [_dev(k) for k in m]
    isa.DpSeamFinder(ctx, "COLOR_GRAD").find([_dev(i) for i in im], c, dm)
    _check_masks(dm, want, name, "device tensors")
    hm = [k.copy() for k in m]
    isa.DpSeamFinder(ctx, isa.DpSeamFinder.COLOR_GRAD).find([i.copy() for i in im], c, hm)
    _check_masks(hm, want, name, "host arrays")


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("name", ["six", "near_edges", "bytes"])
def test_colorgrad_pitched_views_at_odd_addresses(ctx, name, device):
    import image_stitching_amd as isa
    im, c, m = scene(name)
    pi = [_pitched(i, device) for i in im]
    pm = [_pitched(k, device) for k in m]
    isa.DpSeamFinder(ctx, "COLOR_GRAD").find([p[1] for p in pi], c, [p[1] for p in pm])
    _check_masks([p[1] for p in pm], grad_reference(name), name, "pitched views")
    for (holder, _, filled), k in zip(pi + pm, im + m):
        got, want = _np(holder).copy(), filled.copy()
        got[1:1 + k.shape[0], 1:1 + k.shape[1]] = 0
        want[1:1 + k.shape[0], 1:1 + k.shape[1]] = 0
        assert np.array_equal(got, want)
    for holder, _, filled in pi:
        assert np.array_equal(_np(holder), filled)


def test_colorgrad_mixed_host_and_device_buffers(ctx):
    import image_stitching_amd as isa
    for name in ("six", "five"):
        im, c, m = scene(name)
        images = [_dev(i) if k % 2 else i.copy() for k, i in enumerate(im)]
        masks = [k_.copy() if k % 3 else _dev(k_) for k, k_ in enumerate(m)]
        isa.DpSeamFinder(ctx, "COLOR_GRAD").find(images, c, masks)
        _check_masks(masks, grad_reference(name), name, "mixed buffers")


def test_edge_scene_colorgrad_differs_from_color_and_equals_reference(ctx):
    """The library's COLOR_GRAD masks are not its COLOR masks (the option reaches the costs) and are the reference's."""
    import image_stitching_amd as isa
    (im, c, m), color, grad = edge_reference()
    di = [_dev(i) for i in im]
    mc, mg, ms = [_dev(k) for k in m], [_dev(k) for k in m], [_dev(k) for k in m]
    isa.DpSeamFinder(ctx, "COLOR").find(di, c, mc)
    isa.DpSeamFinder(ctx, "COLOR_GRAD").find(di, c, mg)
    isa.DpSeamFinder(ctx).find(di, c, ms)
    _check_masks(mc, color, "edge", "COLOR by name")
    _check_masks(ms, color, "edge", "COLOR by default")
    _check_masks(mg, grad, "edge", "COLOR_GRAD")
    assert any(not np.array_equal(_np(a), _np(b)) for a, b in zip(mc, mg))


def test_refusals_and_no_state_between_the_finders(ctx):
    """A size mismatch is MIS_E_INVALID with the masks untouched; the old entry keeps refusing cost_func = 1; the context serves a
    good COLOR and a good COLOR_GRAD call afterwards; a COLOR call after a COLOR_GRAD call gives COLOR's bytes."""
    import image_stitching_amd as isa
    from image_stitching_amd import _capi as capi
    from image_stitching_amd.stitching import as_image

    def c_grad_call(images, corners, masks, n):
        k = max(1, len(masks))
        return ctx.lib.mis_seam_dp_colorgrad(ctx.h, (capi.MisPoint * k)(*[capi.MisPoint(int(c[0]), int(c[1])) for c in corners]),
                                             (capi.MisImage * k)(*[as_image(i) for i in images]), (capi.MisImage * k)(*[as_image(m) for m in masks]), n)
    im, c, m = scene("side_by_side")
    dm = [_dev(x) for x in m]
    di = [_dev(i) for i in im]
    assert c_grad_call(di, c, [dm[0], dm[1][:-1]], 2) == MIS_E_INVALID
    assert c_grad_call([di[0][:, :-1], di[1]], c, dm, 2) == MIS_E_INVALID
    assert c_grad_call(di, c, dm, 0) == 0
    assert _c_call(ctx, di, c, dm, 2, cost_func=1) == MIS_E_UNSUPPORTED
    with pytest.raises(isa.stitching.MisError) as e:
        isa.DpSeamFinder(ctx, 1).find(di, c, dm)
    assert e.value.code == MIS_E_UNSUPPORTED
    for g, w in zip(dm, m):
        assert np.array_equal(_np(g), w)
    color_want, grad_want = reference("side_by_side")[0], grad_reference("side_by_side")
    assert any(not np.array_equal(a, b) for a, b in zip(color_want, grad_want))
    for kind, want in (("COLOR", color_want), ("COLOR_GRAD", grad_want), ("COLOR", color_want), ("COLOR_GRAD", grad_want), ("COLOR", color_want)):
        dm = [_dev(x) for x in m]
        isa.DpSeamFinder(ctx, kind).find(di, c, dm)
        _check_masks(dm, want, "side_by_side", "%s in the sequence" % kind)
    # a large COLOR_GRAD call, then a small COLOR call on host buffers: the staging grown for the planes carries nothing over
    im2, c2, m2 = scene("seam_scale")
    dm2 = [_dev(x) for x in m2]
    isa.DpSeamFinder(ctx, "COLOR_GRAD").find([_dev(i) for i in im2], c2, dm2)
    _check_masks(dm2, grad_reference("seam_scale"), "seam_scale", "COLOR_GRAD")
    hm = [x.copy() for x in m]
    isa.DpSeamFinder(ctx, "COLOR").find([i.copy() for i in im], c, hm)
    _check_masks(hm, color_want, "side_by_side", "COLOR on host buffers after COLOR_GRAD")
