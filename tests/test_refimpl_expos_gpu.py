"""GPU: the kernels of the step between warp and blend (expos.hip: overlap statistics, gain application; seam_voronoi.hip: the
Voronoi distance scans; imgops.hip: the fused seam-mask kernel) against the numpy reference of tests/refimpl_expos.py, over the scenes and block
geometries of test_refimpl_expos_cpu.py: gain maps within the derived float32 bound, Voronoi and seam masks exactly, every
applied byte inside its candidate range; then the memory forms (dense device tensors, host arrays, pitched device views that
start at an odd address), which must agree byte for byte and leave everything outside a view untouched."""
import numpy as np
import pytest

import refimpl_expos as rx
from test_refimpl_expos_cpu import PARAM_IDS, apply_images, check_candidates, one_sample_apply, ref_maps, scene

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def _pitched(a):
    """-> (holder, view, holder as filled): `a` at [1:1+h, 1:1+w] of a larger device tensor full of a sentinel pattern.  The holder's
    width is even, so the row pitch exceeds the row and the view's first byte (8-bit types) sits at an odd address."""
    import torch
    h, w = a.shape[:2]
    shape = (h + 2, w + 2 + w % 2) + a.shape[2:]
    filled = (np.arange(int(np.prod(shape)), dtype=np.int64) % 251 + 1).astype(a.dtype).reshape(shape)
    filled[1:1 + h, 1:1 + w] = a
    holder = torch.from_numpy(filled.copy()).cuda()
    view = holder[1:1 + h, 1:1 + w]
    assert view.stride(0) * view.element_size() > a.shape[1] * a[0, 0].nbytes
    assert a.itemsize != 1 or view.data_ptr() % 2 == 1
    return holder, view, filled


def _outside_untouched(holder, filled, h, w):
    got = holder.cpu().numpy().copy()
    want = filled.copy()
    got[1:1 + h, 1:1 + w] = 0
    want[1:1 + h, 1:1 + w] = 0
    return np.array_equal(got, want)


def _fed(ctx, name, params):
    from image_stitching_amd import stitching as S
    corners, images, masks = scene(name)
    comp = S.BlocksGainCompensator(ctx, *params)
    comp.feed(corners, [_dev(i) for i in images], [_dev(m) for m in masks])
    return comp


@pytest.mark.parametrize("params", rx.PARAMS, ids=PARAM_IDS)
def test_gain_maps_match_reference(ctx, params):
    worst = 0.0
    for name in rx.SCENES:
        grid, maps = ref_maps(name, params)
        comp = _fed(ctx, name, params)
        for k, ref in enumerate(maps):
            got = comp.gain_map(k)
            assert got.dtype == np.float32 and got.shape == ref.shape, (name, k, got.shape, ref.shape)
            err = float(np.abs(got.astype(np.float64) - ref).max())
            worst = max(worst, err / (rx.U24 * np.abs(ref).max()))
            assert err <= rx.gain_map_tol(ref, params[2]), (name, k, err, rx.gain_map_tol(ref, params[2]))
            if name in rx.ALL_ONES:
                assert np.all(got == np.float32(1)), name
    print("gain maps %s: max |kernel - ref| = %.2f x 2^-24 max|map| (bound %d)" % (params, worst, 1 + 4 * params[2]))


@pytest.mark.parametrize("name", list(rx.SCENES))
def test_voronoi_matches_reference(ctx, name):
    from image_stitching_amd import stitching as S
    corners, _, masks = scene(name)
    want = rx.voronoi(corners, masks)
    ms = [_dev(m) for m in masks]
    S.VoronoiSeamFinder(ctx).find(None, corners, ms)
    for k, (g, w) in enumerate(zip(ms, want)):
        g = g.cpu().numpy()
        assert np.array_equal(g, w), (name, k, int((g != w).sum()))


@pytest.mark.parametrize("name", ["three_way", "tiny"])
def test_apply_inside_candidates(ctx, name):
    """Images larger than the map, of its own size, smaller, one row high, one column wide (517 wide: a second blockIdx.x)."""
    comp = _fed(ctx, name, (64, 64, 2))
    gmap = comp.gain_map(0)
    if name == "tiny":
        assert gmap.shape == (1, 1)
    for im in apply_images(gmap.shape):
        t8 = _dev(im)
        comp.apply(0, (0, 0), t8)
        got = t8.cpu().numpy()
        share = check_candidates(got, gmap, im, "%s %s" % (name, im.shape))
        if name == "tiny":
            assert np.array_equal(got, one_sample_apply(gmap, im)), im.shape
        print("apply %s map %s image %s: %.3f %% undecided" % (name, gmap.shape, im.shape[:2], 100 * share))
        t16 = _dev(im.astype(np.int16))
        comp.apply(0, (0, 0), t16)
        assert np.array_equal(t16.cpu().numpy(), got.astype(np.int16)), im.shape
        host8, host16 = im.copy(), im.astype(np.int16)
        comp.apply(0, (0, 0), host8)
        comp.apply(0, (0, 0), host16)
        assert np.array_equal(host8, got) and np.array_equal(host16, got.astype(np.int16)), im.shape


def _run_form(ctx, name, form):
    """feed -> gain maps, apply (8UC3 and 16SC3, the fed size and another), Voronoi, seam_mask_apply, with every image and mask in
    one memory form -> the outputs as numpy arrays."""
    from image_stitching_amd import stitching as S
    corners, images, masks = scene(name)
    rng = np.random.default_rng(9)
    holders = []

    def put(a):
        if form == "host":
            return np.array(a)
        if form == "dense":
            return _dev(a)
        holder, view, filled = _pitched(a)
        holders.append((holder, filled, a.shape[0], a.shape[1]))
        return view

    def get(t):
        return t if isinstance(t, np.ndarray) else t.cpu().numpy()

    out = {}
    comp = S.BlocksGainCompensator(ctx, 64, 64, 2)
    comp.feed(corners, [put(i) for i in images], [put(m) for m in masks])
    out["maps"] = [comp.gain_map(k) for k in range(len(images))]
    other = rng.integers(0, 256, (2 * images[0].shape[0] - 3, 2 * images[0].shape[1] - 5, 3)).astype(np.uint8)
    for tag, im in (("fed", images[0]), ("other", other)):
        for dt in (np.uint8, np.int16):
            t = put(im.astype(dt))
            comp.apply(0, corners[0], t)
            out["apply-%s-%s" % (tag, np.dtype(dt).name)] = get(t)
    ms = [put(m) for m in masks]
    S.VoronoiSeamFinder(ctx).find(None, corners, ms)
    out["voronoi"] = [get(m) for m in ms]
    compose = rng.integers(0, 2, (3 * masks[0].shape[0] - 2, 3 * masks[0].shape[1] - 1)).astype(np.uint8) * 255
    compose[rng.random(compose.shape) < 0.6] = 255
    cm = put(compose)
    S.seam_mask_apply(ctx, put(out["voronoi"][0]), cm)
    out["seam"] = get(cm)
    for holder, filled, h, w in holders:
        assert _outside_untouched(holder, filled, h, w), "%s: bytes outside a %dx%d view changed" % (name, w, h)
    out["inputs"] = (images[0], other, compose)
    return out


@pytest.mark.parametrize("name", ["three_way", "byte_masks", "thin_col"])
def test_memory_forms_agree(ctx, name):
    corners, images, masks = scene(name)
    dense = _run_form(ctx, name, "dense")
    # the dense outputs against the reference
    _, maps = ref_maps(name, (64, 64, 2))
    for got, ref in zip(dense["maps"], maps):
        assert np.abs(got - ref).max() <= rx.gain_map_tol(ref, 2)
    fed, other, compose = dense["inputs"]
    check_candidates(dense["apply-fed-uint8"], dense["maps"][0], fed, name + " fed")
    check_candidates(dense["apply-other-uint8"], dense["maps"][0], other, name + " other")
    want = rx.voronoi(corners, masks)
    assert all(np.array_equal(g, w) for g, w in zip(dense["voronoi"], want))
    assert np.array_equal(dense["seam"], rx.seam_mask_apply(want[0], compose))
    assert dense["seam"].any()
    if name != "thin_col":                       # a cut one pixel wide is closed again by the dilate
        assert (dense["seam"] != compose).any()
    # the other forms against the dense one, byte for byte
    for form in ("host", "pitched"):
        alt = _run_form(ctx, name, form)
        for key in dense:
            if key == "inputs":
                continue
            a, b = dense[key], alt[key]
            if isinstance(a, list):
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (form, key)
            else:
                assert a.dtype == b.dtype and np.array_equal(a, b), (form, key)
        assert np.array_equal(alt["apply-other-int16"], alt["apply-other-uint8"].astype(np.int16)), form


@pytest.mark.parametrize("geometry", rx.SEAM_GEOMETRIES, ids=lambda g: "%dx%d-to-%dx%d" % (g[0] + g[1]))
def test_seam_mask_apply_matches_reference(ctx, geometry):
    """Up, down, same size, the ragged tails of the 4-pixels-per-thread loop (widths 1, 2, 3, 5) and a 1 x 1 seam mask; 0 / 255
    masks and masks of arbitrary bytes (the AND is on bytes)."""
    from image_stitching_amd import stitching as S
    for byte_values in (False, True):
        seam, mask = rx.seam_case(geometry, byte_values)
        want = rx.seam_mask_apply(seam, mask)
        m = _dev(mask)
        S.seam_mask_apply(ctx, _dev(seam), m)
        got = m.cpu().numpy()
        assert np.array_equal(got, want), (byte_values, int((got != want).sum()))
        host = mask.copy()
        S.seam_mask_apply(ctx, seam.copy(), host)
        assert np.array_equal(host, want), byte_values
