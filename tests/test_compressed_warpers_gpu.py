"""The compressed-plane and Panini warpers (HIP, the column-hoisted map kernels) against the float64 numpy reference of
tests/refimpl_compressed_warpers.py: the device roi scan equals the host scan and lies in the reference sets (tiny sources up to two
4K frames in one call), the fused single / batched and general warps lie within the reference candidates on every case and on the
smallest shapes at which the tile code can go wrong, the kernels' map equals the unsplit per-pixel sequence bit for bit, and the
refusals.  Every test here needs MIS_WARP_COMPRESSED_PLANE_A2B1 .. MIS_WARP_PANINI_A15B1: on a library without them each fails with
MIS_E_UNSUPPORTED."""
import ctypes as C
import functools

import numpy as np
import pytest

import refimpl as ri
import refimpl_compressed_warpers as rc

pytestmark = pytest.mark.gpu

MAX_BAND_SHARE = 0.40            # refimpl's limits (test_warpers_gpu.py)
MAX_UNDETERMINED_SHARE = 0.10
KINDS = [pytest.param(k, id=n) for n, k in rc.KINDS.items()]
SOURCES = [pytest.param(w, h, m, id="%dx%d-s%g" % (w, h, m)) for w, h, m in rc.sources()]
T = rc.T                         # the fused tile's height (warp.hip: PC_TH)


def _ties(maps, q):
    t = np.zeros(maps["x"].shape, bool)
    for c in ("x", "y"):
        t |= np.abs(np.modf(maps[c] * q)[0]) == 0.5
    return t


def _check(tag, out, cands, band, und, ties=None):
    bad, nb, nu = ri.check_candidates(out, cands, band, und)
    n = bad.size
    nt = int((band & ~und & ties).sum()) if ties is not None else 0
    print("%s: %d px, in band %d (%.2f %%; exact ties %d), undetermined %d (%.2f %%)" % (tag, n, nb, 100.0 * nb / n, nt, nu, 100.0 * nu / n))
    assert not bad.any(), "%s: %d pixels outside the reference candidates, first at %s" % (tag, int(bad.sum()), np.argwhere(bad)[0])
    if n >= 256:
        assert nb - nt <= MAX_BAND_SHARE * n and nu <= MAX_UNDETERMINED_SHARE * n, tag


def _warper(ctx, kind, scale):
    import image_stitching_amd as isa
    cls = isa.PaniniWarper if rc.is_panini(kind) else isa.CompressedRectilinearWarper
    return cls(ctx, scale, *rc.AB[kind])


def _roi_single(kind, scale, w, h, K, R):
    from image_stitching_amd import _capi as capi
    r = capi.MisRect()
    K, R = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(R, np.float32)
    rv = capi.load().mis_warper_roi(kind, float(scale), w, h, K.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.byref(r))
    return rv, (r.x, r.y, r.width, r.height)


def _roi_batch(ctx, kind, scale, w, h, Ks, Rs):
    from image_stitching_amd import _capi as capi
    n = len(Ks)
    Ks = np.ascontiguousarray(np.stack([np.asarray(k, np.float32).reshape(9) for k in Ks]))
    Rs = np.ascontiguousarray(np.stack([np.asarray(r, np.float32).reshape(9) for r in Rs]))
    rr = (capi.MisRect * n)()
    rv = ctx.lib.mis_warper_roi_batch(ctx.h, kind, float(scale), w, h, n, Ks.ctypes.data_as(C.c_void_p), Rs.ctypes.data_as(C.c_void_p), rr)
    return rv, [(r.x, r.y, r.width, r.height) for r in rr]


def _warp_roi(ctx, kind, src, scale, K, R, roi, interp, border):
    """mis_warper_warp_roi of a device tensor into a fresh device image of the roi's size -> (tl, numpy output)."""
    import torch
    from image_stitching_amd import _capi as capi, stitching as st
    simg = st.as_image(src)
    dst = st._empty_image(ctx, roi[3], roi[2], simg.channels, torch.uint8)
    rr, tl = capi.MisRect(*[int(v) for v in roi]), capi.MisPoint()
    ctx.check(ctx.lib.mis_warper_warp_roi(ctx.h, kind, C.byref(simg), float(scale), st._mat9(K)[1], st._mat9(R)[1], C.byref(rr), interp, border,
                                          C.byref(st.as_image(dst)), C.byref(tl)))
    return (tl.x, tl.y), dst.cpu().numpy()


def _map(ctx, kind, scale, K, R, roi):
    """mis_debug_warper_map_f32: the unsplit sequence on the host (ctx None) or the kernels' tile walk -> (h, w, 2) float32."""
    from image_stitching_amd import _capi as capi
    K, R = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(R, np.float32)
    xy = np.full((roi[3], roi[2], 2), np.nan, np.float32)
    rr = capi.MisRect(*[int(v) for v in roi])
    rv = capi.load().mis_debug_warper_map_f32(ctx.h if ctx is not None else None, kind, float(scale), K.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p),
                                              C.byref(rr), xy.ctypes.data_as(C.c_void_p))
    assert rv == 0, rv
    return xy


@functools.lru_cache(maxsize=None)
def _ref_rois(kind, w, h, mult):
    """The reference's roi candidates of every geometry of one source: computed once, shared by the tests below."""
    return [(name, K, R, scale, rc.warp_roi_f64(kind, scale, w, h, K, R)) for name, K, R, scale in rc.geometry_cases(w, h, mult)]


def _cases(ctx, kind, w, h, mult):
    """-> [(name, K, R, scale, roi)] of the geometries whose roi the library accepts; the device (batch, frame alone: a refused
    frame fails its whole call) roi equals the host (single) roi, both lie in the reference sets where the reference decides, and
    both refuse where it says refused -- asserted on the way."""
    out = []
    for name, K, R, scale, ref in _ref_rois(kind, w, h, mult):
        rv, roi = _roi_single(kind, scale, w, h, K, R)
        brv, (broi,) = _roi_batch(ctx, kind, scale, w, h, [K], [R])
        assert brv == rv and (rv != 0 or broi == roi), (name, rv, brv, roi, broi)
        if ref["refused"] is True:
            assert rv == -1, name
        elif ref["refused"] is False:
            assert rv == 0 and rc.roi_matches(roi, ref), (name, roi, ref.get("intervals"))
            out.append((name, K, R, scale, roi))
    return out


def _warped(cases, kind, w, h, mult):
    return [c for c in cases if c[4][2] * c[4][3] <= rc.MAX_REF_PIXELS and (kind, w, h, mult, c[0]) not in rc.WARP_DROPPED]


# ------------------------------------------------------------------------------------------------ roi
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_roi_device_scan_equals_host_scan_within_reference(ctx, kind, w, h, mult):
    """mis_warper_roi_batch (the grid-wide device reduction) against mis_warper_roi (the host loop) and the reference's candidate
    sets; the accepted geometries of one scale once more in ONE call, several cameras per launch."""
    cases = _cases(ctx, kind, w, h, mult)
    assert len(cases) >= 6
    scales = [c[3] for c in cases]
    scale = max(set(scales), key=scales.count)
    same = [c for c in cases if c[3] == scale]
    rv, rois = _roi_batch(ctx, kind, scale, w, h, [c[1] for c in same], [c[2] for c in same])
    assert rv == 0 and rois == [c[4] for c in same] and len(same) >= 4


@pytest.mark.parametrize("kind", KINDS)
def test_roi_two_4k_frames_in_one_call(ctx, kind):
    """Two 3840 x 2160 frames (yaw 5 pitch 2, roll+30) in one batch call: 720 workgroups per frame, two frames per launch."""
    w, h, geoms = rc.FRAMES_4K
    cams = [ri.camera(w, h, *g) for g in geoms]
    scale = cams[0][2]
    assert cams[1][2] == scale
    rv, rois = _roi_batch(ctx, kind, scale, w, h, [c[0] for c in cams], [c[1] for c in cams])
    assert rv == 0, ctx.lib.mis_last_error(ctx.h)
    for (K, R, _), roi, g in zip(cams, rois, geoms):
        ref = rc.warp_roi_f64(kind, scale, w, h, K, R)
        assert rc.roi_matches(roi, ref), (g, roi, ref.get("intervals"))
    assert _roi_single(kind, scale, w, h, cams[1][0], cams[1][1]) == (0, rois[1])      # (one host scan of 8.3 M pixels)
    rv, swapped = _roi_batch(ctx, kind, scale, w, h, [c[0] for c in cams[::-1]], [c[1] for c in cams[::-1]])
    assert rv == 0 and swapped == rois[::-1]


# ------------------------------------------------------------------------------------------------ the hoist
@pytest.mark.parametrize("kind", KINDS)
def test_hoisted_map_equals_the_unsplit_sequence_bit_for_bit(ctx, kind):
    """The kernels' tile walk (column terms once per column) against the host's evaluation of the reference's unsplit per-pixel
    sequence with the same dev_math.h functions: every float of (x, y) equal in every bit.  The rois straddle u = 0 with the
    column u = 0 at each of a lane's 4 column slots (the Panini |lam| <= 1e-7 branch in one lane beside the other branch), in the
    first lane and past a tile; heights 1, T - 1, T, T + 1, 2 T + 1; a 4K-scale camera turned so that cos(lam) changes sign inside."""
    shapes = [(-4, 9, 1), (-5, 11, T - 1), (-6, 130, T), (-7, 257, T + 1), (-130, 261, 2 * T + 1), (-129, 131, 3), (-3, 4, 5), (-2, 3, 2)]
    for w, h, hfov, yaw, pitch, roll, mult in ((65, 9, 60.0, 3.0, 2.0, 5.0, 1.0), (3840, 2160, 60.0, 80.0, -4.0, 0.0, 1.0), (333, 217, 90.0, -20.0, 30.0, 10.0, 0.37)):
        K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, mult, seam=mult < 1)
        for x0, rw, rh in shapes:
            roi = (x0, -(rh // 3), rw, rh)
            host, dev = _map(None, kind, scale, K, R, roi), _map(ctx, kind, scale, K, R, roi)
            assert not np.isnan(host).any()
            assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)), (w, roi, np.argwhere(host.view(np.uint32) != dev.view(np.uint32))[0])
    # a roi whose columns run past lam = 90 degrees (u' = a tan(90 / a): 2 scale for a = 2, 2.6 scale for a = 1.5)
    K, R, scale = ri.camera(65, 9, 60.0, 100.0, 0.0, 0.0)
    roi = (int(1.8 * scale), -20, int(1.2 * scale), 41)
    host, dev = _map(None, kind, scale, K, R, roi), _map(ctx, kind, scale, K, R, roi)
    assert (host[..., 0] >= 0).any() and np.array_equal(host.view(np.uint32), dev.view(np.uint32))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_and_a_good_call_afterwards(ctx, kind):
    """A projection past what an int holds (scale 1e10, 1e36) gives MIS_E_INVALID from both roi entries, alone and beside a good
    frame, and from the warps; a roi of area >= 2^31 is returned by the roi entries and refused by the warp entries; a `known` roi
    of another size than the destination is MIS_E_INVALID; a non-8UC3 source to the fused entries MIS_E_UNSUPPORTED; an unknown
    kind stays MIS_E_UNSUPPORTED; the context serves a good call afterwards."""
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd import _capi as capi, stitching as st
    w, h = 64, 8
    K, R, scale = ri.camera(w, h, 60.0, 0.0)
    for bad in (1e10, 1e36):
        assert rc.warp_roi_f64(kind, bad, w, h, K, R)["refused"] is True
        assert _roi_single(kind, bad, w, h, K, R)[0] == -1
        assert _roi_batch(ctx, kind, bad, w, h, [K], [R])[0] == -1
    # the refused roi beside a good frame: a compressed-plane frame across u_ = 90 degrees (test_refimpl_compressed_warpers_cpu.py),
    # for Panini a camera whose sin(u_) passes 0 behind it (u_ = 180 degrees: tg = a tan(90 degrees) for a = 2) at a scale past 2^31 / tg
    if rc.is_panini(kind):
        bK, bR, bscale = K, ri.camera(w, h, 60.0, 179.0)[1], 1e8
    else:
        bK, bR, _ = ri.camera(w, h, 120.0, 50.0, 10.0, 0.0)
        bscale = 1e8
    assert rc.warp_roi_f64(kind, bscale, w, h, bK, bR)["refused"] is True and rc.warp_roi_f64(kind, bscale, w, h, K, R)["refused"] is False
    assert _roi_batch(ctx, kind, bscale, w, h, [K], [R])[0] == 0
    assert _roi_batch(ctx, kind, bscale, w, h, [K, bK], [R, bR])[0] == -1 and _roi_batch(ctx, kind, bscale, w, h, [bK, K], [bR, R])[0] == -1
    src = torch.from_numpy(ri.content("rand", (h, w, 3), seed=3)).cuda()
    with pytest.raises(isa.MisError):
        _warper(ctx, kind, 1e10).warp_fused(src, K, R)
    with pytest.raises(isa.MisError):
        _warper(ctx, kind, 1e10).warp(src, K, R)
    # an enormous roi: scale 3e5 (u spans 3.5e5 columns, v 4e4 rows)
    big_scale = 3e5
    rv, (roi,) = _roi_batch(ctx, kind, big_scale, w, h, [K], [R])
    assert rv == 0 and (0, roi) == _roi_single(kind, big_scale, w, h, K, R) and roi[2] * roi[3] >= 2 ** 31, roi
    assert rc.roi_matches(roi, rc.warp_roi_f64(kind, big_scale, w, h, K, R))
    small_dst, small_msk = _warper(ctx, kind, big_scale).alloc_fused((0, 0, 8, 8))
    for known in (roi, None):       # refused for the roi's area (setup), before the destination's size is looked at
        with pytest.raises(isa.MisError) as e:
            _warper(ctx, kind, big_scale).warp_fused_into(src, K, R, known, small_dst, small_msk)
        assert e.value.code == -1 and "degenerate warp roi %dx%d" % (roi[2], roi[3]) in str(e.value), str(e.value)
    small_u8 = st._empty_image(ctx, 8, 8, 3, torch.uint8)
    for known in (None, roi):       # the general warp, computing its own roi and with the enormous one handed over
        rr, tl = capi.MisRect(*roi), capi.MisPoint()
        args = (ctx.h, kind, C.byref(st.as_image(src)), float(big_scale), st._mat9(K)[1], st._mat9(R)[1])
        tail = (isa.INTER_LINEAR, isa.BORDER_REFLECT, C.byref(st.as_image(small_u8)), C.byref(tl))
        rv = ctx.lib.mis_warper_warp(*args, *tail) if known is None else ctx.lib.mis_warper_warp_roi(*args, C.byref(rr), *tail)
        assert rv == -1 and b"degenerate warp roi" in ctx.lib.mis_last_error(ctx.h), (rv, ctx.lib.mis_last_error(ctx.h))
    # a known roi of another size than the destination; a one-channel source to the fused entries, single and batched
    warper = _warper(ctx, kind, scale)
    good = warper.warp_roi((w, h), K, R)
    dst, msk = warper.alloc_fused(good)
    with pytest.raises(isa.MisError) as e:
        warper.warp_fused_into(src, K, R, (good[0], good[1], good[2] + 1, good[3]), dst, msk)
    assert e.value.code == -1
    gray = torch.from_numpy(ri.content("rand", (h, w), seed=4)).cuda()
    with pytest.raises(isa.MisError) as e:
        warper.warp_fused_into(gray, K, R, good, dst, msk)
    assert e.value.code == -6
    with pytest.raises(isa.MisError) as e:
        warper.warp_fused_batch([src, gray], [{"K": K, "R": R}] * 2, [good, good])
    assert e.value.code == -6
    for unknown in (6, 7):
        assert _roi_batch(ctx, unknown, scale, w, h, [K], [R])[0] == -6
    # the context serves a good call afterwards
    tl, out, m = warper.warp_fused(src, K, R)
    tl2 = warper.warp_fused_into(src, K, R, good, dst, msk)
    ctx.synchronize()
    assert tl == tl2 == good[:2] and torch.equal(out, dst) and torch.equal(m, msk)


# ------------------------------------------------------------------------------------------------ warps
def _check_fused(tag, kind, img, K, R, scale, tl, out, msk, roi, maps=None):
    out = out.cpu().numpy()
    msk = msk.cpu().numpy()
    h, w = img.shape[:2]
    assert (tl[0], tl[1], out.shape[1], out.shape[0]) == tuple(roi)
    assert out.min() >= 0 and out.max() <= 255
    maps = maps or rc.backward_f64(kind, K, R, scale, roi)
    _check(tag + " linear", out.astype(np.uint8), *ri.remap_linear_reflect_candidates(img, maps), ties=_ties(maps, 32.0))
    _check(tag + " mask", msk, *ri.remap_nearest_constant_candidates(np.full((h, w), 255, np.uint8), maps), ties=_ties(maps, 1.0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_fused_single_batched_and_general_vs_reference(ctx, kind, w, h, mult):
    """mis_warper_warp_fused (its own device roi scan), mis_warper_warp_fused_roi per geometry and mis_warper_warp_fused_batch over
    three geometries of one scale with different roi sizes in one grid: within the reference candidates, and byte-identical to
    each other; the mask equals the general NEAREST / CONSTANT warp of an all-255 mask, and the 3-channel LINEAR / REFLECT general
    warp equals the fused image wherever the map is inside the source; random, all-255 and all-0 content."""
    import torch
    import image_stitching_amd as isa
    accepted = _cases(ctx, kind, w, h, mult)
    cases = _warped(accepted, kind, w, h, mult)
    assert len(cases) >= 4
    singles = {}
    for k, (name, K, R, scale, roi) in enumerate(cases):
        warper = _warper(ctx, kind, scale)
        img = ri.content(("rand", "full", "zero")[k % 3] if k else "rand", (h, w, 3), seed=k + 17 * w + h)
        src = torch.from_numpy(img).cuda()
        tl, out, msk = warper.warp_fused(src, K, R, roi)
        tl2, out2, msk2 = warper.warp_fused(src, K, R)             # computes its own roi: the device scan
        ctx.synchronize()
        assert tl2 == tl and torch.equal(out2, out) and torch.equal(msk2, msk), name
        _check_fused("fused k%d %dx%d s%g %s" % (kind, w, h, mult, name), kind, img, K, R, scale, tl, out, msk, roi)
        mtl, gm = _warp_roi(ctx, kind, torch.full((h, w), 255, dtype=torch.uint8).cuda(), scale, K, R, roi, isa.INTER_NEAREST, isa.BORDER_CONSTANT)
        assert mtl == tl and np.array_equal(gm, msk.cpu().numpy()), name
        gtl, gi = _warp_roi(ctx, kind, src, scale, K, R, roi, isa.INTER_LINEAR, isa.BORDER_REFLECT)
        inside = gm == 255
        assert gtl == tl and np.array_equal(gi[inside], out.cpu().numpy()[inside].astype(np.uint8)), name
        singles[name] = (src, tl, out, msk)
    # the batch: three accepted geometries of the most frequent scale (hfov 60) with different roi sizes, the warped ones first; one
    # that is not compared with the reference (dropped, or larger than MAX_REF_PIXELS) is compared with its single call only
    scales = [c[3] for c in accepted]
    scale = max(set(scales), key=scales.count)
    pool = [c for c in cases if c[3] == scale] + [c for c in accepted if c[3] == scale and c not in cases and c[4][2] * c[4][3] <= 4_000_000]
    batch = []
    for c in pool:
        if c[4][2:] not in [b[4][2:] for b in batch] and len(batch) < 3:
            batch.append(c)
    assert len(batch) == 3
    warper = _warper(ctx, kind, scale)
    for name, K, R, _, roi in batch:
        if name not in singles:
            src = torch.from_numpy(ri.content("rand", (h, w, 3), seed=len(name) + w)).cuda()
            singles[name] = (src,) + warper.warp_fused(src, K, R, roi)
    res = warper.warp_fused_batch([singles[c[0]][0] for c in batch], [{"K": c[1], "R": c[2]} for c in batch], [c[4] for c in batch])
    ctx.synchronize()
    for c, (tl, out, msk) in zip(batch, res):
        s1 = singles[c[0]]
        assert tl == s1[1] and torch.equal(out, s1[2]) and torch.equal(msk, s1[3]), c[0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_general_modes_vs_reference(ctx, kind, w, h, mult, cn):
    """mis_warper_warp (1 and 3 channels): INTER_LINEAR + BORDER_REFLECT and INTER_NEAREST + BORDER_CONSTANT, on the sources and
    geometries of the fused test; random, all-255 and all-0 content in turn."""
    import torch
    import image_stitching_amd as isa
    for k, (name, K, R, scale, roi) in enumerate(_warped(_cases(ctx, kind, w, h, mult), kind, w, h, mult)):
        img = ri.content(("rand", "full", "zero")[k % 3], (h, w) if cn == 1 else (h, w, 3), seed=5 * k + cn)
        warper = _warper(ctx, kind, scale)
        maps = rc.backward_f64(kind, K, R, scale, roi)
        for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
            tl, out = warper.warp(torch.from_numpy(img).cuda(), K, R, interp, border)
            out = out.cpu().numpy()
            assert (tl[0], tl[1], out.shape[1], out.shape[0]) == roi
            fn = ri.remap_linear_reflect_candidates if interp == isa.INTER_LINEAR else ri.remap_nearest_constant_candidates
            _check("warp k%d cn%d %dx%d s%g %s %s" % (kind, cn, w, h, mult, name, "linear" if interp == isa.INTER_LINEAR else "nearest"),
                   out, *fn(img, maps), ties=_ties(maps, 32.0 if interp == isa.INTER_LINEAR else 1.0))


@functools.lru_cache(maxsize=None)
def _shape_setup(kind):
    """refimpl_compressed_warpers.EDGE_SHAPES (the smallest shapes at which the tile code can go wrong) on its 65 x 9 seam-scale
    camera, with the float64 maps of every shape: computed once for the tests below."""
    K, R, scale, img, rois = rc.edge_shape_setup(kind)
    return K, R, scale, img, rois, [rc.backward_f64(kind, K, R, scale, r) for r in rois]


def _strided_source(img):
    """The image as a device view with an odd start (3 bytes in) and a row pitch wider than the row."""
    import torch
    h, w = img.shape[:2]
    pitch = 3 * w + 13
    buf = torch.zeros(h * pitch + 16, dtype=torch.uint8).cuda()
    view = buf[3:3 + h * pitch].as_strided((h, w, 3), (pitch, 3, 1), 3)
    view.copy_(torch.from_numpy(img).cuda())
    assert view.data_ptr() % 2 == 1
    return view


@pytest.mark.parametrize("kind", KINDS)
def test_edge_shapes_fused_single_batch_and_pitched_rows(ctx, kind):
    """Every shape through the single fused warp from the odd-start strided source (within the reference candidates), all 18 of
    them in one batch call (two launches: 16 + 2 frames of different sizes) from the dense source byte-identical to the single
    calls (the odd start takes the source loads' narrow path), and once more into destinations with a row pitch of the roi's width plus a few elements, whose guard fill must stay
    untouched."""
    import torch
    K, R, scale, img, rois, maps = _shape_setup(kind)
    warper = _warper(ctx, kind, scale)
    src = torch.from_numpy(img).cuda()
    odd = _strided_source(img)
    singles = []
    for roi, mp in zip(rois, maps):
        tl, out, msk = warper.warp_fused(odd, K, R, roi)
        ctx.synchronize()
        _check_fused("shape k%d %dx%d" % (kind, roi[2], roi[3]), kind, img, K, R, scale, tl, out, msk, roi, maps=mp)
        singles.append((out, msk))
    res = warper.warp_fused_batch([src] * len(rois), [{"K": K, "R": R}] * len(rois), rois)
    ctx.synchronize()
    for roi, (tl, out, msk), (sout, smsk) in zip(rois, res, singles):
        assert tl == roi[:2] and torch.equal(out, sout) and torch.equal(msk, smsk), roi
    for roi, (sout, smsk) in zip(rois, singles):
        x, y, rw, rh = roi
        ipitch, mpitch = 3 * rw + 2 + (rw & 1) * 1, rw + 2 + (rw & 1)       # int16 elements (even: 4-byte rows), bytes (even)
        assert (ipitch * 2) % 4 == 0 and mpitch % 2 == 0
        ibuf = torch.full((rh + 1, ipitch), -77, dtype=torch.int16, device=src.device)
        mbuf = torch.full((rh + 1, mpitch), 99, dtype=torch.uint8, device=src.device)
        dst = ibuf.as_strided((rh, rw, 3), (ipitch, 3, 1))
        msk = mbuf.as_strided((rh, rw), (mpitch, 1))
        assert warper.warp_fused_into(src, K, R, roi, dst, msk) == (x, y)
        ctx.synchronize()
        assert torch.equal(dst, sout) and torch.equal(msk, smsk), roi
        assert bool((ibuf[:rh, 3 * rw:] == -77).all()) and bool((ibuf[rh] == -77).all()), roi
        assert bool((mbuf[:rh, rw:] == 99).all()) and bool((mbuf[rh] == 99).all()), roi


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cn", [1, 3])
def test_edge_shapes_general_warp(ctx, kind, cn):
    """The same shapes through mis_warper_warp_roi, both modes, 1 and 3 channels; the 3-channel source is the odd-start strided view."""
    import torch
    import image_stitching_amd as isa
    K, R, scale, img3, rois, maps = _shape_setup(kind)
    img = img3 if cn == 3 else np.ascontiguousarray(img3[..., 1])
    src = _strided_source(img3) if cn == 3 else torch.from_numpy(img).cuda()
    for roi, mp in zip(rois, maps):
        for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
            tl, out = _warp_roi(ctx, kind, src, scale, K, R, roi, interp, border)
            assert tl == roi[:2] and out.shape[:2] == (roi[3], roi[2])
            fn = ri.remap_linear_reflect_candidates if interp == isa.INTER_LINEAR else ri.remap_nearest_constant_candidates
            _check("shape warp k%d cn%d %dx%d %d" % (kind, cn, roi[2], roi[3], interp), out, *fn(img, mp),
                   ties=_ties(mp, 32.0 if interp == isa.INTER_LINEAR else 1.0))


@pytest.mark.parametrize("kind", KINDS)
def test_batch_of_three_720p_frames_equals_single_calls(ctx, kind):
    """Three 1280 x 720 frames through warp_fused_batch (hundreds of tiles per frame, three frames of different roi sizes in one
    grid) equal their single calls byte for byte; the first is checked against the reference."""
    import torch
    w, h, geoms = rc.FRAMES_720P
    cams = [ri.camera(w, h, *g) for g in geoms]
    scale = cams[0][2]
    rv, rois = _roi_batch(ctx, kind, scale, w, h, [c[0] for c in cams], [c[1] for c in cams])
    assert rv == 0 and len({r[2:] for r in rois}) == 3
    warper = _warper(ctx, kind, scale)
    imgs = [ri.content("rand", (h, w, 3), seed=40 + k) for k in range(3)]
    srcs = [torch.from_numpy(i).cuda() for i in imgs]
    res = warper.warp_fused_batch(srcs, [{"K": c[0], "R": c[1]} for c in cams], rois)
    ctx.synchronize()
    for k, (src, (K, R, _), roi, (tl, out, msk)) in enumerate(zip(srcs, cams, rois, res)):
        stl, sout, smsk = warper.warp_fused(src, K, R, roi)
        ctx.synchronize()
        assert stl == tl and torch.equal(sout, out) and torch.equal(smsk, msk), k
    assert rc.roi_matches(rois[1], rc.warp_roi_f64(kind, scale, w, h, cams[1][0], cams[1][1]))
    _check_fused("fused 720p k%d" % kind, kind, imgs[1], cams[1][0], cams[1][1], scale, res[1][0], res[1][1], res[1][2], rois[1])
