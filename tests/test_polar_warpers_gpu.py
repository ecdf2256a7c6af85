"""The fisheye and stereographic warpers (HIP, the per-pixel map kernels) against the float64 numpy reference of
tests/refimpl_polar_warpers.py: the device roi scan equals the host scan and lies in the reference sets (tiny sources up to two
4K frames in one call), the fused single / batched and general warps lie within the reference candidates on every case and on
the smallest shapes at which the kernels can go wrong, and the refusals.  Every test here needs MIS_WARP_FISHEYE /
MIS_WARP_STEREOGRAPHIC: on a library without them each fails with MIS_E_UNSUPPORTED."""
import ctypes as C
import functools

import numpy as np
import pytest

import refimpl as ri
import refimpl_polar_warpers as rp

pytestmark = pytest.mark.gpu

MAX_BAND_SHARE = 0.40            # refimpl's limits (test_warpers_gpu.py)
MAX_UNDETERMINED_SHARE = 0.10
KINDS = [pytest.param(k, id=n) for n, k in rp.KINDS.items()]
SOURCES = [pytest.param(w, h, m, id="%dx%d-s%g" % (w, h, m)) for w, h, m in rp.sources()]


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
    return (isa.FisheyeWarper if kind == rp.FISHEYE else isa.StereographicWarper)(ctx, scale)


def _roi_single(kind, scale, w, h, K, R):
    from image_stitching_amd import _capi as capi
    r = capi.MisRect()
    K, R = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(R, np.float32)
    rc = capi.load().mis_warper_roi(kind, float(scale), w, h, K.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.byref(r))
    return rc, (r.x, r.y, r.width, r.height)


def _roi_batch(ctx, kind, scale, w, h, Ks, Rs):
    from image_stitching_amd import _capi as capi
    n = len(Ks)
    Ks = np.ascontiguousarray(np.stack([np.asarray(k, np.float32).reshape(9) for k in Ks]))
    Rs = np.ascontiguousarray(np.stack([np.asarray(r, np.float32).reshape(9) for r in Rs]))
    rr = (capi.MisRect * n)()
    rc = ctx.lib.mis_warper_roi_batch(ctx.h, kind, float(scale), w, h, n, Ks.ctypes.data_as(C.c_void_p), Rs.ctypes.data_as(C.c_void_p), rr)
    return rc, [(r.x, r.y, r.width, r.height) for r in rr]


def _warp_roi(ctx, kind, img, scale, K, R, roi, interp, border):
    """mis_warper_warp_roi into a fresh device image of the roi's size -> (tl, numpy output)."""
    import torch
    from image_stitching_amd import _capi as capi, stitching as st
    src = torch.from_numpy(img).cuda()
    simg = st.as_image(src)
    dst = st._empty_image(ctx, roi[3], roi[2], simg.channels, torch.uint8)
    rr, tl = capi.MisRect(*[int(v) for v in roi]), capi.MisPoint()
    ctx.check(ctx.lib.mis_warper_warp_roi(ctx.h, kind, C.byref(simg), float(scale), st._mat9(K)[1], st._mat9(R)[1], C.byref(rr), interp, border,
                                          C.byref(st.as_image(dst)), C.byref(tl)))
    return (tl.x, tl.y), dst.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref_rois(kind, w, h, mult):
    """The reference's roi candidates of every geometry of one source: computed once, shared by the tests below."""
    return [(name, K, R, scale, rp.warp_roi_f64(kind, scale, w, h, K, R)) for name, K, R, scale in rp.geometry_cases(w, h, mult)]


def _cases(ctx, kind, w, h, mult):
    """-> [(name, K, R, scale, roi)]; the device (batch) roi equals the host (single) roi and both lie in the reference sets,
    asserted on the way."""
    out = []
    refs = _ref_rois(kind, w, h, mult)
    rois = [None] * len(refs)
    for scale in sorted({r[3] for r in refs}):          # one batch call per warper scale: several cameras per call
        idx = [k for k, r in enumerate(refs) if r[3] == scale]
        rc, got = _roi_batch(ctx, kind, scale, w, h, [refs[k][1] for k in idx], [refs[k][2] for k in idx])
        assert rc == 0, ctx.lib.mis_last_error(ctx.h)
        for k, g in zip(idx, got):
            rois[k] = g
    for (name, K, R, scale, ref), broi in zip(refs, rois):
        assert ref["refused"] is False, name
        rc, roi = _roi_single(kind, scale, w, h, K, R)
        assert rc == 0 and roi == broi and rp.roi_matches(roi, ref), (name, roi, broi, ref.get("intervals"))
        out.append((name, K, R, scale, roi))
    return out


def _warped(cases, kind, w, h, mult):
    return [c for c in cases if c[4][2] * c[4][3] <= rp.MAX_REF_PIXELS and (kind, w, h, mult, c[0]) not in rp.WARP_DROPPED]


# ------------------------------------------------------------------------------------------------ roi
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_roi_device_scan_equals_host_scan_within_reference(ctx, kind, w, h, mult):
    """mis_warper_roi_batch (the grid-wide device reduction, several cameras per call) against mis_warper_roi (the host loop) and
    the reference's candidate sets."""
    assert len(_cases(ctx, kind, w, h, mult)) == len(ri.WARP_GEOMS)


@pytest.mark.parametrize("kind", KINDS)
def test_roi_two_4k_frames_in_one_call(ctx, kind):
    """Two 3840 x 2160 frames (front, roll+30) in one batch call: 720 workgroups per frame, two frames per launch."""
    w, h = 3840, 2160
    geoms = [g for g in ri.WARP_GEOMS if g[0] in ("front", "roll+30")]
    cams = [ri.camera(w, h, hfov, yaw, pitch, roll) for _, hfov, yaw, pitch, roll in geoms]
    scale = cams[0][2]
    assert cams[1][2] == scale
    rc, rois = _roi_batch(ctx, kind, scale, w, h, [c[0] for c in cams], [c[1] for c in cams])
    assert rc == 0, ctx.lib.mis_last_error(ctx.h)
    for (K, R, _), roi, g in zip(cams, rois, geoms):
        ref = rp.warp_roi_f64(kind, scale, w, h, K, R)
        assert rp.roi_matches(roi, ref), (g[0], roi, ref.get("intervals"))
    assert _roi_single(kind, scale, w, h, cams[1][0], cams[1][1]) == (0, rois[1])      # (one host scan of 8.3 M pixels)
    rc, swapped = _roi_batch(ctx, kind, scale, w, h, [c[0] for c in cams[::-1]], [c[1] for c in cams[::-1]])
    assert rc == 0 and swapped == rois[::-1]


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kind", KINDS)
def test_refusals_and_a_good_call_afterwards(ctx, kind):
    """A projection past what an int holds (scale 1e10; scale 3e38, where the fisheye's scale * v_ overflows to +inf) gives
    MIS_E_INVALID from both roi entries, alone and beside a good frame; a roi of area >= 2^31 is returned by the roi entries and
    refused by the warp entries; a `known` roi of another size than the destination is MIS_E_INVALID; an unknown kind stays
    MIS_E_UNSUPPORTED; the context serves a good call afterwards."""
    import torch
    import image_stitching_amd as isa
    w, h = 64, 8
    K, R, scale = ri.camera(w, h, 60.0, 0.0)
    for bad in (1e10, 3e38):
        assert rp.warp_roi_f64(kind, bad, w, h, K, R)["refused"] is True
        assert _roi_single(kind, bad, w, h, K, R)[0] == -1
        assert _roi_batch(ctx, kind, bad, w, h, [K], [R])[0] == -1
        assert _roi_batch(ctx, kind, bad, w, h, [K, K], [R, R])[0] == -1
    src = torch.from_numpy(ri.content("rand", (h, w, 3), seed=3)).cuda()
    with pytest.raises(isa.MisError):
        _warper(ctx, kind, 1e10).warp_fused(src, K, R)
    with pytest.raises(isa.MisError):
        _warper(ctx, kind, 1e10).warp(src, K, R)
    # an enormous roi: stereographic pitch+70 at 333 x 217 (a pixel next to the singular ray), fisheye at scale 2e5
    if kind == rp.STEREOGRAPHIC:
        bw, bh = 333, 217
        name, hfov, yaw, pitch, roll = [g for g in ri.WARP_GEOMS if g[0] == "pitch+70"][0]
        bK, bR, bscale = ri.camera(bw, bh, hfov, yaw, pitch, roll)
    else:
        bw, bh, bK, bR, bscale = w, h, K, R, 2e5
    rc, (roi,) = _roi_batch(ctx, kind, bscale, bw, bh, [bK], [bR])
    assert rc == 0 and (0, roi) == _roi_single(kind, bscale, bw, bh, bK, bR) and roi[2] * roi[3] >= 2 ** 31, roi
    assert rp.roi_matches(roi, rp.warp_roi_f64(kind, bscale, bw, bh, bK, bR))
    big = torch.zeros((bh, bw, 3), dtype=torch.uint8).cuda()
    small_dst, small_msk = _warper(ctx, kind, bscale).alloc_fused((0, 0, 8, 8))
    with pytest.raises(isa.MisError):
        _warper(ctx, kind, bscale).warp_fused_into(big, bK, bR, roi, small_dst, small_msk)
    with pytest.raises(isa.MisError):
        _warper(ctx, kind, bscale).warp_fused_into(big, bK, bR, None, small_dst, small_msk)
    from image_stitching_amd import _capi as capi, stitching as st
    small_u8 = st._empty_image(ctx, 8, 8, 3, torch.uint8)
    for known in (None, roi):       # the general warp, computing its own roi and with the enormous one handed over
        rr, tl = capi.MisRect(*roi), capi.MisPoint()
        args = (ctx.h, kind, C.byref(st.as_image(big)), float(bscale), st._mat9(bK)[1], st._mat9(bR)[1])
        tail = (isa.INTER_LINEAR, isa.BORDER_REFLECT, C.byref(st.as_image(small_u8)), C.byref(tl))
        rc = ctx.lib.mis_warper_warp(*args, *tail) if known is None else ctx.lib.mis_warper_warp_roi(*args, C.byref(rr), *tail)
        assert rc == -1, rc
    # a known roi of another size than the destination
    warper = _warper(ctx, kind, scale)
    good = warper.warp_roi((w, h), K, R)
    dst, msk = warper.alloc_fused(good)
    with pytest.raises(isa.MisError) as e:
        warper.warp_fused_into(src, K, R, (good[0], good[1], good[2] + 1, good[3]), dst, msk)
    assert e.value.code == -1
    assert _roi_batch(ctx, 7, scale, w, h, [K], [R])[0] == -6
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
    maps = maps or rp.backward_f64(kind, K, R, scale, roi)
    _check(tag + " linear", out.astype(np.uint8), *ri.remap_linear_reflect_candidates(img, maps), ties=_ties(maps, 32.0))
    _check(tag + " mask", msk, *ri.remap_nearest_constant_candidates(np.full((h, w), 255, np.uint8), maps), ties=_ties(maps, 1.0))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_fused_single_and_batched_vs_reference(ctx, kind, w, h, mult):
    """mis_warper_warp_fused (its own device roi scan), mis_warper_warp_fused_roi per geometry and mis_warper_warp_fused_batch over
    the geometries of one scale (frames of different roi sizes in one grid): within the reference candidates, and byte-identical
    to each other; the mask equals the general NEAREST / CONSTANT warp of an all-255 mask; random, all-255 and all-0 content."""
    import torch
    import image_stitching_amd as isa
    cases = _warped(_cases(ctx, kind, w, h, mult), kind, w, h, mult)
    assert len(cases) >= 6
    singles = []
    for k, (name, K, R, scale, roi) in enumerate(cases):
        warper = _warper(ctx, kind, scale)
        img = ri.content(("rand", "full", "zero")[k % 3] if k else "rand", (h, w, 3), seed=k + 17 * w + h)
        src = torch.from_numpy(img).cuda()
        tl, out, msk = warper.warp_fused(src, K, R, roi)
        tl2, out2, msk2 = warper.warp_fused(src, K, R)             # computes its own roi: the device scan
        ctx.synchronize()
        assert tl2 == tl and torch.equal(out2, out) and torch.equal(msk2, msk), name
        _check_fused("fused k%d %dx%d s%g %s" % (kind, w, h, mult, name), kind, img, K, R, scale, tl, out, msk, roi)
        mtl, gm = _warp_roi(ctx, kind, np.full((h, w), 255, np.uint8), scale, K, R, roi, isa.INTER_NEAREST, isa.BORDER_CONSTANT)
        assert mtl == tl and np.array_equal(gm, msk.cpu().numpy()), name
        singles.append((src, tl, out, msk))
    scale = cases[0][3]                                 # the batch: the cases of the first one's scale (hfov 60: most of them)
    idx = [k for k, c in enumerate(cases) if c[3] == scale]
    assert len(idx) >= 4 and len({cases[k][4][2:] for k in idx}) >= 2
    res = _warper(ctx, kind, scale).warp_fused_batch([singles[k][0] for k in idx], [{"K": cases[k][1], "R": cases[k][2]} for k in idx],
                                                     [cases[k][4] for k in idx])
    ctx.synchronize()
    for k, (tl, out, msk) in zip(idx, res):
        s = singles[k]
        assert tl == s[1] and torch.equal(out, s[2]) and torch.equal(msk, s[3]), cases[k][0]


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
        maps = rp.backward_f64(kind, K, R, scale, roi)
        for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
            tl, out = warper.warp(torch.from_numpy(img).cuda(), K, R, interp, border)
            out = out.cpu().numpy()
            assert (tl[0], tl[1], out.shape[1], out.shape[0]) == roi
            fn = ri.remap_linear_reflect_candidates if interp == isa.INTER_LINEAR else ri.remap_nearest_constant_candidates
            _check("warp k%d cn%d %dx%d s%g %s %s" % (kind, cn, w, h, mult, name, "linear" if interp == isa.INTER_LINEAR else "nearest"),
                   out, *fn(img, maps), ties=_ties(maps, 32.0 if interp == isa.INTER_LINEAR else 1.0))


# The smallest shapes at which the kernels can go wrong, as `known` rois (the warp entries take the roi the caller hands them):
# narrower than one lane group of 4, one pixel wide or high, one below / at / one above the fused tile (128 x 8) and the general
# tile (128 x 16), two tiles and a bit.  Each is placed so that it contains the centre pixel (0, 0).
SHAPES = [(1, 1), (1, 9), (3, 1), (2, 2), (4, 8), (5, 3), (127, 7), (128, 8), (129, 9), (127, 15), (128, 16), (129, 17), (257, 17), (131, 1),
          (1, 33), (255, 8), (256, 9), (7, 16)]


@functools.lru_cache(maxsize=None)
def _shape_setup(kind):
    """A 65 x 9 seam-scale source whose roi contains the centre pixel (fisheye pitch-85: roi 128 x 127 about it; stereographic
    pitch+70: 157 x 157), its content and the float64 maps of every shape: computed once for the three tests below."""
    geom = "pitch-85" if kind == rp.FISHEYE else "pitch+70"
    name, hfov, yaw, pitch, roll = [g for g in ri.WARP_GEOMS if g[0] == geom][0]
    w, h = 65, 9
    K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, 0.37, seam=True)
    full = rp.warp_roi_f64(kind, scale, w, h, K, R)
    assert max(full["tl_x"]) <= 0 <= min(full["br_x"]) and max(full["tl_y"]) <= 0 <= min(full["br_y"])     # the real roi holds the centre
    img = ri.content("rand", (h, w, 3), seed=91 + kind)
    rois = [(-(sw // 2), -(sh // 3), sw, sh) for sw, sh in SHAPES]
    assert all(x <= 0 < x + sw and y <= 0 < y + sh for x, y, sw, sh in rois)
    return K, R, scale, img, rois, [rp.backward_f64(kind, K, R, scale, r) for r in rois]


@pytest.mark.parametrize("kind", KINDS)
def test_edge_shapes_fused_single_batch_and_pitched_rows(ctx, kind):
    """Every shape through the single fused warp (within the reference candidates, the centre pixel included), all 18 of them in
    one batch call (two launches: 16 + 2 frames of different sizes) byte-identical to the single calls, and once more into
    destinations with a row pitch of the roi's width plus a few elements, whose padding must stay untouched."""
    import torch
    K, R, scale, img, rois, maps = _shape_setup(kind)
    warper = _warper(ctx, kind, scale)
    src = torch.from_numpy(img).cuda()
    singles = []
    for roi, mp in zip(rois, maps):
        tl, out, msk = warper.warp_fused(src, K, R, roi)
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
    """The same shapes through mis_warper_warp_roi, both modes, 1 and 3 channels."""
    import image_stitching_amd as isa
    K, R, scale, img3, rois, maps = _shape_setup(kind)
    img = img3 if cn == 3 else np.ascontiguousarray(img3[..., 1])
    for roi, mp in zip(rois, maps):
        for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
            tl, out = _warp_roi(ctx, kind, img, scale, K, R, roi, interp, border)
            assert tl == roi[:2] and out.shape[:2] == (roi[3], roi[2])
            fn = ri.remap_linear_reflect_candidates if interp == isa.INTER_LINEAR else ri.remap_nearest_constant_candidates
            _check("shape warp k%d cn%d %dx%d %d" % (kind, cn, roi[2], roi[3], interp), out, *fn(img, mp),
                   ties=_ties(mp, 32.0 if interp == isa.INTER_LINEAR else 1.0))


@pytest.mark.parametrize("kind", KINDS)
def test_batch_of_three_720p_frames_equals_single_calls(ctx, kind):
    """Three 1280 x 720 frames through warp_fused_batch (thousands of tiles per frame, three frames in one grid) equal their single
    calls byte for byte; the first is checked against the reference."""
    import torch
    w, h = 1280, 720
    cams = [ri.camera(w, h, 60.0, yaw, pitch, roll) for yaw, pitch, roll in ((-25.0, 2.0, 0.0), (0.0, -4.0, 3.0), (25.0, 10.0, -5.0))]
    scale = cams[0][2]
    rc, rois = _roi_batch(ctx, kind, scale, w, h, [c[0] for c in cams], [c[1] for c in cams])
    assert rc == 0
    warper = _warper(ctx, kind, scale)
    imgs = [ri.content("rand", (h, w, 3), seed=40 + k) for k in range(3)]
    srcs = [torch.from_numpy(i).cuda() for i in imgs]
    res = warper.warp_fused_batch(srcs, [{"K": c[0], "R": c[1]} for c in cams], rois)
    ctx.synchronize()
    for k, (src, (K, R, _), roi, (tl, out, msk)) in enumerate(zip(srcs, cams, rois, res)):
        stl, sout, smsk = warper.warp_fused(src, K, R, roi)
        ctx.synchronize()
        assert stl == tl and torch.equal(sout, out) and torch.equal(smsk, msk), k
    assert rp.roi_matches(rois[0], rp.warp_roi_f64(kind, scale, w, h, cams[0][0], cams[0][1]))
    _check_fused("fused 720p k%d" % kind, kind, imgs[0], cams[0][0], cams[0][1], scale, res[0][0], res[0][1], res[0][2], rois[0])
