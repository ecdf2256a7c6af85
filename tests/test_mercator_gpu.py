"""The Mercator warper (HIP) against the float64 numpy reference of tests/refimpl_mercator.py: the six float32 functions give
the host's bits on the device, the device roi scan equals the host scan and lies in the reference sets (tiny sources up to two
4K frames in one call), refusals from every entry, and the fused single / batched and general warps within the reference
candidates.  Every test here needs MIS_WARP_MERCATOR: on a library without it each fails with MIS_E_UNSUPPORTED."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import refimpl as ri
import refimpl_mercator as rm

pytestmark = pytest.mark.gpu

MAX_BAND_SHARE = 0.40            # refimpl's limits (test_warpers_gpu.py)
MAX_UNDETERMINED_SHARE = 0.10
KIND = rm.MERCATOR


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


def _roi_single(scale, w, h, K, R, kind=KIND):
    from image_stitching_amd import _capi as capi
    r = capi.MisRect()
    K, R = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(R, np.float32)
    rc = capi.load().mis_warper_roi(kind, float(scale), w, h, K.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.byref(r))
    return rc, (r.x, r.y, r.width, r.height)


def _roi_batch(ctx, scale, w, h, Ks, Rs, kind=KIND):
    from image_stitching_amd import _capi as capi
    n = len(Ks)
    Ks = np.ascontiguousarray(np.stack([np.asarray(k, np.float32).reshape(9) for k in Ks]))
    Rs = np.ascontiguousarray(np.stack([np.asarray(r, np.float32).reshape(9) for r in Rs]))
    rr = (capi.MisRect * n)()
    rc = ctx.lib.mis_warper_roi_batch(ctx.h, kind, float(scale), w, h, n, Ks.ctypes.data_as(C.c_void_p), Rs.ctypes.data_as(C.c_void_p), rr)
    return rc, [(r.x, r.y, r.width, r.height) for r in rr]


@functools.lru_cache(maxsize=None)
def _ref_rois(w, h, mult):
    """The reference's roi candidates of every geometry of one source: computed once, shared by the tests below."""
    return [(name, K, R, scale, rm.warp_roi_f64(scale, w, h, K, R)) for name, K, R, scale in rm.geometry_cases(w, h, mult)]


def _cases(ctx, w, h, mult):
    """-> [(name, K, R, scale, roi)] of the geometries whose roi is accepted; the device (batch) roi equals the host (single) roi
    and both lie in the reference sets, asserted on the way."""
    out = []
    refs = _ref_rois(w, h, mult)
    rois = [None] * len(refs)
    for scale in sorted({r[3] for r in refs}):          # one batch call per warper scale (the scale follows the field of view)
        idx = [k for k, r in enumerate(refs) if r[3] == scale]
        rc, got = _roi_batch(ctx, scale, w, h, [refs[k][1] for k in idx], [refs[k][2] for k in idx])
        assert rc == 0, ctx.lib.mis_last_error(ctx.h)
        for k, g in zip(idx, got):
            rois[k] = g
    for (name, K, R, scale, ref), broi in zip(refs, rois):
        assert ref["refused"] is False, name
        rc, roi = _roi_single(scale, w, h, K, R)
        assert rc == 0 and roi == broi and rm.roi_matches(roi, ref), (name, roi, broi, ref.get("intervals"))
        out.append((name, K, R, scale, roi))
    return out


def _warped(cases, w, h, mult):
    return [c for c in cases if c[4][2] * c[4][3] <= rm.MAX_REF_PIXELS and (w, h, mult, c[0]) not in rm.WARP_DROPPED]


SOURCES = [pytest.param(w, h, m, id="%dx%d-s%g" % (w, h, m)) for w, h, m in rm.sources()]


# ------------------------------------------------------------------------------------------------ math
SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.5, -0.5, 1e-45, -1e-45, 1.1754944e-38, 3.4028235e38, -3.4028235e38, 1e-4,
            0.70710678, 0.41421357, 2.4142137, math.pi / 4, math.pi / 2, float(np.float32(math.pi / 2)), 88.0, 89.0, -104.0, 12.0, -12.0,
            8192.0, 8193.0, 1e5, -1e5]


@pytest.mark.parametrize("fn,lo,hi", [("LOG", -20.0, 20.0), ("TAN", 0.0, math.pi / 2), ("SINH", -12.0, 12.0), ("ASIN", -1.0, 1.0),
                                      ("ATAN", -1e5, 1e5), ("EXP", -104.0, 89.0)])
def test_device_math_bits_equal_host_bits(ctx, fn, lo, hi):
    """mis_debug_math_f32 with a context (a one-thread-per-element kernel) gives the bits of the host evaluation: 64 K seeded
    inputs over the range the warp uses plus the special values.  The roi scan's host / device equality rests on this."""
    from image_stitching_amd import _capi as capi
    code = getattr(capi, "MATH_" + fn)
    rng = np.random.default_rng(code + 11)
    x = rng.uniform(lo, hi, 1 << 16)
    if fn == "LOG":
        x = np.exp2(x)
    if fn == "ATAN":
        x[: 1 << 15] = rng.uniform(-10.0, 10.0, 1 << 15)
    x = np.ascontiguousarray(np.concatenate([x, SPECIALS]), np.float32)
    host, dev = np.empty_like(x), np.empty_like(x)
    assert ctx.lib.mis_debug_math_f32(None, code, x.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p), x.size) == 0
    ctx.check(ctx.lib.mis_debug_math_f32(ctx.h, code, x.ctypes.data_as(C.c_void_p), dev.ctypes.data_as(C.c_void_p), x.size))
    nan = np.isnan(host)
    assert np.array_equal(nan, np.isnan(dev))
    diff = (host.view(np.uint32) != dev.view(np.uint32)) & ~nan
    assert not diff.any(), (fn, x[diff][:8], host[diff][:8], dev[diff][:8])


# ------------------------------------------------------------------------------------------------ roi
@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_roi_device_scan_equals_host_scan_within_reference(ctx, w, h, mult):
    """mis_warper_roi_batch (the grid-wide device reduction, all geometries of the source in one call) against mis_warper_roi
    (the host loop) and the reference's candidate sets."""
    assert len(_cases(ctx, w, h, mult)) == len(ri.WARP_GEOMS)


def test_roi_two_4k_frames_in_one_call(ctx):
    """Two 3840 x 2160 frames (front, roll+30) in one batch call: 720 workgroups per frame, two frames per launch."""
    w, h = 3840, 2160
    geoms = [g for g in ri.WARP_GEOMS if g[0] in ("front", "roll+30")]
    cams = [ri.camera(w, h, hfov, yaw, pitch, roll) for _, hfov, yaw, pitch, roll in geoms]
    assert cams[0][2] == cams[1][2]
    scale = cams[0][2]
    rc, rois = _roi_batch(ctx, scale, w, h, [c[0] for c in cams], [c[1] for c in cams])
    assert rc == 0, ctx.lib.mis_last_error(ctx.h)
    for (K, R, _), roi, g in zip(cams, rois, geoms):
        ref = rm.warp_roi_f64(scale, w, h, K, R)
        assert rm.roi_matches(roi, ref), (g[0], roi, ref.get("intervals"))
        assert _roi_single(scale, w, h, K, R) == (0, roi)
    # the frames in the other order give the same rois (a frame's partials are its own)
    rc, swapped = _roi_batch(ctx, scale, w, h, [c[0] for c in cams[::-1]], [c[1] for c in cams[::-1]])
    assert rc == 0 and swapped == rois[::-1]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_from_every_entry(ctx):
    """R turns the principal ray onto the lower pole: the pixel at the principal point projects to v = -inf, and both roi entries
    return MIS_E_INVALID (alone and beside a good frame); warp_fused and warp, which compute their own roi, raise.  A pole frame
    whose roi area reaches 2^31 is refused by the warp entries.  An unknown kind stays MIS_E_UNSUPPORTED."""
    import torch
    import image_stitching_amd as isa
    w, h = 64, 8
    K, Rgood, scale = ri.camera(w, h, 60.0, 0.0)
    R = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    assert rm.warp_roi_f64(scale, w, h, K, R)["refused"] is True
    assert _roi_single(scale, w, h, K, R)[0] == -1
    assert _roi_batch(ctx, scale, w, h, [K], [R])[0] == -1
    assert _roi_batch(ctx, scale, w, h, [K, K], [Rgood, R])[0] == -1
    assert _roi_batch(ctx, scale, w, h, [K, K], [Rgood, Rgood])[0] == 0
    src = torch.zeros((h, w, 3), dtype=torch.uint8).cuda()
    with pytest.raises(isa.MisError):
        isa.MercatorWarper(ctx, scale).warp_fused(src, K, R)
    with pytest.raises(isa.MisError):
        isa.MercatorWarper(ctx, scale).warp(src, K, R)
    # pitch+85 at 333 x 217 magnified 100-fold: the pole is inside the frame and the roi is ~1.8e5 x 1.4e5 pixels
    w, h = 333, 217
    name, hfov, yaw, pitch, roll = [g for g in ri.WARP_GEOMS if g[0] == "pitch+85"][0]
    K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, 100.0)
    rc, (roi,) = _roi_batch(ctx, scale, w, h, [K], [R])
    assert rc == 0 and roi == _roi_single(scale, w, h, K, R)[1] and roi[2] * roi[3] >= 2 ** 31
    src = torch.zeros((h, w, 3), dtype=torch.uint8).cuda()
    with pytest.raises(isa.MisError):
        isa.MercatorWarper(ctx, scale).warp_fused(src, K, R)
    with pytest.raises(isa.MisError):
        isa.MercatorWarper(ctx, scale).warp(src, K, R)
    assert _roi_batch(ctx, scale, w, h, [K], [R], kind=7)[0] == -6


# ------------------------------------------------------------------------------------------------ warps
def _check_fused(tag, img, K, R, scale, tl, out, msk, roi):
    out = out.cpu().numpy()
    msk = msk.cpu().numpy()
    h, w = img.shape[:2]
    assert (tl[0], tl[1], out.shape[1], out.shape[0]) == roi
    assert out.min() >= 0 and out.max() <= 255
    maps = rm.backward_f64(K, R, scale, roi)
    _check(tag + " linear", out.astype(np.uint8), *ri.remap_linear_reflect_candidates(img, maps), ties=_ties(maps, 32.0))
    _check(tag + " mask", msk, *ri.remap_nearest_constant_candidates(np.full((h, w), 255, np.uint8), maps), ties=_ties(maps, 1.0))


@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_fused_single_and_batched_vs_reference(ctx, w, h, mult):
    """mis_warper_warp_fused (its own device roi scan), mis_warper_warp_fused_roi per geometry and mis_warper_warp_fused_batch over
    all of them: within the reference candidates, and byte-identical to each other; random, all-0 and all-255 content."""
    import torch
    import image_stitching_amd as isa
    cases = _warped(_cases(ctx, w, h, mult), w, h, mult)
    assert len(cases) >= 6
    singles = []
    for k, (name, K, R, scale, roi) in enumerate(cases):
        warper = isa.MercatorWarper(ctx, scale)
        img = ri.content(("rand", "full", "zero")[k % 3] if k else "rand", (h, w, 3), seed=k + 17 * w + h)
        src = torch.from_numpy(img).cuda()
        tl, out, msk = warper.warp_fused(src, K, R, roi)
        tl2, out2, msk2 = warper.warp_fused(src, K, R)             # computes its own roi: the device scan
        ctx.synchronize()
        assert tl2 == tl and torch.equal(out2, out) and torch.equal(msk2, msk), name
        _check_fused("fused %dx%d s%g %s" % (w, h, mult, name), img, K, R, scale, tl, out, msk, roi)
        singles.append((src, tl, out, msk))
    scale = cases[0][3]                                 # the batch: the cases of the first one's scale (hfov 60: most of them)
    idx = [k for k, c in enumerate(cases) if c[3] == scale]
    assert len(idx) >= 4
    res = isa.MercatorWarper(ctx, scale).warp_fused_batch([singles[k][0] for k in idx], [{"K": cases[k][1], "R": cases[k][2]} for k in idx],
                                                          [cases[k][4] for k in idx])
    ctx.synchronize()
    for k, (tl, out, msk) in zip(idx, res):
        s = singles[k]
        assert tl == s[1] and torch.equal(out, s[2]) and torch.equal(msk, s[3]), cases[k][0]


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_general_modes_vs_reference(ctx, w, h, mult, cn):
    """mis_warper_warp (1 and 3 channels): INTER_LINEAR + BORDER_REFLECT and INTER_NEAREST + BORDER_CONSTANT, on the sources and
    geometries of the fused test; random, all-255 and all-0 content in turn."""
    import torch
    import image_stitching_amd as isa
    for k, (name, K, R, scale, roi) in enumerate(_warped(_cases(ctx, w, h, mult), w, h, mult)):
        img = ri.content(("rand", "full", "zero")[k % 3], (h, w) if cn == 1 else (h, w, 3), seed=5 * k + cn)
        warper = isa.MercatorWarper(ctx, scale)
        maps = rm.backward_f64(K, R, scale, roi)
        for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
            tl, out = warper.warp(torch.from_numpy(img).cuda(), K, R, interp, border)
            out = out.cpu().numpy()
            assert (tl[0], tl[1], out.shape[1], out.shape[0]) == roi
            fn = ri.remap_linear_reflect_candidates if interp == isa.INTER_LINEAR else ri.remap_nearest_constant_candidates
            _check("warp cn%d %dx%d s%g %s %s" % (cn, w, h, mult, name, "linear" if interp == isa.INTER_LINEAR else "nearest"),
                   out, *fn(img, maps), ties=_ties(maps, 32.0 if interp == isa.INTER_LINEAR else 1.0))


def test_batch_of_three_720p_frames_equals_single_calls(ctx):
    """Three 1280 x 720 frames through warp_fused_batch (strips of more than one tile, three frames in one grid) equal their
    single calls byte for byte; the first is checked against the reference."""
    import torch
    import image_stitching_amd as isa
    w, h = 1280, 720
    cams = [ri.camera(w, h, 60.0, yaw, pitch, roll) for yaw, pitch, roll in ((-25.0, 2.0, 0.0), (0.0, -4.0, 3.0), (25.0, 10.0, -5.0))]
    scale = cams[0][2]
    rc, rois = _roi_batch(ctx, scale, w, h, [c[0] for c in cams], [c[1] for c in cams])
    assert rc == 0
    warper = isa.MercatorWarper(ctx, scale)
    imgs = [ri.content("rand", (h, w, 3), seed=40 + k) for k in range(3)]
    srcs = [torch.from_numpy(i).cuda() for i in imgs]
    res = warper.warp_fused_batch(srcs, [{"K": c[0], "R": c[1]} for c in cams], rois)
    ctx.synchronize()
    for k, (src, (K, R, _), roi, (tl, out, msk)) in enumerate(zip(srcs, cams, rois, res)):
        stl, sout, smsk = warper.warp_fused(src, K, R, roi)
        ctx.synchronize()
        assert stl == tl and torch.equal(sout, out) and torch.equal(smsk, msk), k
        assert rm.roi_matches(roi, rm.warp_roi_f64(scale, w, h, K, R))
    _check_fused("fused 720p", imgs[0], cams[0][0], cams[0][1], scale, res[0][0], res[0][1], res[0][2], rois[0])
