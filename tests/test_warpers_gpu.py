"""The cylindrical and plane warps (HIP) against the float64 numpy reference of tests/refimpl_warpers.py, at the warp's edge
regimes: fused single / batched and general (u8, 1 and 3 channels) warps within the reference candidates, single and batched
results identical, host and device rois equal and within the reference sets, refused rois refused by both entries.  The
spherical kind through the kind-taking entries is byte-identical to the spherical entries."""
import ctypes as C

import numpy as np
import pytest

import refimpl as ri
import refimpl_warpers as rw

pytestmark = pytest.mark.gpu

MAX_BAND_SHARE = 0.40            # refimpl's limits (test_refimpl_warp_gpu.py)
MAX_UNDETERMINED_SHARE = 0.10
MAX_REF_PIXELS = 2_000_000       # rois past this are checked for their bounds only (the float64 reference is slow)
KINDS = [pytest.param(rw.CYLINDRICAL, id="cylindrical"), pytest.param(rw.PLANE, id="plane")]


def _ties(maps, q):
    """Pixels whose float64 coordinate times q lies exactly on a rounding tie (k + 1/2): in the band whatever its width.  The plane
    at R = I is a translation by the principal point, which sits on a half pixel for odd widths: every pixel of such a warp is a
    tie of INTER_NEAREST, and the band-share limit would measure the geometry, not the error model."""
    t = np.zeros(maps["x"].shape, bool)
    for c in ("x", "y"):
        f = np.abs(np.modf(maps[c] * q)[0])
        t |= f == 0.5
    return t


def _check(tag, out, cands, band, und, ties=None):
    bad, nb, nu = ri.check_candidates(out, cands, band, und)
    n = bad.size
    nt = int((band & ~und & ties).sum()) if ties is not None else 0
    print("%s: %d px, in band %d (%.2f %%; exact ties %d), undetermined %d (%.2f %%)" % (tag, n, nb, 100.0 * nb / n, nt, nu, 100.0 * nu / n))
    assert not bad.any(), "%s: %d pixels outside the reference candidates, first at %s" % (tag, int(bad.sum()), np.argwhere(bad)[0])
    if n >= 256:
        assert nb - nt <= MAX_BAND_SHARE * n and nu <= MAX_UNDETERMINED_SHARE * n, tag


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


def _geoms(kind, w, h, mult):
    big = w * mult > 300
    gs = [g for g in ri.WARP_GEOMS if not (big and g[0] in ("pitch+85", "pitch-85"))]
    return gs + (rw.PLANE_GEOMS if kind == rw.PLANE else [])


def _cases(kind, w, h, mult):
    """-> [(name, K, R, scale, roi)] of the geometries whose roi the library gives and the reference accepts; asserts the refusals
    and the roi agreement on the way."""
    import image_stitching_amd as isa
    out = []
    for name, hfov, yaw, pitch, roll in _geoms(kind, w, h, mult):
        K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, mult, seam=mult < 1)
        ref = rw.warp_roi_f64(kind, scale, w, h, K, R)
        rc, roi = _roi_single(kind, scale, w, h, K, R)
        if ref["refused"] is None:
            continue
        if ref["refused"]:
            assert rc == -1, (name, rc)     # MIS_E_INVALID
            continue
        assert rc == 0 and rw.roi_matches(roi, ref), (name, roi)
        out.append((name, K, R, scale, roi))
    return out


def _check_fused(tag, kind, img, K, R, scale, tl, out, msk, roi):
    out = out.cpu().numpy()
    msk = msk.cpu().numpy()
    h, w = img.shape[:2]
    assert (tl[0], tl[1], out.shape[1], out.shape[0]) == roi
    assert out.min() >= 0 and out.max() <= 255
    if roi[2] * roi[3] > MAX_REF_PIXELS:
        return None
    maps = rw.backward_f64(kind, K, R, scale, roi)
    _check(tag + " linear", out.astype(np.uint8), *ri.remap_linear_reflect_candidates(img, maps), ties=_ties(maps, 32.0))
    _check(tag + " mask", msk, *ri.remap_nearest_constant_candidates(np.full((h, w), 255, np.uint8), maps), ties=_ties(maps, 1.0))
    return maps


def _sources():
    for (w, h), mults in ri.WARP_SOURCES:
        for m in mults:
            yield pytest.param(w, h, m, id="%dx%d-s%g" % (w, h, m))
    yield pytest.param(333, 217, 1.0, id="333x217-s1")
    yield pytest.param(333, 217, 0.37, id="333x217-s0.37")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,mult", list(_sources()))
def test_warper_fused_single_and_batched_vs_reference(ctx, kind, w, h, mult):
    """mis_warper_warp_fused_roi per geometry and mis_warper_warp_fused_batch over all of them: within the reference
    candidates, and identical to each other; random, all-0 and all-255 content."""
    import torch
    import image_stitching_amd as isa
    cases = _cases(kind, w, h, mult)
    assert cases
    singles = []
    for k, (name, K, R, scale, roi) in enumerate(cases):
        img = ri.content(("rand", "full", "zero")[k % 3] if k else "rand", (h, w, 3), seed=k + 17 * w + h)
        src = torch.from_numpy(img).cuda()
        warper = isa.RotationWarper(ctx, scale, kind)
        tl, out, msk = warper.warp_fused(src, K, R, roi)
        ctx.synchronize()
        maps = _check_fused("fused k%d %dx%d s%g %s" % (kind, w, h, mult, name), kind, img, K, R, scale, tl, out, msk, roi)
        if kind == rw.PLANE and name == "behind" and maps is not None:
            # the plane's no-sign-test branch ran: pixels with z < 0 (beyond its band) inside the roi
            assert (maps["z"] < -maps["zband"]).sum() > 0
        singles.append((img, src, tl, out.cpu().numpy(), msk.cpu().numpy()))
    scale = cases[0][3]
    idx = [k for k, c in enumerate(cases) if c[3] == scale]
    # the single-call roi equals the batch roi
    rc, rois = _roi_batch(ctx, kind, scale, w, h, [cases[k][1] for k in idx], [cases[k][2] for k in idx])
    assert rc == 0 and rois == [cases[k][4] for k in idx]
    warper = isa.RotationWarper(ctx, scale, kind)
    res = warper.warp_fused_batch([singles[k][1] for k in idx], [{"K": cases[k][1], "R": cases[k][2]} for k in idx], rois)
    ctx.synchronize()
    for k, (tl, out, msk) in zip(idx, res):
        assert tl == singles[k][2]
        assert np.array_equal(out.cpu().numpy(), singles[k][3]) and np.array_equal(msk.cpu().numpy(), singles[k][4]), cases[k][0]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("w,h,mult", [(2, 2, 25.0), (5, 7, 20.0), (65, 9, 1.0), (333, 217, 0.37)])
def test_warper_general_modes_vs_reference(ctx, kind, w, h, mult, cn):
    """mis_warper_warp (1 and 3 channels): INTER_LINEAR + BORDER_REFLECT and INTER_NEAREST + BORDER_CONSTANT."""
    import torch
    import image_stitching_amd as isa
    for k, (name, K, R, scale, roi) in enumerate(_cases(kind, w, h, mult)):
        img = ri.content("rand", (h, w) if cn == 1 else (h, w, 3), seed=5 * k + cn)
        warper = isa.RotationWarper(ctx, scale, kind)
        maps = None
        for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
            tl, out = warper.warp(torch.from_numpy(img).cuda(), K, R, interp, border)
            out = out.cpu().numpy()
            assert (tl[0], tl[1], out.shape[1], out.shape[0]) == roi
            if roi[2] * roi[3] > MAX_REF_PIXELS:
                continue
            maps = maps or rw.backward_f64(kind, K, R, scale, roi)
            fn = ri.remap_linear_reflect_candidates if interp == isa.INTER_LINEAR else ri.remap_nearest_constant_candidates
            _check("warp k%d cn%d %dx%d s%g %s %s" % (kind, cn, w, h, mult, name, "linear" if interp == isa.INTER_LINEAR else "nearest"),
                   out, *fn(img, maps), ties=_ties(maps, 32.0 if interp == isa.INTER_LINEAR else 1.0))


@pytest.mark.parametrize("kind", KINDS)
def test_warper_fused_4k_vs_reference(ctx, kind):
    """One 3840 x 2160 frame at scale = f (the benchmark's size), single and batched, all-255 and random content."""
    import torch
    import image_stitching_amd as isa
    w, h = 3840, 2160
    K, R, scale = ri.camera(w, h, 60.0, 15.0, 0.3, -0.2)
    rc, roi = _roi_single(kind, scale, w, h, K, R)
    assert rc == 0 and rw.roi_matches(roi, rw.warp_roi_f64(kind, scale, w, h, K, R))
    warper = isa.RotationWarper(ctx, scale, kind)
    maps = rw.backward_f64(kind, K, R, scale, roi)
    for content in ("rand", "full"):
        img = ri.content(content, (h, w, 3), seed=4)
        src = torch.from_numpy(img).cuda()
        tl, out, msk = warper.warp_fused(src, K, R, roi)
        (btl, bout, bmsk), = warper.warp_fused_batch([src], [{"K": K, "R": R}], [roi])
        ctx.synchronize()
        assert btl == tl and torch.equal(bout, out) and torch.equal(bmsk, msk)
        out, msk = out.cpu().numpy(), msk.cpu().numpy()
        _check("fused 4K k%d %s linear" % (kind, content), out.astype(np.uint8), *ri.remap_linear_reflect_candidates(img, maps))
        _check("fused 4K k%d %s mask" % (kind, content), msk, *ri.remap_nearest_constant_candidates(np.full((h, w), 255, np.uint8), maps))


def test_plane_refused_rois_from_both_entries(ctx):
    """A plane frame turned past 90 degrees (yaw +-175) has no roi: MIS_E_INVALID from the single and the batched entry, and the
    warps that compute their own roi refuse too; an unknown kind is MIS_E_UNSUPPORTED everywhere."""
    import torch
    import image_stitching_amd as isa
    w, h = 320, 180
    good = ri.camera(w, h, 60.0, 0.0)
    for yaw in (175.0, -175.0):
        K, R, scale = ri.camera(w, h, 60.0, yaw)
        assert _roi_single(rw.PLANE, scale, w, h, K, R)[0] == -1
        assert _roi_batch(ctx, rw.PLANE, scale, w, h, [good[0], K], [good[1], R])[0] == -1
        with pytest.raises(isa.MisError):
            isa.RotationWarper(ctx, scale, rw.PLANE).warp_fused(torch.zeros((h, w, 3), dtype=torch.uint8).cuda(), K, R)
    K, R, scale = good
    assert _roi_single(7, scale, w, h, K, R)[0] == -6
    assert _roi_batch(ctx, 7, scale, w, h, [K], [R])[0] == -6


@pytest.mark.parametrize("w,h,mult", [(65, 9, 1.0), (333, 217, 0.37), (3840, 2160, 1.0)])
def test_spherical_kind_is_byte_identical_to_the_spherical_entries(ctx, w, h, mult):
    """MIS_WARP_SPHERICAL through the kind-taking entries gives the spherical entries' bytes (rois, fused single and batched,
    general warp).  The spherical entries forward to the kind-taking ones, so this guards the wrappers (argument order, the kind
    they pass) only; that the spherical kernels are the parent commit's is shown by their disassembly."""
    import torch
    import image_stitching_amd as isa
    geoms = [g for g in ri.WARP_GEOMS if w < 1000 or g[0] in ("front", "roll+30")]
    Ks, Rs, srcs = [], [], []
    for k, (name, hfov, yaw, pitch, roll) in enumerate(geoms):
        K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, mult, seam=mult < 1)
        img = torch.from_numpy(ri.content("rand", (h, w, 3), seed=k)).cuda()
        old, new = isa.SphericalWarper(ctx, scale), isa.RotationWarper(ctx, scale, isa.WARP_SPHERICAL)
        roi = isa.warp_roi(scale, (w, h), K, R)
        assert _roi_single(isa.WARP_SPHERICAL, scale, w, h, K, R) == (0, roi)
        lib = ctx.lib
        a = isa.stitching._empty_image(ctx, roi[3], roi[2], 3, torch.int16), isa.stitching._empty_image(ctx, roi[3], roi[2], 1, torch.uint8)
        b = isa.stitching._empty_image(ctx, roi[3], roi[2], 3, torch.int16), isa.stitching._empty_image(ctx, roi[3], roi[2], 1, torch.uint8)
        si, kp, rp = isa.stitching.as_image(img), isa.stitching._mat9(K)[1], isa.stitching._mat9(R)[1]
        tl1, tl2 = isa._capi.MisPoint(), isa._capi.MisPoint()
        ctx.check(lib.mis_warp_spherical_fused(ctx.h, C.byref(si), scale, kp, rp, C.byref(isa.stitching.as_image(a[0])), C.byref(isa.stitching.as_image(a[1])), C.byref(tl1)))
        ctx.check(lib.mis_warper_warp_fused(ctx.h, isa.WARP_SPHERICAL, C.byref(si), scale, kp, rp, C.byref(isa.stitching.as_image(b[0])),
                                            C.byref(isa.stitching.as_image(b[1])), C.byref(tl2)))
        ctx.synchronize()
        assert (tl1.x, tl1.y) == (tl2.x, tl2.y) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
        if w < 1000:
            g = img[:, :, 0].contiguous()
            for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
                o1 = isa.stitching._empty_image(ctx, roi[3], roi[2], 1, torch.uint8)
                gi = isa.stitching.as_image(g)
                ctx.check(lib.mis_warp_spherical(ctx.h, C.byref(gi), scale, kp, rp, interp, border, C.byref(isa.stitching.as_image(o1)), C.byref(tl1)))
                _, o2 = new.warp(g, K, R, interp, border)
                ctx.synchronize()
                assert torch.equal(o1, o2), name
        Ks.append(K); Rs.append(R); srcs.append(img)
        if k == 0:
            s0 = scale
    idx = [k for k in range(len(geoms)) if ri.camera(w, h, *geoms[k][1:], mult, seam=mult < 1)[2] == s0]
    rc, rois = _roi_batch(ctx, isa.WARP_SPHERICAL, s0, w, h, [Ks[k] for k in idx], [Rs[k] for k in idx])
    assert rc == 0 and rois == isa.stitching.warp_rois(ctx, s0, (w, h), [{"K": Ks[k], "R": Rs[k]} for k in idx])


@pytest.mark.parametrize("w,h", [(65, 9), (64, 8)])
def test_plane_divides_by_negative_z_inside_its_roi(ctx, w, h):
    """The "behind" geometry: its plane roi (a slanted trapezoid's bounding box) reaches past the camera's horizon, so pixels with
    z < 0 (beyond their band) lie inside it -- the plane's no-sign-test branch of warp_fused_kernel<false>,
    warp_strip_batch_kernel<false> and the u8 warp runs on them, and the results are within the reference candidates there too."""
    import torch
    import image_stitching_amd as isa
    name, hfov, yaw, pitch, roll = rw.PLANE_GEOMS[0]
    assert name == "behind"
    K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll)
    ref = rw.warp_roi_f64(rw.PLANE, scale, w, h, K, R)
    rc, roi = _roi_single(rw.PLANE, scale, w, h, K, R)
    assert ref["refused"] is False and rc == 0 and rw.roi_matches(roi, ref)
    maps = rw.backward_f64(rw.PLANE, K, R, scale, roi)
    neg = maps["z"] < -maps["zband"]
    assert neg.sum() > 100, int(neg.sum())
    img = ri.content("rand", (h, w, 3), seed=w)
    src = torch.from_numpy(img).cuda()
    warper = isa.RotationWarper(ctx, scale, rw.PLANE)
    tl, out, msk = warper.warp_fused(src, K, R, roi)
    (btl, bout, bmsk), = warper.warp_fused_batch([src], [{"K": K, "R": R}], [roi])
    ctx.synchronize()
    assert btl == tl and torch.equal(bout, out) and torch.equal(bmsk, msk)
    _check_fused("behind fused %dx%d" % (w, h), rw.PLANE, img, K, R, scale, tl, out, msk, roi)
    # those pixels are constrained by the check above (their quotient is determined: outside the z band), not skipped
    assert not rw.z_undecided(maps)[neg].any()
    g = np.ascontiguousarray(img[:, :, 1])
    tl, out = warper.warp(torch.from_numpy(g).cuda(), K, R)
    _check("behind warp cn1 %dx%d" % (w, h), out.cpu().numpy(), *ri.remap_linear_reflect_candidates(g, maps), ties=_ties(maps, 32.0))


def test_cylindrical_roi_with_a_pole_on_the_border_is_refused(ctx):
    """A camera pitched by exactly 90 degrees whose principal point lies on its top row: that border pixel's ray is the cylinder's
    axis (x_ = z_ = 0, exactly in float32), so v = scale y_ / 0 is infinite -- MIS_E_INVALID from both roi entries, and the batch
    names the frame.  (A camera one degree off gives a finite roi.)"""
    import image_stitching_amd as isa
    w, h = 64, 32
    K = np.array([[64.0, 0, 32.0], [0, 64.0, 0.0], [0, 0, 1]], np.float32)
    R = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    scale = 64.0
    assert rw.warp_roi_f64(rw.CYLINDRICAL, scale, w, h, K, R)["refused"] is True
    assert _roi_single(rw.CYLINDRICAL, scale, w, h, K, R)[0] == -1
    good_K, good_R, _ = ri.camera(w, h, 60.0, 0.0)
    assert _roi_batch(ctx, rw.CYLINDRICAL, scale, w, h, [good_K, K], [good_R, R])[0] == -1
    with pytest.raises(isa.MisError, match="frame 1"):
        isa.stitching.warp_rois(ctx, scale, (w, h), [{"K": good_K, "R": good_R}, {"K": K, "R": R}], rw.CYLINDRICAL)
    R1 = ri.camera(w, h, 60.0, 0.0, 89.0)[1]
    rc, roi = _roi_single(rw.CYLINDRICAL, scale, w, h, K, R1)
    assert rc == 0 and rw.roi_matches(roi, rw.warp_roi_f64(rw.CYLINDRICAL, scale, w, h, K, R1))


def test_roi_wider_than_an_int_is_refused(ctx):
    """A plane frame whose corners project to about -1.6e9 and +1.55e9 (tiny focal length, large scale): each extreme fits an
    int, the width does not -- MIS_E_INVALID from both roi entries instead of a wrapped width."""
    import image_stitching_amd as isa
    w, h = 64, 8
    K = np.array([[1e-3, 0, 32.0], [0, 1e-3, 4.0], [0, 0, 1]], np.float32)
    R = np.eye(3, dtype=np.float32)
    scale = 50000.0
    ref = rw.warp_roi_f64(rw.PLANE, scale, w, h, K, R)
    assert ref["refused"] is False and max(ref["br_x"]) - min(ref["tl_x"]) + 1 > 2 ** 31
    assert _roi_single(rw.PLANE, scale, w, h, K, R)[0] == -1
    assert _roi_batch(ctx, rw.PLANE, scale, w, h, [K], [R])[0] == -1
    with pytest.raises(isa.MisError, match="does not fit an int"):
        isa.stitching.warp_rois(ctx, scale, (w, h), [{"K": K, "R": R}], rw.PLANE)
