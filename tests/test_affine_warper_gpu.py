"""The affine warper (kind 13, HIP) against the float64 numpy reference of tests/refimpl_affine_family.py on its scene list
(identity, integer / fractional / half-pixel translations, rotations, similarities of scale 1.25 and 0.8, a roi far from the
origin; K = I and a sensor-style K) at 65 x 9 and 333 x 217: rois from both entries, the general warp in both modes, the fused
warp single and batched (17 frames: two grids), pitched and odd-address buffers, the plane's bytes where the two kinds coincide,
the device map's floats, and a refused roi."""
import ctypes as C
import functools

import numpy as np
import pytest

import refimpl as ri
import refimpl_affine_family as ra
import refimpl_warpers as rw

pytestmark = pytest.mark.gpu

SIZES = [(65, 9), (333, 217)]
REFUSED_K = np.array([[60, 0, 30], [0, 60, 4], [1, 0, 1]], np.float32)      # a projective bottom row: z_ < 0 past column 60


def _check(tag, out, cands, band, und, ties):
    bad, nb, nu = ri.check_candidates(out, cands, band, und)
    n = bad.size
    nt = int((band & ~und & ties).sum())
    print("%s: %d px, in band %d (%.2f %%; exact ties %d), undetermined %d (%.2f %%)" % (tag, n, nb, 100.0 * nb / n, nt, nu, 100.0 * nu / n))
    assert not bad.any(), "%s: %d pixels outside the reference candidates, first at %s" % (tag, int(bad.sum()), np.argwhere(bad)[0])
    if n >= 256:
        assert nb - nt <= ra.MAX_BAND_SHARE * n and nu <= ra.MAX_UNDETERMINED_SHARE * n, tag


def _roi_single(scale, w, h, K, H, kind=ra.AFFINE):
    from image_stitching_amd import _capi as capi
    r = capi.MisRect()
    K, H = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(H, np.float32)
    rc = capi.load().mis_warper_roi(kind, float(scale), w, h, K.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p), C.byref(r))
    return rc, (r.x, r.y, r.width, r.height)


def _roi_batch(ctx, scale, w, h, Ks, Hs, kind=ra.AFFINE):
    from image_stitching_amd import _capi as capi
    n = len(Ks)
    Ks = np.ascontiguousarray(np.stack([np.asarray(k, np.float32).reshape(9) for k in Ks]))
    Hs = np.ascontiguousarray(np.stack([np.asarray(r, np.float32).reshape(9) for r in Hs]))
    rr = (capi.MisRect * n)()
    rc = ctx.lib.mis_warper_roi_batch(ctx.h, kind, float(scale), w, h, n, Ks.ctypes.data_as(C.c_void_p), Hs.ctypes.data_as(C.c_void_p), rr)
    return rc, [(r.x, r.y, r.width, r.height) for r in rr]


@functools.lru_cache(maxsize=None)
def _setup(w, h):
    """-> (img, [(tag, K, H, scale, roi, maps)]): the library's host roi of every scene (asserted within the reference's candidates)
    and the float64 maps on it, computed once for the tests below."""
    img = ri.content("rand", (h, w, 3), seed=3 * w + h)
    out = []
    for tag, K, H, scale in ra.warp_cases(w, h):
        rc, roi = _roi_single(scale, w, h, K, H)
        assert rc == 0 and ra.roi_matches(roi, ra.warp_roi_f64(scale, w, h, K, H)), (tag, roi)
        out.append((tag, K, H, scale, roi, ra.backward_f64(K, H, scale, roi)))
    return img, out


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


@pytest.mark.parametrize("w,h", SIZES)
def test_rois_single_and_batched(ctx, w, h):
    """mis_warper_roi and mis_warper_roi_batch (per scale: one call for its scenes) give the same roi, within the reference's
    candidates; AffineWarper.warp_roi is the single entry."""
    import image_stitching_amd as isa
    _, cases = _setup(w, h)
    for scale in sorted({c[3] for c in cases}):
        sel = [c for c in cases if c[3] == scale]
        rc, rois = _roi_batch(ctx, scale, w, h, [c[1] for c in sel], [c[2] for c in sel])
        assert rc == 0 and rois == [c[4] for c in sel]
        assert isa.stitching.warp_rois(ctx, scale, (w, h), [{"K": c[1], "R": c[2]} for c in sel], isa.WARP_AFFINE) == rois
        assert isa.AffineWarper(ctx, scale).warp_roi((w, h), sel[0][1], sel[0][2]) == rois[0]


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("w,h", SIZES)
def test_general_warp_both_modes(ctx, w, h, cn):
    """mis_warper_warp (1 and 3 channels): INTER_LINEAR + BORDER_REFLECT and INTER_NEAREST + BORDER_CONSTANT on every scene."""
    import torch
    import image_stitching_amd as isa
    img3, cases = _setup(w, h)
    img = img3 if cn == 3 else np.ascontiguousarray(img3[..., 1])
    src = torch.from_numpy(img).cuda()
    for tag, K, H, scale, roi, maps in cases:
        warper = isa.AffineWarper(ctx, scale)
        for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
            tl, out = warper.warp(src, K, H, interp, border)
            out = out.cpu().numpy()
            assert (tl[0], tl[1], out.shape[1], out.shape[0]) == roi, tag
            linear = interp == isa.INTER_LINEAR
            fn = ri.remap_linear_reflect_candidates if linear else ri.remap_nearest_constant_candidates
            _check("warp cn%d %dx%d %s %s" % (cn, w, h, tag, "linear" if linear else "nearest"), out, *fn(img, maps),
                   ties=ra.ties(maps, 32.0 if linear else 1.0))


def _check_fused(tag, img, out, msk, maps):
    h, w = img.shape[:2]
    out, msk = out.cpu().numpy(), msk.cpu().numpy()
    assert out.min() >= 0 and out.max() <= 255
    _check(tag + " linear", out.astype(np.uint8), *ri.remap_linear_reflect_candidates(img, maps), ties=ra.ties(maps, 32.0))
    _check(tag + " mask", msk, *ri.remap_nearest_constant_candidates(np.full((h, w), 255, np.uint8), maps), ties=ra.ties(maps, 1.0))


@pytest.mark.parametrize("w,h", SIZES)
def test_fused_single_and_batch_of_17(ctx, w, h):
    """mis_warper_warp_fused_roi on every scene (s16 image + mask within the reference candidates; with and without a known roi),
    and per scale mis_warper_warp_fused_batch over its scenes repeated to 17 frames -- two grids of 16 + 1 -- byte for byte the
    single calls."""
    import torch
    import image_stitching_amd as isa
    img, cases = _setup(w, h)
    src = torch.from_numpy(img).cuda()
    singles = {}
    for tag, K, H, scale, roi, maps in cases:
        warper = isa.AffineWarper(ctx, scale)
        tl, out, msk = warper.warp_fused(src, K, H, roi)
        tl2, out2, msk2 = warper.warp_fused(src, K, H)          # the entry that computes the roi itself
        ctx.synchronize()
        assert tl == tl2 == roi[:2] and out.shape[:2] == (roi[3], roi[2]) and torch.equal(out, out2) and torch.equal(msk, msk2), tag
        _check_fused("fused %dx%d %s" % (w, h, tag), img, out, msk, maps)
        singles[tag] = (out, msk)
    for scale in sorted({c[3] for c in cases}):
        sel = [c for c in cases if c[3] == scale]
        sel = (sel * 3)[:17]
        assert len(sel) == 17
        res = isa.AffineWarper(ctx, scale).warp_fused_batch([src] * 17, [{"K": c[1], "R": c[2]} for c in sel], [c[4] for c in sel])
        ctx.synchronize()
        for c, (tl, out, msk) in zip(sel, res):
            assert tl == c[4][:2] and torch.equal(out, singles[c[0]][0]) and torch.equal(msk, singles[c[0]][1]), c[0]


def test_pitched_and_odd_address_buffers(ctx):
    """65 x 9: the source as a strided view at an odd address (the source loads' narrow path) and destinations with a row pitch of
    the roi's width plus a few elements whose guard fill stays untouched: the bytes of the dense buffers."""
    import torch
    import image_stitching_amd as isa
    w, h = 65, 9
    img, cases = _setup(w, h)
    src, odd = torch.from_numpy(img).cuda(), _strided_source(img)
    for tag, K, H, scale, roi, maps in cases:
        warper = isa.AffineWarper(ctx, scale)
        _, sout, smsk = warper.warp_fused(src, K, H, roi)
        tl, out, msk = warper.warp_fused(odd, K, H, roi)
        (btl, bout, bmsk), = warper.warp_fused_batch([odd], [{"K": K, "R": H}], [roi])
        ctx.synchronize()
        assert tl == btl == roi[:2] and torch.equal(out, sout) and torch.equal(msk, smsk) and torch.equal(bout, sout) and torch.equal(bmsk, smsk), tag
        x, y, rw_, rh = roi
        ipitch, mpitch = 3 * rw_ + 2 + (rw_ & 1), rw_ + 2 + (rw_ & 1)       # int16 elements (even: 4-byte rows), bytes (even)
        ibuf = torch.full((rh + 1, ipitch), -77, dtype=torch.int16, device=src.device)
        mbuf = torch.full((rh + 1, mpitch), 99, dtype=torch.uint8, device=src.device)
        dst, dmsk = ibuf.as_strided((rh, rw_, 3), (ipitch, 3, 1)), mbuf.as_strided((rh, rw_), (mpitch, 1))
        assert warper.warp_fused_into(src, K, H, roi, dst, dmsk) == (x, y)
        ctx.synchronize()
        assert torch.equal(dst, sout) and torch.equal(dmsk, smsk), tag
        assert bool((ibuf[:rh, 3 * rw_:] == -77).all()) and bool((ibuf[rh] == -77).all()), tag
        assert bool((mbuf[:rh, rw_:] == 99).all()) and bool((mbuf[rh] == 99).all()), tag
        _, u8 = warper.warp(odd, K, H)
        _, u8d = warper.warp(src, K, H)
        assert torch.equal(u8, u8d), tag


@pytest.mark.parametrize("w,h", SIZES)
def test_orthonormal_H_without_translation_gives_the_plane_bytes(ctx, w, h):
    """Translation column zero and H orthonormal (in-plane rotations): kind 13 gives kind 2's bytes on the same K and projector R
    (getRTfromHomogeneous makes R the transpose of H; T = -0 leaves every float as it is) -- roi, fused single and batched, both
    general modes."""
    import torch
    import image_stitching_amd as isa
    img = ri.content("rand", (h, w, 3), seed=w)
    src = torch.from_numpy(img).cuda()
    for roll in (0.0, 7.0, -30.0, 90.0):
        K, R, scale = ri.camera(w, h, 60.0, 0.0, 0.0, roll)
        H = np.ascontiguousarray(R.T)
        assert H[0, 2] == 0 and H[1, 2] == 0
        rc, roi = _roi_single(scale, w, h, K, R, kind=rw.PLANE)
        assert rc == 0 and _roi_single(scale, w, h, K, H) == (0, roi)
        assert _roi_batch(ctx, scale, w, h, [K], [H]) == _roi_batch(ctx, scale, w, h, [K], [R], kind=rw.PLANE) == (0, [roi])
        plane, affine = isa.PlaneWarper(ctx, scale), isa.AffineWarper(ctx, scale)
        a, b = plane.warp_fused(src, K, R, roi), affine.warp_fused(src, K, H, roi)
        (c,), (d,) = plane.warp_fused_batch([src], [{"K": K, "R": R}], [roi]), affine.warp_fused_batch([src], [{"K": K, "R": H}], [roi])
        ctx.synchronize()
        for p, q in ((a, b), (c, d)):
            assert p[0] == q[0] and torch.equal(p[1], q[1]) and torch.equal(p[2], q[2]), roll
        for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
            assert torch.equal(plane.warp(src, K, R, interp, border)[1], affine.warp(src, K, H, interp, border)[1]), roll


def _map(ctx, scale, K, H, roi):
    from image_stitching_amd import _capi as capi
    K, H = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(H, np.float32)
    rr = capi.MisRect(*[int(v) for v in roi])
    xy = np.empty((roi[3], roi[2], 2), np.float32)
    rc = capi.load().mis_debug_warper_map_f32(ctx.h if ctx is not None else None, ra.AFFINE, float(scale), K.ctypes.data_as(C.c_void_p),
                                              H.ctypes.data_as(C.c_void_p), C.byref(rr), xy.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return xy


def test_device_map_floats_are_the_host_sequence(ctx):
    """mis_debug_warper_map_f32 with a context (the kernels' separable terms) gives the floats of the unsplit host sequence."""
    _, cases = _setup(65, 9)
    for tag, K, H, scale, roi, maps in cases:
        assert np.array_equal(_map(ctx, scale, K, H, roi).view(np.uint32), _map(None, scale, K, H, roi).view(np.uint32)), tag


def test_refused_roi_and_the_context_afterwards(ctx):
    """A corner with z_ <= 0 (through a general K) is MIS_E_INVALID from the single and the batched entry and from the warps that
    compute their own roi; the context serves a good call afterwards."""
    import torch
    import image_stitching_amd as isa
    w, h = 65, 9
    I = np.eye(3, dtype=np.float32)
    assert ra.warp_roi_f64(60.0, w, h, REFUSED_K, I)["refused"] is True
    assert _roi_single(60.0, w, h, REFUSED_K, I)[0] == -1
    assert _roi_batch(ctx, 60.0, w, h, [I, REFUSED_K], [I, I])[0] == -1
    with pytest.raises(isa.MisError, match="frame 1"):
        isa.stitching.warp_rois(ctx, 60.0, (w, h), [{"K": I, "R": I}, {"K": REFUSED_K, "R": I}], isa.WARP_AFFINE)
    img, cases = _setup(w, h)
    src = torch.from_numpy(img).cuda()
    with pytest.raises(isa.MisError):
        isa.AffineWarper(ctx, 60.0).warp_fused(src, REFUSED_K, I)
    with pytest.raises(isa.MisError):
        isa.AffineWarper(ctx, 60.0).warp(src, REFUSED_K, I)
    dst, msk = isa.AffineWarper(ctx, 60.0).alloc_fused((0, 0, w, h))
    with pytest.raises(isa.MisError, match="behind the panorama plane"):      # the library's own roi computation (no known roi)
        isa.AffineWarper(ctx, 60.0).warp_fused_into(src, REFUSED_K, I, None, dst, msk)
    tag, K, H, scale, roi, maps = cases[4]
    tl, out, msk = isa.AffineWarper(ctx, scale).warp_fused(src, K, H)
    ctx.synchronize()
    assert tl == roi[:2]
    _check_fused("after the refusal %s" % tag, img, out, msk, maps)
