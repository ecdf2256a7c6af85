"""The spherical warp (HIP) against the float64 numpy reference of tests/refimpl.py, at the warp's edge regimes.

Every INTER_LINEAR pixel must be one of its reference candidates (the quantisations within the float32 error band of the
float64 map); the mask must equal the reference outside the band; the roi may differ by 1 only where the float64 extreme lies
within the band of an integer.  Each check prints how many pixels fell in the band."""
import numpy as np
import pytest

import refimpl as ri

pytestmark = pytest.mark.gpu

MAX_BAND_SHARE = 0.40        # the 4K frame at scale = f has the widest band (~35 %); small frames stay below 10 %
MAX_UNDETERMINED_SHARE = 0.10


def _check(tag, out, cands, band, und):
    bad, nb, nu = ri.check_candidates(out, cands, band, und)
    n = bad.size
    print("%s: %d px, in band %d (%.2f %%), undetermined %d (%.2f %%)" % (tag, n, nb, 100.0 * nb / n, nu, 100.0 * nu / n))
    assert not bad.any(), "%s: %d pixels outside the reference candidates, first at %s" % (tag, int(bad.sum()), np.argwhere(bad)[0])
    if n >= 256:         # (a share of a handful of pixels says nothing)
        assert nb <= MAX_BAND_SHARE * n and nu <= MAX_UNDETERMINED_SHARE * n, tag


def _check_fused(tag, img, K, R, scale, tl, out, msk):
    import image_stitching_amd as isa
    out = out.cpu().numpy()
    msk = msk.cpu().numpy()
    h, w = img.shape[:2]
    roi = (tl[0], tl[1], out.shape[1], out.shape[0])
    assert roi == isa.warp_roi(scale, (w, h), K, R)
    assert ri.roi_matches(roi, ri.warp_roi_f64(scale, w, h, K, R)), (tag, roi)
    assert out.min() >= 0 and out.max() <= 255
    maps = ri.spherical_backward_f64(K, R, scale, roi)
    _check(tag + " linear", out.astype(np.uint8), *ri.remap_linear_reflect_candidates(img, maps))
    _check(tag + " mask", msk, *ri.remap_nearest_constant_candidates(np.full((h, w), 255, np.uint8), maps))


def _sources():
    for (w, h), mults in ri.WARP_SOURCES:
        for m in mults:
            yield pytest.param(w, h, m, id="%dx%d-s%g" % (w, h, m))
    yield pytest.param(333, 217, 1.0, id="333x217-s1")
    yield pytest.param(333, 217, 0.37, id="333x217-s0.37")


def _geoms(w, h, mult):
    # large sources at scale = f keep away from the poles (a pole roi spans 2 pi scale x pi scale: slow to reference)
    big = w * mult > 300
    return [g for g in ri.WARP_GEOMS if not (big and g[0] in ("pitch+85", "pitch-85"))]


@pytest.mark.parametrize("w,h,mult", list(_sources()))
def test_warp_fused_single_and_batched_vs_reference(ctx, w, h, mult):
    """mis_warp_spherical_fused per geometry, then mis_warp_spherical_fused_batch over all geometries of the source size in one
    grid, with random, all-0 and all-255 content."""
    import torch
    import image_stitching_amd as isa
    geoms = _geoms(w, h, mult)
    frames, cams, rois = [], [], []
    for k, (name, hfov, yaw, pitch, roll) in enumerate(geoms):
        K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, mult, seam=mult < 1)
        img = ri.content(("rand", "full", "zero")[k % 3] if k else "rand", (h, w, 3), seed=k + 17 * w + h)
        warper = isa.SphericalWarper(ctx, scale)
        src = torch.from_numpy(img).cuda()
        tl, out, msk = warper.warp_fused(src, K, R)
        ctx.synchronize()
        _check_fused("fused %dx%d s%g %s" % (w, h, mult, name), img, K, R, scale, tl, out, msk)
        frames.append((img, src))
        cams.append((K, R, scale))
        rois.append(isa.warp_roi(scale, (w, h), K, R))
    # the batched grid needs one scale: group the geometries by it (seam scale and magnified sources share f's multiple)
    scale = cams[0][2]
    idx = [k for k, c in enumerate(cams) if c[2] == scale]
    warper = isa.SphericalWarper(ctx, scale)
    res = warper.warp_fused_batch([frames[k][1] for k in idx], [{"K": cams[k][0], "R": cams[k][1]} for k in idx],
                                  [rois[k] for k in idx])
    ctx.synchronize()
    for k, (tl, out, msk) in zip(idx, res):
        _check_fused("batch %dx%d s%g %s" % (w, h, mult, geoms[k][0]), frames[k][0], cams[k][0], cams[k][1], scale, tl, out, msk)


@pytest.mark.parametrize("cn", [1, 3])
@pytest.mark.parametrize("w,h,mult", [(2, 2, 25.0), (5, 7, 20.0), (65, 9, 1.0), (333, 217, 0.37)])
def test_warp_general_modes_vs_reference(ctx, w, h, mult, cn):
    """mis_warp_spherical (1 and 3 channels): INTER_LINEAR + BORDER_REFLECT and INTER_NEAREST + BORDER_CONSTANT."""
    import torch
    import image_stitching_amd as isa
    for k, (name, hfov, yaw, pitch, roll) in enumerate(_geoms(w, h, mult)):
        K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, mult, seam=mult < 1)
        img = ri.content("rand", (h, w) if cn == 1 else (h, w, 3), seed=5 * k + cn)
        warper = isa.SphericalWarper(ctx, scale)
        ref_roi = ri.warp_roi_f64(scale, w, h, K, R)
        maps = None
        for interp, border in ((isa.INTER_LINEAR, isa.BORDER_REFLECT), (isa.INTER_NEAREST, isa.BORDER_CONSTANT)):
            tl, out = warper.warp(torch.from_numpy(img).cuda(), K, R, interp, border)
            out = out.cpu().numpy()
            roi = (tl[0], tl[1], out.shape[1], out.shape[0])
            assert ri.roi_matches(roi, ref_roi), (name, roi)
            maps = maps or ri.spherical_backward_f64(K, R, scale, roi)
            fn = ri.remap_linear_reflect_candidates if interp == isa.INTER_LINEAR else ri.remap_nearest_constant_candidates
            _check("warp cn%d %dx%d s%g %s %s" % (cn, w, h, mult, name, "linear" if interp == isa.INTER_LINEAR else "nearest"),
                   out, *fn(img, maps))


@pytest.mark.parametrize("w,h,geom", [(333, 217, "roll+30"), (64, 8, "hfov150"), (3840, 2160, "front")])
def test_warp_strided_source_vs_reference(ctx, w, h, geom):
    """A source that is a column slice of a wider tensor starting at column 1: the base address is not dword aligned and the
    row stride exceeds width * 3 (the strip pipeline's cold route), through the fused and the general warp."""
    import torch
    import image_stitching_amd as isa
    name, hfov, yaw, pitch, roll = [g for g in ri.WARP_GEOMS if g[0] == geom][0]
    K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll)
    wide = ri.content("rand", (h, w + 5, 3), seed=w)
    img = np.ascontiguousarray(wide[:, 1:w + 1])
    src = torch.from_numpy(wide).cuda()[:, 1:w + 1]
    assert src.stride(0) == (w + 5) * 3 and src.data_ptr() % 4 != 0
    warper = isa.SphericalWarper(ctx, scale)
    tl, out, msk = warper.warp_fused(src, K, R)
    ctx.synchronize()
    _check_fused("strided fused %dx%d %s" % (w, h, name), img, K, R, scale, tl, out, msk)
    if w < 1000:
        tl, out = warper.warp(torch.from_numpy(wide[:, :, 0].copy()).cuda()[:, 1:w + 1], K, R)
        maps = ri.spherical_backward_f64(K, R, scale, (tl[0], tl[1], out.shape[1], out.shape[0]))
        _check("strided warp cn1 %dx%d %s" % (w, h, name), out.cpu().numpy(),
               *ri.remap_linear_reflect_candidates(np.ascontiguousarray(wide[:, 1:w + 1, 0]), maps))


def test_warp_fused_4k_vs_reference(ctx):
    """One 3840 x 2160 frame (the benchmark's size) on the strip pipeline's fast path, all-255 and random content."""
    import torch
    import image_stitching_amd as isa
    w, h = 3840, 2160
    K, R, scale = ri.camera(w, h, 60.0, 15.0, 0.3, -0.2)
    warper = isa.SphericalWarper(ctx, scale)
    for kind in ("rand", "full"):
        img = ri.content(kind, (h, w, 3), seed=4)
        tl, out, msk = warper.warp_fused(torch.from_numpy(img).cuda(), K, R)
        ctx.synchronize()
        _check_fused("fused 4K %s" % kind, img, K, R, scale, tl, out, msk)
