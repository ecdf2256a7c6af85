"""The compressed-plane / Panini numpy reference (tests/refimpl_compressed_warpers.py) on its own: the tangent's error constant,
forward o backward, the conditions the GPU tests' cases must meet on the reference alone, the host roi scan against the reference
sets (libmistitch.so loads without a device), the refusals, and the warp_type plumbing.  The sections on the reference itself and
on the conditions of the cases are evaluated on the reference's own rois and hold whatever the library; the host scan, the refusals
and the plumbing need the kinds MIS_WARP_COMPRESSED_PLANE_A2B1 .. MIS_WARP_PANINI_A15B1 and fail on a library without them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import refimpl as ri
import refimpl_compressed_warpers as rc

W, H = 320, 180
MAX_BAND_SHARE = 0.40            # test_warpers_gpu.py's caps: conditions on the cases, not measurements
MAX_UNDETERMINED_SHARE = 0.10
MAX_DROPPED_SHARE = 0.10         # of a kind's cases that are not roi-only by size
KINDS = [pytest.param(k, id=n) for n, k in rc.KINDS.items()]
SOURCES = [pytest.param(w, h, m, id="%dx%d-s%g" % (w, h, m)) for w, h, m in rc.sources()]


# ------------------------------------------------------------------------------------------------ 1. the reference itself
def _math(fn, x):
    from image_stitching_amd import _capi as capi
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    assert capi.load().mis_debug_math_f32(None, fn, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), x.size) == 0
    return out


def _tan_sweep(lim):
    """2^21 + 1 points linear over [-lim, lim], 2^19 geometric over [1e-30, lim] with both signs, and the 4001 floats around
    +-float32(pi / 2) in steps of 2^-22 (those within the limit)."""
    lin = np.linspace(-lim, lim, (1 << 21) + 1)
    g = np.logspace(-30.0, math.log10(lim), 1 << 19)
    pole = np.float32(math.pi / 2) + np.arange(-2000, 2001) * np.float32(2.0 ** -22)
    x = np.concatenate([lin, g, -g, pole, -pole]).astype(np.float32)
    return x[np.abs(x.astype(np.float64)) <= lim]


@pytest.mark.parametrize("lim", [math.pi / 2 * (1 - 2.0 ** -20), 2 * math.pi / 3], ids=["below-the-pole", "to-120-degrees"])
def test_tan_angle_error_constant_is_twice_the_measured_maximum(lim):
    """mis_tanf(x) = tan(x + d): |d| = |atan(mis_tanf(x)) - x| (mod pi) over the arguments the maps can reach, the pole included."""
    from image_stitching_amd import _capi as capi
    x = _tan_sweep(lim)
    assert x.size >= 2_500_000
    xd = x.astype(np.float64)
    d = np.arctan(_math(capi.MATH_TAN, x).astype(np.float64)) - xd
    d -= math.pi * np.round(d / math.pi)
    m = float(np.abs(d).max())
    print("tan, |x| <= %.6f: measured angle error %.4e, constant %.4e" % (lim, m, rc.TAN_ANGLE_ERR))
    assert m <= rc.TAN_ANGLE_ERR / 2 * 1.01
    assert rc.TAN_ANGLE_ERR <= 4 * m, "the constant is looser than the measurement supports"


def test_tangent_is_relatively_accurate_at_small_arguments():
    """SMALL_REL_ERR (stated from the function's construction) holds for mis_tanf over 0 < |x| <= SMALL_ANGLE."""
    from image_stitching_amd import _capi as capi
    g = np.exp2(np.linspace(-100.0, math.log2(rc.SMALL_ANGLE), 1 << 20)).astype(np.float32)
    x = np.concatenate([g, -g])
    want = np.tan(x.astype(np.float64))
    rel = np.abs(_math(capi.MATH_TAN, x).astype(np.float64) - want) / np.abs(want)
    print("tan, |x| <= 2^-8: measured relative error %.4e, bound %.4e" % (rel.max(), rc.SMALL_REL_ERR))
    assert rel.max() <= rc.SMALL_REL_ERR


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", ["front", "roll+30", "hfov90", "pitch-70", "pitch+70", "hfov150"])
def test_forward_inverts_backward(kind, geom):
    """mapForward o mapBackward is the identity (float64, to 1e-7 px) on a grid of output pixels in front of the camera; the grid
    reaches past lam = 90 degrees (cos(lam) < 0) and contains the column u = 0 (the Panini branch)."""
    name, hfov, yaw, pitch, roll = [g for g in ri.WARP_GEOMS if g[0] == geom][0]
    K, R, scale = ri.camera(W, H, hfov, yaw, pitch, roll)
    _, _, _, k_rinv, _ = ri._mats(K, R)
    r_kinv = np.linalg.inv(k_rinv)
    uu, vv = np.meshgrid(np.round(np.linspace(-2.5, 2.5, 41) * scale), np.round(np.linspace(-0.8, 0.8, 17) * scale))
    assert (uu == 0).any()
    ray = rc.ray_backward_f64(kind, scale, uu, vv)
    keep = sum(k_rinv[2, j] * r for j, r in enumerate(ray)) > 1e-3
    x, y = rc.map_backward_exact_f64(kind, k_rinv, scale, uu[keep], vv[keep])
    u2, v2 = rc.map_forward_f64(kind, r_kinv, scale, x, y)
    assert keep.sum() > 50
    assert np.abs(u2 - uu[keep]).max() < 1e-7 and np.abs(v2 - vv[keep]).max() < 1e-7


@pytest.mark.parametrize("kind", KINDS)
def test_float32_intervals_contain_the_float64_map(kind):
    """The forward intervals contain the float64 value wherever the model speaks, and the backward bands are finite and small on
    a frame's own roi (the column u = 0 included)."""
    K, R, scale = ri.camera(65, 9, 60.0, 5.0, 2.0, 0.0)
    _, _, _, _, r_kinv = ri._mats(K, R)
    xs, ys = np.meshgrid(np.arange(65.0), np.arange(9.0))
    u, v, (ulo, uhi), (vlo, vhi), ok = rc.forward_f64(kind, r_kinv, scale, xs.ravel(), ys.ravel())
    assert ok.all() and (ulo <= u).all() and (u <= uhi).all() and (vlo <= v).all() and (v <= vhi).all()
    assert (uhi - ulo).max() < 0.05 and (vhi - vlo).max() < 0.05      # (a sanity bound on the reference: far below a pixel)
    ref = rc.warp_roi_f64(kind, scale, 65, 9, K, R)
    roi = rc.ref_roi(ref)
    assert roi[0] < 0 < roi[0] + roi[2]
    maps = rc.backward_f64(kind, K, R, scale, roi)
    assert np.isfinite(maps["zband"]).all() and maps["dx"].max() < 2.0 ** -8 and maps["dy"].max() < 2.0 ** -8


# ------------------------------------------------------------------------------------------------ the host scan (no device)
def _roi_host(kind, scale, w, h, K, R):
    from image_stitching_amd import _capi as capi
    r = capi.MisRect()
    K, R = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(R, np.float32)
    rv = capi.load().mis_warper_roi(kind, float(scale), w, h, K.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.byref(r))
    return rv, (r.x, r.y, r.width, r.height)


@functools.lru_cache(maxsize=None)
def _host_cases(kind, w, h, mult):
    """-> [(name, K, R, scale, reference roi dict, rc, roi)] of one source: computed once, shared by the tests below."""
    out = []
    for name, K, R, scale in rc.geometry_cases(w, h, mult):
        out.append((name, K, R, scale, rc.warp_roi_f64(kind, scale, w, h, K, R)) + _roi_host(kind, scale, w, h, K, R))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_host_roi_scan_within_the_reference_sets(kind, w, h, mult):
    """mis_warper_roi -- the plain host loop over all pixels -- on refimpl.WARP_GEOMS and refimpl_warpers.PLANE_GEOMS: in the
    reference's candidate sets where it decides, MIS_E_INVALID where it says refused; at most a third of a source's geometries are
    undecided."""
    undecided = 0
    for name, K, R, scale, ref, rv, roi in _host_cases(kind, w, h, mult):
        if ref["refused"] is None:
            undecided += 1
        elif ref["refused"]:
            assert rv == -1, (name, rv, roi)
        else:
            assert rv == 0 and rc.roi_matches(roi, ref), (name, rv, roi, ref.get("intervals"))
    assert 3 * undecided <= len(ri.WARP_GEOMS) + 3, undecided


@pytest.mark.parametrize("kind", KINDS)
def test_host_roi_refusals(kind):
    """A scale that carries the projection past what an int holds: refused by the reference and by the library; one within
    reach is accepted.  A compressed-plane frame whose rays cross u_ = 90 degrees (hfov 120 turned by 50: u_ from -11 to 111
    degrees), at scale 1e8: u stays below 2^31 (scale a tan(55.5 degrees) = 2.9e8) and a pixel next to the crossing has
    tan(v_) / cos(u_) past 21: refused, while the same frame at scale 1e7 and the Panini maps (no divisor there) at both are
    accepted.  Kinds 6 and 7 are unknown."""
    w, h = 64, 8
    K, R, scale = ri.camera(w, h, 60.0, 0.0)
    for bad in (1e10, 1e36):
        assert rc.warp_roi_f64(kind, bad, w, h, K, R)["refused"] is True
        assert _roi_host(kind, bad, w, h, K, R)[0] == -1
    ref = rc.warp_roi_f64(kind, 1e5, w, h, K, R)
    rv, roi = _roi_host(kind, 1e5, w, h, K, R)
    assert ref["refused"] is False and rv == 0 and rc.roi_matches(roi, ref)
    K, R, _ = ri.camera(65, 9, 120.0, 50.0, 10.0, 0.0)
    _, _, _, _, r_kinv = ri._mats(K, R)
    xs, ys = np.meshgrid(np.arange(65.0), np.arange(9.0))
    xyz = r_kinv @ np.stack([xs.ravel(), ys.ravel(), np.ones(xs.size)])
    assert (xyz[2] < 0).any() and (xyz[2] > 0).any()
    for big, refused in ((1e7, False), (1e8, not rc.is_panini(kind))):
        ref = rc.warp_roi_f64(kind, big, 65, 9, K, R)
        rv, roi = _roi_host(kind, big, 65, 9, K, R)
        assert ref["refused"] is refused, (big, ref["refused"])
        assert rv == -1 if refused else (rv == 0 and rc.roi_matches(roi, ref)), (big, rv, roi)
    for unknown in (6, 7):
        assert _roi_host(unknown, 1e7, 65, 9, K, R)[0] == -6


# ------------------------------------------------------------------------------------------------ conditions on the cases
def _warped_cases(kind, w, h, mult):
    """The cases the GPU test warps: decided by the reference, the roi at most MAX_REF_PIXELS -> [(name, K, R, scale, ref, roi)] with
    the reference's widest roi (the library's lies within it: test_host_roi_scan_within_the_reference_sets), so the conditions
    are evaluated on real rois whatever the library answers."""
    out = []
    for name, K, R, scale, ref, rv, _ in _host_cases(kind, w, h, mult):
        if ref["refused"] is False:
            roi = rc.ref_roi(ref)
            if roi[2] * roi[3] <= rc.MAX_REF_PIXELS:
                out.append((name, K, R, scale, ref, roi))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,mult", SOURCES)
def test_reference_conditions_hold_for_every_warped_case(kind, w, h, mult):
    """For every (source, multiplier, geometry) the GPU test warps: over the roi the in-band share (exact rounding ties apart)
    stays <= 0.40 and the undetermined share <= 0.10, for both quantisations.  A case that breaks a cap is listed in
    refimpl_compressed_warpers.WARP_DROPPED with its reason -- the caps stay."""
    warped = 0
    for name, K, R, scale, ref, roi in _warped_cases(kind, w, h, mult):
        if (kind, w, h, mult, name) in rc.WARP_DROPPED:
            continue
        maps = rc.backward_f64(kind, K, R, scale, roi)
        warped += 1
        if roi[2] * roi[3] < 256:
            continue
        for q in (32.0, 1.0):
            band, und = rc.band_shares(maps, q)
            print("kind %d %dx%d s%g %s q%g: roi %s, in band %.3f, undetermined %.3f" % (kind, w, h, mult, name, q, roi, band, und))
            assert band <= MAX_BAND_SHARE and und <= MAX_UNDETERMINED_SHARE, (name, q, band, und)
    assert warped >= 4


@pytest.mark.parametrize("kind", KINDS)
def test_case_census(kind):
    """At most 10 % of a kind's cases that are not roi-only are dropped, and at least one warped case per source past 2 x 2
    straddles the column u = 0."""
    total = dropped = 0
    for w, h, mult in rc.sources():
        straddle = 0
        for name, K, R, scale, ref, roi in _warped_cases(kind, w, h, mult):
            total += 1
            if (kind, w, h, mult, name) in rc.WARP_DROPPED:
                dropped += 1
            elif roi[0] < 0 < roi[0] + roi[2] - 1:
                straddle += 1
        assert straddle >= 1 or (w, h) == (2, 2), (w, h, mult)
    print("kind %d: %d warped cases, %d dropped" % (kind, total, dropped))
    assert total >= 60 and dropped <= MAX_DROPPED_SHARE * total


@pytest.mark.parametrize("kind", KINDS)
def test_reference_conditions_hold_for_the_gpu_tests_other_frames(kind):
    """The edge shapes (those of 256 pixels and more) and the 720p frame the GPU tests check against the reference hold the same
    caps (the 4K pair's rois are checked for their bounds only, there); the refusal cases of the GPU test are decided as it expects."""
    K, R, scale, img, rois = rc.edge_shape_setup(kind)
    for roi in rois:
        maps = rc.backward_f64(kind, K, R, scale, roi)
        for q in (32.0, 1.0):
            band, und = rc.band_shares(maps, q)
            assert roi[2] * roi[3] < 256 or (band <= MAX_BAND_SHARE and und <= MAX_UNDETERMINED_SHARE), (roi, q, band, und)
    w, h, geoms = rc.FRAMES_720P
    K, R, scale = ri.camera(w, h, *geoms[1])
    ref = rc.warp_roi_f64(kind, scale, w, h, K, R)
    assert ref["refused"] is False
    maps = rc.backward_f64(kind, K, R, scale, rc.ref_roi(ref))
    for q in (32.0, 1.0):
        band, und = rc.band_shares(maps, q)
        print("kind %d 720p q%g: in band %.3f, undetermined %.3f" % (kind, q, band, und))
        assert band <= MAX_BAND_SHARE and und <= MAX_UNDETERMINED_SHARE
    w, h = 64, 8
    K, R, scale = ri.camera(w, h, 60.0, 0.0)
    bK, bR = (K, ri.camera(w, h, 60.0, 179.0)[1]) if rc.is_panini(kind) else ri.camera(w, h, 120.0, 50.0, 10.0, 0.0)[:2]
    assert rc.warp_roi_f64(kind, 1e8, w, h, bK, bR)["refused"] is True and rc.warp_roi_f64(kind, 1e8, w, h, K, R)["refused"] is False
    ref = rc.warp_roi_f64(kind, 3e5, w, h, K, R)
    assert ref["refused"] is False and rc.ref_roi(ref)[2] * rc.ref_roi(ref)[3] >= 2 ** 31


def test_the_three_frame_sweep_of_the_job_tests_has_finite_rois():
    """The cameras of tests/test_compressed_warpers_job_gpu.py (yaw -14, 0, 14 and -10, 4, 18 at hfov 60): every roi is decided and
    finite."""
    import synth
    w, h = 480, 270
    sweeps = ([synth.make_camera(w, h, 60.0, 14.0 * i - 14.0, 0.4 * (i - 1), 0.3 * i) for i in range(3)],
              [synth.make_camera(w, h, 60.0, 14.0 * i - 10.0, 0.5 * (i - 1), -0.3 * i) for i in range(3)])      # (test_host_cpp._write_job's, for stitch_main)
    for cams in sweeps:
        scale = float(np.median([c["K"][0, 0] for c in cams]))
        for kind in rc.KINDS.values():
            for c in cams:
                ref = rc.warp_roi_f64(kind, scale, w, h, c["K"], c["R"])
                assert ref["refused"] is False and rc.ref_roi(ref)[2] < 2 * w and rc.ref_roi(ref)[3] < 2 * h


# ------------------------------------------------------------------------------------------------ plumbing
def test_warp_type_plumbing():
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as st
    assert st.warp_kind("compressedPlaneA2B1") == 8 == isa.WARP_COMPRESSED_PLANE_A2B1 == rc.COMPRESSED_A2B1
    assert st.warp_kind("compressedPlaneA1.5B1") == 9 == isa.WARP_COMPRESSED_PLANE_A15B1 == rc.COMPRESSED_A15B1
    assert st.warp_kind("paniniA1.5B1") == 11 == isa.WARP_PANINI_A15B1 == rc.PANINI_A15B1
    assert isa.WARP_PANINI_A2B1 == 10 == rc.PANINI_A2B1
    for name in ("paniniA2B1", "compressedPlanePortraitA2B1", "compressedPlanePortraitA1.5B1", "paniniPortraitA2B1", "paniniPortraitA1.5B1",
                 "transverseMercator", "affine"):
        with pytest.raises(NotImplementedError, match=name.replace(".", r"\.")):
            st.warp_kind(name)
        assert name in st.REFUSED_WARP_TYPES
    assert len(st.REFUSED_WARP_TYPES) == 7
    for kind in rc.KINDS.values():
        assert isa._capi.roi_is_full_scan(kind) and kind in st.BUILT_WARP_KINDS
    assert not isa._capi.roi_is_full_scan(6) and not isa._capi.roi_is_full_scan(7)
    for name in ("compressedPlaneA2B1", "compressedPlaneA1.5B1", "paniniA1.5B1"):
        assert st.check_warp_config(st.StitchConfig.hot_path(warp_type=name)) == rc.KINDS[name]


def test_warper_classes_take_the_built_pairs_only():
    import image_stitching_amd as isa
    assert isa.PaniniWarper(None, 100.0, 2, 1).kind == 10 and isa.PaniniWarper(None, 100.0).kind == 10
    assert isa.PaniniWarper(None, 100.0, 1.5, 1.0).kind == 11
    assert isa.CompressedRectilinearWarper(None, 100.0).kind == 8 and isa.CompressedRectilinearWarper(None, 100.0, A=1.5, B=1).kind == 9
    for cls in (isa.PaniniWarper, isa.CompressedRectilinearWarper):
        with pytest.raises(NotImplementedError, match=r"A=3, B=1"):
            cls(None, 100.0, 3, 1)
    for kind in (6, 7, 12):
        with pytest.raises(NotImplementedError):
            isa.RotationWarper(None, 100.0, kind)
    K, R, scale = ri.camera(65, 9, 60.0, 0.0)
    for kind, cls, ab in ((8, isa.CompressedRectilinearWarper, (2, 1)), (11, isa.PaniniWarper, (1.5, 1))):
        assert cls(None, scale, *ab).warp_roi((65, 9), K, R) == _roi_host(kind, scale, 65, 9, K, R)[1]      # no context: the host scan
