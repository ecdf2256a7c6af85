"""The fisheye / stereographic numpy reference (tests/refimpl_polar_warpers.py) on its own: closed forms, the conditions the GPU
test's cases must meet on the reference alone, the host roi scan against the reference sets (libmistitch.so loads without a
device), the singular points, and the warp_type plumbing."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import refimpl as ri
import refimpl_polar_warpers as rp

W, H = 320, 180
MAX_BAND_SHARE = 0.40            # test_warpers_gpu.py's caps: conditions on the cases, not measurements
MAX_UNDETERMINED_SHARE = 0.10
MAX_DROPPED_SHARE = 0.10         # of a kind's cases that are not roi-only by size
KINDS = [pytest.param(k, id=n) for n, k in rp.KINDS.items()]


# ------------------------------------------------------------------------------------------------ 1. the reference itself
def _looking_along_y(sign):
    """R whose third column is (0, sign, 0): the principal ray r_kinv (cx, cy, 1) = R (0, 0, 1) points along sign * y."""
    return np.array([[1, 0, 0], [0, 0, sign], [0, -sign, 0]], np.float64)


@pytest.mark.parametrize("kind", KINDS)
def test_principal_point_of_a_camera_on_the_axis_maps_to_the_centre(kind):
    """Fisheye: the ray (0, -1, 0) has v_ = 0 and maps to (0, 0).  Stereographic: the ray (0, +1, 0) has v_ = pi,
    r = sin pi / (1 - cos pi) = 0 and maps to (0, 0).  The backward map of the centre pixel gives that ray back."""
    K, _, scale = ri.camera(W, H, 60.0, 0.0)
    sign = -1.0 if kind == rp.FISHEYE else 1.0
    R = _looking_along_y(sign)
    _, _, _, _, r_kinv = ri._mats(K, R)
    u, v = rp.map_forward_f64(kind, r_kinv, scale, W / 2.0, H / 2.0)
    assert abs(u) < 1e-9 and abs(v) < 1e-9
    ray = rp.ray_backward_f64(kind, scale, 0.0, 0.0)
    assert np.allclose(ray, (0.0, sign, 0.0), atol=1e-15)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("yaw", [0.0, 35.0, -120.0, 180.0])
def test_horizontal_ray_maps_to_the_equator_circle(kind, yaw):
    """A ray in the plane y_ = 0 has v_ = pi / 2: radius scale * pi / 2 (fisheye), scale (stereographic: 1 / (1 - 0))."""
    K, R, scale = ri.camera(W, H, 60.0, yaw)
    _, _, _, _, r_kinv = ri._mats(K, R)
    u, v = rp.map_forward_f64(kind, r_kinv, scale, W / 2.0, H / 2.0)
    want = scale * math.pi / 2 if kind == rp.FISHEYE else scale
    assert abs(math.hypot(u, v) - want) < 1e-6 * want       # (the float32 R is orthogonal to ~1e-7 only)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", ["front", "roll+30", "hfov90", "pitch-70", "pitch+70"])
def test_forward_inverts_backward(kind, geom):
    """mapForward o mapBackward is the identity (float64, to 1e-8 px) on the pixels in front of the camera, away from the
    singular points."""
    name, hfov, yaw, pitch, roll = [g for g in ri.WARP_GEOMS if g[0] == geom][0]
    K, R, scale = ri.camera(W, H, hfov, yaw, pitch, roll)
    _, _, _, k_rinv, _ = ri._mats(K, R)
    r_kinv = np.linalg.inv(k_rinv)
    u0, v0 = rp.map_forward_f64(kind, r_kinv, scale, W / 2.0, H / 2.0)
    uu, vv = np.meshgrid(u0 + np.linspace(-0.3, 0.3, 13) * scale, v0 + np.linspace(-0.2, 0.2, 11) * scale)
    ray = rp.ray_backward_f64(kind, scale, uu, vv)
    keep = (sum(k_rinv[2, j] * r for j, r in enumerate(ray)) > 0) & (np.hypot(uu, vv) > 1e-3 * scale)
    if kind == rp.FISHEYE:
        keep &= np.hypot(uu, vv) < scale * (math.pi - 1e-3)      # rho = pi is the other pole; beyond it the map folds back
    x, y = rp.map_backward_exact_f64(kind, k_rinv, scale, uu[keep], vv[keep])
    u2, v2 = rp.map_forward_f64(kind, r_kinv, scale, x, y)
    assert keep.sum() > 50
    assert np.abs(u2 - uu[keep]).max() < 1e-8 and np.abs(v2 - vv[keep]).max() < 1e-8


@pytest.mark.parametrize("kind", KINDS)
def test_band_is_finite_at_the_centre_pixel(kind):
    """The roi of a pitch geometry contains (0, 0): the bands there are finite and small, z is decided, and no pixel of the
    3 x 3 block around the centre is undetermined at either quantisation."""
    geom = "pitch+70" if kind == rp.FISHEYE else "pitch-70"
    name, hfov, yaw, pitch, roll = [g for g in ri.WARP_GEOMS if g[0] == geom][0]
    K, R, scale = ri.camera(65, 9, hfov, yaw, pitch, roll)
    maps = rp.backward_f64(kind, K, R, scale, (-1, -1, 3, 3))
    assert np.isfinite(maps["dx"]).all() and np.isfinite(maps["dy"]).all() and (maps["z"] > maps["zband"]).all()
    assert maps["dx"].max() < 2.0 ** -8 and maps["dy"].max() < 2.0 ** -8
    for q in (32.0, 1.0):
        assert rp.band_shares(maps, q)[1] == 0.0


# ------------------------------------------------------------------------------------------------ the host scan (no device)
def _roi_host(kind, scale, w, h, K, R):
    from image_stitching_amd import _capi as capi
    r = capi.MisRect()
    K, R = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(R, np.float32)
    rc = capi.load().mis_warper_roi(kind, float(scale), w, h, K.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.byref(r))
    return rc, (r.x, r.y, r.width, r.height)


@functools.lru_cache(maxsize=None)
def _host_cases(kind, w, h, mult):
    """-> [(name, K, R, scale, reference roi dict, rc, roi)] of one source: computed once, shared by the tests below."""
    out = []
    for name, K, R, scale in rp.geometry_cases(w, h, mult):
        out.append((name, K, R, scale, rp.warp_roi_f64(kind, scale, w, h, K, R)) + _roi_host(kind, scale, w, h, K, R))
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,mult", rp.sources())
def test_host_roi_scan_within_the_reference_sets(kind, w, h, mult):
    """mis_warper_roi -- the plain host loop over all pixels -- lies in the reference's candidate sets on every geometry, and
    returns MIS_E_INVALID exactly where the reference says so.  (The reference decides every one of these cases.)"""
    for name, K, R, scale, ref, rc, roi in _host_cases(kind, w, h, mult):
        assert ref["refused"] is False, name
        assert rc == 0 and rp.roi_matches(roi, ref), (name, rc, roi, ref.get("intervals"))


@pytest.mark.parametrize("kind", KINDS)
def test_host_roi_refusals(kind):
    """A scale that carries the projection past what an int holds: the reference says refused, the library MIS_E_INVALID; one
    within reach is accepted.  Kind 7 stays MIS_E_UNSUPPORTED."""
    w, h = 64, 8
    K, R, scale = ri.camera(w, h, 60.0, 0.0)
    assert rp.warp_roi_f64(kind, 1e10, w, h, K, R)["refused"] is True
    assert _roi_host(kind, 1e10, w, h, K, R)[0] == -1
    assert rp.warp_roi_f64(kind, 1e36, w, h, K, R)["refused"] is True
    assert _roi_host(kind, 1e36, w, h, K, R)[0] == -1
    ref = rp.warp_roi_f64(kind, 1e5, w, h, K, R)
    rc, roi = _roi_host(kind, 1e5, w, h, K, R)
    assert ref["refused"] is False and rc == 0 and rp.roi_matches(roi, ref)
    assert _roi_host(7, scale, w, h, K, R)[0] == -6


def test_stereographic_singular_ray_is_skipped_or_huge():
    """The stereographic forward map on the ray (0, -1, 0): v_ = 0, the quotient is 0 / 0 = NaN in float32 and the pixel is
    skipped -- a 3 x 3 source whose centre pixel lies exactly on that ray still gets a finite roi from the library, made of its
    other eight pixels; the reference calls the case undecided (it cannot tell which side of the singularity float32 falls)."""
    K = np.array([[1, 0, 1], [0, 1, 1], [0, 0, 1]], np.float32)
    R = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)        # the principal ray (0, 0, 1) -> (0, -1, 0)
    assert rp.warp_roi_f64(rp.STEREOGRAPHIC, 10.0, 3, 3, K, R)["refused"] is None
    rc, roi = _roi_host(rp.STEREOGRAPHIC, 10.0, 3, 3, K, R)
    # the eight neighbours have v_ = atan(1) or atan(sqrt 2): r = cot(v_ / 2) = 2.414 or 1.932, within +-24.2 px
    assert rc == 0 and roi[0] in (-24, -23) and roi[1] in (-24, -23) and roi[2] in (47, 48, 49) and roi[3] in (47, 48, 49), (rc, roi)
    # the fisheye map has no singular ray there: v_ = 0 at the centre pixel, (0, 0)
    ref = rp.warp_roi_f64(rp.FISHEYE, 10.0, 3, 3, K, R)
    rc, roi = _roi_host(rp.FISHEYE, 10.0, 3, 3, K, R)
    assert rc == 0 and rp.roi_matches(roi, ref), (roi, ref.get("intervals"))


# ------------------------------------------------------------------------------------------------ conditions on the cases
def _warped_cases(kind, w, h, mult):
    """The cases the GPU test warps: the library's roi (in the reference sets, above) is at most MAX_REF_PIXELS."""
    return [c for c in _host_cases(kind, w, h, mult) if c[5] == 0 and c[6][2] * c[6][3] <= rp.MAX_REF_PIXELS]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h,mult", rp.sources())
def test_reference_conditions_hold_for_every_warped_case(kind, w, h, mult):
    """For every (source, multiplier, geometry) the GPU test warps: over the roi the in-band share (exact rounding ties apart)
    stays <= 0.40 and the undetermined share <= 0.10, for both quantisations.  A case that breaks a cap is listed in
    refimpl_polar_warpers.WARP_DROPPED with its reason -- the caps stay."""
    warped = 0
    for name, K, R, scale, ref, rc, roi in _warped_cases(kind, w, h, mult):
        if (kind, w, h, mult, name) in rp.WARP_DROPPED:
            continue
        maps = rp.backward_f64(kind, K, R, scale, roi)
        warped += 1
        if roi[2] * roi[3] < 256:
            continue
        for q in (32.0, 1.0):
            band, und = rp.band_shares(maps, q)
            print("kind %d %dx%d s%g %s q%g: roi %s, in band %.3f, undetermined %.3f" % (kind, w, h, mult, name, q, roi, band, und))
            assert band <= MAX_BAND_SHARE and und <= MAX_UNDETERMINED_SHARE, (name, q, band, und)
    assert warped >= 6


@pytest.mark.parametrize("kind", KINDS)
def test_case_census(kind):
    """At most 10 % of a kind's cases that are not roi-only by size are dropped; the roi-only ones are the pole geometries; at
    least one warped case contains the centre pixel (0, 0), so the singular point of the backward map is exercised."""
    total = dropped = centre = 0
    roi_only = []
    for w, h, mult in rp.sources():
        for name, K, R, scale, ref, rc, roi in _host_cases(kind, w, h, mult):
            if roi[2] * roi[3] > rp.MAX_REF_PIXELS:
                roi_only.append((w, h, mult, name))
                continue
            total += 1
            if (kind, w, h, mult, name) in rp.WARP_DROPPED:
                dropped += 1
            elif roi[0] <= 0 < roi[0] + roi[2] and roi[1] <= 0 < roi[1] + roi[3]:
                centre += 1
    print("kind %d: %d cases, %d dropped, %d roi-only %s, %d contain the centre" % (kind, total, dropped, len(roi_only), roi_only, centre))
    assert dropped <= MAX_DROPPED_SHARE * total
    assert all(n.startswith("pitch") for _, _, _, n in roi_only)
    assert centre >= 1


# ------------------------------------------------------------------------------------------------ plumbing
def test_warp_type_plumbing():
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as st
    assert st.warp_kind("fisheye") == 4 == isa.WARP_FISHEYE == rp.FISHEYE
    assert st.warp_kind("stereographic") == 5 == isa.WARP_STEREOGRAPHIC == rp.STEREOGRAPHIC
    for name, kind in rp.KINDS.items():
        assert name not in st.UNBUILT_WARP_TYPES and st.WARP_KINDS[name] == kind
        assert st.check_warp_config(st.StitchConfig.hot_path(warp_type=name)) == kind
        assert isa._capi.roi_is_full_scan(kind)
    assert isa.FisheyeWarper.kind == 4 and isa.StereographicWarper.kind == 5
    assert not isa._capi.roi_is_full_scan(isa.WARP_SPHERICAL) and isa._capi.roi_is_full_scan(isa.WARP_MERCATOR)
    assert len(st.UNBUILT_WARP_TYPES) == 10
    with pytest.raises(NotImplementedError, match="paniniA2B1"):
        st.warp_kind("paniniA2B1")
    with pytest.raises(ValueError):
        st.warp_kind("Fisheye")
