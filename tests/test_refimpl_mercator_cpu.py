"""The Mercator numpy reference (tests/refimpl_mercator.py) on its own: self-checks, the measured error constants of the five
float32 functions its error model names (through mis_debug_math_f32 on the host: libmistitch.so loads without a device), the
conditions the GPU test's cases must meet on the reference alone, the two frames whose roi extreme lies at an interior pixel,
the host roi scan against the reference sets, and the warp_type plumbing."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import refimpl as ri
import refimpl_mercator as rm

W, H = 320, 180
MAX_BAND_SHARE = 0.40            # test_warpers_gpu.py's caps: conditions on the cases, not measurements
MAX_UNDETERMINED_SHARE = 0.10


# ------------------------------------------------------------------------------------------------ 1. the reference itself
@pytest.mark.parametrize("geom", ["front", "roll+30", "hfov90", "pitch-70"])
def test_forward_inverts_backward(geom):
    """mapForward o mapBackward is the identity (float64, to 1e-9 px) on the pixels in front of the camera."""
    name, hfov, yaw, pitch, roll = [g for g in ri.WARP_GEOMS if g[0] == geom][0]
    K, R, scale = ri.camera(W, H, hfov, yaw, pitch, roll)
    _, _, _, k_rinv, _ = ri._mats(K, R)
    r_kinv = np.linalg.inv(k_rinv)       # (the float32 R is orthogonal to ~1e-7 only: R^T and R^-1 differ at that level)
    u0, v0 = rm.map_forward_f64(r_kinv, scale, W / 2.0, H / 2.0)      # a grid about the frame centre's image
    uu, vv = np.meshgrid(u0 + np.linspace(-0.3, 0.3, 13) * scale, v0 + np.linspace(-0.2, 0.2, 11) * scale)
    x, y = rm.map_backward_exact_f64(k_rinv, scale, uu, vv)
    v_ = np.arctan(np.sinh(vv / scale))
    ray = (np.cos(v_) * np.sin(uu / scale), np.sin(v_), np.cos(v_) * np.cos(uu / scale))
    keep = sum(k_rinv[2, j] * r for j, r in enumerate(ray)) > 0
    u2, v2 = rm.map_forward_f64(r_kinv, scale, x[keep], y[keep])
    assert keep.sum() > 50
    assert np.abs(u2 - uu[keep]).max() < 1e-9 and np.abs(v2 - vv[keep]).max() < 1e-9


def test_gudermannian_identities():
    """v_ = atan(sinh v'): cos v_ = 1 / cosh v' and sin v_ = tanh v' (to 1e-12), the row table of the warp kernels."""
    vp = np.linspace(-12.0, 12.0, 48001)
    v_ = np.arctan(np.sinh(vp))
    assert np.abs(np.cos(v_) - 1.0 / np.cosh(vp)).max() < 1e-12
    assert np.abs(np.sin(v_) - np.tanh(vp)).max() < 1e-12
    # and the forward direction: log tan(pi/4 + v_/2) = v' away from the poles
    mid = np.abs(vp) < 6
    assert np.abs(np.log(np.tan(math.pi / 4 + v_[mid] / 2)) - vp[mid]).max() < 1e-9


# ------------------------------------------------------------------------------------------------ 2. the measured constants
def _math(fn, x):
    from image_stitching_amd import _capi as capi
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    rc = capi.load().mis_debug_math_f32(None, fn, x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), x.size)
    assert rc == 0
    return out.astype(np.float64)


def _f32(a):
    return np.unique(np.asarray(a, np.float64).astype(np.float32))


# The sweeps (float32 inputs; the reference is numpy float64 of the float32 input).  Each covers the range the warp uses.
def _sweep_log():
    """2^21 points geometric over [2^-20, 2^20], 2^19 linear over [1/2, 2] (log near its zero), 2^18 geometric over the normal
    range beyond, and every power of two."""
    return _f32(np.concatenate([np.exp2(np.linspace(-20.0, 20.0, 1 << 21)), np.linspace(0.5, 2.0, 1 << 19),
                                np.exp2(np.linspace(-126.0, 127.0, 1 << 18)), np.exp2(np.arange(-126.0, 128.0))]))


def _sweep_tan():
    """2^21 points linear over (0, pi/2), 2^18 geometric from 2^-30 up to pi/4 (the lower pole side: tan -> 0) and 2^18 with
    pi/2 - x geometric from 2^-23 (the upper pole side); inputs below float32(pi/2) only."""
    hp = float(np.float32(math.pi / 2))
    x = _f32(np.concatenate([np.linspace(0.0, math.pi / 2, (1 << 21) + 2)[1:-1], np.exp2(np.linspace(-30.0, math.log2(math.pi / 4), 1 << 18)),
                             math.pi / 2 - np.exp2(np.linspace(-23.0, math.log2(math.pi / 4), 1 << 18))]))
    return x[(x > 0) & (x < hp)]


def _sweep_sinh():
    """2^20 points linear over [-12, 12], 2^18 linear over [-1.25, 1.25] (both branches either side of |x| = 1) and 2^16 geometric
    down to 2^-40 with both signs."""
    g = np.exp2(np.linspace(-40.0, 0.0, 1 << 16))
    return _f32(np.concatenate([np.linspace(-12.0, 12.0, 1 << 20), np.linspace(-1.25, 1.25, 1 << 18), g, -g]))


def _sweep_asin():
    """2^20 points linear over [-1, 1] and 2^17 with 1 - |x| geometric from 2^-24 (the poles), both signs."""
    g = 1.0 - np.exp2(np.linspace(-24.0, -1.0, 1 << 17))
    return _f32(np.concatenate([np.linspace(-1.0, 1.0, (1 << 20) + 1), g, -g]))


def _sweep_atan():
    """2^19 points linear over [-10, 10], 2^19 geometric over [2^-20, 1e5] with both signs, and +-inf."""
    g = np.exp2(np.linspace(-20.0, math.log2(1e5), 1 << 19))
    return np.concatenate([_f32(np.concatenate([np.linspace(-10.0, 10.0, (1 << 19) + 1), g, -g])), np.array([np.inf, -np.inf], np.float32)])


def _rel(got, want):
    nz = want != 0
    assert np.array_equal(got[~nz], want[~nz])
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))


@functools.lru_cache(maxsize=None)
def _measured(name):
    from image_stitching_amd import _capi as capi
    if name == "log":
        x = _sweep_log()
        assert x.size >= 2_000_000
        return _rel(_math(capi.MATH_LOG, x), np.log(x.astype(np.float64)))
    if name == "tan":
        x = _sweep_tan()
        assert x.size >= 2_000_000
        return _rel(_math(capi.MATH_TAN, x), np.tan(x.astype(np.float64)))
    if name == "sinh":
        x = _sweep_sinh()
        assert x.size >= 1_000_000
        return _rel(_math(capi.MATH_SINH, x), np.sinh(x.astype(np.float64)))
    if name == "asin":
        x = _sweep_asin()
        return float(np.max(np.abs(_math(capi.MATH_ASIN, x) - np.arcsin(x.astype(np.float64)))))
    x = _sweep_atan()
    return float(np.max(np.abs(_math(capi.MATH_ATAN, x) - np.arctan(x.astype(np.float64)))))


@pytest.mark.parametrize("name,const", [("log", "LOG_REL_ERR"), ("tan", "TAN_REL_ERR"), ("sinh", "SINH_REL_ERR"), ("asin", "ASIN_ERR"),
                                        ("atan", "ATAN_ERR")])
def test_error_constants_are_twice_the_measured_maximum(name, const):
    """Each constant of refimpl_mercator is twice the maximum error of the library's function over the sweep above (a sweep is a
    finite sample): measured <= constant / 2 * 1.01."""
    m = _measured(name)
    c = getattr(rm, const)
    print("%s: measured %.4e, constant %.4e" % (name, m, c))
    assert m <= c / 2 * 1.01
    assert c <= 4 * m, "the constant is looser than the measurement supports"


def test_special_values_of_the_new_functions():
    """The edge cases the roi scan relies on: log(0) = -inf, log(< 0) = NaN, sinh overflows to +-inf (never NaN),
    atan(+-inf) = +-pi/2, tan(0) = 0, tan(float32(pi/2)) < 0 (so log gives NaN there and the pixel is skipped)."""
    from image_stitching_amd import _capi as capi
    inf = np.inf
    lg = _math(capi.MATH_LOG, [0.0, -0.0, -1.0, inf, 1.0, np.nan])
    assert lg[0] == -inf and lg[1] == -inf and np.isnan(lg[2]) and lg[3] == inf and lg[4] == 0.0 and np.isnan(lg[5])
    sh = _math(capi.MATH_SINH, [89.0, -89.0, 1000.0, -1000.0, inf, -inf, 0.0])
    assert list(sh) == [inf, -inf, inf, -inf, inf, -inf, 0.0]
    at = _math(capi.MATH_ATAN, [inf, -inf])
    hp = float(np.float32(math.pi / 2))
    assert list(at) == [hp, -hp]
    tn = _math(capi.MATH_TAN, [0.0, hp])
    assert tn[0] == 0.0 and tn[1] < -1e7
    ex = _math(capi.MATH_EXP, [0.0, 1.0])
    assert ex[0] == 1.0 and abs(ex[1] - math.e) < 3e-7


# ------------------------------------------------------------------------------------------------ 3. conditions on the cases
def _ref_roi(ref):
    x0, y0 = min(ref["tl_x"]), min(ref["tl_y"])
    return (x0, y0, max(ref["br_x"]) - x0 + 1, max(ref["br_y"]) - y0 + 1)


@pytest.mark.parametrize("w,h,mult", rm.sources())
def test_reference_conditions_hold_for_every_warped_case(w, h, mult):
    """For every (source, multiplier, geometry) the GPU test warps: the reference decides the roi, and over the roi the in-band
    share (exact rounding ties apart) stays <= 0.40 and the undetermined share <= 0.10, for both quantisations.  A case that
    breaks a cap is listed in refimpl_mercator.WARP_DROPPED with its reason -- the caps stay."""
    warped = 0
    for name, K, R, scale in rm.geometry_cases(w, h, mult):
        ref = rm.warp_roi_f64(scale, w, h, K, R)
        assert ref["refused"] is False, name
        roi = _ref_roi(ref)
        if roi[2] * roi[3] > rm.MAX_REF_PIXELS or (w, h, mult, name) in rm.WARP_DROPPED:
            continue
        maps = rm.backward_f64(K, R, scale, roi)
        warped += 1
        if roi[2] * roi[3] < 256:
            continue
        for q in (32.0, 1.0):
            band, und = rm.band_shares(maps, q)
            print("%dx%d s%g %s q%g: roi %s, in band %.3f, undetermined %.3f" % (w, h, mult, name, q, roi, band, und))
            assert band <= MAX_BAND_SHARE and und <= MAX_UNDETERMINED_SHARE, (name, q, band, und)
    assert warped >= 6


# ------------------------------------------------------------------------------------------------ 4. interior extremes
@pytest.mark.parametrize("w,h,mult", [(5, 7, 20.0), (333, 217, 0.37)])
def test_pole_frame_extreme_lies_at_an_interior_pixel(w, h, mult):
    """pitch+70: the frame contains the lower pole, and the smallest v of the full scan lies below the smallest v of the border
    by more than the band + 1: a border walk gives another roi."""
    name, hfov, yaw, pitch, roll = [g for g in ri.WARP_GEOMS if g[0] == "pitch+70"][0]
    K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, mult, seam=mult < 1)
    full = rm.warp_roi_f64(scale, w, h, K, R)
    border = rm.warp_roi_f64(scale, w, h, K, R, border_only=True)
    assert full["refused"] is False and border["refused"] is False
    (flo, fhi), (blo, bhi) = full["intervals"]["tl_y"], border["intervals"]["tl_y"]
    print("%dx%d s%g: full-scan min v in [%.3f, %.3f], border-only min v in [%.3f, %.3f]" % (w, h, mult, flo, fhi, blo, bhi))
    assert blo - fhi > (fhi - flo) + (bhi - blo) + 1
    assert not (full["tl_y"] & border["tl_y"])


# ------------------------------------------------------------------------------------------------ the host scan (no device)
def _roi_host(scale, w, h, K, R, kind=rm.MERCATOR):
    from image_stitching_amd import _capi as capi
    r = capi.MisRect()
    K, R = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(R, np.float32)
    rc = capi.load().mis_warper_roi(kind, float(scale), w, h, K.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p), C.byref(r))
    return rc, (r.x, r.y, r.width, r.height)


@pytest.mark.parametrize("w,h,mult", rm.sources())
def test_host_roi_scan_within_the_reference_sets(w, h, mult):
    """mis_warper_roi(MIS_WARP_MERCATOR) -- the plain host loop over all pixels -- lies in the reference's candidate sets."""
    for name, K, R, scale in rm.geometry_cases(w, h, mult):
        ref = rm.warp_roi_f64(scale, w, h, K, R)
        rc, roi = _roi_host(scale, w, h, K, R)
        assert rc == 0 and rm.roi_matches(roi, ref), (name, roi, ref.get("intervals"))


def test_host_roi_refuses_the_pole_pixel_and_an_unknown_kind():
    """R turns the principal ray onto the lower pole: the pixel at the principal point has v = -inf -> MIS_E_INVALID, as the
    reference says; kind 7 stays MIS_E_UNSUPPORTED."""
    K, _, scale = ri.camera(64, 8, 60.0, 0.0)
    R = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    assert rm.warp_roi_f64(scale, 64, 8, K, R)["refused"] is True
    assert _roi_host(scale, 64, 8, K, R)[0] == -1
    assert _roi_host(scale, 64, 8, K, np.eye(3, dtype=np.float32), kind=7)[0] == -6


# ------------------------------------------------------------------------------------------------ 5. plumbing
def test_warp_type_plumbing():
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as st
    assert st.warp_kind("mercator") == 3 == isa._capi.WARP_MERCATOR == rm.MERCATOR
    assert "mercator" not in st.UNBUILT_WARP_TYPES and st.WARP_KINDS["mercator"] == 3
    assert st.MercatorWarper.kind == 3
    assert st.check_warp_config(st.StitchConfig.hot_path(warp_type="mercator")) == 3
    with pytest.raises(NotImplementedError, match="transverseMercator"):
        st.warp_kind("transverseMercator")
    with pytest.raises(ValueError):
        st.warp_kind("Mercator")
