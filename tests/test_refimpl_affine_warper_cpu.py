"""Known answers of the affine warper's numpy reference (tests/refimpl_affine_family.py), its error model against a float32
emulation of the operation sequence, the project's band caps on every scene of the GPU test (on the reference alone), the
library's host paths (roi, debug map) against it, and the plumbing: kind 13, AffineWarper, the refusals that stay."""
import ctypes as C
import math

import numpy as np
import pytest

import refimpl as ri
import refimpl_affine_family as ra
import refimpl_warpers as rw

SIZES = [(65, 9), (333, 217)]


def _first_roi(ref):
    return (min(ref["tl_x"]), min(ref["tl_y"]), max(ref["br_x"]) - min(ref["tl_x"]) + 1, max(ref["br_y"]) - min(ref["tl_y"]) + 1)


def _roi_host(scale, w, h, K, H):
    from image_stitching_amd import _capi as capi
    r = capi.MisRect()
    K, H = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(H, np.float32)
    rc = capi.load().mis_warper_roi(ra.AFFINE, float(scale), w, h, K.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p), C.byref(r))
    return rc, (r.x, r.y, r.width, r.height)


def _map_host(scale, K, H, roi):
    from image_stitching_amd import _capi as capi
    K, H = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(H, np.float32)
    rr = capi.MisRect(*[int(v) for v in roi])
    xy = np.empty((roi[3], roi[2], 2), np.float32)
    rc = capi.load().mis_debug_warper_map_f32(None, ra.AFFINE, float(scale), K.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p), C.byref(rr),
                                              xy.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return xy


# ------------------------------------------------------------------------------------------------ known answers
def test_rt_from_homogeneous():
    H = ra.similarity(30.0, 1.25, 3.0, -2.0)
    R, T = ra.rt_from_homogeneous(H)
    c, s = np.float32(1.25 * math.cos(math.radians(30.0))), np.float32(1.25 * math.sin(math.radians(30.0)))
    assert np.array_equal(R, np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], np.float32))
    want = -(R.astype(np.float64) @ np.array([3.0, -2.0, 0.0]))
    assert np.array_equal(T[:2], want[:2].astype(np.float32)) and T[2] == 0.0 and R.dtype == T.dtype == np.float32
    # a pure translation: R = I, T = -T0; the identity: T = -0 (the product by -1), and 1 - T[2] = 1
    R, T = ra.rt_from_homogeneous(ra.similarity(0, 1, 5.5, -2.5))
    assert np.array_equal(R, np.eye(3, dtype=np.float32)) and np.array_equal(T, np.array([-5.5, 2.5, 0], np.float32))
    _, T = ra.rt_from_homogeneous(np.eye(3))
    assert (T == 0).all() and 1.0 - float(T[2]) == 1.0


def test_backward_is_K_H_and_forward_its_inverse_at_unit_scale():
    """s = 1: the backward map of panorama pixel p is K H (p / scale, 1), the forward map its inverse."""
    for tag, K, H, scale in ra.warp_cases(333, 217):
        if tag.split("-")[0] in ("enlarge", "reduce"):
            continue
        roi = (-40, -30, 90, 70)
        maps = ra.backward_f64(K, H, scale, roi)
        u, v = np.meshgrid(roi[0] + np.arange(roi[2], dtype=np.float64), roi[1] + np.arange(roi[3], dtype=np.float64))
        p = K.astype(np.float64) @ H.astype(np.float64) @ np.stack([u.ravel() / scale, v.ravel() / scale, np.ones(u.size)])
        tol = 1e-6 * max(1.0, float(np.abs(p).max()))      # float32 sin / cos in H: orthonormal to 1e-7
        assert np.abs(maps["x"].ravel() - p[0] / p[2]).max() < tol and np.abs(maps["y"].ravel() - p[1] / p[2]).max() < tol, tag
        u2, v2, _, _, z_, _ = ra.forward_f64(K, H, scale, maps["x"], maps["y"])
        assert (z_ > 0).all() and np.abs(u2 - u).max() < 10 * tol * scale and np.abs(v2 - v).max() < 10 * tol * scale, tag


@pytest.mark.parametrize("s", [1.25, 0.8])
def test_forward_and_backward_differ_by_s_squared(s):
    """The quirk: Rinv is R's transpose, so forward(backward(u)) = scale (t0 + s^2 (u / scale - t0))."""
    K, scale = ra.scene_cameras(333, 217)[1][1:]
    H = ra.similarity(11.0, s, 0.05, -0.07)
    _, T = ra.rt_from_homogeneous(H)
    roi = (-20, -10, 50, 30)
    maps = ra.backward_f64(K, H, scale, roi)
    u, v = np.meshgrid(roi[0] + np.arange(roi[2], dtype=np.float64), roi[1] + np.arange(roi[3], dtype=np.float64))
    u2, v2, _, _, _, _ = ra.forward_f64(K, H, scale, maps["x"], maps["y"])
    s2 = float(H[0, 0]) ** 2 + float(H[1, 0]) ** 2
    assert abs(s2 - s * s) < 1e-6
    assert np.abs(u2 - scale * (T[0] + s2 * (u / scale - T[0]))).max() < 1e-4
    assert np.abs(v2 - scale * (T[1] + s2 * (v / scale - T[1]))).max() < 1e-4


def test_roi_known_answers():
    w, h = 65, 9
    I = np.eye(3, dtype=np.float32)
    ref = ra.warp_roi_f64(1.0, w, h, I, I)
    # (an extreme that is an integer has the integers on either side of its band as candidates)
    assert ref["refused"] is False and ra.roi_matches((0, 0, w, h), ref) and not ra.roi_matches((1, 0, w, h), ref)
    # H maps panorama coordinates to frame coordinates: the frame shifted by (37, -12) lands at (-37, 12)
    ref = ra.warp_roi_f64(1.0, w, h, I, ra.similarity(0, 1, 37.0, -12.0))
    assert ra.roi_matches((-37, 12, w, h), ref) and not ra.roi_matches((-37, 13, w, h), ref) and not ra.roi_matches((37, -12, w, h), ref)
    # a corner behind the panorama plane through a general K (a projective bottom row): refused
    K = np.array([[60, 0, 30], [0, 60, 4], [1, 0, 1]], np.float32)
    assert ra.warp_roi_f64(60.0, w, h, K, I)["refused"] is True


# ------------------------------------------------------------------------------------------------ the error model
def _backward_f32(K, H, scale, roi):
    """The float32 operation sequence of PlaneProjector::mapBackward with t, k_rinv formed as ProjectorBase::setCameraParams does
    (double products and sums of the float32 matrices, one rounding)."""
    R, T = ra.rt_from_homogeneous(H)
    k = (np.asarray(K, np.float32).astype(np.float64) @ R.T.astype(np.float64)).astype(np.float32)
    f = np.float32
    x0, y0, rw_, rh = roi
    u = (x0 + np.arange(rw_)).astype(np.float32)[None, :] / f(scale) - T[0]
    v = (y0 + np.arange(rh)).astype(np.float32)[:, None] / f(scale) - T[1]
    w = f(1.0) - T[2]
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (k[0, 0] * u + k[0, 1] * v) + k[0, 2] * w
        y = (k[1, 0] * u + k[1, 1] * v) + k[1, 2] * w
        z = (k[2, 0] * u + k[2, 1] * v) + k[2, 2] * w
        return x / z, y / z


@pytest.mark.parametrize("w,h", SIZES)
def test_error_model_holds_the_float32_sequence_and_the_host_map(w, h):
    """Every scene: the float32 emulation of the sequence and the library's host map (mis_debug_warper_map_f32 without a
    context) lie within the model's band of the float64 map, and the library's floats are the emulation's."""
    for tag, K, H, scale in ra.warp_cases(w, h):
        ref = ra.warp_roi_f64(scale, w, h, K, H)
        assert ref["refused"] is False, tag
        roi = _first_roi(ref)
        maps = ra.backward_f64(K, H, scale, roi)
        assert not rw.z_undecided(maps).any(), tag
        x32, y32 = _backward_f32(K, H, scale, roi)
        assert (np.abs(x32 - maps["x"]) <= maps["dx"]).all() and (np.abs(y32 - maps["y"]) <= maps["dy"]).all(), tag
        xy = _map_host(scale, K, H, roi)
        assert np.array_equal(xy[..., 0], x32) and np.array_equal(xy[..., 1], y32), tag


@pytest.mark.parametrize("w,h", SIZES)
def test_every_scene_stays_within_the_band_caps(w, h):
    """On the reference alone: in-band share (exact ties apart) <= MAX_BAND_SHARE, undetermined share <= MAX_UNDETERMINED_SHARE,
    for the INTER_LINEAR colour warp and the INTER_NEAREST mask; the tie scene is all ties."""
    img = ri.content("rand", (h, w, 3), seed=w)
    full = np.full((h, w), 255, np.uint8)
    for tag, K, H, scale in ra.warp_cases(w, h):
        roi = _first_roi(ra.warp_roi_f64(scale, w, h, K, H))
        maps = ra.backward_f64(K, H, scale, roi)
        n = roi[2] * roi[3]
        for what, q, (cands, band, und) in (("linear", 32.0, ri.remap_linear_reflect_candidates(img, maps)),
                                             ("mask", 1.0, ri.remap_nearest_constant_candidates(full, maps))):
            t = ra.ties(maps, q)
            nb, nt, nu = int((band & ~und).sum()), int((band & ~und & t).sum()), int(und.sum())
            assert nb - nt <= ra.MAX_BAND_SHARE * n and nu <= ra.MAX_UNDETERMINED_SHARE * n, (tag, what, nb, nt, nu, n)
            if tag == "tie-KI" and what == "mask":
                assert nt == n


# ------------------------------------------------------------------------------------------------ the library's host roi
@pytest.mark.parametrize("w,h", SIZES)
def test_host_roi_matches_the_reference(w, h):
    for tag, K, H, scale in ra.warp_cases(w, h):
        rc, roi = _roi_host(scale, w, h, K, H)
        assert rc == 0 and ra.roi_matches(roi, ra.warp_roi_f64(scale, w, h, K, H)), (tag, roi)
    K = np.array([[60, 0, 30], [0, 60, 4], [1, 0, 1]], np.float32)
    assert _roi_host(60.0, w, h, K, np.eye(3, dtype=np.float32))[0] == -1     # MIS_E_INVALID


def test_orthonormal_H_without_translation_has_the_plane_roi():
    """Translation column zero and H orthonormal (an in-plane rotation): kind 13 is kind 2 on the same K and projector R, which
    getRTfromHomogeneous makes H's transpose."""
    from image_stitching_amd import _capi as capi
    w, h = 333, 217
    for roll in (0.0, 7.0, -30.0, 90.0):
        K, R, scale = ri.camera(w, h, 60.0, 0.0, 0.0, roll)
        assert R[0, 2] == 0 and R[1, 2] == 0 and R[2, 0] == 0 and R[2, 1] == 0
        Kc, Rc = np.ascontiguousarray(K, np.float32), np.ascontiguousarray(R, np.float32)
        r = capi.MisRect()
        rc = capi.load().mis_warper_roi(rw.PLANE, float(scale), w, h, Kc.ctypes.data_as(C.c_void_p), Rc.ctypes.data_as(C.c_void_p), C.byref(r))
        assert rc == 0 and (rc, (r.x, r.y, r.width, r.height)) == _roi_host(scale, w, h, K, np.ascontiguousarray(R.T)), roll


# ------------------------------------------------------------------------------------------------ plumbing
def test_kind_13_plumbing_and_the_refusals_that_stay():
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as st
    assert isa.WARP_AFFINE == 13 == ra.AFFINE and isa._capi.WARP_AFFINE == 13
    assert isa.AffineWarper(None, 2.5).kind == 13 and isinstance(isa.AffineWarper(None, 1.0), isa.RotationWarper)
    assert isa.RotationWarper(None, 1.0, 13).kind == 13 and 13 in st.BUILT_WARP_KINDS
    assert not isa._capi.roi_is_full_scan(13)
    assert isa.AffineWarper(None, 1.0).warp_roi((65, 9), np.eye(3), ra.similarity(0, 1, 37.0, -12.0)) == (-37, 12, 65, 9)
    for kind in (6, 7, 12):
        with pytest.raises(NotImplementedError):
            isa.RotationWarper(None, 1.0, kind)
    # the configuration names stay refused: the family is reached through the warper class, not through warp_type / ba_cost_func
    with pytest.raises(NotImplementedError, match="affine"):
        st.warp_kind("affine")
    assert "affine" in st.REFUSED_WARP_TYPES and len(st.REFUSED_WARP_TYPES) == 7 and "affine" not in st.WARP_KINDS
    with pytest.raises(NotImplementedError, match="affine"):
        isa.StitchConfig.hot_path(ba_cost_func="affine")
