"""Plain numpy reference of the fisheye and stereographic warps, written from OpenCV's documented semantics (warpers_inl.hpp:
FisheyeProjector, StereographicProjector; cv::FisheyeWarper and cv::StereographicWarper are RotationWarperBase without a
detectResultRoi of their own, so the roi is the extreme of EVERY source pixel's forward projection, std::min / std::max skipping
NaN, static_cast<int> of the four floats, no fix-up).

    forward:   (x_, y_, z_) = r_kinv (x, y, 1),  u_ = atan2(x_, z_),  v_ = pi - acos(y_ / |(x_, y_, z_)|)
               fisheye:        u = scale v_ cos u_,  v = scale v_ sin u_
               stereographic:  r = sin v_ / (1 - cos v_);  u = scale r cos u_,  v = scale r sin u_
    backward:  u' = u / scale,  v' = v / scale,  u_ = atan2(v', u'),  rho = sqrt(u'^2 + v'^2)
               fisheye v_ = rho;  stereographic v_ = 2 atan(1 / rho)
               ray = (sin(pi - v_) sin u_, cos(pi - v_), sin(pi - v_) cos u_);  (x, y, z) = k_rinv ray;  z > 0: (x / z, y / z) else (-1, -1)

Nothing here calls the oracle or the product library.  The method is tests/refimpl.py's, whose remap candidate and check helpers
are reused: the maps are computed in float64 from the float32 K, R and scale the ABI receives, and per pixel the candidate
quantisations within a first-order float32 error band of the float64 map are the legitimate outputs.

Error model of the float32 backward map (the band delta; stated once, not tuned to the tests), first order in every error:
  * u' = u / scale and v' = v / scale: one float32 rounding each, relative 2^-24 (u, v are integers, exact in float32).
  * rho = sqrt(u'^2 + v'^2): the inputs' relative 2^-24, the squares, the sum and the root round once each: e_rho = 3 * 2^-24 rho.
  * u_ = atan2(v', u') = atan(v' / u') (+- float32 pi): the quotient t carries the relative error 3 * 2^-24 (two inputs, one
    division), which reaches the angle through |t| / (1 + t^2) <= 1/2; atan adds ATAN_ERR; the quadrant fix adds the float32 pi and
    one rounding:  e_u_ = ATAN_ERR + 1.5 * 2^-24 + PI_F32_ERR + 2^-24 |u_|.  The errors of u' and v' are RELATIVE, so this does not
    grow towards the centre; at the centre pixel itself u' = v' = 0 exactly and atan2(0, 0) = 0 on both sides.  An absolute
    perturbation of (u', v') would turn the angle by ~1 / rho -- but the angle reaches the ray only through sin(pi - v_), which
    vanishes like rho (fisheye) or 2 rho (stereographic: v_ = 2 atan(1 / rho) ~ pi - 2 rho), so the band is finite at the centre
    either way and no disc around it is left undetermined.
  * v_: fisheye e_v_ = e_rho.  Stereographic: 1 / rho carries 4 * 2^-24 relative, through |t| / (1 + t^2) with t = 1 / rho (0 at
    rho = 0, where t = +inf and atan gives float32(pi / 2)), plus ATAN_ERR, doubled: e_v_ = 2 (ATAN_ERR + 4 * 2^-24 t / (1 + t^2)).
  * phi = pi - v_ in float32: e_phi = e_v_ + PI_F32_ERR + 2^-24 |phi|.
  * sin / cos of phi and of u_: TRIG_ERR each plus the angle errors through the derivatives; ray r = (sin phi sin u_, cos phi,
    sin phi cos u_) with 2^-24 |r_i| for the products of the first and third components.
  * x = (m0 . r) / (m2 . r) with m = K R^-1 in float32, as refimpl_warpers.backward_f64: the ray errors through
    dx/dr_i = (m0_i - x m2_i) / z, the dot products' 3 * 2^-24 (sum_i |m0_i r_i| + |x| sum_i |m2_i r_i|) / |z|, the division
    2^-24 |x|.  The same for y with row 1.  z <= 0 maps to (-1, -1): pixels whose z lies within its band of 0 are undecided.
ROI extremes (forward map of every pixel): (x_, y_, z_) carry 3 * 2^-24 of their terms' magnitudes (e_x, e_y, e_z).
  * u_ = atan2(x_, z_): refimpl's atan2 band INV_TRIG_ERR + 8 * 2^-24 (1 + |u_|) plus (e_x + e_z) / |(x_, z_)|, as the cylinder's.
  * w = y_ / |r| as refimpl_mercator: e_w = (c^2 e_y + |w| (|x_| e_x + |z_| e_z) / |r|) / |r| + 4 * 2^-24 |w|, c = |(x_, z_)| / |r|.
  * acos is not differentiable at w = +-1, so its input error is carried as an interval, not to first order:
    e_acos = max |acos(clip(w +- e_w)) - acos(w)| + INV_TRIG_ERR + 8 * 2^-24 (1 + acos w);  e_v_ = e_acos + PI_F32_ERR + 2^-24 |v_|.
  * cos u_, sin u_: TRIG_ERR + the angle error through the derivative, and never more than 2 (on the axis x_ = z_ = 0 the angle
    is arbitrary; the radius it multiplies is 0 there for the fisheye map).
  * fisheye: u = scale v_ cos u_ has the band scale (e_v_ |cos u_| + |v_| e_cos) + 2 * 2^-24 |u|, v likewise.
  * stereographic: N = sin v_ has e_N = TRIG_ERR + |cos v_| e_v_;  D = 1 - cos v_ has e_D = TRIG_ERR + |sin v_| e_v_ + 2^-24 D.
    D vanishes at v_ = 0 (the ray (0, -1, 0)), so the quotient is carried as an interval too:
    r in [(N - e_N) / (D + e_D), (N + e_N) / (D - e_D)], plus 2^-24 |r|, valid while e_D <= D / 2.  A pixel beyond that (within
    ~1.3e-3 rad of the singular ray: float32 gives NaN -- skipped -- on it and a value of either magnitude next to it) or a
    pixel whose float64 image is NaN makes the roi undecided (`refused` None: either answer, any roi).
  * A refusal (`refused` True; the library returns MIS_E_INVALID where OpenCV would cast to int a float the int cannot hold): some
    pixel's |u| or |v|, less its band, is at least 2^31 (infinite included).  Within the band of 2^31: undecided.

No new constant: U24, TRIG_ERR, INV_TRIG_ERR and PI_F32_ERR are refimpl's, ATAN_ERR is refimpl_mercator's (twice the maximum
measured for mis_atanf over +-[0, 1e5] and +-inf, pinned by test_refimpl_mercator_cpu.py).
"""
import math

import numpy as np

import refimpl as ri
import refimpl_mercator as rm
from refimpl import U24, TRIG_ERR, INV_TRIG_ERR, PI_F32_ERR
from refimpl_mercator import ATAN_ERR

FISHEYE, STEREOGRAPHIC = 4, 5
KINDS = {"fisheye": FISHEYE, "stereographic": STEREOGRAPHIC}
D_REL_LIMIT = 0.5               # e_D / D beyond this: the stereographic quotient's interval says nothing, the roi is undecided
INT_LIMIT = 2147483520.0        # the largest float32 below 2^31 (roi_from_extremes refuses what lies beyond)


def forward_f64(kind, r_kinv, scale, x, y):
    """{Fisheye,Stereographic}Projector::mapForward in float64 -> (u, v, band_u, band_v, ok): ok False where the model says
    nothing about the pixel (stereographic next to the singular ray, or a NaN)."""
    (x_, y_, z_), (sx, sy, sz) = rm._row_terms(r_kinv, x, y)
    ex, ey, ez = 3 * U24 * sx, 3 * U24 * sy, 3 * U24 * sz
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rho = np.sqrt(x_ * x_ + z_ * z_)
        n = np.sqrt(x_ * x_ + y_ * y_ + z_ * z_)
        th = np.arctan2(x_, z_)
        e_th = INV_TRIG_ERR + 8 * U24 * (1 + np.abs(th)) + (ex + ez) / rho
        w = y_ / n
        c = rho / n
        e_w = (c * c * ey + np.abs(w) * (np.abs(x_) * ex + np.abs(z_) * ez) / n) / n + 4 * U24 * np.abs(w)
        wc = np.clip(w, -1.0, 1.0)
        ph = np.arccos(wc)
        e_ac = np.maximum(np.abs(np.arccos(np.clip(wc - e_w, -1.0, 1.0)) - ph), np.abs(np.arccos(np.clip(wc + e_w, -1.0, 1.0)) - ph))
        e_ac = e_ac + INV_TRIG_ERR + 8 * U24 * (1 + ph)
        v_ = math.pi - ph
        e_v_ = e_ac + PI_F32_ERR + U24 * np.abs(v_)
        cu, su = np.cos(th), np.sin(th)
        e_cu, e_su = np.fmin(TRIG_ERR + np.abs(su) * e_th, 2.0), np.fmin(TRIG_ERR + np.abs(cu) * e_th, 2.0)     # (fmin: 0 * inf on the axis -> 2)
        if kind == FISHEYE:
            r, e_r = v_, e_v_
            ok = np.isfinite(r)
        else:
            N, D = np.sin(v_), 1.0 - np.cos(v_)
            e_N = TRIG_ERR + np.abs(np.cos(v_)) * e_v_
            e_D = TRIG_ERR + np.abs(N) * e_v_ + U24 * D
            ok = np.isfinite(N / D) & (e_D <= D_REL_LIMIT * D)
            Ds = np.where(ok, D, 1.0)
            r = np.where(ok, N / Ds, 0.0)
            e_r = np.maximum((N + e_N) / np.maximum(Ds - e_D, 1e-300) - r, r - (N - e_N) / (Ds + e_D)) + U24 * np.abs(r)
        u, v = scale * r * cu, scale * r * su
        bu = scale * (e_r * np.abs(cu) + np.abs(r) * e_cu) + 2 * U24 * np.abs(u)
        bv = scale * (e_r * np.abs(su) + np.abs(r) * e_su) + 2 * U24 * np.abs(v)
        ok = ok & np.isfinite(th) & ~np.isnan(u) & ~np.isnan(v) & ~np.isnan(bu) & ~np.isnan(bv)
    return u, v, bu, bv, ok


def warp_roi_f64(kind, scale, w, h, K, R):
    """RotationWarperBase::detectResultRoi (every pixel) -> dict: candidate sets tl_x, tl_y, br_x, br_y (inclusive br) and
    `refused`: True (the library must return MIS_E_INVALID), False, or None (either answer, any roi)."""
    scale = float(np.float32(scale))
    _, _, _, _, r_kinv = ri._mats(K, R)
    bx, by = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    u, v, bu, bv, ok = forward_f64(kind, r_kinv, scale, bx.ravel(), by.ravel())
    if not ok.all():
        return {"refused": None}
    big = np.maximum(np.abs(u) - bu, np.abs(v) - bv)
    if (big >= INT_LIMIT).any():
        return {"refused": True}
    if (np.maximum(np.abs(u) + bu, np.abs(v) + bv) >= INT_LIMIT).any():
        return {"refused": None}
    out = {"refused": False}
    ivl = {"tl_x": ((u - bu).min(), (u + bu).min()), "br_x": ((u - bu).max(), (u + bu).max()),
           "tl_y": ((v - bv).min(), (v + bv).min()), "br_y": ((v - bv).max(), (v + bv).max())}
    out.update({k: set(range(int(math.trunc(lo)), int(math.trunc(hi)) + 1)) if hi - lo < 1e6 else _Range(int(math.trunc(lo)), int(math.trunc(hi)))
                for k, (lo, hi) in ivl.items()})
    out["intervals"] = ivl
    return out


class _Range:
    """A candidate set too wide to enumerate (a stereographic bound next to the singular ray): lo .. hi inclusive."""

    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def __contains__(self, k):
        return self.lo <= k <= self.hi

    def __iter__(self):
        return iter((self.lo, self.hi))


def roi_matches(roi, ref):
    return ref["refused"] is False and ri.roi_matches(roi, ref)


def ref_roi(ref):
    """The widest roi of the candidate sets (the one the reference conditions are evaluated on)."""
    x0, y0 = min(ref["tl_x"]), min(ref["tl_y"])
    return (x0, y0, max(ref["br_x"]) - x0 + 1, max(ref["br_y"]) - y0 + 1)


def backward_f64(kind, K, R, scale, roi):
    """{Fisheye,Stereographic}Projector::mapBackward for every pixel (u, v) of roi = (x, y, width, height) in float64
    -> dict(x, y, dx, dy, z, zband) in refimpl.spherical_backward_f64's form (z <= 0 maps to (-1, -1))."""
    scale = float(np.float32(scale))
    _, _, _, m, _ = ri._mats(K, R)
    x0, y0, rw, rh = roi
    shape = (rh, rw)
    up = np.broadcast_to(((x0 + np.arange(rw, dtype=np.float64)) / scale)[None, :], shape)
    vp = np.broadcast_to(((y0 + np.arange(rh, dtype=np.float64)) / scale)[:, None], shape)
    rho = np.sqrt(up * up + vp * vp)
    u_ = np.arctan2(vp, up)
    e_u_ = ATAN_ERR + 1.5 * U24 + PI_F32_ERR + U24 * np.abs(u_)
    if kind == FISHEYE:
        v_ = rho
        e_v_ = 3 * U24 * rho
    else:
        with np.errstate(divide="ignore"):
            t = 1.0 / rho
        v_ = 2.0 * np.arctan(t)
        tt = np.where(np.isfinite(t), t / (1.0 + np.where(np.isfinite(t), t, 0.0) ** 2), 0.0)
        e_v_ = 2.0 * (ATAN_ERR + 4 * U24 * tt)
    ph = math.pi - v_
    e_ph = e_v_ + PI_F32_ERR + U24 * np.abs(ph)
    sv, cv, su, cu = np.sin(ph), np.cos(ph), np.sin(u_), np.cos(u_)
    d_sv, d_cv = TRIG_ERR + np.abs(cv) * e_ph, TRIG_ERR + np.abs(sv) * e_ph
    d_su, d_cu = TRIG_ERR + np.abs(cu) * e_u_, TRIG_ERR + np.abs(su) * e_u_
    r = [sv * su, cv, sv * cu]
    dr = [np.abs(su) * d_sv + np.abs(sv) * d_su + U24 * np.abs(r[0]), d_cv, np.abs(cu) * d_sv + np.abs(sv) * d_cu + U24 * np.abs(r[2])]
    xx = sum(m[0, i] * r[i] for i in range(3))
    yy = sum(m[1, i] * r[i] for i in range(3))
    z = sum(m[2, i] * r[i] for i in range(3))
    az2 = sum(np.abs(m[2, i] * r[i]) for i in range(3))
    zband = sum(abs(m[2, i]) * dr[i] for i in range(3)) + 3 * U24 * az2
    live = z > 0
    zs = np.where(live, z, 1.0)
    x = np.where(live, xx / zs, -1.0)
    y = np.where(live, yy / zs, -1.0)
    out = {"x": x, "y": y, "z": z, "zband": zband}
    for name, row, val in (("dx", 0, x), ("dy", 1, y)):
        g = [(m[row, i] - val * m[2, i]) / zs for i in range(3)]
        band = sum(np.abs(g[i]) * dr[i] for i in range(3))
        terms = sum(np.abs(m[row, i] * r[i]) for i in range(3)) + np.abs(val) * az2
        band = band + 3 * U24 * terms / np.abs(zs) + U24 * np.abs(val)
        out[name] = np.where(live, band, 0.0)
    return out


z_undecided = rm.z_undecided
band_shares = rm.band_shares


def map_forward_f64(kind, r_kinv, scale, x, y):
    u, v, _, _, _ = forward_f64(kind, r_kinv, scale, np.asarray(x, np.float64), np.asarray(y, np.float64))
    return u, v


def ray_backward_f64(kind, scale, u, v):
    """The ray of mapBackward in float64 -> (x_, y_, z_)."""
    u, v = np.asarray(u, np.float64) / scale, np.asarray(v, np.float64) / scale
    u_ = np.arctan2(v, u)
    rho = np.sqrt(u * u + v * v)
    with np.errstate(divide="ignore"):
        v_ = rho if kind == FISHEYE else 2.0 * np.arctan(1.0 / rho)
    s = np.sin(math.pi - v_)
    return s * np.sin(u_), np.cos(math.pi - v_), s * np.cos(u_)


def map_backward_exact_f64(kind, k_rinv, scale, u, v):
    """mapBackward without the z test, in float64 -> (x, y)."""
    r = ray_backward_f64(kind, scale, u, v)
    xx, yy, z = (sum(k_rinv[i, j] * r[j] for j in range(3)) for i in range(3))
    return xx / z, yy / z


# The (source, multiplier, geometry) cases: refimpl_mercator's sources (refimpl's plus 333 x 217) over refimpl.WARP_GEOMS.
MAX_REF_PIXELS = 2_000_000      # rois past this are checked for their bounds only
sources = rm.sources
geometry_cases = rm.geometry_cases

# (kind, w, h, multiplier, geometry) whose WARP is left out (the roi is still checked), each with its reason; filled from the conditions
# tests/test_refimpl_polar_warpers_cpu.py::test_reference_conditions_hold_for_every_warped_case states on the reference alone
WARP_DROPPED = {
}
