"""Plain numpy reference of the Mercator warp, written from OpenCV's documented semantics (warpers_inl.hpp: MercatorProjector;
cv::MercatorWarper is a RotationWarperBase without a detectResultRoi of its own, so its roi is the extreme of EVERY source
pixel's forward projection, std::min / std::max skipping NaN, static_cast<int> of the four floats, no pole fix-up).

Nothing here calls the oracle or the product library.  The method is tests/refimpl.py's, whose remap candidate and check
helpers are reused: the maps are computed in float64 from the float32 K, R and scale the ABI receives, and per pixel the
candidate quantisations within a first-order float32 error band of the float64 map are the legitimate outputs.

Error model of the float32 map (the band delta; stated once, not tuned to the tests), first order in every error:
  * u' = u / scale and v' = v / scale: one float32 rounding each, e_u = 2^-24 |u'|, e_v = 2^-24 |v'|.
  * v_ = atan(sinh v'): sinh carries its relative error SINH_REL_ERR |sinh v'| and e_v through its derivative, e_v cosh v';
    both pass through d atan / d s = 1 / (1 + sinh^2 v') = 1 / cosh^2 v'; atan adds its absolute error ATAN_ERR:
    e_v_ = (SINH_REL_ERR |sinh v'| + e_v cosh v') / cosh^2 v' + ATAN_ERR.
  * ray r = (cos v_ sin u', sin v_, cos v_ cos u'): the sin / cos errors of refimpl.TRIG_ERR plus the angle errors through the
    derivatives (e_v_ |sin v_| on cos v_, e_v_ |cos v_| on sin v_, e_u |cos u'| on sin u', e_u |sin u'| on cos u'), and
    2^-24 |r_i| for the products of the first and third components.
  * x = (m0 . r) / (m2 . r) with m = K R^-1 in float32, as refimpl_warpers.backward_f64: the ray errors through
    dx/dr_i = (m0_i - x m2_i) / z, the dot products' 3 * 2^-24 (sum_i |m0_i r_i| + |x| sum_i |m2_i r_i|) / |z|, the division
    2^-24 |x|.  The same for y with row 1.  z <= 0 maps to (-1, -1): pixels whose z lies within its band of 0 are undecided.
ROI extremes (forward map of every pixel): (x_, y_, z_) = r_kinv (x, y, 1) carry 3 * 2^-24 of their terms' magnitudes
(e_x, e_y, e_z).  u = scale atan2(x_, z_) carries refimpl's atan2 band and (e_x + e_z) / rho like the cylinder's.  For v:
  w = y_ / |r| (dw/dy_ = cos^2 v_ / |r|, dw/dx_ = -w x_ / |r|^2, dw/dz_ = -w z_ / |r|^2; the squares, sums, square root and
    division round 4 times) has e_w = (cos^2 v_ e_y + |w| (|x_| e_x + |z_| e_z) / |r|) / |r| + 4 * 2^-24 |w|;
  v_ = asin w has e_v_ = ASIN_ERR + e_w / cos v_;
  a = pi/4 + v_/2 has e_a = e_v_ / 2 + 2^-24 a + |pi/4 - float32(pi/4)|;
  t = tan a has the relative error TAN_REL_ERR + e_a / (sin a cos a) = TAN_REL_ERR + 2 e_a / cos v_   (sin 2a = cos v_);
  v = scale log t has the error scale (LOG_REL_ERR |log t| + rel(t)) + 2^-24 |v|:
so the asin, tan and log errors all reach v through 1 / cos v_.  First order is meaningless once rel(t) is large: a pixel whose
rel(t) exceeds 1/8 (a source pixel within ~1e-6 rad of a pole: float32 gives -inf at the lower pole, NaN -- skipped -- or a huge
value at the upper one) makes the roi undecided (`refused` None).  A float64 v that is not finite (a pixel exactly at the lower
pole, v = -inf) is a refusal: the library returns MIS_E_INVALID where OpenCV would cast an infinity to int.

The five constants below are twice the maximum that tests/test_refimpl_mercator_cpu.py measures for the library's functions
against numpy float64 on the sweeps stated there (twice: a sweep is a finite sample); that test pins them.
"""
import math

import numpy as np

import refimpl as ri
from refimpl import U24, TRIG_ERR, INV_TRIG_ERR

MERCATOR = 3

LOG_REL_ERR = 2 * 7.94e-8       # mis_logf, relative; measured maximum 7.94e-8
TAN_REL_ERR = 2 * 1.65e-7       # mis_tanf, relative; measured maximum 1.65e-7
SINH_REL_ERR = 2 * 1.35e-7      # mis_sinhf, relative; measured maximum 1.35e-7
ASIN_ERR = 2 * 1.64e-7          # mis_asinf, absolute; measured maximum 1.64e-7
ATAN_ERR = 2 * 1.39e-7          # mis_atanf, absolute; measured maximum 1.39e-7
PI4_F32_ERR = abs(math.pi / 4 - float(np.float32(math.pi / 4)))
TAN_REL_LIMIT = 0.125           # beyond this relative error of tan the first-order model says nothing: the roi is undecided


def _row_terms(m, x, y):
    v = [m[i, 0] * x + m[i, 1] * y + m[i, 2] for i in range(3)]
    s = [np.abs(m[i, 0] * x) + np.abs(m[i, 1] * y) + abs(m[i, 2]) for i in range(3)]
    return v, s


def forward_f64(r_kinv, scale, x, y):
    """MercatorProjector::mapForward in float64 -> (u, v, band_u, band_v, rel): rel = the relative error bound of tan (the
    first-order model holds while it is small)."""
    (x_, y_, z_), (sx, sy, sz) = _row_terms(r_kinv, x, y)
    ex, ey, ez = 3 * U24 * sx, 3 * U24 * sy, 3 * U24 * sz
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = np.sqrt(x_ * x_ + z_ * z_)
        n = np.sqrt(x_ * x_ + y_ * y_ + z_ * z_)
        th = np.arctan2(x_, z_)
        u = scale * th
        bu = scale * (INV_TRIG_ERR + 8 * U24 * (1 + np.abs(th)) + (ex + ez) / rho) + U24 * np.abs(u)
        w = np.clip(y_ / n, -1.0, 1.0)
        v_ = np.arcsin(w)
        cosv = rho / n                       # cos v_ without the cancellation of sqrt(1 - w^2)
        a = math.pi / 4 + v_ / 2
        t = np.tan(a)
        lt = np.log(t)
        v = scale * lt
        e_w = (cosv * cosv * ey + np.abs(w) * (np.abs(x_) * ex + np.abs(z_) * ez) / n) / n + 4 * U24 * np.abs(w)
        e_v_ = ASIN_ERR + e_w / cosv
        e_a = e_v_ / 2 + U24 * np.abs(a) + PI4_F32_ERR
        rel = TAN_REL_ERR + 2 * e_a / cosv
        bv = scale * (LOG_REL_ERR * np.abs(lt) + rel) + U24 * np.abs(v)
    return u, v, bu, bv, rel


def warp_roi_f64(scale, w, h, K, R, border_only=False):
    """RotationWarperBase::detectResultRoi (every pixel; border_only: the 2(w + h) border pixels, for comparison only) -> dict:
    candidate sets tl_x, tl_y, br_x, br_y (inclusive br) and `refused`: True (the library must return MIS_E_INVALID), False, or
    None (a pixel too close to a pole for the first-order model: either answer, any roi)."""
    scale = float(np.float32(scale))
    _, _, _, _, r_kinv = ri._mats(K, R)
    if border_only:
        xs, ys = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
        bx = np.concatenate([xs, xs, np.zeros(h), np.full(h, w - 1.0)])
        by = np.concatenate([np.zeros(w), np.full(w, h - 1.0), ys, ys])
    else:
        bx, by = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        bx, by = bx.ravel(), by.ravel()
    u, v, bu, bv, rel = forward_f64(r_kinv, scale, bx, by)
    if not (np.isfinite(u).all() and np.isfinite(v).all()):
        return {"refused": True}
    if not (rel <= TAN_REL_LIMIT).all():
        return {"refused": None}
    out = {"refused": False}
    ivl = {"tl_x": ((u - bu).min(), (u + bu).min()), "br_x": ((u - bu).max(), (u + bu).max()),
           "tl_y": ((v - bv).min(), (v + bv).min()), "br_y": ((v - bv).max(), (v + bv).max())}
    out.update({k: set(range(int(math.trunc(lo)), int(math.trunc(hi)) + 1)) for k, (lo, hi) in ivl.items()})
    out["intervals"] = ivl
    return out


def roi_matches(roi, ref):
    return ref["refused"] is False and ri.roi_matches(roi, ref)


def backward_f64(K, R, scale, roi):
    """MercatorProjector::mapBackward for every pixel (u, v) of roi = (x, y, width, height) in float64
    -> dict(x, y, dx, dy, z, zband) in refimpl.spherical_backward_f64's form (z <= 0 maps to (-1, -1))."""
    scale = float(np.float32(scale))
    _, _, _, m, _ = ri._mats(K, R)
    x0, y0, rw, rh = roi
    shape = (rh, rw)
    up = ((x0 + np.arange(rw, dtype=np.float64)) / scale)[None, :]
    vp = ((y0 + np.arange(rh, dtype=np.float64)) / scale)[:, None]
    e_u, e_v = U24 * np.abs(up), U24 * np.abs(vp)
    with np.errstate(over="ignore"):
        sh, ch = np.sinh(vp), np.cosh(vp)
        e_v_ = np.where(np.isfinite(ch), (SINH_REL_ERR * np.abs(sh) / ch + e_v) / ch, 0.0) + ATAN_ERR
    v_ = np.arctan(sh)
    su, cu, sv, cv = np.sin(up), np.cos(up), np.sin(v_), np.cos(v_)
    d_su, d_cu = TRIG_ERR + np.abs(cu) * e_u, TRIG_ERR + np.abs(su) * e_u
    d_cv, d_sv = TRIG_ERR + np.abs(sv) * e_v_, TRIG_ERR + np.abs(cv) * e_v_
    r = [np.broadcast_to(c, shape) for c in (cv * su, sv, cv * cu)]
    dr = [np.abs(su) * d_cv + np.abs(cv) * d_su + U24 * np.abs(r[0]), np.broadcast_to(d_sv, shape),
          np.abs(cu) * d_cv + np.abs(cv) * d_cu + U24 * np.abs(r[2])]
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


def z_undecided(maps):
    return np.abs(maps["z"]) <= maps["zband"]


def map_forward_f64(r_kinv, scale, x, y):
    u, v, _, _, _ = forward_f64(r_kinv, scale, np.asarray(x, np.float64), np.asarray(y, np.float64))
    return u, v


def map_backward_exact_f64(k_rinv, scale, u, v):
    """mapBackward without the z test, in float64 -> (x, y)."""
    u, v = np.asarray(u, np.float64) / scale, np.asarray(v, np.float64) / scale
    v_ = np.arctan(np.sinh(v))
    r = (np.cos(v_) * np.sin(u), np.sin(v_), np.cos(v_) * np.cos(u))
    xx, yy, z = (sum(k_rinv[i, j] * r[j] for j in range(3)) for i in range(3))
    return xx / z, yy / z


def band_shares(maps, q):
    """The shares refimpl's candidate helpers would report for these maps at quantisation q (32: INTER_LINEAR, 1: INTER_NEAREST),
    whatever the content -> (in-band share excluding exact rounding ties, undetermined share)."""
    zu = z_undecided(maps)
    xl, xh, xd = ri._axis_candidates(maps["x"], maps["dx"], q, zu)
    yl, yh, yd = ri._axis_candidates(maps["y"], maps["dy"], q, zu)
    und = ~(xd & yd)
    band = ((xl != xh) | (yl != yh)) & ~und
    ties = np.zeros(band.shape, bool)
    for c in ("x", "y"):
        ties |= np.abs(np.modf(maps[c] * q)[0]) == 0.5
    n = band.size
    return float((band & ~ties).sum()) / n, float(und.sum()) / n


# The (source, multiplier, geometry) cases of the Mercator tests: refimpl's sources plus 333 x 217, over refimpl.WARP_GEOMS.
MAX_REF_PIXELS = 2_000_000      # rois past this are checked for their bounds only (pole geometries: v runs to +-scale * 15)


def sources():
    out = [(w, h, m) for (w, h), mults in ri.WARP_SOURCES for m in mults]
    return out + [(333, 217, 1.0), (333, 217, 0.37)]


def geometry_cases(w, h, mult):
    """-> [(name, K, R, scale)] over refimpl.WARP_GEOMS for one source."""
    return [(name,) + ri.camera(w, h, hfov, yaw, pitch, roll, mult, seam=mult < 1) for name, hfov, yaw, pitch, roll in ri.WARP_GEOMS]


# (w, h, multiplier, geometry) whose WARP is left out (the roi is still checked), each with its reason; filled from the conditions
# tests/test_refimpl_mercator_cpu.py::test_reference_conditions_hold_for_every_warped_case states on the reference alone
WARP_DROPPED = {
}
