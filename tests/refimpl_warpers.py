"""Plain numpy references of the cylindrical and plane warps, written from OpenCV's documented semantics (warpers_inl.hpp:
CylindricalProjector, PlaneProjector with T = 0; CylindricalWarper::detectResultRoi = detectResultRoiByBorder,
PlaneWarper::detectResultRoi = the four corners).

Nothing here calls the oracle or the product library.  The method is tests/refimpl.py's, whose remap candidate and check
helpers are reused: the maps are computed in float64 from the float32 K, R and scale the ABI receives, and per pixel the
candidate quantisations within a first-order float32 error band of the float64 map are the legitimate outputs.

Error model of the float32 map (the band delta; stated once, not tuned to the tests), first order in every error:
  * u' = u / scale and v' = v / scale: one float32 rounding each, e_u = 2^-24 |u'|, e_v = 2^-24 |v'|.
  * cylindrical ray r = (sin u', v', cos u'): the sin / cos errors of refimpl.TRIG_ERR plus e_u through the derivative on the
    first and third components, e_v on the second (the products by the row factor 1 are exact).
  * plane ray r = (u', v', 1): e_u, e_v and 0 -- division, product and sum roundings only.
  * x = (m0 . r) / (m2 . r) with m = K R^-1 in float32, as refimpl.spherical_backward_f64: the ray errors through
    dx/dr_i = (m0_i - x m2_i) / z, the dot products' 3 * 2^-24 (sum_i |m0_i r_i| + |x| sum_i |m2_i r_i|) / |z|, the division
    2^-24 |x|.  The same for y with row 1.
  The cylinder maps z <= 0 to (-1, -1): pixels whose z lies within its band of 0 are the z-sign-undecided ones.  The plane divides
  whatever the sign of z: pixels whose z lies within its band of 0 (near-zero z: the quotient is unbounded) are reported the
  same way.  Both are left unconstrained by the candidate helpers and counted apart.
ROI extremes: u = scale atan2(x_, z_) carries refimpl's atan2 band; the quotients v = scale y_ / sqrt(x_^2 + z_^2) and
u, v = scale x_ / z_, scale y_ / z_ carry the float32 roundings of the r_kinv products (3 * 2^-24 of their terms) through the
quotient plus 4 * 2^-24 of the value.  A bound has two candidates only where the float64 extreme lies within that band of an
integer.  Refusals (the library's departures from OpenCV): a plane corner with z_ <= 0, a cylindrical extreme that is not
finite; a corner whose z_ is within its band of 0 makes the plane's refusal undecided.
"""
import math

import numpy as np

import refimpl as ri
from refimpl import U24, TRIG_ERR, INV_TRIG_ERR

CYLINDRICAL, PLANE = 1, 2


def _row_terms(m, x, y):
    """r_kinv (x, y, 1) in float64 -> (x_, y_, z_) and the sums of their terms' magnitudes (the float32 rounding scale)."""
    v = [m[i, 0] * x + m[i, 1] * y + m[i, 2] for i in range(3)]
    s = [np.abs(m[i, 0] * x) + np.abs(m[i, 1] * y) + abs(m[i, 2]) for i in range(3)]
    return v, s


def forward_f64(kind, r_kinv, scale, x, y):
    """{Cylindrical,Plane}Projector::mapForward in float64 -> (u, v, band_u, band_v, z_ and its band)."""
    (x_, y_, z_), (sx, sy, sz) = _row_terms(r_kinv, x, y)
    ex, ey, ez = 3 * U24 * sx, 3 * U24 * sy, 3 * U24 * sz
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == CYLINDRICAL:
            rho = np.sqrt(x_ * x_ + z_ * z_)
            th = np.arctan2(x_, z_)
            u = scale * th
            v = scale * y_ / rho
            bu = scale * (INV_TRIG_ERR + 8 * U24 * (1 + np.abs(th)) + (ex + ez) / rho) + U24 * np.abs(u)
            bv = scale * (ey + np.abs(y_ / rho) * (ex + ez)) / rho + 4 * U24 * np.abs(v)
        else:
            u = scale * x_ / z_
            v = scale * y_ / z_
            bu = scale * (ex + np.abs(x_ / z_) * ez) / np.abs(z_) + 4 * U24 * np.abs(u)
            bv = scale * (ey + np.abs(y_ / z_) * ez) / np.abs(z_) + 4 * U24 * np.abs(v)
    return u, v, bu, bv, z_, ez


def warp_roi_f64(kind, scale, w, h, K, R):
    """detectResultRoi of the kind -> dict: candidate sets tl_x, tl_y, br_x, br_y (inclusive br) and `refused`: True (the library
    must return MIS_E_INVALID), False, or None (a plane corner's z_ sign within its band: either answer)."""
    scale = float(np.float32(scale))
    _, _, _, _, r_kinv = ri._mats(K, R)
    if kind == PLANE:
        bx = np.array([0.0, 0.0, w - 1.0, w - 1.0])
        by = np.array([0.0, h - 1.0, 0.0, h - 1.0])
    else:
        xs, ys = np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64)
        bx = np.concatenate([xs, xs, np.zeros(h), np.full(h, w - 1.0)])
        by = np.concatenate([np.zeros(w), np.full(w, h - 1.0), ys, ys])
    u, v, bu, bv, z_, ez = forward_f64(kind, r_kinv, scale, bx, by)
    if kind == PLANE and (np.abs(z_) <= ez).any():
        return {"refused": None}
    if (kind == PLANE and (z_ <= 0).any()) or not (np.isfinite(u).all() and np.isfinite(v).all()):
        return {"refused": True}
    out = {"refused": False}
    ivl = {"tl_x": ((u - bu).min(), (u + bu).min()), "br_x": ((u - bu).max(), (u + bu).max()),
           "tl_y": ((v - bv).min(), (v + bv).min()), "br_y": ((v - bv).max(), (v + bv).max())}
    out.update({k: set(range(int(math.trunc(lo)), int(math.trunc(hi)) + 1)) for k, (lo, hi) in ivl.items()})
    out["intervals"] = ivl
    return out


def roi_matches(roi, ref):
    return not ref["refused"] and ri.roi_matches(roi, ref)


def backward_f64(kind, K, R, scale, roi):
    """{Cylindrical,Plane}Projector::mapBackward for every pixel (u, v) of roi = (x, y, width, height) in float64
    -> dict(x, y, dx, dy, z, zband) in refimpl.spherical_backward_f64's form (the cylinder maps z <= 0 to (-1, -1); the plane
    divides by any z)."""
    scale = float(np.float32(scale))
    _, _, _, m, _ = ri._mats(K, R)
    x0, y0, rw, rh = roi
    shape = (rh, rw)
    up = ((x0 + np.arange(rw, dtype=np.float64)) / scale)[None, :]
    vp = ((y0 + np.arange(rh, dtype=np.float64)) / scale)[:, None]
    e_u, e_v = U24 * np.abs(up), U24 * np.abs(vp)
    if kind == CYLINDRICAL:
        su, cu = np.sin(up), np.cos(up)
        r = [np.broadcast_to(su, shape), np.broadcast_to(vp, shape), np.broadcast_to(cu, shape)]
        dr = [np.broadcast_to(TRIG_ERR + np.abs(cu) * e_u, shape), np.broadcast_to(e_v, shape),
              np.broadcast_to(TRIG_ERR + np.abs(su) * e_u, shape)]
    else:
        r = [np.broadcast_to(up, shape), np.broadcast_to(vp, shape), np.ones(shape)]
        dr = [np.broadcast_to(e_u, shape), np.broadcast_to(e_v, shape), np.zeros(shape)]
    xx = sum(m[0, i] * r[i] for i in range(3))
    yy = sum(m[1, i] * r[i] for i in range(3))
    z = sum(m[2, i] * r[i] for i in range(3))
    az2 = sum(np.abs(m[2, i] * r[i]) for i in range(3))
    zband = sum(abs(m[2, i]) * dr[i] for i in range(3)) + 3 * U24 * az2
    live = z > 0 if kind == CYLINDRICAL else z != 0
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
    """The pixels whose z lies within its band of 0 (cylinder: sign test undecided; plane: near-zero z)."""
    return np.abs(maps["z"]) <= maps["zband"]


def map_forward_f64(kind, r_kinv, scale, x, y):
    u, v, _, _, _, _ = forward_f64(kind, r_kinv, scale, np.asarray(x, np.float64), np.asarray(y, np.float64))
    return u, v


def map_backward_exact_f64(kind, k_rinv, scale, u, v):
    """mapBackward without the z test, in float64 -> (x, y)."""
    u, v = np.asarray(u, np.float64) / scale, np.asarray(v, np.float64) / scale
    r = (np.sin(u), v, np.cos(u)) if kind == CYLINDRICAL else (u, v, np.ones_like(u))
    xx, yy, z = (sum(k_rinv[i, j] * r[j] for j in range(3)) for i in range(3))
    return xx / z, yy / z


# the kinds' own edge regimes on top of refimpl.WARP_GEOMS: a plane whose roi rectangle reaches behind the camera (the bounding
# box of a slanted trapezoid), and plane geometries that are refused (a corner turned past 90 degrees)
PLANE_GEOMS = [
    ("behind", 120.0, 50.0, 20.0, 60.0),
    ("yaw+175", 60.0, 175.0, 0.0, 0.0),
    ("yaw-175", 60.0, -175.0, 0.0, 0.0),
]
