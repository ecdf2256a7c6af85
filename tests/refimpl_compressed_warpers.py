"""Plain numpy reference of the compressed-rectilinear and Panini warps, written from OpenCV's documented semantics (warpers_inl.hpp:
CompressedRectilinearProjector(a, b), PaniniProjector(a, b); cv::CompressedRectilinearWarper and cv::PaniniWarper are
RotationWarperBase without a detectResultRoi of their own, so the roi is the extreme of EVERY source pixel's forward projection,
std::min / std::max skipping NaN, static_cast<int> of the four floats, no fix-up).

    forward:   (x_, y_, z_) = r_kinv (x, y, 1),  u_ = atan2(x_, z_),  v_ = asin(y_ / |(x_, y_, z_)|)
               compressed:  u = scale a tan(u_ / a),  v = scale b tan(v_) / cos(u_)
               Panini:      tg = a tan(u_ / a),  u = scale tg,  S = sin(u_);
                            |S| < 1e-7: v = scale b tan(v_), else v = scale b tg tan(v_) / S
    backward:  u' = u / scale,  v' = v / scale,  lam = a atan(u' / a)
               compressed:  v_ = atan(v' cos(lam) / b)
               Panini:      |lam| > 1e-7: v_ = atan(v' sin(lam) / (b a tan(lam / a))), else v_ = atan(v' / b)
               ray = (sin(lam) cos(v_), sin(v_), cos(lam) cos(v_));  (x, y, z) = k_rinv ray;  z > 0: (x / z, y / z) else (-1, -1)

Nothing here calls the oracle or the product library.  The method is tests/refimpl.py's, whose remap candidate and check helpers
are reused: the maps are computed in float64 from the float32 K, R and scale the ABI receives, and per pixel the candidate
quantisations within a float32 error band of the float64 map are the legitimate outputs.

The tangent.  mis_tanf is used on both sides of its pole (a = 1.5: u_ / a reaches 120 degrees), where neither an absolute nor a
relative error is bounded.  Its error is therefore stated in the ARGUMENT: mis_tanf(x) = tan(x + d) with |d| <= TAN_ANGLE_ERR, which
is bounded everywhere (a relative error e of tan is the angle error e |sin x cos x| <= e / 2; at the pole it is the error of the
reduced argument).  TAN_ANGLE_ERR is twice the maximum of |atan(mis_tanf(x)) - x| (mod pi) measured against float64 over
|x| <= pi/2 (1 - 2^-20) and |x| <= 2 pi / 3 -- the arguments the maps can reach -- as refimpl_mercator's constants were obtained;
tests/test_refimpl_compressed_warpers_cpu.py pins it.  A tangent whose argument carries the error e is the INTERVAL
[tan(x - e - TAN_ANGLE_ERR), tan(x + e + TAN_ANGLE_ERR)], widened by its own rounding 2^-24 |t|; where a pole lies inside the
argument's interval the value is unknown (`ok` False).

Error model of the float32 backward map (stated once, not tuned to the tests); first order except where an interval is named:
  * u' = u / scale, v' = v / scale: one rounding each, relative 2^-24 (u, v are integers, exact in float32).
  * g = u' / a: e_g = 2 * 2^-24 |g|.  lam = a atan(g): e_lam = a (ATAN_ERR + e_g / (1 + g^2)) + 2^-24 |lam|.
  * sin(lam), cos(lam): d_sl = TRIG_ERR + |cos lam| e_lam,  d_cl = TRIG_ERR + |sin lam| e_lam.
  * compressed: q = v' cos(lam) / b: e_q = |v'| d_cl + 3 * 2^-24 |q| (v', the product, the division); q in [q - e_q, q + e_q].
  * Panini, |lam| > 1e-7: h = lam / a has e_h = e_lam / a + 2^-24 |h|; T = tan(h) is the interval above (|h| < pi / 2: no pole);
    the divisor D = b a T carries 2 * 2^-24 |D| more.  D vanishes with lam (so does the numerator), so the quotient is carried as
    an interval: N = v' sin(lam) in [N - e_N, N + e_N], e_N = |v'| d_sl + 2 * 2^-24 |N|; q in the hull of N / D over the corners,
    plus 2^-24 |q|, valid while the half-width of D is at most D_REL_LIMIT |D|.  Beyond it (|lam| below ~1e-6: |u| < 1e-6 scale,
    no integer column but 0 for any scale below 1e6) the pixel is undetermined.
    |lam| <= 1e-7: q = v' / b with 2 * 2^-24 |q|.  A pixel whose |lam| lies within e_lam of 1e-7 is undetermined (either branch).
    The column u = 0 has lam = 0 exactly on both sides and takes the second branch.
  * v_ = atan(q): e_v_ = ATAN_ERR + max |atan(q_lo) - atan q|, |atan(q_hi) - atan q|.
  * sin(v_), cos(v_): TRIG_ERR plus e_v_ through the derivatives; the ray r = (sin lam cos v_, sin v_, cos lam cos v_) with
    2^-24 |r_i| for the products of the first and third components.
  * x = (m0 . r) / (m2 . r) with m = K R^-1 in float32, as refimpl_warpers.backward_f64: the ray errors through
    dx/dr_i = (m0_i - x m2_i) / z, the dot products' 3 * 2^-24 (sum_i |m0_i r_i| + |x| sum_i |m2_i r_i|) / |z|, the division
    2^-24 |x|.  The same for y with row 1.  z <= 0 maps to (-1, -1): pixels whose z lies within its band of 0 are undecided.
    Undetermined pixels are reported through the same channel (their z band is infinite).
ROI extremes (forward map of every pixel): (x_, y_, z_) carry 3 * 2^-24 of their terms' magnitudes (e_x, e_y, e_z).
  * u_ = atan2(x_, z_): e_u_ = INV_TRIG_ERR + 8 * 2^-24 (1 + |u_|) + (e_x + e_z) / |(x_, z_)|, as the cylinder's.
  * w = y_ / |r| as refimpl_mercator: e_w = (c^2 e_y + |w| (|x_| e_x + |z_| e_z) / |r|) / |r| + 4 * 2^-24 |w|, c = |(x_, z_)| / |r|;
    v_ = asin w: e_v_ = ASIN_ERR + e_w / c.
  * tan(v_) and tan(u_ / a) (e_g = e_u_ / a + 2^-24 |u_ / a|): the intervals above.
  * compressed: u = scale a tan(u_ / a): the interval times scale a, plus 3 * 2^-24 |u|.  v = scale b tan(v_) / cos(u_): the divisor
    C = cos(u_) has e_C = TRIG_ERR + |sin u_| e_u_ and vanishes at u_ = +-90 degrees, so the quotient is the hull of the corners of
    [tan v_] / [C - e_C, C + e_C], valid while e_C <= D_REL_LIMIT |C|; times scale b, plus 4 * 2^-24 |v|.
  * Panini: u = scale tg likewise.  S = sin(u_) has e_S = TRIG_ERR + |cos u_| e_u_.  Away from u_ = 0 the second branch is certain:
    v = scale b [tg] [tan v_] / [S - e_S, S + e_S] (hull of the corners, valid while e_S <= D_REL_LIMIT |S|), plus 5 * 2^-24 |v|.
    Next to u_ = 0 -- |u_| + e_u_ <= SMALL_ANGLE = 2^-8, which every frame with a pixel on the axis x_ = 0 has -- the absolute
    TRIG_ERR says nothing about S (and the branch is unknown), but there both functions are relatively accurate by construction:
    for |x| <= 2^-8 the octant reduction of mis_sincosf / mis_tanf leaves x as it is (j = 0), and the value is p + x with
    |p| <= |x|^3 <= 2^-16 |x| (sine: the odd polynomial's cubic part; tangent: the same, or p = 0 below 1e-4), so it carries the
    final sum's rounding 2^-24, the rounding of p scaled by 2^-16, and a truncation error below x^2 * 2e-6 <= 2^-34 of the value:
    relative error at most SMALL_REL_ERR = 2 * 2^-24, stated with a factor 2 to spare (the CPU test measures the tangent's).
    Whatever the float u_f, |u_f| <= |u_| + e_u_, the second branch then multiplies tan(v_) by
    rho = a tan(u_f / a) / sin(u_f) = 1 + u_f^2 (1 / (3 a^2) + 1 / 6) + O(u_f^4), and the first by 1:
    v = scale b [tan v_] [1 - 2 SMALL_REL_ERR - 2^-23, 1 + 1.01 (|u_| + e_u_)^2 (1 / (3 a^2) + 1 / 6) + 2 SMALL_REL_ERR + 2^-23]
    (2^-23: the division u_f / a and the product by a), plus 5 * 2^-24 |v| -- one interval for both branches.
  * A pixel whose value is unknown (a pole inside a tangent's argument interval, a divisor beyond D_REL_LIMIT, an unknown branch, a
    NaN) makes the roi undecided (`refused` None: either answer, any roi).
  * A refusal (`refused` True; the library returns MIS_E_INVALID where OpenCV would cast to int a float the int cannot hold): some
    pixel's whole interval of u or v lies at or beyond 2^31 in magnitude.  An interval that only reaches it: undecided.

U24, TRIG_ERR, INV_TRIG_ERR and PI_F32_ERR are refimpl's, ASIN_ERR and ATAN_ERR refimpl_mercator's; TAN_ANGLE_ERR is new (above).
"""
import math

import numpy as np

import refimpl as ri
import refimpl_mercator as rm
from refimpl import U24, TRIG_ERR, INV_TRIG_ERR, PI_F32_ERR  # noqa: F401  (PI_F32_ERR: no float32 pi enters these maps)
from refimpl_mercator import ASIN_ERR, ATAN_ERR

COMPRESSED_A2B1, COMPRESSED_A15B1, PANINI_A2B1, PANINI_A15B1 = 8, 9, 10, 11
KINDS = {"compressedPlaneA2B1": COMPRESSED_A2B1, "compressedPlaneA1.5B1": COMPRESSED_A15B1, "paniniA2B1": PANINI_A2B1, "paniniA1.5B1": PANINI_A15B1}
AB = {COMPRESSED_A2B1: (2.0, 1.0), COMPRESSED_A15B1: (1.5, 1.0), PANINI_A2B1: (2.0, 1.0), PANINI_A15B1: (1.5, 1.0)}
TAN_ANGLE_ERR = 2 * 8.3e-8      # mis_tanf as an error of its argument; measured maximum 8.22e-8
D_REL_LIMIT = 0.5               # half-width / |divisor| beyond this: the quotient's interval says nothing
SMALL_ANGLE = 2.0 ** -8          # |x| up to which mis_sinf / mis_tanf are relatively accurate by construction (the docstring)
SMALL_REL_ERR = 2 * U24          # their relative error there
BRANCH = 1e-7                   # the Panini projector's threshold on |sin u_| (forward) and |lam| (backward)
INT_LIMIT = 2147483520.0        # the largest float32 below 2^31 (roi_from_extremes refuses what lies beyond)


def is_panini(kind):
    return kind >= PANINI_A2B1


def tan_interval(x, e):
    """tan of an argument known to +-e, as mis_tanf evaluates it -> (lo, hi, ok); ok False where a pole lies inside."""
    w = e + TAN_ANGLE_ERR
    with np.errstate(invalid="ignore", over="ignore"):
        ok = np.isfinite(x) & np.isfinite(w) & (np.floor((x - w) / math.pi + 0.5) == np.floor((x + w) / math.pi + 0.5))
        xs, ws = np.where(ok, x, 0.0), np.where(ok, w, 0.0)
        lo, hi = np.tan(xs - ws), np.tan(xs + ws)
    pad = U24 * np.maximum(np.abs(lo), np.abs(hi))
    return lo - pad, hi + pad, ok


def _hull(*vals):
    return np.minimum.reduce(vals), np.maximum.reduce(vals)


def _mul_interval(alo, ahi, blo, bhi):
    return _hull(alo * blo, alo * bhi, ahi * blo, ahi * bhi)


def _div_interval(nlo, nhi, d, e_d):
    """[nlo, nhi] / [d - e_d, d + e_d] -> (lo, hi, ok): ok while e_d <= D_REL_LIMIT |d| (the divisor keeps its sign)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.isfinite(d) & (e_d <= D_REL_LIMIT * np.abs(d)) & (d != 0)
        ds, es = np.where(ok, d, 1.0), np.where(ok, e_d, 0.0)
        lo, hi = _hull(nlo / (ds - es), nlo / (ds + es), nhi / (ds - es), nhi / (ds + es))
    return lo, hi, ok


def forward_f64(kind, r_kinv, scale, x, y):
    """mapForward in float64 with its float32 intervals -> (u, v, (u_lo, u_hi), (v_lo, v_hi), ok): ok False where the model says
    nothing about the pixel."""
    a, b = AB[kind]
    (x_, y_, z_), (sx, sy, sz) = rm._row_terms(r_kinv, x, y)
    ex, ey, ez = 3 * U24 * sx, 3 * U24 * sy, 3 * U24 * sz
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rho = np.sqrt(x_ * x_ + z_ * z_)
        n = np.sqrt(x_ * x_ + y_ * y_ + z_ * z_)
        u_ = np.arctan2(x_, z_)
        e_u_ = INV_TRIG_ERR + 8 * U24 * (1 + np.abs(u_)) + (ex + ez) / rho
        w = np.clip(y_ / n, -1.0, 1.0)
        c = rho / n
        e_w = (c * c * ey + np.abs(w) * (np.abs(x_) * ex + np.abs(z_) * ez) / n) / n + 4 * U24 * np.abs(w)
        v_ = np.arcsin(w)
        e_v_ = ASIN_ERR + e_w / c
        g = u_ / a
        tg_lo, tg_hi, ok_g = tan_interval(g, e_u_ / a + U24 * np.abs(g))
        tv_lo, tv_hi, ok_v = tan_interval(v_, e_v_)
        ok = ok_g & ok_v
        u = scale * a * np.tan(g)
        u_lo, u_hi = _hull(scale * a * tg_lo, scale * a * tg_hi)
        pad = 3 * U24 * np.maximum(np.abs(u_lo), np.abs(u_hi))
        u_lo, u_hi = u_lo - pad, u_hi + pad
        if not is_panini(kind):
            C = np.cos(u_)
            q_lo, q_hi, ok_q = _div_interval(tv_lo, tv_hi, C, TRIG_ERR + np.abs(np.sin(u_)) * e_u_)
            v = scale * b * np.tan(v_) / C
            v_lo, v_hi = scale * b * q_lo, scale * b * q_hi
            pad = 4 * U24 * np.maximum(np.abs(v_lo), np.abs(v_hi))
            ok = ok & ok_q
        else:
            S = np.sin(u_)
            e_S = TRIG_ERR + np.abs(np.cos(u_)) * e_u_
            ub = np.abs(u_) + e_u_
            small = ub <= SMALL_ANGLE           # next to u_ = 0: either branch, one interval
            large = ~small
            p_lo, p_hi = _mul_interval(a * tg_lo, a * tg_hi, tv_lo, tv_hi)
            q_lo, q_hi, ok_q = _div_interval(p_lo, p_hi, S, e_S)
            rho_lo = 1.0 - 2 * SMALL_REL_ERR - 2 * U24
            rho_hi = 1.0 + 1.01 * ub * ub * (1.0 / (3 * a * a) + 1.0 / 6) + 2 * SMALL_REL_ERR + 2 * U24
            s_lo, s_hi = _mul_interval(tv_lo, tv_hi, rho_lo, np.where(small, rho_hi, 1.0))
            v = np.where(np.abs(S) < BRANCH, scale * b * np.tan(v_), scale * b * a * np.tan(g) * np.tan(v_) / np.where(S == 0, 1.0, S))
            v_lo = np.where(small, scale * b * s_lo, scale * b * q_lo)
            v_hi = np.where(small, scale * b * s_hi, scale * b * q_hi)
            pad = 5 * U24 * np.maximum(np.abs(v_lo), np.abs(v_hi))
            ok = ok & (small | (large & ok_q))
        v_lo, v_hi = v_lo - pad, v_hi + pad
        ok = ok & np.isfinite(u_) & ~np.isnan(u_lo) & ~np.isnan(u_hi) & ~np.isnan(v_lo) & ~np.isnan(v_hi)
    return u, v, (u_lo, u_hi), (v_lo, v_hi), ok


def warp_roi_f64(kind, scale, w, h, K, R):
    """RotationWarperBase::detectResultRoi (every pixel) -> dict: candidate sets tl_x, tl_y, br_x, br_y (inclusive br) and
    `refused`: True (the library must return MIS_E_INVALID), False, or None (either answer, any roi)."""
    scale = float(np.float32(scale))
    _, _, _, _, r_kinv = ri._mats(K, R)
    bx, by = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    _, _, (u_lo, u_hi), (v_lo, v_hi), ok = forward_f64(kind, r_kinv, scale, bx.ravel(), by.ravel())
    if not ok.all():
        return {"refused": None}
    # the magnitude an interval certainly has / may have
    sure = np.maximum(np.where(u_lo * u_hi > 0, np.minimum(np.abs(u_lo), np.abs(u_hi)), 0.0), np.where(v_lo * v_hi > 0, np.minimum(np.abs(v_lo), np.abs(v_hi)), 0.0))
    may = np.maximum(np.maximum(np.abs(u_lo), np.abs(u_hi)), np.maximum(np.abs(v_lo), np.abs(v_hi)))
    if (sure >= INT_LIMIT).any():
        return {"refused": True}
    if (may >= INT_LIMIT).any():
        return {"refused": None}
    out = {"refused": False}
    ivl = {"tl_x": (u_lo.min(), u_hi.min()), "br_x": (u_lo.max(), u_hi.max()), "tl_y": (v_lo.min(), v_hi.min()), "br_y": (v_lo.max(), v_hi.max())}
    out.update({k: set(range(int(math.trunc(lo)), int(math.trunc(hi)) + 1)) if hi - lo < 1e6 else _Range(int(math.trunc(lo)), int(math.trunc(hi)))
                for k, (lo, hi) in ivl.items()})
    out["intervals"] = ivl
    return out


class _Range:
    """A candidate set too wide to enumerate (a bound next to a vanishing divisor): lo .. hi inclusive."""

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


def _backward_angles(kind, scale, up, vp):
    """-> (lam, e_lam, v_, e_v_, undetermined) for u' = up (a row vector), v' = vp (a column vector)."""
    a, b = AB[kind]
    g = up / a
    lam = a * np.arctan(g)
    e_lam = a * (ATAN_ERR + 2 * U24 * np.abs(g) / (1 + g * g)) + U24 * np.abs(lam)
    e_lam = np.where(up == 0, 0.0, e_lam)       # mis_atanf(0) = 0 exactly: the column u = 0 has lam = 0 on both sides
    sl, cl = np.sin(lam), np.cos(lam)
    d_sl, d_cl = TRIG_ERR + np.abs(cl) * e_lam, TRIG_ERR + np.abs(sl) * e_lam
    if not is_panini(kind):
        q = vp * cl / b
        e_q = np.abs(vp) * d_cl + 3 * U24 * np.abs(q)
        q_lo, q_hi = q - e_q, q + e_q
        und = np.zeros(q.shape, bool)
    else:
        hh = lam / a
        t_lo, t_hi, ok_t = tan_interval(hh, e_lam / a + U24 * np.abs(hh))
        D = b * a * np.tan(hh)
        d_lo, d_hi = _hull(b * a * t_lo, b * a * t_hi)
        e_D = np.maximum(D - d_lo, d_hi - D) + 2 * U24 * np.abs(D)
        N = vp * sl
        e_N = np.abs(vp) * d_sl + 2 * U24 * np.abs(N)
        shape = np.broadcast(N, D).shape
        ql, qh, ok_q = _div_interval(np.broadcast_to(N - e_N, shape), np.broadcast_to(N + e_N, shape), np.broadcast_to(D, shape), np.broadcast_to(e_D, shape))
        small = np.broadcast_to(np.abs(lam) + e_lam <= BRANCH, shape)
        large = np.broadcast_to((np.abs(lam) - e_lam > BRANCH) & ok_t, shape) & ok_q
        q1 = np.broadcast_to(vp / b, shape)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(small, q1, np.broadcast_to(N, shape) / np.where(np.broadcast_to(D, shape) == 0, 1.0, np.broadcast_to(D, shape)))
        q_lo = np.where(small, q1 - 2 * U24 * np.abs(q1), ql - U24 * np.maximum(np.abs(ql), np.abs(qh)))
        q_hi = np.where(small, q1 + 2 * U24 * np.abs(q1), qh + U24 * np.maximum(np.abs(ql), np.abs(qh)))
        und = ~(small | large)
        q, q_lo, q_hi = (np.where(und, 0.0, t) for t in (q, q_lo, q_hi))
    v_ = np.arctan(q)
    e_v_ = ATAN_ERR + np.maximum(np.abs(np.arctan(q_lo) - v_), np.abs(np.arctan(q_hi) - v_))
    return lam, e_lam, v_, e_v_, und


def backward_f64(kind, K, R, scale, roi):
    """mapBackward for every pixel (u, v) of roi = (x, y, width, height) in float64 -> dict(x, y, dx, dy, z, zband) in
    refimpl.spherical_backward_f64's form (z <= 0 maps to (-1, -1)); an undetermined pixel has an infinite zband."""
    scale = float(np.float32(scale))
    _, _, _, m, _ = ri._mats(K, R)
    x0, y0, rw, rh = roi
    shape = (rh, rw)
    up = ((x0 + np.arange(rw, dtype=np.float64)) / scale)[None, :]
    vp = ((y0 + np.arange(rh, dtype=np.float64)) / scale)[:, None]
    lam, e_lam, v_, e_v_, und = _backward_angles(kind, scale, up, vp)
    sl, cl, sv, cv = np.sin(lam), np.cos(lam), np.sin(v_), np.cos(v_)
    d_sl, d_cl = TRIG_ERR + np.abs(cl) * e_lam, TRIG_ERR + np.abs(sl) * e_lam
    d_sv, d_cv = TRIG_ERR + np.abs(cv) * e_v_, TRIG_ERR + np.abs(sv) * e_v_
    r = [np.broadcast_to(c, shape) for c in (sl * cv, sv, cl * cv)]
    dr = [np.abs(sl) * d_cv + np.abs(cv) * d_sl + U24 * np.abs(r[0]), np.broadcast_to(d_sv, shape), np.abs(cl) * d_cv + np.abs(cv) * d_cl + U24 * np.abs(r[2])]
    xx = sum(m[0, i] * r[i] for i in range(3))
    yy = sum(m[1, i] * r[i] for i in range(3))
    z = sum(m[2, i] * r[i] for i in range(3))
    az2 = sum(np.abs(m[2, i] * r[i]) for i in range(3))
    zband = sum(abs(m[2, i]) * dr[i] for i in range(3)) + 3 * U24 * az2
    zband = np.where(np.broadcast_to(und, shape), np.inf, zband)
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
    a, b = AB[kind]
    u, v = np.asarray(u, np.float64) / scale, np.asarray(v, np.float64) / scale
    lam = a * np.arctan(u / a)
    if is_panini(kind):
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(np.abs(lam) > BRANCH, v * np.sin(lam) / (b * a * np.tan(lam / a)), v / b)
    else:
        q = v * np.cos(lam) / b
    v_ = np.arctan(q)
    return np.sin(lam) * np.cos(v_), np.sin(v_), np.cos(lam) * np.cos(v_)


def map_backward_exact_f64(kind, k_rinv, scale, u, v):
    """mapBackward without the z test, in float64 -> (x, y)."""
    r = ray_backward_f64(kind, scale, u, v)
    xx, yy, z = (sum(k_rinv[i, j] * r[j] for j in range(3)) for i in range(3))
    return xx / z, yy / z


# The cases: the sources the issue names over refimpl.WARP_GEOMS and refimpl_warpers.PLANE_GEOMS (frames turned past 90 degrees: the
# compressed map's divisor cos(u_) changes sign inside them).
MAX_REF_PIXELS = 300_000        # rois past this are checked for their bounds only (tan(u_ / a) stretches the wide geometries)
SOURCES = [(2, 2, 1.0), (5, 7, 1.0), (5, 7, 20.0), (65, 9, 1.0), (65, 9, 0.37), (333, 217, 1.0), (333, 217, 0.37)]


def sources():
    return list(SOURCES)


def geometry_cases(w, h, mult):
    """-> [(name, K, R, scale)] over refimpl.WARP_GEOMS and refimpl_warpers.PLANE_GEOMS for one source."""
    import refimpl_warpers as rw
    return [(name,) + ri.camera(w, h, hfov, yaw, pitch, roll, mult, seam=mult < 1) for name, hfov, yaw, pitch, roll in ri.WARP_GEOMS + rw.PLANE_GEOMS]


# The smallest shapes at which the tile code can go wrong, as `known` rois: widths 1, 3, 4, 5 (a lane's 4 columns), 127, 128, 129 (the
# tile's 128), 257; heights 1, T - 1, T, T + 1, 2 T + 1 of the fused tile (T = 32 rows, warp.hip's PC_TH) and 15, 16, 17 of the general
# tile.  Each straddles u = 0 where it is wider than one pixel.
T = 32
EDGE_SHAPES = [(1, 1), (3, T - 1), (4, T), (5, T + 1), (127, 2 * T + 1), (128, 1), (129, T - 1), (257, T), (1, T + 1), (3, 2 * T + 1), (128, T), (129, T + 1),
               (257, 1), (4, 2 * T + 1), (127, 15), (128, 16), (129, 17), (5, 2)]


def edge_shape_setup(kind):
    """A 65 x 9 seam-scale camera, its content and the rois of EDGE_SHAPES -> (K, R, scale, img, rois)."""
    w, h = 65, 9
    K, R, scale = ri.camera(w, h, 60.0, 4.0, 3.0, 6.0, 0.37, seam=True)
    img = ri.content("rand", (h, w, 3), seed=91 + kind)
    return K, R, scale, img, [(-(sw // 2), -(sh // 3), sw, sh) for sw, sh in EDGE_SHAPES]


# the cameras of the GPU tests' larger frames: (w, h, [(hfov, yaw, pitch, roll)])
FRAMES_4K = (3840, 2160, [(60.0, 5.0, 2.0, 0.0), (60.0, 10.0, 5.0, 30.0)])
FRAMES_720P = (1280, 720, [(60.0, -25.0, 2.0, 0.0), (60.0, 3.0, -4.0, 3.0), (60.0, 25.0, 10.0, -5.0)])


# (kind, w, h, multiplier, geometry) whose WARP is left out (the roi is still checked), each with its reason; filled from the conditions
# tests/test_refimpl_compressed_warpers_cpu.py::test_reference_conditions_hold_for_every_warped_case states on the reference alone
# A compressed-plane camera that is not rotated maps row v to y = v + h / 2 (scale = f: f tan(v_) / cos(lam) = f v' cos(lam) / cos(lam)),
# so on a source of odd height every row is a rounding tie of the INTER_NEAREST quantisation up to float32 rounding: the in-band share
# of the mask exceeds 0.40 (0.44 .. 0.52).
_TIE = "an unrotated camera on an odd-height source: y = v + h / 2, every row a rounding tie of the nearest quantisation"
WARP_DROPPED = {(kind, w, h, 1.0, name): _TIE for kind in (COMPRESSED_A2B1, COMPRESSED_A15B1) for w, h in ((65, 9), (333, 217))
                for name in ("front", "hfov90")}
