"""Plain numpy references of the warpers' point, map and backward methods: warpPoint / warpPointBackward,
buildMaps and warpBackward.  Nothing here calls the product library or the oracle.

Two parts:
  * The exact integer cv::remap of a FLOAT32 map on u8 (remap_exact, nearest_mask): given the map the result has one value -- the
    INTER_BITS = 5 quantisation cvRound(32 x), Q15 weights 32 (32 - fy)(32 - fx) ..., rounding at bit 14, saturate_cast<short> of the
    integer part, BORDER_REFLECT folded as OpenCV's loop folds it, BORDER_CONSTANT(0) taps contributing 0 -- so a library result is
    compared byte for byte, without bands.
  * A per-kind dispatcher to the float64 map references with their first-order float32 error bands (refimpl, refimpl_warpers,
    refimpl_mercator, refimpl_polar_warpers, refimpl_compressed_warpers, refimpl_affine_family): forward_ref / backward_ref.  A
    point is `decided` where its reference says something: ok, bands finite and at most MAX_BAND.
"""
import numpy as np

import refimpl as ri
import refimpl_affine_family as ra
import refimpl_compressed_warpers as rc
import refimpl_mercator as rmc
import refimpl_polar_warpers as rp
import refimpl_warpers as rm
from refimpl import U24, INV_TRIG_ERR

SPHERICAL, CYLINDRICAL, PLANE, MERCATOR, FISHEYE, STEREOGRAPHIC = 0, 1, 2, 3, 4, 5
COMPRESSED_A2B1, COMPRESSED_A15B1, PANINI_A2B1, PANINI_A15B1, AFFINE = 8, 9, 10, 11, 13
KINDS = {"spherical": SPHERICAL, "cylindrical": CYLINDRICAL, "plane": PLANE, "mercator": MERCATOR, "fisheye": FISHEYE,
         "stereographic": STEREOGRAPHIC, "compressedA2B1": COMPRESSED_A2B1, "compressedA1.5B1": COMPRESSED_A15B1,
         "paniniA2B1": PANINI_A2B1, "paniniA1.5B1": PANINI_A15B1, "affine": AFFINE}
INTER_NEAREST, INTER_LINEAR = 0, 1
BORDER_CONSTANT, BORDER_REFLECT = 0, 2
PAIRS = [(INTER_LINEAR, BORDER_REFLECT), (INTER_NEAREST, BORDER_CONSTANT), (INTER_LINEAR, BORDER_CONSTANT)]
MAX_BAND = 1.0 / 64             # a wider band says nothing about a 1/32-pixel quantisation: the point is left out
MAX_UNDECIDED_SHARE = 0.02      # of the points of one (kind, geometry)


# ------------------------------------------------------------------------------------------------ exact remap of a float32 map
def _sample_q(s3, xq, yq, linear, reflect):
    """remap of the quantised coordinates (int64 arrays): linear: xq = cvRound(32 x); nearest: xq = cvRound(x) -> (H, W, cn) uint8."""
    h, w = s3.shape[:2]
    if not linear:
        sx, sy = ri.sat_short(xq), ri.sat_short(yq)
        inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        v = s3[np.where(inside, sy, 0), np.where(inside, sx, 0)]
        return np.where(inside[..., None], v, 0).astype(np.uint8)
    fx, fy = xq & 31, yq & 31
    sx, sy = ri.sat_short(xq >> 5), ri.sat_short(yq >> 5)
    wts = [(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32]
    taps = [(sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1)]
    acc = np.zeros(xq.shape + (s3.shape[2],), np.int64)
    for wt, (ty, tx) in zip(wts, taps):
        if reflect:
            acc += s3[ri.reflect_array(ty, h), ri.reflect_array(tx, w)].astype(np.int64) * wt[..., None]
        else:
            inside = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
            v = s3[np.where(inside, ty, 0), np.where(inside, tx, 0)].astype(np.int64)
            acc += np.where(inside[..., None], v, 0) * wt[..., None]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def _mode(interp, border):
    assert (interp, border) in PAIRS, (interp, border)
    return interp == INTER_LINEAR, border == BORDER_REFLECT


def remap_exact(src, xmap, ymap, interp, border):
    """cv::remap(src u8, xmap, ymap float32, interp, border) for the three pairs -> uint8 of the maps' shape (x channels)."""
    linear, reflect = _mode(interp, border)
    src = np.asarray(src)
    s3 = src.reshape(src.shape[0], src.shape[1], -1)
    x, y = np.asarray(xmap, np.float32), np.asarray(ymap, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        q = np.float32(32.0) if linear else np.float32(1.0)
        xq, yq = ri.cv_round((x * q).astype(np.float64)), ri.cv_round((y * q).astype(np.float64))
    out = _sample_q(s3, xq, yq, linear, reflect)
    return out[..., 0] if src.ndim == 2 else out


def nearest_mask(src_shape, xmap, ymap):
    """warpBackward of an all-255 mask with (NEAREST, CONSTANT): 255 where the nearest source pixel lies inside."""
    return remap_exact(np.full(src_shape[:2], 255, np.uint8), xmap, ymap, INTER_NEAREST, BORDER_CONSTANT)


def back_maps_f32(uv, src_tl, shape):
    """warpBackward's maps from the float32 forward points uv (n, 2) of the view's pixels, row-major: xmap = u - tl.x, ymap = v -
    tl.y, both subtractions in float32 -> (xmap, ymap) of `shape` = (h, w)."""
    uv = np.asarray(uv, np.float32).reshape(shape[0], shape[1], 2)
    with np.errstate(invalid="ignore", over="ignore"):
        return uv[..., 0] - np.float32(src_tl[0]), uv[..., 1] - np.float32(src_tl[1])


def view_points(w, h):
    """The pixel coordinates of a w x h view, row-major -> (w h, 2) float32."""
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return np.stack([x.ravel(), y.ravel()], 1)


# ------------------------------------------------------------------------------------------------ float64 references per kind
def forward_ref(kind, K, R, scale, x, y):
    """mapForward of `kind` in float64 at the points (x, y) -> (u, v, band_u, band_v, ok); R is H for the affine kind."""
    scale = float(np.float32(scale))
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if kind == AFFINE:
        u, v, bu, bv, z_, ez = ra.forward_f64(K, R, scale, x, y)
        ok = np.abs(z_) > ez
    else:
        _, _, _, _, r_kinv = ri._mats(K, R)
        if kind == SPHERICAL:
            u, v, th, ph = ri._forward(r_kinv, scale, x, y)
            (_, _, _), (sx, sy, sz) = rm._row_terms(r_kinv, x, y)
            xyz = r_kinv @ np.stack([x, y, np.ones_like(x)])
            with np.errstate(divide="ignore", invalid="ignore"):
                # the r_kinv products' roundings through the angles: atan2 over rho, acos over the ray's length (first order)
                e_in = 3 * U24 * (sx + sy + sz) / np.sqrt(xyz[0] ** 2 + xyz[2] ** 2)
            bu = scale * (INV_TRIG_ERR + 8 * U24 * (1 + th) + e_in) + U24 * np.abs(u)
            bv = scale * (INV_TRIG_ERR + 8 * U24 * (1 + ph) + e_in) + U24 * np.abs(v)
            ok = np.isfinite(u) & np.isfinite(v)
        elif kind in (CYLINDRICAL, PLANE):
            u, v, bu, bv, z_, ez = rm.forward_f64(kind, r_kinv, scale, x, y)
            ok = (np.abs(z_) > ez) if kind == PLANE else np.ones(u.shape, bool)
        elif kind == MERCATOR:
            u, v, bu, bv, rel = rmc.forward_f64(r_kinv, scale, x, y)
            ok = rel <= rmc.TAN_REL_LIMIT
        elif kind in (FISHEYE, STEREOGRAPHIC):
            u, v, bu, bv, ok = rp.forward_f64(kind, r_kinv, scale, x, y)
        else:
            u, v, (ulo, uhi), (vlo, vhi), ok = rc.forward_f64(kind, r_kinv, scale, x, y)
            with np.errstate(invalid="ignore"):
                bu, bv = np.maximum(uhi - u, u - ulo), np.maximum(vhi - v, v - vlo)
        if kind not in (PLANE, FISHEYE, STEREOGRAPHIC):
            # u = scale f(atan2(x_, z_)) jumps by 2 pi scale across the cut z_ < 0, x_ = 0 (the +-180 degree seam): where the float32
            # rounding of x_ (the references' 3 * 2^-24 of its terms) decides its sign, either side is a legitimate answer and the
            # first-order band says nothing.  (The polar kinds take sin and cos of the angle, which are continuous across the cut.)
            (x_, _, z_), (sx, _, _) = rm._row_terms(r_kinv, x, y)
            ok = ok & ~((z_ < 0) & (np.abs(x_) <= 3 * U24 * sx))
    ok = ok & np.isfinite(u) & np.isfinite(v) & np.isfinite(bu) & np.isfinite(bv)
    return u, v, bu, bv, ok


def backward_ref(kind, K, R, scale, roi):
    """mapBackward of `kind` in float64 at every integer pixel of roi = (x, y, width, height) -> dict(x, y, dx, dy, z, zband)."""
    if kind == SPHERICAL:
        return ri.spherical_backward_f64(K, R, scale, roi)
    if kind in (CYLINDRICAL, PLANE):
        return rm.backward_f64(kind, K, R, scale, roi)
    if kind == MERCATOR:
        return rmc.backward_f64(K, R, scale, roi)
    if kind in (FISHEYE, STEREOGRAPHIC):
        return rp.backward_f64(kind, K, R, scale, roi)
    if kind == AFFINE:
        return ra.backward_f64(K, R, scale, roi)
    return rc.backward_f64(kind, K, R, scale, roi)


def decided_forward(bu, bv, ok):
    with np.errstate(invalid="ignore"):
        return ok & (bu <= MAX_BAND) & (bv <= MAX_BAND)


def decided_backward(maps):
    """The roi pixels whose backward reference says something: the sign of z decided, the bands finite and at most MAX_BAND."""
    with np.errstate(invalid="ignore"):
        zu = np.abs(maps["z"]) <= maps["zband"]
        return ~zu & np.isfinite(maps["x"]) & np.isfinite(maps["y"]) & (maps["dx"] <= MAX_BAND) & (maps["dy"] <= MAX_BAND)


def back_candidates(src, u, v, bu, bv, ok, src_tl, interp, border):
    """The float64 candidate check of warpBackward: the remap results of the quantisations within the band of the float64 map
    x = u - tl.x, y = v - tl.y (its float32 subtraction adds U24 |x|) -> (cands (4, H, W[, cn]), in_band, undecided), in the form
    refimpl.check_candidates takes.  u, v, bu, bv, ok: forward_ref's, shaped (H, W)."""
    linear, reflect = _mode(interp, border)
    src = np.asarray(src)
    s3 = src.reshape(src.shape[0], src.shape[1], -1)
    x, y = u - float(src_tl[0]), v - float(src_tl[1])
    with np.errstate(invalid="ignore"):
        dx, dy = bu + U24 * (np.abs(u) + np.abs(x)), bv + U24 * (np.abs(v) + np.abs(y))
        dec = decided_forward(dx, dy, ok)
    q = 32.0 if linear else 1.0
    z0 = np.zeros(x.shape, bool)
    xs, ys, dxs, dys = (np.where(dec, a, 0.0) for a in (x, y, dx, dy))
    xl, xh, xd = ri._axis_candidates(xs, dxs, q, z0)
    yl, yh, yd = ri._axis_candidates(ys, dys, q, z0)
    und = ~(dec & xd & yd)
    outs = [_sample_q(s3, xq, yq, linear, reflect) for xq in (xl, xh) for yq in (yl, yh)]
    cands = np.stack(outs)
    if src.ndim == 2:
        cands = cands[..., 0]
    return cands, ((xl != xh) | (yl != yh)) & ~und, und
