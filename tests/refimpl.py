"""Plain numpy references of the spherical warp and of the 2-NN matchers, written from OpenCV's documented semantics.

Nothing here calls the oracle (oracle/mo_*.c) or the product library: the two are checked against these functions, so a
misreading of OpenCV that the kernels and the oracle share shows up as a disagreement with this module.

Warp (cv::detail::SphericalWarper + cv::remap): the maps are computed in float64 from the float32 K, R and scale the ABI
receives.  The kernels compute them in float32, so near a rounding boundary of 32 x (INTER_LINEAR) or x (INTER_NEAREST) either
neighbouring cell is legitimate.  The reference therefore returns, per pixel, the candidate quantisations that lie within the
band delta(x, y) of the float64 value (at most 2 per axis, 4 per pixel) and the output values they give.

Error model of the float32 map (the band delta; stated once, not tuned to the tests), first order in every error:
  * angles theta = u / scale and phi = pi - v / scale: float32 roundings of the quotient and the difference plus the float32
    pi:  e_theta = 2^-24 |theta|,  e_phi = 2^-24 (|v / scale| + |phi|) + 8.8e-8.
  * sin / cos: the 3e-7 absolute error pinned by test_dev_math_cpu.py (the library's own functions) per evaluation, so the unit ray
    r = (sin phi sin theta, cos phi, sin phi cos theta) has component errors 3e-7 (|sin phi| + |sin theta|), 3e-7,
    3e-7 (|sin phi| + |cos theta|), plus 2^-24 |r_i| for the product, plus the angle errors through dr/dtheta, dr/dphi.
  * x = (m0 . r) / (m2 . r), m = K R^-1 rounded to float32: the ray errors propagate through the exact derivative
    dx/dr_i = (m0_i - x m2_i) / z; the dot products (entry, product and two sums rounded) add
    3 * 2^-24 (sum_i |m0_i r_i| + |x| sum_i |m2_i r_i|) / z, and the division 2^-24 |x|.  The same for y with row 1.
  Where z is within its own band of 0 the sign test `z > 0` is undecided and the pixel is left unconstrained (reported
  separately, as are pixels whose band spans more than two cells).  delta stays below 2^-8 px wherever the map lands on the
  source, except on the 4K frame at scale = f (5.3e-3 px at its corners: the 3e-7 trig error times f = 3325 alone is 1e-3).
ROI (detectResultRoi) extremes of the forward map u = scale atan2(x_, z_), v = scale (pi - acos(y_ / |r|)): the atan2 / acos
polynomials are pinned to 1e-6 there, so a bound is ambiguous where the float64 extreme lies within
scale (1e-6 + 8 * 2^-24 (1 + |angle|)) of an integer.

2-NN: exact integer distances; ties go to the smaller train index (cv::BFMatcher's stable order).
"""
import math

import numpy as np

U24 = 2.0 ** -24
TRIG_ERR = 3e-7          # test_dev_math_cpu.py::test_trig_err_is_tied_to_the_library (the library's mis_sinf / mis_cosf)
INV_TRIG_ERR = 1e-6      # test_dev_math_cpu.py::test_inv_trig_err_is_tied_to_the_library (mis_acosf, mis_atan2f)
PI_F32_ERR = 8.8e-8      # |pi - float32(pi)|
PI_F32 = float(np.float32(math.pi))

INTER_NEAREST, INTER_LINEAR = 0, 1
BORDER_CONSTANT, BORDER_REFLECT = 0, 2


# ------------------------------------------------------------------------------------------------ warp
def _mats(K, R):
    K = np.asarray(K, np.float32).astype(np.float64).reshape(3, 3)
    R = np.asarray(R, np.float32).astype(np.float64).reshape(3, 3)
    rinv = R.T                        # ProjectorBase::setCameraParams: Rinv = R.t()
    return K, R, rinv, K @ rinv, R @ np.linalg.inv(K)


def _forward(r_kinv, scale, x, y):
    """SphericalProjector::mapForward in float64 -> (u, v, |theta|, |phi|)."""
    xyz = r_kinv @ np.stack([x, y, np.ones_like(x)])
    x_, y_, z_ = xyz
    th = np.arctan2(x_, z_)
    w = y_ / np.sqrt(x_ * x_ + y_ * y_ + z_ * z_)
    w = np.where(np.isnan(w), 0.0, w)
    ph = np.arccos(np.clip(w, -1.0, 1.0))
    return scale * th, scale * (math.pi - ph), np.abs(th), np.abs(ph)


def _trunc_candidates(val, band):
    """int(float) truncates toward zero; the set of truncations of values within `band` of `val`."""
    return sorted({int(math.trunc(val - band)), int(math.trunc(val)), int(math.trunc(val + band))})


def warp_roi_f64(scale, w, h, K, R):
    """SphericalWarper::detectResultRoi -> dict of candidate sets for tl_x, tl_y, br_x, br_y (inclusive br), and the float64
    extremes.  A bound has two candidates only where the float64 extreme lies within the band of an integer."""
    scale = float(np.float32(scale))
    K, R, rinv, k_rinv, r_kinv = _mats(K, R)
    xs = np.arange(w, dtype=np.float64)
    ys = np.arange(h, dtype=np.float64)
    bx = np.concatenate([xs, xs, np.zeros(h), np.full(h, w - 1.0)])
    by = np.concatenate([np.zeros(w), np.full(w, h - 1.0), ys, ys])
    u, v, th, ph = _forward(r_kinv, scale, bx, by)
    bu = scale * (INV_TRIG_ERR + 8 * U24 * (1 + th)) + U24 * np.abs(u)
    bv = scale * (INV_TRIG_ERR + 8 * U24 * (1 + ph)) + U24 * np.abs(v)
    # the float32 extreme is one of the border values, each within its band of the float64 value: the minimum lies in
    # [min(u - b), min(u + b)], the maximum in [max(u - b), max(u + b)]
    ivl = {"tl_x": ((u - bu).min(), (u + bu).min()), "br_x": ((u - bu).max(), (u + bu).max()),
           "tl_y": ((v - bv).min(), (v + bv).min()), "br_y": ((v - bv).max(), (v + bv).max())}
    cand = {k: set(range(int(math.trunc(lo)), int(math.trunc(hi)) + 1)) for k, (lo, hi) in ivl.items()}
    # the two pole tests of the spherical override, with OpenCV's expressions (the second keeps x and z of the first); a test
    # whose image point lies within a small band of the source border may go either way
    pole_band = 1e-3
    for sign, pv in ((1.0, math.pi * scale), (-1.0, 0.0)):
        px, py, pz = rinv[0, 1], sign * rinv[1, 1], rinv[2, 1]
        if not py > 0:
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            x_ = (K[0, 0] * px + K[0, 1] * py) / pz + K[0, 2]
            y_ = K[1, 1] * py / pz + K[1, 2]
        inside = 0 < x_ < w and 0 < y_ < h
        edge = min(abs(x_), abs(x_ - w), abs(y_), abs(y_ - h)) <= pole_band
        if not (inside or edge):
            continue
        pvs = _trunc_candidates(pv, U24 * pv)     # float32(pi * scale)
        with_pole = {"tl_x": {min(t, 0) for t in cand["tl_x"]}, "br_x": {max(t, 0) for t in cand["br_x"]},
                     "tl_y": {min(t, p) for t in cand["tl_y"] for p in pvs},
                     "br_y": {max(t, p) for t in cand["br_y"] for p in pvs}}
        cand = with_pole if not edge else {k: cand[k] | with_pole[k] for k in cand}
    cand["intervals"] = ivl
    return cand


def roi_matches(roi, ref):
    """roi (x, y, width, height) against warp_roi_f64's candidate sets."""
    x, y, rw, rh = roi
    return x in ref["tl_x"] and y in ref["tl_y"] and x + rw - 1 in ref["br_x"] and y + rh - 1 in ref["br_y"]


def spherical_backward_f64(K, R, scale, roi):
    """SphericalProjector::mapBackward for every pixel (u, v) of roi = (x, y, width, height) in float64
    -> dict(x, y, dx, dy, z, zband): the map ((-1, -1) where z <= 0), its bands and z with the band of its sign test."""
    scale = float(np.float32(scale))
    _, _, _, m, _ = _mats(K, R)
    x0, y0, rw, rh = roi
    u = (x0 + np.arange(rw, dtype=np.float64))[None, :]
    v = (y0 + np.arange(rh, dtype=np.float64))[:, None]
    th = u / scale
    vs = v / scale
    ph = math.pi - vs
    sv, cv, su, cu = np.sin(ph), np.cos(ph), np.sin(th), np.cos(th)
    shape = (rh, rw)
    r = [np.broadcast_to(c, shape) for c in (sv * su, cv, sv * cu)]
    # first-order error of each ray component: sin / cos errors (TRIG_ERR each), the angles' roundings, the product's rounding
    e_th = U24 * np.abs(th)
    e_ph = U24 * (np.abs(vs) + np.abs(ph)) + PI_F32_ERR
    dr_trig = [TRIG_ERR * (np.abs(sv) + np.abs(su)), np.broadcast_to(TRIG_ERR, shape), TRIG_ERR * (np.abs(sv) + np.abs(cu))]
    dr_dth = [sv * cu, np.zeros(shape), -sv * su]
    dr_dph = [cv * su, np.broadcast_to(-sv, shape), cv * cu]
    xx = m[0, 0] * r[0] + m[0, 1] * r[1] + m[0, 2] * r[2]
    yy = m[1, 0] * r[0] + m[1, 1] * r[1] + m[1, 2] * r[2]
    z = m[2, 0] * r[0] + m[2, 1] * r[1] + m[2, 2] * r[2]
    az2 = sum(np.abs(m[2, i] * r[i]) for i in range(3))
    zband = sum(abs(m[2, i]) * (dr_trig[i] + np.abs(dr_dth[i]) * e_th + np.abs(dr_dph[i]) * e_ph + U24 * np.abs(r[i]))
                for i in range(3)) + 3 * U24 * az2
    pos = z > 0
    zs = np.where(pos, z, 1.0)
    x = np.where(pos, xx / zs, -1.0)
    y = np.where(pos, yy / zs, -1.0)
    out = {"x": x, "y": y, "z": z, "zband": zband}
    for name, row, val in (("dx", 0, x), ("dy", 1, y)):
        g = [(m[row, i] - val * m[2, i]) / zs for i in range(3)]        # d(value) / d(r_i)
        band = sum(np.abs(g[i]) * (dr_trig[i] + U24 * np.abs(r[i])) for i in range(3))
        band = band + np.abs(sum(g[i] * dr_dth[i] for i in range(3))) * e_th + np.abs(sum(g[i] * dr_dph[i] for i in range(3))) * e_ph
        terms = sum(np.abs(m[row, i] * r[i]) for i in range(3)) + np.abs(val) * az2
        band = band + 3 * U24 * terms / np.abs(zs) + U24 * np.abs(val)
        out[name] = np.where(pos, band, 0.0)
    return out


def reflect(p, n):
    """borderInterpolate(p, n, BORDER_REFLECT) as OpenCV's loop writes it: fedcba|abcdefgh|hgfedcb, folded as often as needed."""
    if n == 1:
        return 0
    while not 0 <= p < n:
        if p < 0:
            p = -p - 1
        else:
            p = n - 1 - (p - n)
    return p


def reflect_array(p, n):
    """reflect() over an integer array: the same loop, run on the distinct values until every one is inside."""
    u, inv = np.unique(np.asarray(p, np.int64), return_inverse=True)
    if n == 1:
        return np.zeros(np.shape(p), np.int64)
    while True:
        out = (u < 0) | (u >= n)
        if not out.any():
            break
        u = np.where(u < 0, -u - 1, np.where(u >= n, n - 1 - (u - n), u))
    return u[inv].reshape(np.shape(p))


def cv_round(a):
    """x86 cvRound of float values given in float64: half to even, |a| >= 2^31 (and NaN) -> INT_MIN."""
    a = np.asarray(a, np.float64)
    bad = ~(np.abs(a) < 2147483648.0)
    return np.where(bad, -2 ** 31, np.rint(np.where(bad, 0, a))).astype(np.int64)


def sat_short(a):
    return np.clip(a, -32768, 32767)


def _axis_candidates(val, band, scale_q, z_undecided):
    """Quantisations cvRound(scale_q * value) of the values within band of val -> (lo, hi, determined).  Undetermined where more
    than two cells are possible or where the sign of z is undecided."""
    lo = cv_round(scale_q * (val - band))
    hi = cv_round(scale_q * (val + band))
    mid = cv_round(scale_q * val)
    lo = np.minimum(lo, mid)
    hi = np.maximum(hi, mid)
    det = ((hi - lo) <= 1) & ~z_undecided
    hi = np.where(det, hi, lo)
    return lo, hi, det


def remap_linear_reflect_candidates(src, maps):
    """cv::remap(src, INTER_LINEAR, BORDER_REFLECT) on u8 for the maps of spherical_backward_f64
    -> (cands (4, H, W[, cn]) uint8, in_band (H, W) bool, undetermined (H, W) bool)."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    s3 = src.reshape(h, w, -1).astype(np.int64)
    zu = np.abs(maps["z"]) <= maps["zband"]
    xl, xh, xd = _axis_candidates(maps["x"], maps["dx"], 32.0, zu)
    yl, yh, yd = _axis_candidates(maps["y"], maps["dy"], 32.0, zu)
    # where z <= 0 is possible, (-1, -1) is one of the candidates: undecided pixels are left unconstrained (in `und`)
    und = ~(xd & yd)
    outs = []
    for xq in (xl, xh):
        for yq in (yl, yh):
            fx, fy = xq & 31, yq & 31
            sx, sy = sat_short(xq >> 5), sat_short(yq >> 5)
            x0, x1 = reflect_array(sx, w), reflect_array(sx + 1, w)
            y0, y1 = reflect_array(sy, h), reflect_array(sy + 1, h)
            w00 = ((32 - fy) * (32 - fx) * 32)[..., None]
            w01 = ((32 - fy) * fx * 32)[..., None]
            w10 = (fy * (32 - fx) * 32)[..., None]
            w11 = (fy * fx * 32)[..., None]
            s = s3[y0, x0] * w00 + s3[y0, x1] * w01 + s3[y1, x0] * w10 + s3[y1, x1] * w11
            outs.append(np.clip((s + (1 << 14)) >> 15, 0, 255).astype(np.uint8))
    cands = np.stack(outs)
    if src.ndim == 2:
        cands = cands[..., 0]
    in_band = ((xl != xh) | (yl != yh)) & ~und
    return cands, in_band, und


def remap_nearest_constant_candidates(src, maps):
    """cv::remap(src, INTER_NEAREST, BORDER_CONSTANT(0)) on u8 -> (cands (4, H, W[, cn]), in_band, undetermined)."""
    src = np.asarray(src)
    h, w = src.shape[:2]
    s3 = src.reshape(h, w, -1)
    zu = np.abs(maps["z"]) <= maps["zband"]
    xl, xh, xd = _axis_candidates(maps["x"], maps["dx"], 1.0, zu)
    yl, yh, yd = _axis_candidates(maps["y"], maps["dy"], 1.0, zu)
    und = ~(xd & yd)
    outs = []
    for xq in (xl, xh):
        for yq in (yl, yh):
            sx, sy = sat_short(xq), sat_short(yq)
            inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
            v = s3[np.where(inside, sy, 0), np.where(inside, sx, 0)]
            outs.append(np.where(inside[..., None], v, 0).astype(np.uint8))
    cands = np.stack(outs)
    if src.ndim == 2:
        cands = cands[..., 0]
    in_band = ((xl != xh) | (yl != yh)) & ~und
    return cands, in_band, und


def check_candidates(out, cands, in_band, und):
    """-> (mismatch mask (H, W), in-band count, undetermined count): a pixel (all its channels) must equal one candidate;
    outside the band that is the single float64 answer."""
    out = np.asarray(out)
    eq = cands == out[None]
    if eq.ndim == 4:
        eq = eq.all(-1)
    ok = eq.any(0) | und
    return ~ok, int((in_band & ~und).sum()), int(und.sum())


# ------------------------------------------------------------------------------------------------ 2-NN
def _knn2_from_dist(d, nt):
    """Two smallest per row of an int64 distance block, ties to the smaller train index -> (idx (n, 2), d (n, 2))."""
    n = d.shape[0]
    idx = np.full((n, 2), -1, np.int64)
    dd = np.full((n, 2), -1, np.int64)
    if nt == 0:
        return idx, dd
    # (the first two of a stable sort, without the sort: argmin returns the first of equal minima)
    rows = np.arange(n)
    idx[:, 0] = np.argmin(d, axis=1)
    dd[:, 0] = d[rows, idx[:, 0]]
    if nt >= 2:
        rest = np.array(d, np.int64)
        rest[rows, idx[:, 0]] = np.iinfo(np.int64).max
        idx[:, 1] = np.argmin(rest, axis=1)
        dd[:, 1] = rest[rows, idx[:, 1]]
    return idx, dd


def knn2_hamming_exact(q, t, chunk=256):
    """Exact Hamming 2-NN of 32-byte descriptors: popcount of XOR over uint64 words -> (idx (nq, 2) int32, dist (nq, 2) int64).
    Missing neighbours (fewer than 2 trains) are -1."""
    q = np.ascontiguousarray(q, np.uint8).view(np.uint64)
    t = np.ascontiguousarray(t, np.uint8).view(np.uint64)
    nq, nt = q.shape[0], t.shape[0]
    idx = np.full((nq, 2), -1, np.int64)
    dist = np.full((nq, 2), -1, np.int64)
    words = np.ascontiguousarray(t.T)            # word by word: a (chunk, nt) block at a time, not (chunk, nt, 4)
    for a in range(0, nq, chunk):
        d = np.zeros((min(chunk, nq - a), nt), np.int64)
        for w in range(4):
            d += np.bitwise_count(q[a:a + chunk, w, None] ^ words[w][None, :])
        idx[a:a + chunk], dist[a:a + chunk] = _knn2_from_dist(d, nt)
    return idx.astype(np.int32), dist


def knn2_l2_exact(q, t, chunk=256):
    """Exact L2 2-NN of integer-valued descriptors: int64 squared distances, float32(sqrt(d2))
    -> (idx (nq, 2) int32, dist (nq, 2) float32).  Missing neighbours are -1 / -1.0."""
    q = np.asarray(q)
    t = np.asarray(t)
    assert q.shape[1] == t.shape[1], "descriptor widths differ"
    qi, ti = q.astype(np.int64), t.astype(np.int64)
    assert np.array_equal(qi, q) and np.array_equal(ti, t), "integer-valued descriptors only"
    nq, nt = q.shape[0], t.shape[0]
    idx = np.full((nq, 2), -1, np.int64)
    d2 = np.full((nq, 2), -1, np.int64)
    tn = (ti * ti).sum(1)
    for a in range(0, nq, chunk):
        qa = qi[a:a + chunk]
        d = (qa * qa).sum(1)[:, None] + tn[None, :] - 2 * (qa @ ti.T)
        idx[a:a + chunk], d2[a:a + chunk] = _knn2_from_dist(d, nt)
    dist = np.where(d2 >= 0, np.sqrt(np.maximum(d2, 0).astype(np.float64)), -1.0).astype(np.float32)
    return idx.astype(np.int32), dist


DMATCH_DTYPE = np.dtype([("query_idx", "i4"), ("train_idx", "i4"), ("img_idx", "i4"), ("distance", "f4")])


def knn2_exact(q, t):
    q = np.asarray(q)
    if q.dtype == np.uint8:
        i, d = knn2_hamming_exact(q, t)
        return i, d.astype(np.float32)
    return knn2_l2_exact(q, t)


def best_of_2_nearest_matches(d1, d2, match_conf):
    """CpuMatcher::match (BestOf2NearestMatcher) on descriptor sets d1 (image 1) and d2 (image 2) -> DMATCH_DTYPE array.
    Ratio test in float32: d0 < float32(1 - conf) * d1.  A direction runs only when its train set has >= 2 points.  Accepted
    1->2 matches (img_idx 0) in query order, then accepted 2->1 matches whose (t, q) pair is not in the 1->2 set, as
    DMatch(t, q, d) (img_idx -1), in query order."""
    ratio = np.float32(1.0) - np.float32(match_conf)
    out = []
    got = set()
    if len(d2) >= 2 and len(d1):
        i12, e12 = knn2_exact(d1, d2)
        ok = e12[:, 0] < np.float32(ratio * e12[:, 1])
        for q in np.nonzero(ok)[0]:
            out.append((int(q), int(i12[q, 0]), 0, e12[q, 0]))
            got.add((int(q), int(i12[q, 0])))
    if len(d1) >= 2 and len(d2):
        i21, e21 = knn2_exact(d2, d1)
        ok = e21[:, 0] < np.float32(ratio * e21[:, 1])
        for q in np.nonzero(ok)[0]:
            t = int(i21[q, 0])
            if (t, int(q)) not in got:
                out.append((t, int(q), -1, e21[q, 0]))
    return np.array(out, DMATCH_DTYPE) if out else np.zeros(0, DMATCH_DTYPE)


# ------------------------------------------------------------------------------------------------ shared test regimes
def _rot(axis, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def camera(w, h, hfov, yaw, pitch=0.0, roll=0.0, scale_mult=1.0, seam=False):
    """A pinhole camera (principal point at the centre) turned by yaw (y), pitch (x), roll (z) -> (K, R, scale) as the ABI
    receives them (float32).  scale = scale_mult * f; seam=True scales K with it (the seam-scale warper of the job)."""
    f = (w / 2.0) / math.tan(math.radians(hfov) / 2.0)
    R = _rot("y", yaw) @ _rot("x", pitch) @ _rot("z", roll)
    k = scale_mult if seam else 1.0
    K = np.array([[f * k, 0, w * 0.5 * k], [0, f * k, h * 0.5 * k], [0, 0, 1]])
    return K.astype(np.float32), R.astype(np.float32), float(np.float32(f * scale_mult))


# (name, hfov, yaw, pitch, roll): the seam, the poles (pitch 85: the pole is inside the roi), roll, narrow and wide fields of
# view (hfov 150: rays with z <= 0 inside the roi and coordinates past +-2^15)
WARP_GEOMS = [
    ("front", 60.0, 0.0, 0.0, 0.0),
    ("seam+", 90.0, 175.0, 0.0, 0.0),
    ("seam-", 60.0, -178.0, 3.0, 0.0),
    ("pitch+70", 60.0, 20.0, 70.0, 0.0),
    ("pitch-70", 60.0, -20.0, -70.0, 0.0),
    ("pitch+85", 60.0, 0.0, 85.0, 0.0),
    ("pitch-85", 60.0, 10.0, -85.0, 0.0),
    ("roll+30", 60.0, 10.0, 5.0, 30.0),
    ("roll-30", 60.0, -10.0, -5.0, -30.0),
    ("hfov30", 30.0, 5.0, 2.0, 0.0),
    ("hfov90", 90.0, 0.0, 0.0, 0.0),
    ("hfov150", 150.0, 0.0, 10.0, 0.0),
]
# (w, h, scale multipliers, seam flags): tiny sources (the ABI accepts 2 x 2) magnified 25-fold fold their taps several times
WARP_SOURCES = [
    ((2, 2), (1.0, 25.0)), ((3, 2), (1.0, 25.0)), ((2, 3), (1.0, 25.0)), ((5, 7), (1.0, 0.37, 20.0)),
    ((63, 9), (1.0, 0.37)), ((64, 8), (1.0, 0.37)), ((65, 9), (1.0, 0.37)),
]


def content(kind, shape, seed=0):
    if kind == "zero":
        return np.zeros(shape, np.uint8)
    if kind == "full":
        return np.full(shape, 255, np.uint8)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
