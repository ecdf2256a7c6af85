"""Independent reference of cv::findHomography(src, dst, mask, RANSAC) and of the MatchesInfo that
cv::detail::BestOf2NearestMatcher builds from a match list, written from OpenCV's documented semantics (calib3d fundam.cpp,
ptsetreg.cpp, stitching matchers.cpp, core RNG) in plain numpy / Python.  It imports neither the oracle nor the product and
takes a different numerical road wherever the road is not part of the semantics.

The reading
-----------
* cv::RNG: state = (uint32)state * 4164903690 + (state >> 32) on 64 bits, seeded with (uint64)-1; next() is the low 32 bits;
  uniform(a, b) = a + next() % (b - a).  Python integers.
* getSubset: four indices, each redrawn while it repeats an earlier one; the subset is kept when checkSubset accepts it, at most
  10000 attempts; an exhausted getSubset ends the loop (at iteration 0: no model at all).
* checkSubset: haveCollinearPoints on either side, which tests only the triples that contain the LAST point:
  |dx2*dy1 - dy2*dx1| <= FLT_EPSILON * (|dx1| + |dy1| + |dx2| + |dy2|), the differences being float32 subtractions of the
  float32 coordinates; then the orientation test: over the triples (0,1,2), (1,2,3), (0,2,3), (0,1,3) the count of
  det(src triple) * det(dst triple) < 0 must be 0 or 4.  Both are decided here in EXACT rational arithmetic (the inputs are
  float32, so fractions.Fraction holds them exactly); 0 * x < 0 is false, so an exactly zero determinant is decided.
* Hypothesis: the homography through the four correspondences, normalised to h22 = 1.  Here: the solution of the 8 x 8 linear
  system in float64 (numpy.linalg.solve), not a normalised DLT with a Jacobi eigen solver.
* Inlier test: the model rounded to float32, the squared reprojection error in float32, err <= (float)(thresh * thresh).
* Loop: niters = max(max_iters, 1); a model replaces the best when good > max(max_good, 3) (strict); then
  niters = RANSACUpdateNumIters(confidence, (n - good) / n, 4, niters): p, ep clamped to [0, 1], num = max(1 - p, DBL_MIN),
  denom = 1 - (1 - ep)^4, denom < DBL_MIN -> 0, and with the logs: denom >= 0 or -num >= niters * -denom -> niters, else
  cvRound(num / denom) (round half to even).  n < 4: no model; n == 4: the model of all four points, mask all ones, no
  checkSubset; n > 4: the loop, and a model exists when max_good > 0.
* Tail (n > 4): the inliers are compressed, the normalised DLT runs over all of them (centroid, per-axis scale
  count / sum|x - c|) and LMSolver refines the 8 free parameters for at most 10 iterations.
* MatchesInfo: points are keypoints - size * 0.5f in float32; fewer matches than num_matches_thresh1 -> nothing; first estimate
  with mask; no H or |det H| < DBL_EPSILON -> stop; num_inliers; confidence = inliers / (8 + 0.3 * matches), > 3 -> 0;
  num_inliers < num_matches_thresh2 -> stop; second estimate on the inliers only replaces H (and may leave none).  The entry
  (j, i) has the swapped matches, the same mask, counts and confidence, and the inverse H.

The error model (stated once, not tuned to any test)
----------------------------------------------------
The reference evaluates the squared error e in float64 from the float32-rounded model.  A float32 evaluation of the same
expression differs from it to first order by
    d(px) = 3u * (|h0 X| + |h1 Y| + |h2|) / |w|  +  |px| * (3u * (|h6 X| + |h7 Y| + 1) / |w| + 2u),      u = 2^-24
(each of the three terms of a sum passes at most three roundings; the reciprocal and the product add two), the subtraction adds
u * |dx|, and e = dx^2 + dy^2 moves by at most  band = 2|dx| d(dx) + 2|dy| d(dy) + 3u * e.  At +-900 px and the 3 px threshold
this is about 1e-3 to 2e-3.  A point with |e - t| <= band is "in the band"; each count is the interval [lo, hi] without / with
the band points.

Undecided
---------
The replay returns decided = True or the reason it is not decided: "count straddles max" (a count interval contains the
running maximum's boundary), "point in band" (a winning model has a band point), "niters boundary" (num / denom within 1e-9 of
k + 1/2, or the two sides of the max-iterations comparison within 1e-12 relative), "orientation boundary" / "collinear
boundary" (the exact expression is non-zero but within 8 ulps of the sum of the absolute terms: the float64 evaluation the
semantics prescribe could land on either side), "degenerate subset" (an accepted subset whose 8 x 9 DLT matrix, on points
scaled to unit mean deviation, has a second-smallest singular value below 1e-6 of the largest: three collinear points plus
one off the line pass checkSubset, and their homography is a one-parameter family from which every solver picks its own
member).  An undecided case is reported by the tests and left out of the value comparisons.

The tail is held through its fixed point: H0 is the normalised DLT over the inliers by numpy.linalg.svd, H* the minimiser of
the reprojection cost S by this file's own Gauss-Newton from H0 (to a step below 1e-13).  LMSolver's lambda schedule is not
restated.  S is evaluated in extended precision (numpy.longdouble).

Two places where the bounds of the tail need the reference's own resolution (both derived here, neither from a result):
* Solver residue.  Every solver takes the points through some tens of float64 roundings, so a residual below
  rho = 16 * 2^-52 * max|coordinate| is residue of the solver that produced H, not a property of H.  The cost inequalities carry
  the absolute slack n_inliers * rho^2 (5e-21 for 200 points at +-1500 px): it decides nothing unless all residuals are at that
  level, which is the exact-lattice data, where S(H0), S(H*) and S(H) are ~1e-23 and carry no order.
* Start beside the minimiser.  The 2 * FLT_EPSILON parameter bound rests on LMSolver reaching its undamped iterations (lambda
  1 -> 1/2 -> 0) before a step falls below FLT_EPSILON.  Its first step is damped (lambda = 1: at most half of the Gauss-Newton
  step in every eigen-direction, less in weak ones), so from a start H0 within 4 * FLT_EPSILON of H* that first step can already be
  below FLT_EPSILON and end the run where it stands; every accepted damped step shrinks each eigen-component of H - H*, so H stays
  within the start's distance.  Where D0 = max|H0 - H*| lies in (2, 4) * FLT_EPSILON the parameters are therefore held to D0
  instead ("near start"); such a case counts towards the cap like a cost-only one.  Below 2 * FLT_EPSILON the plain bound holds
  as it is.
"""
import math
from fractions import Fraction

import numpy as np

FLT_EPSILON = 2.0 ** -23
DBL_EPSILON = 2.0 ** -52
DBL_MIN = 2.2250738585072014e-308
U32 = 2.0 ** -24
DMATCH_DTYPE = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("img_idx", "<i4"), ("distance", "<f4")])


# ------------------------------------------------------------------------------------------------ cv::RNG
class Rng:
    def __init__(self, state=(1 << 64) - 1):
        self.state = state if state else 0xFFFFFFFF
        self.draws = 0

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        self.draws += 1
        return self.state & 0xFFFFFFFF

    def uniform(self, a, b):
        return a if a == b else a + self.next() % (b - a)


# ------------------------------------------------------------------------------------------------ checkSubset, exact
_NEAR_ULPS = 8


def _to_ints(*arrays):
    """float arrays -> (lists of Python integers on one common power-of-two scale, the scale).  Exact."""
    ratios = [[float(v).as_integer_ratio() for v in np.asarray(a).ravel()] for a in arrays]
    scale = max(d for r in ratios for _, d in r)
    return [[n * (scale // d) for n, d in r] for r in ratios], scale


def have_collinear_exact(pts):
    """haveCollinearPoints(pts, count) on float32 points -> (collinear, near_boundary).  The differences to the last point are
    float32 subtractions (Point2f); everything after them is exact integer arithmetic on a common power-of-two scale."""
    pts = np.asarray(pts, np.float32)
    i = len(pts) - 1
    (dif,), sc = _to_ints(pts[:i] - pts[i])
    near = False
    for j in range(i):
        dx1, dy1 = dif[2 * j], dif[2 * j + 1]
        for k in range(j):
            dx2, dy2 = dif[2 * k], dif[2 * k + 1]
            t1, t2 = dx2 * dy1, dy2 * dx1
            lhs = abs(t1 - t2) << 23                                            # scale sc^2 * 2^23 on both sides
            rhs = (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)) * sc
            if lhs != 0 and (abs(lhs - rhs) << 52) <= _NEAR_ULPS * (((abs(t1) + abs(t2)) << 23) + rhs):
                near = True
            if lhs <= rhs:
                return True, near
    return False, near


def _det3_int(x0, y0, x1, y1, x2, y2):
    terms = (x0 * y1, -x0 * y2, -y0 * x1, y0 * x2, x1 * y2, -y1 * x2)
    return sum(terms), sum(abs(t) for t in terms)


def det3_exact(p0, p1, p2):
    """det [x0 y0 1; x1 y1 1; x2 y2 1] of float32 points as a Fraction, and the sum of the absolute terms."""
    (v,), sc = _to_ints(np.array([p0, p1, p2], np.float64))
    det, mag = _det3_int(*v)
    return Fraction(det, sc * sc), Fraction(mag, sc * sc)


_TRIPLES = ((0, 1, 2), (1, 2, 3), (0, 2, 3), (0, 1, 3))


def orientation_negative_exact(s, d):
    """The count of det(src triple) * det(dst triple) < 0 over the four triples -> (negative, near_boundary)."""
    (si, di), _ = _to_ints(np.asarray(s, np.float64), np.asarray(d, np.float64))
    negative, near = 0, False
    for t in _TRIPLES:
        a, sa = _det3_int(*(si[2 * q + c] for q in t for c in (0, 1)))
        b, sb = _det3_int(*(di[2 * q + c] for q in t for c in (0, 1)))
        for v, sv in ((a, sa), (b, sb)):
            if v != 0 and (abs(v) << 52) <= _NEAR_ULPS * sv:
                near = True
        negative += (a * b) < 0
    return negative, near


def check_subset_exact(s, d):
    """HomographyEstimatorCallback::checkSubset on four correspondences -> (accepted, reason-or-None)."""
    for pts in (s, d):
        col, near = have_collinear_exact(pts)
        if near:
            return False, "collinear boundary"
        if col:
            return False, None
    negative, near = orientation_negative_exact(s, d)
    if near:
        return False, "orientation boundary"
    return negative in (0, 4), None


# ------------------------------------------------------------------------------------------------ models
def _dlt_rows(s, d):
    A = np.zeros((2 * len(s), 9))
    X, Y, x, y = s[:, 0], s[:, 1], d[:, 0], d[:, 1]
    A[0::2, 0], A[0::2, 1], A[0::2, 2] = X, Y, 1.0
    A[0::2, 6], A[0::2, 7], A[0::2, 8] = -x * X, -x * Y, -x
    A[1::2, 3], A[1::2, 4], A[1::2, 5] = X, Y, 1.0
    A[1::2, 6], A[1::2, 7], A[1::2, 8] = -y * X, -y * Y, -y
    return A


def _unit_deviation(p):
    c = p.mean(0)
    dev = np.abs(p - c).mean(0)
    return (p - c) / np.where(dev > 0, dev, 1.0)


def subset_sv_ratio(s, d):
    """Second-smallest over largest singular value of the 8 x 9 DLT matrix of four correspondences scaled to unit mean
    deviation: ~0 when the four points leave a family of homographies."""
    sv = np.linalg.svd(_dlt_rows(_unit_deviation(np.asarray(s, np.float64)), _unit_deviation(np.asarray(d, np.float64))), compute_uv=False)
    return sv[-2] / sv[0] if len(sv) == 9 else sv[-1] / sv[0]


def homography_4pt(s, d):
    """The homography through four correspondences with h22 = 1: the 8 x 8 system in float64 -> 3 x 3, or None."""
    s, d = np.asarray(s, np.float64), np.asarray(d, np.float64)
    A = _dlt_rows(s, d)
    try:
        h = np.linalg.solve(A[:, :8], -A[:, 8])
    except np.linalg.LinAlgError:
        return None
    return np.append(h, 1.0).reshape(3, 3)


def dlt_normalized_svd(s, d):
    """runKernel over many points: centroid and count / sum|x - c| scaling per axis, the null vector of the stacked system by
    SVD, denormalised and scaled to h22 = 1."""
    s, d = np.asarray(s, np.float64), np.asarray(d, np.float64)
    cs, cd = s.mean(0), d.mean(0)
    ss, sd = np.abs(s - cs).sum(0), np.abs(d - cd).sum(0)
    if min(ss.min(), sd.min()) < DBL_EPSILON:
        return None
    ss, sd = len(s) / ss, len(d) / sd
    A = _dlt_rows((s - cs) * ss, (d - cd) * sd)
    Hn = np.linalg.svd(A)[2][-1].reshape(3, 3)
    inv_d = np.array([[1 / sd[0], 0, cd[0]], [0, 1 / sd[1], cd[1]], [0, 0, 1]])
    T_s = np.array([[ss[0], 0, -cs[0] * ss[0]], [0, ss[1], -cs[1] * ss[1]], [0, 0, 1]])
    H = inv_d @ Hn @ T_s
    return H / H[2, 2]


def _residuals(h8, s, d, dtype=np.float64):
    s, d, h = s.astype(dtype), d.astype(dtype), np.asarray(h8, dtype)
    w = h[6] * s[:, 0] + h[7] * s[:, 1] + 1
    px = (h[0] * s[:, 0] + h[1] * s[:, 1] + h[2]) / w
    py = (h[3] * s[:, 0] + h[4] * s[:, 1] + h[5]) / w
    return px - d[:, 0], py - d[:, 1], w, px, py


def reproj_cost(H, s, d):
    """S(H): the squared reprojection error summed over the correspondences, in extended precision."""
    H = np.asarray(H, np.float64)
    rx, ry = _residuals((H / H[2, 2]).reshape(9)[:8], np.asarray(s), np.asarray(d), np.longdouble)[:2]
    return float((rx * rx + ry * ry).sum())


def gauss_newton(H0, s, d, tol=1e-13, max_steps=50):
    """Plain Gauss-Newton on the 8 parameters from H0 -> (H*, [max-norm of each step])."""
    s, d = np.asarray(s, np.float64), np.asarray(d, np.float64)
    h = (np.asarray(H0, np.float64) / H0[2, 2]).reshape(9)[:8].copy()
    steps = []
    for _ in range(max_steps):
        rx, ry, w, px, py = _residuals(h, s, d)
        J = np.zeros((2 * len(s), 8))
        X, Y = s[:, 0] / w, s[:, 1] / w
        J[0::2, 0], J[0::2, 1], J[0::2, 2], J[0::2, 6], J[0::2, 7] = X, Y, 1 / w, -X * px, -Y * px
        J[1::2, 3], J[1::2, 4], J[1::2, 5], J[1::2, 6], J[1::2, 7] = X, Y, 1 / w, -X * py, -Y * py
        r = np.empty(2 * len(s))
        r[0::2], r[1::2] = rx, ry
        cn = np.sqrt((J * J).sum(0))                                            # column scaling: the columns span 1/w .. X^2/w
        step = np.linalg.lstsq(J / cn, r, rcond=None)[0] / cn
        h -= step
        steps.append(float(np.abs(step).max()))
        if steps[-1] < tol:
            break
    return np.append(h, 1.0).reshape(3, 3), steps


def converged_fast(steps):
    """A step below FLT_EPSILON within 5 steps, consecutive step ratios below 1/2 up to it."""
    for k, st in enumerate(steps[:5]):
        if k and st >= 0.5 * steps[k - 1]:
            return False
        if st < FLT_EPSILON:
            return True
    return False


# ------------------------------------------------------------------------------------------------ inliers with the band
def inlier_intervals(H, src, dst, t):
    """-> (sure, maybe): sure[i] the point is an inlier whatever the float32 rounding, maybe[i] it lies in the band."""
    h = np.asarray(H, np.float64).reshape(9).astype(np.float32).astype(np.float64)
    X, Y = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        w = h[6] * X + h[7] * Y + 1.0
        aw = np.abs(w)
        px, py = (h[0] * X + h[1] * Y + h[2]) / w, (h[3] * X + h[4] * Y + h[5]) / w
        dx, dy = px - dst[:, 0], py - dst[:, 1]
        e = dx * dx + dy * dy
        den = 3 * U32 * (np.abs(h[6] * X) + np.abs(h[7] * Y) + 1.0) / aw + 2 * U32
        ddx = 3 * U32 * (np.abs(h[0] * X) + np.abs(h[1] * Y) + abs(h[2])) / aw + np.abs(px) * den + U32 * np.abs(dx)
        ddy = 3 * U32 * (np.abs(h[3] * X) + np.abs(h[4] * Y) + abs(h[5])) / aw + np.abs(py) * den + U32 * np.abs(dy)
        band = 2 * np.abs(dx) * ddx + 2 * np.abs(dy) * ddy + 3 * U32 * e
        bad = ~np.isfinite(e) | ~np.isfinite(band)
        sure = (e < t - band) & ~bad
        maybe = ((np.abs(e - t) <= band) & ~bad) | (bad & (aw < 1e-3))
    return sure, maybe


def update_num_iters(p, ep, max_iters):
    """RANSACUpdateNumIters(p, ep, 4, max_iters) -> (niters, near_boundary)."""
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** 4
    if denom < DBL_MIN:
        return 0, False
    num, denom = math.log(num), math.log(denom)
    if denom >= 0:
        return max_iters, False
    a, b = -num, max_iters * -denom
    if abs(a - b) <= 1e-12 * max(abs(a), abs(b)):
        return max_iters, True
    if a >= b:
        return max_iters, False
    q = num / denom
    return int(round(q)), abs(q - math.floor(q) - 0.5) < 1e-9


# ------------------------------------------------------------------------------------------------ findHomography
class Estimate:
    """What the replay found.  decided: True, or the reason string.  ok, mask (uint8), iters (loop iterations that drew a
    subset), draws (RNG draws); for ok with n > 4: H0, Hstar, steps, fast (converged_fast), D0 = max|H0 - H*|, near_start, inl_src /
    inl_dst; for ok with n == 4: H4 and sv_ratio."""

    def __init__(self, n):
        self.n, self.decided, self.ok = n, True, False
        self.mask = np.zeros(n, np.uint8)
        self.iters = self.draws = 0
        self.H0 = self.Hstar = self.H4 = None
        self.steps, self.fast, self.D0, self.near_start = [], False, 0.0, False
        self.inl_src = self.inl_dst = None
        self.sv_ratio = self.src = self.dst = None

    @property
    def is_decided(self):
        return self.decided is True


def find_homography(src, dst, thresh=3.0, max_iters=2000, confidence=0.995):
    src, dst = np.ascontiguousarray(src, np.float32).reshape(-1, 2), np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    n = len(src)
    est = Estimate(n)
    est.src, est.dst = src, dst
    if thresh <= 0:
        thresh = 3.0
    if n < 4:
        return est
    if n == 4:
        est.sv_ratio = float(subset_sv_ratio(src, dst))
        H = homography_4pt(src, dst)
        if est.sv_ratio < 1e-3 or H is None:
            est.decided = "degenerate subset"
            return est
        est.ok, est.H4 = True, H
        est.mask[:] = 1
        return est
    t = float(np.float32(thresh * thresh))
    rng = Rng()
    niters, max_good, it = max(max_iters, 1), 0, 0
    best = None
    while it < niters:
        found = False
        for _ in range(10000):
            idx = []
            for i in range(4):
                k = rng.uniform(0, n)
                while k in idx:
                    k = rng.uniform(0, n)
                idx.append(k)
            okk, why = check_subset_exact(src[idx], dst[idx])
            if why:
                est.decided, est.draws = why, rng.draws
                return est
            if okk:
                found = True
                break
        if not found:
            break
        est.iters = it + 1
        it += 1
        if subset_sv_ratio(src[idx], dst[idx]) < 1e-6:
            est.decided, est.draws = "degenerate subset", rng.draws
            return est
        H = homography_4pt(src[idx], dst[idx])
        if H is None:
            est.decided, est.draws = "degenerate subset", rng.draws
            return est
        sure, maybe = inlier_intervals(H, src, dst, t)
        lo, hi = int(sure.sum()), int(sure.sum() + maybe.sum())
        bar = max(max_good, 3)
        if hi <= bar:
            continue
        if lo <= bar:
            est.decided, est.draws = "count straddles max", rng.draws
            return est
        if hi != lo:
            est.decided, est.draws = "point in band", rng.draws
            return est
        best, max_good = sure, lo
        niters, near = update_num_iters(confidence, (n - lo) / n, niters)
        if near:
            est.decided, est.draws = "niters boundary", rng.draws
            return est
    est.draws = rng.draws
    if max_good <= 0:
        return est
    est.ok = True
    est.mask = best.astype(np.uint8)
    est.inl_src, est.inl_dst = src[best], dst[best]
    est.H0 = dlt_normalized_svd(est.inl_src, est.inl_dst)
    if est.H0 is None:
        est.decided = "degenerate subset"
        return est
    est.Hstar, est.steps = gauss_newton(est.H0, est.inl_src, est.inl_dst)
    est.fast = converged_fast(est.steps) and est.steps[-1] < 1e-13
    est.D0 = float(np.abs(est.H0 / est.H0[2, 2] - est.Hstar).reshape(9)[:8].max())
    est.near_start = 2 * FLT_EPSILON < est.D0 < 4 * FLT_EPSILON
    return est


# ------------------------------------------------------------------------------------------------ MatchesInfo
def centred_points(matches, xy1, size1, xy2, size2):
    xy1, xy2 = np.asarray(xy1, np.float32), np.asarray(xy2, np.float32)
    c1 = np.array([np.float32(size1[0]) * np.float32(0.5), np.float32(size1[1]) * np.float32(0.5)], np.float32)
    c2 = np.array([np.float32(size2[0]) * np.float32(0.5), np.float32(size2[1]) * np.float32(0.5)], np.float32)
    return (xy1[matches["query_idx"]] - c1).astype(np.float32), (xy2[matches["train_idx"]] - c2).astype(np.float32)


class PairInfo:
    """MatchesInfo of one pair (i < j) by the reference.  decided as in Estimate; has_H, num_inliers, confidence, mask (empty
    when no estimate ran), and `final`: the Estimate whose tail gives the reported H (the second one when it ran)."""

    def __init__(self):
        self.decided, self.has_H, self.num_inliers, self.confidence = True, False, 0, 0.0
        self.mask = np.zeros(0, np.uint8)
        self.first = self.second = self.final = None

    @property
    def is_decided(self):
        return self.decided is True


def matches_info(matches, xy1, size1, xy2, size2, thresh1=6, thresh2=6):
    out = PairInfo()
    nm = len(matches)
    if nm < thresh1:
        return out
    sp, dp = centred_points(matches, xy1, size1, xy2, size2)
    e1 = out.first = out.final = find_homography(sp, dp)
    if not e1.is_decided:
        out.decided = e1.decided
        return out
    out.mask = e1.mask.copy()
    if not e1.ok:
        return out
    out.has_H = True
    Href = e1.Hstar if e1.Hstar is not None else e1.H4
    det = abs(np.linalg.det(Href))
    if det < 1e3 * DBL_EPSILON:
        if det > 1e-3 * DBL_EPSILON:
            out.decided = "det boundary"
        return out
    out.num_inliers = int(e1.mask.sum())
    conf = out.num_inliers / (8 + 0.3 * nm)
    out.confidence = 0.0 if conf > 3.0 else conf
    if out.num_inliers < thresh2:
        return out
    keep = e1.mask.astype(bool)
    e2 = out.second = out.final = find_homography(sp[keep], dp[keep])
    if not e2.is_decided:
        out.decided = e2.decided
        return out
    out.has_H = e2.ok
    return out


# ------------------------------------------------------------------------------------------------ the assertions
def check_estimate(est, ok, H, mask, iters=None):
    """Hold one findHomography result (ok, H 3x3 float64 or None, mask uint8) to a DECIDED Estimate.  -> dict(kind, dH) where
    kind is "params" (the parameters were compared with H*), "cost" (cost inequalities only) or "none" (nothing to compare),
    dH = max |H - H*| over the 8 parameters (None when there is no H*)."""
    assert est.is_decided
    assert bool(ok) == est.ok, (ok, est.ok)
    assert np.asarray(mask, np.uint8).tobytes() == est.mask.tobytes(), np.nonzero(np.asarray(mask) != est.mask)[0][:8]
    if iters is not None:
        assert iters == est.iters, (iters, est.iters)
    if not est.ok:
        return dict(kind="none", dH=None)
    H = np.asarray(H, np.float64).reshape(3, 3)
    assert np.isfinite(H).all() and abs(H[2, 2] - 1.0) <= DBL_EPSILON, H      # x * (1 / x): one rounding from 1
    return check_tail(est, H)


def check_tail(est, H):
    """The H of a decided, ok Estimate against its tail: n == 4 by the mapping of the four points, n > 4 by the cost
    inequalities and, where Gauss-Newton converged fast, the parameters."""
    if est.n == 4:
        s, d = est.src, est.dst
        rx, ry = _residuals(H.reshape(9)[:8], s, d, np.longdouble)[:2]
        bound = U32 * float(max(np.abs(s).max(), np.abs(d).max()))
        assert float(np.abs(rx).max()) <= bound and float(np.abs(ry).max()) <= bound, (rx, ry, bound)
        return dict(kind="params", dH=float(np.abs(H - est.H4).max()))
    s, d = est.inl_src, est.inl_dst
    S, S0, Sstar = reproj_cost(H, s, d), reproj_cost(est.H0, s, d), reproj_cost(est.Hstar, s, d)
    dH = float(np.abs(H - est.Hstar).reshape(9)[:8].max())
    rho = 16 * DBL_EPSILON * float(max(np.abs(s).max(), np.abs(d).max()))
    slack = len(s) * rho * rho
    assert S <= S0 * (1 + 1e-12) + slack, ("the refinement increased the cost", S, S0)
    assert S >= Sstar * (1 - 1e-12) - slack, ("below the minimiser's cost", S, Sstar)
    if not est.fast:
        return dict(kind="cost", dH=dH)
    if est.near_start:
        assert dH <= est.D0, (dH, est.D0, H, est.Hstar)
        return dict(kind="near start", dH=dH)
    assert dH <= 2 * FLT_EPSILON, (dH, H, est.Hstar)
    return dict(kind="params", dH=dH)


def family_gate(name, ests, cap=0.10):
    """The cap of a family, asserted before any comparison: at most `cap` of its cases undecided or without fast convergence of
    the reference's Gauss-Newton or started beside the minimiser ("near start"), and at least one decided case with ok true.  -> (decided, weak) counts."""
    und = [e for e in ests if not e.is_decided]
    weak = [e for e in ests if e.is_decided and e.ok and e.n > 4 and (not e.fast or e.near_start)]
    assert len(und) + len(weak) <= cap * len(ests), (name, "undecided", [e.decided for e in und], "cost only", len(weak), "of", len(ests))
    assert any(e.is_decided and e.ok for e in ests), name
    return len(ests) - len(und), len(weak)


# ------------------------------------------------------------------------------------------------ shared input families
H_BASE = ((0.97, 0.03, 25.0), (-0.02, 1.03, -14.0), (2e-5, -1e-5, 1.0))
H_PERSPECTIVE = ((0.95, 0.04, 12.0), (-0.03, 1.02, -8.0), (1.1e-3, -0.9e-3, 1.0))     # w spans 1 +- 0.8 at +-400 px


def _apply(H, p):
    q = np.c_[np.asarray(p, np.float64), np.ones(len(p))] @ np.asarray(H, np.float64).T
    return q[:, :2] / q[:, 2:]


def synth(seed, n, n_out, lim=900.0, noise=0.4, H=H_BASE, shuffle=True):
    """n float32 correspondences under H with Gaussian noise on the destination; n_out of them get a uniform random
    destination instead.  shuffle spreads the outliers over the list."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-lim, lim, (n, 2)).astype(np.float32)
    dst = _apply(H, src) + rng.normal(0, noise, (n, 2))
    dst[:n_out] = rng.uniform(-lim, lim, (n_out, 2))
    order = rng.permutation(n) if shuffle else np.arange(n)
    return src[order], dst.astype(np.float32)[order]


def _case(name, src, dst, **expect):
    kw = {k: expect.pop(k) for k in ("thresh", "max_iters", "confidence") if k in expect}
    return dict(name=name, src=np.ascontiguousarray(src, np.float32), dst=np.ascontiguousarray(dst, np.float32), kw=kw, expect=expect)


# The seed tables below (ITER_REGIMES, the seeds of family_large, COLLINEAR_SETS, BATCH_SEEDS) hold seeds at which the replay is
# decided and lands where the comment says.  After a change to a generator re-derive them with the replay alone: loop the seed,
# call find_homography (matches_info on the batch's own match list for BATCH_SEEDS: the match order moves the draws) and keep the
# first seed whose Estimate is decided with the wanted iters; for ITER_REGIMES first pick (n, inliers) with
# update_num_iters(0.995, (n - inliers) / n, 2000) equal to the wanted count.
# (n, outliers, seed, iteration count of the replay): picked from the replay itself so that the final count falls below 64, on
# 64 +- 1 and 128 +- 1 (the hypothesis blocks and the boundary between the two phases of the device loop), in the hundreds, at 2000
ITER_REGIMES = ((600, 60, 3, 5), (500, 150, 3, 19), (300, 140, 1, 63), (300, 141, 1, 64), (314, 148, 1, 65), (300, 165, 1, 127),
                (314, 173, 1, 128), (328, 181, 1, 129), (700, 420, 3, 204), (400, 280, 3, 651), (800, 640, 3, 2000))


def family_iters():
    out = [_case("iters n%d out%d seed%d" % (n, no, seed), *synth(seed, n, no, noise=0.3), iters=it) for n, no, seed, it in ITER_REGIMES]
    rng = np.random.default_rng(5)
    out.append(_case("pure noise", rng.uniform(-500, 500, (400, 2)), rng.uniform(-500, 500, (400, 2)), iters=2000))
    out.append(_case("90% outliers", *synth(11, 600, 540), iters=2000))
    return out


def family_small_n():
    out = []
    for n, no, seed in ((3, 0, 1), (4, 0, 2), (4, 0, 3), (5, 0, 4), (5, 1, 5), (6, 0, 6), (6, 1, 7), (7, 0, 8), (7, 2, 9), (8, 0, 10),
                        (8, 3, 11), (10, 4, 12), (10, 3, 13), (10, 0, 14), (33, 0, 15), (33, 10, 16), (33, 20, 17)):
        out.append(_case("n%d out%d" % (n, no), *synth(seed, n, no, lim=300.0)))
    return out


def family_large():
    out = []
    # seeds at which no winning model of the replay has a point in the band (at +-3840 px the band is 4x that at +-900)
    for n, lim, seed in ((2500, 3840.0, 3), (2500, 3840.0, 4), (8000, 3840.0, 2), (8000, 3840.0, 8), (2500, 20.0, 1), (2500, 20.0, 3),
                         (8000, 20.0, 1), (8000, 20.0, 3)):
        out.append(_case("n%d lim%g seed%d" % (n, lim, seed), *synth(seed, n, n // 5, lim=lim, noise=0.3)))
    for n, seed in ((2500, 8), (8000, 9), (600, 10)):
        out.append(_case("perspective n%d" % n, *synth(seed, n, n // 4, lim=400.0, H=H_PERSPECTIVE)))
    return out


def family_exact():
    """Integer points under an integer affine map (every error of the true model is exactly 0, every good model ties), with
    integer outliers; and a projective map without noise (errors are the float32 rounding of the destinations)."""
    out = []
    for seed, n, no in ((1, 60, 0), (2, 200, 0), (3, 200, 50), (4, 500, 250), (5, 35, 5), (6, 1000, 100), (7, 120, 90), (8, 300, 30)):
        rng = np.random.default_rng(seed)
        src = rng.integers(-500, 501, (n, 2)).astype(np.float64)
        A = np.array([[2, 1], [-1, 3]]) if seed % 2 else np.array([[1, -2], [1, 1]])
        dst = src @ A.T + np.array([7, -11])
        dst[:no] = rng.integers(-1500, 1501, (no, 2))
        order = rng.permutation(n)
        out.append(_case("affine lattice seed%d n%d out%d" % (seed, n, no), src[order], dst[order]))
    for seed, n, no in ((9, 300, 0), (10, 300, 100), (11, 50, 10), (12, 2000, 400)):
        out.append(_case("projective exact seed%d" % seed, *synth(seed, n, no, noise=0.0)))
    return out


def _mostly_collinear(seed, n_line, k_off):
    rng = np.random.default_rng(seed)
    t = rng.integers(-400, 401, n_line).astype(np.float64)
    src = np.r_[np.c_[t, 2 * t + 3], rng.uniform(-400, 400, (k_off, 2))].astype(np.float32)
    dst = _apply(H_BASE, src) + rng.normal(0, 0.3, (len(src), 2))
    order = rng.permutation(len(src))
    return src[order], dst.astype(np.float32)[order]


def _mirrored(seed, n, n_mirror):
    """n_mirror correspondences are the mirror image (x -> -x) of a consistent motion: a subset that mixes the two groups fails
    the orientation test, and the mirrored group is itself a homography that ties or competes with the true one."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-600, 600, (n, 2)).astype(np.float32)
    dst = _apply(H_BASE, src) + rng.normal(0, 0.3, (n, 2))
    dst[:n_mirror, 0] = -dst[:n_mirror, 0]
    order = rng.permutation(n)
    return src[order], dst.astype(np.float32)[order]


def _heap(seed, n_heap, n_noise):
    """n_heap correspondences share one source point (with random destinations): two of them in a subset are collinear with
    anything, so most attempts are rejected; the rest is noise, so the loop runs all its iterations."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-500, 500, (n_heap + n_noise, 2))
    src[:n_heap] = (17.0, -33.0)
    dst = rng.uniform(-500, 500, (n_heap + n_noise, 2))
    order = rng.permutation(len(src))
    return src.astype(np.float32)[order], dst.astype(np.float32)[order]


# (points on the line, points off it, seed): seeds at which the replay meets no degenerate subset (three on the line and the
# last one off pass checkSubset; such a case is undecided by nature)
COLLINEAR_SETS = ((65, 5, 13), (70, 6, 4), (75, 7, 5), (80, 8, 1), (85, 9, 12), (90, 10, 2), (95, 11, 3), (100, 12, 11))


def family_rejection():
    out = [_case("line%d off%d seed%d" % (nl, k, seed), *_mostly_collinear(seed, nl, k)) for nl, k, seed in COLLINEAR_SETS]
    out.append(_case("mirrored half", *_mirrored(1, 400, 200)))
    out.append(_case("mirrored minority", *_mirrored(2, 300, 100)))
    out.append(_case("mirrored majority", *_mirrored(3, 300, 200)))
    out.append(_case("heap past the draw table", *_heap(4, 120, 80), draws_gt=131072, iters=2000))
    x = np.random.default_rng(6).uniform(-100, 100, 50).astype(np.float32)
    line = np.stack([x, 2 * x], 1)
    out.append(_case("fully collinear", line, line + 1, no_model=True))
    return out


def family_limits():
    src, dst = synth(21, 500, 300)
    return [_case("max_iters %d confidence %g" % (mi, c), src, dst, max_iters=mi, confidence=c)
            for mi in (1, 50, 128, 129, 2000) for c in (0.9, 0.995)]


FAMILIES = dict(iters=family_iters, small_n=family_small_n, large=family_large, exact=family_exact, rejection=family_rejection,
                limits=family_limits)


def replay(case):
    return find_homography(case["src"], case["dst"], **case["kw"])


def check_expectations(case, est):
    """What a case was built for, asserted on the replay alone."""
    ex = case["expect"]
    if "iters" in ex:
        assert est.iters == ex["iters"], (case["name"], est.iters)
    if "draws_gt" in ex:
        assert est.draws > ex["draws_gt"], (case["name"], est.draws)
    if ex.get("no_model"):
        assert est.is_decided and not est.ok and est.iters == 0 and est.draws >= 40000 and not est.mask.any(), case["name"]


# ------------------------------------------------------------------------------------------------ the matcher batch
BATCH_SIZES = ((1920, 1080), (1921, 1081), (3840, 2160), (1280, 721), (1920, 1080), (1920, 1080))


BATCH_SEEDS = {(0, 1): 41, (0, 3): 43, (1, 3): 5, (3, 4): 49}      # seeds at which the replay of the pair, in the batch's match order, is decided


def _batch_blocks(seeds=None):
    """(i, j) -> centred (src, dst) of the correspondences the pair (i, j) shall have; sizes mixed from the families."""
    seeds = seeds or BATCH_SEEDS
    ident = np.random.default_rng(50).uniform(-500, 500, (300, 2)).astype(np.float32)
    five = synth(51, 12, 7, lim=300.0, noise=0.3, shuffle=False)
    return {
        (0, 1): synth(seeds[(0, 1)], 600, 60, noise=0.3),
        (0, 2): synth(42, 300, 165, noise=0.3),
        (0, 3): synth(seeds[(0, 3)], 2500, 500, lim=600.0, noise=0.3),
        (0, 4): synth(44, 5, 0, lim=300.0),                                    # below num_matches_thresh1
        (0, 5): (ident, ident),                                                # identical keypoints: confidence > 3 -> 0
        (1, 2): five,                                                          # 5 inliers of 12: below num_matches_thresh2
        (1, 3): _mostly_collinear(seeds[(1, 3)], 70, 6),
        (1, 4): synth(45, 33, 10, lim=300.0),
        (1, 5): synth(46, 8, 0, lim=300.0),
        (2, 3): synth(47, 7, 1, lim=300.0),
        (2, 4): _mirrored(2, 300, 100),
        (3, 4): synth(seeds[(3, 4)], 900, 450, lim=600.0),
        (3, 5): synth(49, 6, 0, lim=300.0),
        (4, 5): synth(52, 10, 3, lim=300.0),
    }                                                                          # (2, 5): no common point at all


def matcher_batch(seeds=None):
    """Six frames whose descriptors make every pair's match list one-to-one: each correspondence of a pair owns one random
    256-bit code, present in exactly its two frames (random codes lie ~128 +- 8 bits apart, so the ratio test accepts equal
    codes only).  -> dict(frames=[dict(size, xy float32 (n, 2), desc uint8 (n, 32))])."""
    rng = np.random.default_rng(60)
    xy = [[] for _ in BATCH_SIZES]
    desc = [[] for _ in BATCH_SIZES]
    for (i, j), (src, dst) in sorted(_batch_blocks(seeds).items()):
        codes = rng.integers(0, 256, (len(src), 32), dtype=np.uint8)
        for f, pts in ((i, src), (j, dst)):
            half = np.array([np.float32(BATCH_SIZES[f][0]) * np.float32(0.5), np.float32(BATCH_SIZES[f][1]) * np.float32(0.5)], np.float32)
            xy[f].append((np.asarray(pts, np.float32) + half).astype(np.float32))
            desc[f].append(codes)
    frames = []
    for f, size in enumerate(BATCH_SIZES):
        order = rng.permutation(sum(len(a) for a in xy[f]))
        frames.append(dict(size=size, xy=np.concatenate(xy[f])[order], desc=np.concatenate(desc[f])[order]))
    return dict(frames=frames)


def batch_reference(batch):
    """(i, j), i < j -> PairInfo with .matches, the match list by the pinned 2-NN reference of tests/refimpl.py."""
    import refimpl
    fr = batch["frames"]
    blocks = _batch_blocks()
    out = {}
    for i in range(len(fr)):
        for j in range(i + 1, len(fr)):
            m = refimpl.best_of_2_nearest_matches(fr[i]["desc"], fr[j]["desc"], 0.32).astype(DMATCH_DTYPE)
            assert len(m) == len(blocks.get((i, j), ((), ()))[0]), (i, j, len(m))
            assert len(set(m["query_idx"])) == len(m) == len(set(m["train_idx"])), "the match list must be one-to-one"
            info = matches_info(m, fr[i]["xy"], fr[i]["size"], fr[j]["xy"], fr[j]["size"])
            info.matches = m
            out[(i, j)] = info
    return out


def batch_gate(batch, infos, cap=0.10):
    und = [k for k, v in infos.items() if not v.is_decided]
    weak = [k for k, v in infos.items() if v.is_decided and v.has_H and v.final.n > 4 and (not v.final.fast or v.final.near_start)]
    assert len(und) + len(weak) <= cap * len(infos), ("undecided", [(k, infos[k].decided) for k in und], "cost only", weak)
    assert any(v.is_decided and v.has_H for v in infos.values())
    # what the batch was built for
    assert len(infos[(0, 4)].matches) == 5 and not infos[(0, 4)].has_H and infos[(0, 4)].first is None                 # below thresh1
    assert infos[(1, 2)].is_decided and infos[(1, 2)].has_H and infos[(1, 2)].num_inliers == 5 and infos[(1, 2)].second is None
    assert infos[(0, 5)].num_inliers == 300 and infos[(0, 5)].confidence == 0.0 and infos[(0, 5)].has_H                # > 3 -> 0
    assert infos[(2, 3)].num_inliers == 6 and infos[(4, 5)].num_inliers == 7 and infos[(0, 1)].num_inliers > 500 and infos[(0, 3)].num_inliers > 1900


def check_batch(batch, infos, entries):
    """entries: n * n dicts (src, dst, matches, inliers_mask, num_inliers, H or None, confidence), row-major, as one matcher call
    returned them.  -> the largest |H - H*| over the pairs whose parameters were compared."""
    n = len(batch["frames"])
    worst = 0.0
    for i in range(n):
        assert entries[i * n + i]["src"] == -1 and len(entries[i * n + i]["matches"]) == 0
    for (i, j), info in infos.items():
        a, b = entries[i * n + j], entries[j * n + i]
        assert (a["src"], a["dst"], b["src"], b["dst"]) == (i, j, j, i)
        got = np.asarray(a["matches"])
        for fld in ("query_idx", "train_idx", "img_idx", "distance"):
            assert np.array_equal(got[fld], info.matches[fld]), (i, j, fld)
        back = np.asarray(b["matches"])
        assert np.array_equal(back["query_idx"], got["train_idx"]) and np.array_equal(back["train_idx"], got["query_idx"])
        if not info.is_decided:
            continue
        for e in (a, b):
            assert np.asarray(e["inliers_mask"], np.uint8).tobytes() == info.mask.tobytes(), (i, j)
            assert e["num_inliers"] == info.num_inliers, (i, j, e["num_inliers"], info.num_inliers)
            assert e["confidence"] == info.confidence, (i, j, e["confidence"], info.confidence)
            assert (e["H"] is not None) == info.has_H, (i, j)
        if not info.has_H:
            continue
        H = np.asarray(a["H"], np.float64).reshape(3, 3)
        assert np.isfinite(H).all() and abs(H[2, 2] - 1.0) <= DBL_EPSILON
        try:
            res = check_tail(info.final, H)
        except AssertionError as err:
            raise AssertionError("pair (%d, %d): %s" % (i, j, err)) from err
        if res["kind"] == "params":
            worst = max(worst, res["dH"])
        Href = info.final.Hstar if info.final.Hstar is not None else info.final.H4
        assert np.linalg.cond(Href) < 1e4, (i, j, np.linalg.cond(Href))
        P = np.asarray(b["H"], np.float64).reshape(3, 3) @ H
        assert np.abs(P / P[2, 2] - np.eye(3)).max() <= 1e-9, (i, j, P)
    return worst
