"""Independent reference of cv::estimateAffinePartial2D(src, dst, mask, RANSAC, ...) and of the MatchesInfo that
cv::detail::AffineBestOf2NearestMatcher(full_affine = false) builds from a match list, written from OpenCV's documented
semantics (calib3d ptsetreg.cpp, stitching matchers.cpp, core RNG) in plain numpy / Python.  It imports the RNG and the
constants of tests/refimpl_homography.py and nothing of the product or the oracle, and takes a different numerical road wherever
the road is not part of the semantics.

The reading
-----------
* RANSACPointSetRegistrator with modelPoints = 2; cv::RNG seeded with (uint64)-1 for every call.
* getSubset: two indices, the second redrawn while it equals the first.  [uncertain] checkSubset: Affine2DEstimatorCallback's
  collinearity test looks at triples only, so with two points every subset is accepted.
* n < 2: no model.  n == 2: the model of both points, a mask of all ones, no refinement.  n > 2: the loop --
  niters = max(max_iters, 1); a model replaces the best when good > max(max_good, 1), strictly; then
  niters = RANSACUpdateNumIters(confidence, (n - good) / n, 2, niters) (refimpl_homography.update_num_iters with exponent 2).
  A model exists when max_good > 0.
* Hypothesis: the similarity [a -b tx; b a ty] through the two correspondences.  Here: a + ib = (dX + i dY) / (dx + i dy) and the
  translation that maps the first point, in EXACT rational arithmetic on the float32 inputs (fractions.Fraction), each of the
  four numbers rounded once to float64 -- not the closed-form float64 expression of runKernel.  Coincident source points give no
  finite model: it has no inliers and still counts as an iteration.
* Inlier test: the model rounded to float32, a = F0 x + F1 y + F2 - X, b = F3 x + F4 y + F5 - Y in float32,
  a a + b b <= (float)(thresh thresh).
* Refinement (a model, n > 2, refine_iters > 0): the inliers compressed in order, LMSolver over (a, b, tx, ty) for at most
  refine_iters iterations.  The mask stays the RANSAC mask.
* MatchesInfo: the points are the keypoints AS THEY ARE, float32 (no shift by half the image size); fewer matches than
  num_matches_thresh1 -> nothing; no model -> confidence 0, num_inliers 0, no H; otherwise num_inliers = the mask's count and
  confidence = num_inliers / (8 + 0.3 matches) with NO "> 3" zeroing, no |det H| test, no second estimation; H is extended by
  the row (0, 0, 1); the entry (j, i) has the swapped matches, the same mask, count and confidence, and the inverse H.

The error model (stated once, not tuned to any test)
----------------------------------------------------
As in refimpl_homography, minus the division.  The reference evaluates e = dx^2 + dy^2 in float64 from the float32-rounded
model.  With u = 2^-24 a float32 evaluation differs by at most
    d(dx) = 4u (|F0 x| + |F1 y| + |F2|) + u |dx|
(each term of the sum passes at most three roundings, and one more for the float32 cast of a model reached by another road:
the cast of a float64 value a few ulps away may round to the neighbouring float32), d(dy) likewise, and
    band = 2 |dx| d(dx) + 2 |dy| d(dy) + 3u e.
A point with |e - t| <= band is "in the band"; each count is the interval [lo, hi] without / with the band points.

Undecided: "count straddles max", "point in band", "niters boundary", as in refimpl_homography.

The tail.  The problem is linear in (a, b, tx, ty): H* is the least-squares solution over the inliers (numpy.linalg.lstsq).
* cost: S(H*) (1 - 1e-12) <= S(H) <= S(M_ransac) (1 + 1e-12), with refimpl_homography's solver-residue slack
  n_inliers * (16 * 2^-52 * max|coordinate|)^2; S in extended precision.
* parameters: each within 2 * FLT_EPSILON of H* -- LMSolver's stop rule; on a linear problem its first undamped step lands on
  the minimiser.  "near start" as in refimpl_homography: where D0 = max|M_ransac - H*| lies in (2, 4) * FLT_EPSILON the first,
  damped step may already be below FLT_EPSILON and end the run, so the parameters are held to D0 there.
* exact: H[0][0] == H[1][1], H[0][1] == -H[1][0]; in a MatchesInfo the last row == (0, 0, 1); H_ji H_ij = I within 1e-9.

The hypothesis band (refine_iters = 0 and n == 2 return the RANSAC model itself): runKernel's expression takes each of its
operands through at most 8 float64 roundings, so each entry differs from the exact value by at most
8 * 2^-52 * d * sum|products of the expression| with the products as they stand in the expression (x1 y2, X1 y2, ... before their
differences): hypothesis_band below, from exact rationals.
"""
import math
from fractions import Fraction

import numpy as np

from refimpl_homography import DBL_MIN, DMATCH_DTYPE, FLT_EPSILON, Rng

DBL_EPSILON = 2.0 ** -52
U32 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the model
def _fr(v):
    return Fraction(float(v))


def hypothesis_exact(p1, P1, p2, P2):
    """The similarity through (p1 -> P1), (p2 -> P2), float32 points -> 2 x 3 float64 [a -b tx; b a ty], each entry the exact
    rational value rounded once; None when the source points coincide."""
    x1, y1, X1, Y1, x2, y2, X2, Y2 = (_fr(v) for v in (*p1, *P1, *p2, *P2))
    dx, dy, dX, dY = x1 - x2, y1 - y2, X1 - X2, Y1 - Y2
    den = dx * dx + dy * dy
    if den == 0:
        return None
    a, b = (dX * dx + dY * dy) / den, (dY * dx - dX * dy) / den
    tx, ty = X1 - a * x1 + b * y1, Y1 - b * x1 - a * y1
    a, b, tx, ty = float(a), float(b), float(tx), float(ty)
    return np.array([[a, -b, tx], [b, a, ty]], np.float64)


def hypothesis_band(p1, P1, p2, P2):
    """Per entry of the 2 x 3 model: the largest distance of runKernel's float64 expression from the exact value."""
    x1, y1, X1, Y1, x2, y2, X2, Y2 = (abs(_fr(v)) for v in (*p1, *P1, *p2, *P2))
    fx1, fy1, fx2, fy2 = (_fr(v) for v in (*p1, *p2))
    den = (fx1 - fx2) ** 2 + (fy1 - fy2) ** 2
    sx, sy, sX, sY = x1 + x2, y1 + y2, X1 + X2, Y1 + Y2          # |differences| bounded by the sums of magnitudes
    m0 = sX * sx + sY * sy
    m2 = sY * (x1 * y2 + x2 * y1) + (X1 * y2 + X2 * y1) * sy + (X1 * x2 + X2 * x1) * sx
    m3 = sX * (x1 * y2 + x2 * y1) + (Y1 * x2 + Y2 * x1) * sx + (Y1 * y2 + Y2 * y1) * sy
    k = 8 * DBL_EPSILON
    b0, b2, b3 = (k * float(m / den) for m in (m0, m2, m3))
    return np.array([[b0, b0, b2], [b0, b0, b3]])


def inlier_intervals(M, src, dst, t):
    """-> (sure, maybe) for the 2 x 3 model M (None: no finite model, no inliers)."""
    n = len(src)
    if M is None or not np.isfinite(M).all():
        return np.zeros(n, bool), np.zeros(n, bool)
    F = np.asarray(M, np.float64).reshape(6).astype(np.float32).astype(np.float64)
    x, y = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64)
    with np.errstate(all="ignore"):
        dx = F[0] * x + F[1] * y + F[2] - dst[:, 0]
        dy = F[3] * x + F[4] * y + F[5] - dst[:, 1]
        e = dx * dx + dy * dy
        ddx = 4 * U32 * (np.abs(F[0] * x) + np.abs(F[1] * y) + abs(F[2])) + U32 * np.abs(dx)
        ddy = 4 * U32 * (np.abs(F[3] * x) + np.abs(F[4] * y) + abs(F[5])) + U32 * np.abs(dy)
        band = 2 * np.abs(dx) * ddx + 2 * np.abs(dy) * ddy + 3 * U32 * e
        bad = ~np.isfinite(e) | ~np.isfinite(band)
        sure = (e < t - band) & ~bad
        maybe = (np.abs(e - t) <= band) & ~bad
    return sure, maybe


def update_num_iters(p, ep, max_iters, exponent=2):
    """RANSACUpdateNumIters(p, ep, 2, max_iters) -> (niters, near_boundary).  (exponent: only for the tests that show a case tells
    the model's exponent from the homography's 4.)"""
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** exponent
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


def params_of(M):
    M = np.asarray(M, np.float64).reshape(-1)
    return np.array([M[0], M[3], M[2], M[5]])


def cost(M, s, d):
    """S(M): the squared error summed over the correspondences, in extended precision."""
    a, b, tx, ty = (np.longdouble(v) for v in params_of(M))
    x, y, X, Y = (np.asarray(v, np.longdouble) for v in (s[:, 0], s[:, 1], d[:, 0], d[:, 1]))
    rx, ry = a * x - b * y + tx - X, b * x + a * y + ty - Y
    return float((rx * rx + ry * ry).sum())


def least_squares(s, d):
    """The minimiser of S over (a, b, tx, ty) -> 2 x 3."""
    s, d = np.asarray(s, np.float64), np.asarray(d, np.float64)
    c = s.mean(0)                                                               # centred columns: a well-conditioned system
    x, y = s[:, 0] - c[0], s[:, 1] - c[1]
    J = np.zeros((2 * len(s), 4))
    J[0::2, 0], J[0::2, 1], J[0::2, 2] = x, -y, 1.0
    J[1::2, 0], J[1::2, 1], J[1::2, 3] = y, x, 1.0
    r = np.empty(2 * len(s))
    r[0::2], r[1::2] = d[:, 0], d[:, 1]
    a, b, u, v = np.linalg.lstsq(J, r, rcond=None)[0]
    tx, ty = u - a * c[0] + b * c[1], v - b * c[0] - a * c[1]
    return np.array([[a, -b, tx], [b, a, ty]], np.float64)


# ------------------------------------------------------------------------------------------------ estimateAffinePartial2D
class Estimate:
    """What the replay found.  decided: True or the reason.  ok, mask, iters, draws; for ok: M_ransac (the winning model), band
    (its hypothesis band); for ok with n > 2: Hstar, D0, near_start, inl_src / inl_dst."""

    def __init__(self, n):
        self.n, self.decided, self.ok = n, True, False
        self.mask = np.zeros(n, np.uint8)
        self.iters = self.draws = 0
        self.M_ransac = self.band = self.Hstar = None
        self.D0, self.near_start = 0.0, False
        self.inl_src = self.inl_dst = self.src = self.dst = None
        self.refine_iters = 10

    @property
    def is_decided(self):
        return self.decided is True


def estimate_affine_partial(src, dst, thresh=3.0, max_iters=2000, confidence=0.99, refine_iters=10, exponent=2):
    src, dst = np.ascontiguousarray(src, np.float32).reshape(-1, 2), np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    n = len(src)
    est = Estimate(n)
    est.src, est.dst, est.refine_iters = src, dst, refine_iters
    if thresh <= 0:
        thresh = 3.0
    if n < 2:
        return est
    if n == 2:
        est.ok = True
        est.M_ransac = hypothesis_exact(src[0], dst[0], src[1], dst[1])      # (None: coincident points, runKernel's 1 / 0)
        if est.M_ransac is not None:
            est.band = hypothesis_band(src[0], dst[0], src[1], dst[1])
        est.mask[:] = 1
        return est
    t = float(np.float32(thresh * thresh))
    rng = Rng()
    niters, max_good, it = max(max_iters, 1), 0, 0
    best = best_idx = None
    while it < niters:
        i0 = rng.uniform(0, n)
        i1 = rng.uniform(0, n)
        while i1 == i0:
            i1 = rng.uniform(0, n)
        it += 1
        est.iters = it
        M = hypothesis_exact(src[i0], dst[i0], src[i1], dst[i1])
        sure, maybe = inlier_intervals(M, src, dst, t)
        lo, hi = int(sure.sum()), int(sure.sum() + maybe.sum())
        bar = max(max_good, 1)
        if hi <= bar:
            continue
        if lo <= bar:
            est.decided, est.draws = "count straddles max", rng.draws
            return est
        if hi != lo:
            est.decided, est.draws = "point in band", rng.draws
            return est
        best, best_idx, max_good, est.M_ransac = sure, (i0, i1), lo, M
        niters, near = update_num_iters(confidence, (n - lo) / n, niters, exponent)
        if near:
            est.decided, est.draws = "niters boundary", rng.draws
            return est
    est.draws = rng.draws
    if max_good <= 0:
        return est
    est.ok = True
    est.mask = best.astype(np.uint8)
    i0, i1 = best_idx
    est.band = hypothesis_band(src[i0], dst[i0], src[i1], dst[i1])
    est.inl_src, est.inl_dst = src[best], dst[best]
    est.Hstar = least_squares(est.inl_src, est.inl_dst)
    est.D0 = float(np.abs(params_of(est.M_ransac) - params_of(est.Hstar)).max())
    est.near_start = 2 * FLT_EPSILON < est.D0 < 4 * FLT_EPSILON
    return est


# ------------------------------------------------------------------------------------------------ MatchesInfo
class PairInfo:
    def __init__(self):
        self.decided, self.has_H, self.num_inliers, self.confidence = True, False, 0, 0.0
        self.mask = np.zeros(0, np.uint8)
        self.est = None

    @property
    def is_decided(self):
        return self.decided is True


def matches_info(matches, xy1, xy2, thresh1=6):
    out = PairInfo()
    nm = len(matches)
    if nm < thresh1:
        return out
    sp = np.asarray(xy1, np.float32)[matches["query_idx"]]
    dp = np.asarray(xy2, np.float32)[matches["train_idx"]]
    e = out.est = estimate_affine_partial(sp, dp)
    if not e.is_decided:
        out.decided = e.decided
        return out
    out.mask = e.mask.copy()
    if not e.ok:
        return out
    out.has_H = True
    out.num_inliers = int(e.mask.sum())
    out.confidence = out.num_inliers / (8 + 0.3 * nm)
    return out


# ------------------------------------------------------------------------------------------------ the assertions
def check_estimate(est, ok, M, mask):
    """Hold one result (ok, M 2 x 3 float64, mask uint8) to a DECIDED Estimate -> dict(kind, dH)."""
    assert est.is_decided
    assert bool(ok) == est.ok, (ok, est.ok)
    assert np.asarray(mask, np.uint8).tobytes() == est.mask.tobytes(), np.nonzero(np.asarray(mask) != est.mask)[0][:8]
    if not est.ok:
        return dict(kind="none", dH=None)
    M = np.asarray(M, np.float64).reshape(2, 3)
    if est.M_ransac is None:                                                    # n == 2 with coincident points: runKernel's 1 / 0
        assert not np.isfinite(M).all(), M
        return dict(kind="none", dH=None)
    assert np.isfinite(M).all(), M
    assert M[0, 0] == M[1, 1] and M[0, 1] == -M[1, 0], M
    return check_tail(est, M)


def check_tail(est, M):
    if est.n == 2 or est.refine_iters == 0:
        dM = np.abs(M - est.M_ransac)
        assert (dM <= est.band + 4 * DBL_EPSILON * np.abs(est.M_ransac)).all(), ("outside the hypothesis band", dM, est.band)
        return dict(kind="ransac", dH=float(dM.max()))
    s, d = est.inl_src, est.inl_dst
    S, S0, Sstar = cost(M, s, d), cost(est.M_ransac, s, d), cost(est.Hstar, s, d)
    dH = float(np.abs(params_of(M) - params_of(est.Hstar)).max())
    rho = 16 * DBL_EPSILON * float(max(np.abs(s).max(), np.abs(d).max()))
    slack = len(s) * rho * rho
    assert S <= S0 * (1 + 1e-12) + slack, ("the refinement increased the cost", S, S0)
    assert S >= Sstar * (1 - 1e-12) - slack, ("below the minimiser's cost", S, Sstar)
    if est.near_start:
        assert dH <= est.D0, (dH, est.D0, M, est.Hstar)
        return dict(kind="near start", dH=dH)
    assert dH <= 2 * FLT_EPSILON, (dH, M, est.Hstar)
    return dict(kind="params", dH=dH)


def family_gate(name, ests, cap=0.10):
    """At most `cap` of a family's cases undecided (or near start), at least one decided case with a model."""
    und = [e for e in ests if not e.is_decided]
    weak = [e for e in ests if e.is_decided and e.ok and e.near_start]
    assert len(und) + len(weak) <= cap * len(ests), (name, "undecided", [e.decided for e in und], "near start", len(weak), "of", len(ests))
    assert any(e.is_decided and e.ok for e in ests), name
    return len(ests) - len(und), len(weak)


# ------------------------------------------------------------------------------------------------ input families
SIM_BASE = (0.98, 0.05, 25.0, -14.0)        # a, b, tx, ty


def _apply(sim, p):
    a, b, tx, ty = sim
    p = np.asarray(p, np.float64)
    return np.stack([a * p[:, 0] - b * p[:, 1] + tx, b * p[:, 0] + a * p[:, 1] + ty], 1)


def synth(seed, n, n_out, lo=-900.0, hi=900.0, noise=0.3, sim=SIM_BASE):
    """n float32 correspondences under a similarity with Gaussian noise on the destination; n_out of them get a uniform random
    destination instead; shuffled."""
    rng = np.random.default_rng(seed)
    src = rng.uniform(lo, hi, (n, 2)).astype(np.float32)
    dst = _apply(sim, src) + rng.normal(0, noise, (n, 2))
    dst[:n_out] = rng.uniform(lo, hi, (n_out, 2))
    order = rng.permutation(n)
    return src[order], dst.astype(np.float32)[order]


def _case(name, src, dst, **expect):
    kw = {k: expect.pop(k) for k in ("thresh", "max_iters", "confidence", "refine_iters") if k in expect}
    return dict(name=name, src=np.ascontiguousarray(src, np.float32).reshape(-1, 2), dst=np.ascontiguousarray(dst, np.float32).reshape(-1, 2), kw=kw, expect=expect)


# The seed tables hold seeds at which the replay is decided and lands where the comment says.  After a change to a generator
# re-derive them with the replay alone: pick (n, inliers) with update_num_iters(0.99, (n - inliers) / n, 2000) equal to the wanted
# count, loop the seed, keep the first whose Estimate is decided with the wanted iters.
# (n, outliers, seed, iteration count of the replay): a single digit, both sides of the boundary between the two phases of the
# device loop (127, 128, 129), a few hundred, and the full 2000 (300 points with 14 inliers)
ITER_REGIMES = ((300, 96, 1, 7), (302, 245, 1, 127), (303, 246, 1, 128), (304, 247, 1, 129), (317, 279, 1, 318), (300, 286, 1, 2000))


def family_iters():
    return [_case("iters n%d out%d seed%d" % (n, no, seed), *synth(seed, n, no), iters=it) for n, no, seed, it in ITER_REGIMES]


SMALL_N = ((0, 0, 1), (1, 0, 2), (2, 0, 3), (3, 0, 4), (3, 1, 5), (5, 0, 6), (5, 2, 7), (6, 0, 8), (6, 2, 9))


def family_small_n():
    return [_case("n%d out%d" % (n, no), *synth(seed, n, no, lo=-300.0, hi=300.0)) for n, no, seed in SMALL_N]


EDGE_N = (63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)
def family_edges():
    """The wave and the workgroup / tile edges of the kernels."""
    return [_case("n%d" % n, *synth(1, n, n // 3)) for n in EDGE_N]


LARGE_SEED = 1


def family_large():
    return [_case("n8000 uncentred", *synth(LARGE_SEED, 8000, 3000, lo=0.0, hi=3840.0)),
            _case("n2500 centred", *synth(2, 2500, 1000, lo=-1920.0, hi=1920.0)),
            _case("n2000 uncentred", *synth(3, 2000, 600, lo=0.0, hi=3840.0)),
            _case("n40 outlier-heavy", *synth(4, 40, 36))]


def _lattice(seed, n, no):
    """Integer points under an integer similarity (a, b) = (2, 1): every error of the true model is exactly 0."""
    rng = np.random.default_rng(seed)
    src = rng.integers(-500, 501, (n, 2)).astype(np.float64)
    dst = _apply((2.0, 1.0, 7.0, -11.0), src)
    dst[:no] = rng.integers(-1500, 1501, (no, 2))
    order = rng.permutation(n)
    return src[order], dst[order]


def _coincident(seed, n, n_heap):
    """n_heap correspondences share one source point: a subset of two of them has no finite model."""
    src, dst = synth(seed, n, n // 4)
    src = src.copy()
    src[:n_heap] = (17.0, -33.0)
    return src, dst


def family_exact():
    out = [_case("lattice seed%d n%d out%d" % (seed, n, no), *_lattice(seed, n, no)) for seed, n, no in ((1, 60, 0), (2, 200, 50), (3, 500, 250))]
    out += [_case("coincident seed%d n%d heap%d" % (seed, n, k), *_coincident(seed, n, k)) for seed, n, k in ((4, 40, 30), (5, 300, 150), (6, 12, 10))]
    one = np.tile(np.array([[5.0, 6.0]], np.float32), (20, 1))
    out.append(_case("all coincident", one, synth(7, 20, 0)[1], no_model=True))
    out.append(_case("n2 coincident", one[:2], synth(8, 2, 0)[1]))
    return out


def family_params():
    src, dst = synth(21, 400, 340)
    out = [_case("max_iters %d confidence %g" % (mi, c), src, dst, max_iters=mi, confidence=c) for mi in (1, 5, 2000) for c in (0.5, 0.99, 0.999999)]
    out += [_case("refine_iters 0 %s" % nm, s, d, refine_iters=0) for nm, (s, d) in (("n400", (src, dst)), ("n2500", synth(22, 2500, 1000, lo=-1920.0, hi=1920.0)))]
    return out


# (n, outliers, noise, seed): inlier noise of 1.2 - 1.5 px against the 3 px threshold, so that hypotheses differ in their counts and
# points sit near the threshold.  Seeds at which the replay is decided AND (a) the loop with exponent 4 runs on to a strictly
# better later model (another mask), (b) so does the loop with confidence 0.995, (c) the mask of the refined model H* differs from
# the RANSAC mask in points outside the band.  A device loop with the wrong exponent, confidence or stop, or a mask recomputed
# after the refinement, fails the byte comparison on these.  Re-derive with the replay alone: loop the seed, keep the first with
# all three properties (check_expectations asserts them).
SENSITIVE = ((200, 120, 1.2, 12), (400, 280, 1.2, 2), (150, 60, 1.5, 10), (1200, 700, 1.2, 8))


def family_sensitive():
    return [_case("sensitive n%d out%d noise%g seed%d" % (n, no, noise, seed), *synth(seed, n, no, noise=noise), sensitive=True)
            for n, no, noise, seed in SENSITIVE]


def refined_mask_flips(est):
    """How many points the float32 mask of the refined model H* decides otherwise than the RANSAC mask, band points left out."""
    sure, maybe = inlier_intervals(est.Hstar, est.src, est.dst, float(np.float32(9.0)))
    m = est.mask.astype(bool)
    return int(((sure & ~m) | (~sure & ~maybe & m)).sum())


FAMILIES = dict(sensitive=family_sensitive, iters=family_iters, small_n=family_small_n, edges=family_edges, large=family_large, exact=family_exact, params=family_params)


def replay(case):
    return estimate_affine_partial(case["src"], case["dst"], **case["kw"])


def check_expectations(case, est):
    ex = case["expect"]
    if "iters" in ex:
        assert est.is_decided and est.iters == ex["iters"], (case["name"], est.decided, est.iters)
    if ex.get("sensitive"):
        assert est.is_decided and est.ok and not est.near_start, (case["name"], est.decided)
        e4 = estimate_affine_partial(case["src"], case["dst"], exponent=4)
        ec = estimate_affine_partial(case["src"], case["dst"], confidence=0.995)
        assert e4.is_decided and e4.iters > est.iters and (e4.mask != est.mask).any(), (case["name"], "exponent 4 does not show")
        assert ec.is_decided and ec.iters > est.iters and (ec.mask != est.mask).any(), (case["name"], "confidence 0.995 does not show")
        assert refined_mask_flips(est) > 0, (case["name"], "the refined model's mask equals the RANSAC mask")
    if ex.get("no_model"):
        assert est.is_decided and not est.ok and not est.mask.any(), case["name"]


# ------------------------------------------------------------------------------------------------ the matcher batch
BATCH_SIZES = ((1920, 1080), (1921, 1081), (3840, 2160), (1280, 721), (1920, 1080), (1920, 1080))
BATCH_SEEDS = {(0, 1): 41, (0, 3): 43, (1, 3): 45, (2, 4): 47}


def _batch_blocks():
    """(i, j) -> (src, dst) keypoint positions (uncentred: 0 .. 1900) of the correspondences the pair shall have."""
    ident = np.random.default_rng(50).uniform(0, 1000, (300, 2)).astype(np.float32)
    kw = dict(lo=0.0, hi=1900.0)
    return {
        (0, 1): synth(BATCH_SEEDS[(0, 1)], 100, 40, **kw),
        (0, 2): synth(42, 6, 0, **kw),
        (0, 3): synth(BATCH_SEEDS[(0, 3)], 2500, 1000, **kw),
        (0, 4): synth(44, 5, 0, **kw),                                         # below num_matches_thresh1: matches only
        (0, 5): (ident, ident),                                                # identical frames: confidence > 3, NOT zeroed
        (1, 3): synth(BATCH_SEEDS[(1, 3)], 110, 80, **kw),
        (1, 4): synth(46, 33, 10, **kw),
        (2, 4): synth(BATCH_SEEDS[(2, 4)], 300, 90, **kw),
        (3, 5): synth(48, 8, 3, **kw),
    }


def matcher_batch():
    """Six frames whose descriptors make every pair's match list one-to-one (refimpl_homography.matcher_batch's construction:
    one random 256-bit code per correspondence, present in exactly its two frames); keypoints at the positions as they are."""
    rng = np.random.default_rng(60)
    xy = [[] for _ in BATCH_SIZES]
    desc = [[] for _ in BATCH_SIZES]
    for (i, j), (src, dst) in sorted(_batch_blocks().items()):
        codes = rng.integers(0, 256, (len(src), 32), dtype=np.uint8)
        for f, pts in ((i, src), (j, dst)):
            xy[f].append(np.asarray(pts, np.float32))
            desc[f].append(codes)
    frames = []
    for f, size in enumerate(BATCH_SIZES):
        order = rng.permutation(sum(len(a) for a in xy[f]))
        frames.append(dict(size=size, xy=np.concatenate(xy[f])[order], desc=np.concatenate(desc[f])[order]))
    return dict(frames=frames)


def batch_reference(batch, match_conf=0.3):
    """(i, j), i < j -> PairInfo with .matches, the match list by the pinned 2-NN reference of tests/refimpl.py."""
    import refimpl
    fr = batch["frames"]
    blocks = _batch_blocks()
    out = {}
    for i in range(len(fr)):
        for j in range(i + 1, len(fr)):
            m = refimpl.best_of_2_nearest_matches(fr[i]["desc"], fr[j]["desc"], match_conf).astype(DMATCH_DTYPE)
            assert len(m) == len(blocks.get((i, j), ((), ()))[0]), (i, j, len(m))
            info = matches_info(m, fr[i]["xy"], fr[j]["xy"])
            info.matches = m
            out[(i, j)] = info
    return out


def batch_gate(batch, infos, cap=0.10):
    und = [k for k, v in infos.items() if not v.is_decided]
    weak = [k for k, v in infos.items() if v.is_decided and v.has_H and v.est.near_start]
    assert len(und) + len(weak) <= cap * len(infos), ("undecided", [(k, infos[k].decided) for k in und], "near start", weak)
    # what the batch was built for
    assert len(infos[(0, 4)].matches) == 5 and not infos[(0, 4)].has_H and infos[(0, 4)].est is None and len(infos[(0, 4)].mask) == 0
    assert len(infos[(0, 2)].matches) == 6 and infos[(0, 2)].has_H
    assert len(infos[(0, 1)].matches) == 100 and len(infos[(0, 3)].matches) == 2500 and infos[(0, 3)].num_inliers > 1400
    assert infos[(0, 5)].num_inliers == 300 and infos[(0, 5)].confidence == 300 / (8 + 0.3 * 300) > 3      # NOT zeroed


def check_batch(batch, infos, entries):
    """entries: n * n dicts (src, dst, matches, inliers_mask, num_inliers, H or None, confidence), row-major, as one matcher call
    returned them.  -> the largest parameter distance from H* over the pairs whose parameters were compared."""
    n = len(batch["frames"])
    worst = 0.0
    for i in range(n):
        assert entries[i * n + i]["src"] == -1 and len(entries[i * n + i]["matches"]) == 0
    for i in range(n):
        for j in range(i + 1, n):
            if (i, j) in infos and len(infos[(i, j)].matches):
                continue
            for e in (entries[i * n + j], entries[j * n + i]):                 # a pair without a common point: matched, nothing found
                assert len(e["matches"]) == 0 and e["H"] is None and e["num_inliers"] == 0 and e["confidence"] == 0
    for (i, j), info in infos.items():
        if not len(info.matches):
            continue
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
        assert np.isfinite(H).all() and (H[2] == (0.0, 0.0, 1.0)).all(), (i, j, H)
        assert H[0, 0] == H[1, 1] and H[0, 1] == -H[1, 0], (i, j, H)
        try:
            res = check_tail(info.est, H[:2])
        except AssertionError as err:
            raise AssertionError("pair (%d, %d): %s" % (i, j, err)) from err
        if res["kind"] == "params":
            worst = max(worst, res["dH"])
        P = np.asarray(b["H"], np.float64).reshape(3, 3) @ H
        assert np.abs(P - np.eye(3)).max() <= 1e-9, (i, j, P)
    return worst
