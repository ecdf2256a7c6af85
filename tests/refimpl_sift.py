"""Plain numpy reference of SIFT detect + describe (cv::SIFT::create(nfeatures 0, nOctaveLayers, contrastThreshold, edgeThreshold,
sigma)->detectAndCompute of OpenCV 4.5+: float scale space, firstOctave = -1), written from OpenCV's documented semantics.

Nothing here calls the oracle (oracle/mo_sift.c) or the product library: both are checked against these functions, so a misreading
of OpenCV that the kernels and the oracle share shows up as a disagreement with this module.  Where the oracle's C walks loops the
stages here take another road: separable convolutions as sums of shifted arrays, array maxima / minima for the 26 neighbours,
numpy.linalg.solve for the refinement, one vectorised walk for all candidates of an octave, scatter-adds for the histograms,
sorting for the order.

STAGING.  Every stage starts from the TESTED side's own output of the previous stage (its float32 Gaussian / DoG images, its
keypoints), so float32 error does not accumulate through the pyramid and every band is the error of one stage.  u = 2^-24.  A single
IEEE float32 operation on given float32 inputs (one subtraction, 360 - angle, x * 2^k, cvRound of such a value) is reproduced
exactly with numpy float32; decisions on such results are exact and carry no band.

Reading of OpenCV, stage by stage:
  1 gray: (B 3735 + G 19235 + R 9798 + 2^14) >> 15 (the reading refimpl_orb.py states).  Exact.
  2 base image: resize to 2w x 2h, INTER_LINEAR on float: source coordinate (d + 0.5) / 2 - 0.5 clamped at both ends, i.e. weights
    0.25 / 0.75 on edge-replicated neighbours; the inputs are bytes, so the result is exact in float32.  Then GaussianBlur with
    sqrt(max(sigma^2 - 4 * 0.25, 0.01)) (float32 chain, as createInitialImage computes it).
  3 taps: ksize = cvRound(8 s + 1) | 1, UNCAPPED; exp(-x^2 / 2 s^2) normalised in float64, rounded to float32.  Incremental sigmas
    sig[i] = sqrt((sigma k^i)^2 - (sigma k^(i-1))^2), k = 2^(1/nl).  nOctaves = cvRound(log2(min(2w, 2h)) - 2) + 1.
  4 Gaussian level from the given previous level: separable, BORDER_REFLECT_101 folded with period 2 (len - 1) (an octave can be
    narrower than the kernel: many folds), evaluated in float64.
  5 octave base: every second pixel of level nl of the previous octave.  Exact.
  6 DoG: one float32 subtraction of the two given levels.  Exact.
  7 candidates: 5 <= r < h - 5, 5 <= c < w - 5, DoG layers 1 .. nl, |val| > floor(0.5 contrast / nl * 255), val >= all 26
    neighbours when val > 0, else val <= all 26 (ties are extrema).  Comparisons of given float32 values: the set is EXACT.
  8 adjustLocalExtrema on the given DoG: at most 5 steps; derivative scales 1/255 * {1/2, 1, 1/4}; offset -H^-1 g
    (Matx33f::solve: closed form through the determinant, zeros when it is 0); stop when all |offset| < 0.5; reject when an
    |offset| > (float)(INT_MAX / 3); move by cvRound; reject when the layer leaves [1, nl] or the point enters the 5-pixel border;
    after the loop contr = D / 255 + 1/2 g.x, reject |contr| nl < (float)contrastThreshold; reject det <= 0 or
    tr^2 e >= (e + 1)^2 det.
  9 fields: pt = (c + xc, r + xr) 2^octv; size = sigma 2^((layer + xi) / nl) 2^octv 2; response = |contr|;
    octave = octv + (layer << 8) + (cvRound((xi + 0.5) 255) << 16).
 10 orientation on the given Gaussian level `layer`: scl = size / 2 / 2^octv, radius = cvRound(4.5 scl), weight
    exp(-(i^2 + j^2) / (2 (1.5 scl)^2)), samples with 0 < y < h - 1, 0 < x < w - 1, ori = fastAtan2(dy, dx) (degrees, the 7th-order
    polynomial, float64 here as in refimpl_orb.py), bin = cvRound(36 / 360 ori) wrapped, smoothing 1 4 6 4 1 over 16, a peak is
    strictly above both neighbours and >= 0.8 max; parabolic interpolation, angle = 360 - 10 bin, |angle - 360| < FLT_EPSILON -> 0.
 11 duplicates, stated independently: two raw keypoints are the same when they come from the same final (octave, layer, r, c) and
    the same histogram peak.  Order KeyPoint_LessThan: x, y ascending, size descending, angle ascending, response and octave
    descending.  firstOctave = -1: point and size * 0.5, low byte of the octave field decremented mod 256.
 12 descriptor of a GIVEN keypoint (float32 x, y, size, angle, packed octave) on the given Gaussian level: unpack, scale back (exact),
    centre cvRound(pt), ori = 360 - angle (-> 0 within FLT_EPSILON of 360), hist_width = 3 scl,
    radius = min(cvRound(hist_width sqrt2 5 0.5), (int)sqrt(w^2 + h^2)) in float32 in that order (it feeds an integer); samples with
    -1 < rbin, cbin < 4 inside the image's interior; weight exp(-(c_rot^2 + r_rot^2) / 8); trilinear split into 6 x 6 x 10 with the
    circular fold of the orientation slots; clip at 0.2 norm, scale 512 / max(norm, FLT_EPSILON), saturate_cast<uchar>.  Returned:
    the UNROUNDED scaled value per element with its band; the check is |got - value| <= 0.5 + band on all 128 elements.  The
    histogram is continuous in everything but the integer centre and radius, both exact: no element is undecided.

ERROR MODEL (derived once here, not tuned to any test).  First order; a banded quantity is a pair (value in float64, bound on the
tested side's float32 deviation from it):
  * a float32 sequential sum of n products: (n + 1) u sum |t_k v_k| (one rounding per product, n - 1 additions, one spare for the
    first-order truncation).  Blur: the row pass's band is propagated through the column taps (sum t_k band_row) and the column
    pass adds its own (n + 1) u sum t_k (|row| + band_row).
  * every other float32 operation adds u |result| to the propagated bands of its operands: sum e_a + e_b; product
    |a| e_b + |b| e_a; quotient (e_a + |a / b| e_b) / |b|.  The closed-form 3 x 3 solve is carried through these rules (numerator and
    denominator bands, then (dN + |x| dD) / |D|), its value comes from numpy.linalg.solve.  Exact operations (times a power of two,
    integer plus float with a representable sum excepted: that one rounds) add nothing.
  * the shared exponential polynomial: 2e-7 relative (test_oracle_kat.py::test_sift_helpers); sin / cos 3e-7 absolute
    (test_dev_math_cpu.py, which also holds mis_expf to the 2e-7); fastAtan2: refimpl_orb.fast_atan2_f64's band u (27 T + 1080) degrees; sqrt: u relative.
  * a branch on a banded quantity is DECIDED when its margin exceeds the band (or the band is 0: exact data, e.g. flat plateaus),
    otherwise the candidate (or the keypoint's orientation) is UNDECIDED, the reason recorded: `singular` (|det H| within its
    band), `converge` (an |offset| within its band of 0.5), `overflow`, `round` (an offset within its band of a half-integer
    where cvRound is taken), `contrast`, `edge`, and for orientations `radius` and `peak` (a peak comparison inside the bands).
    A sample of non-zero magnitude whose bin argument lies within its band of a half-integer may fall into either bin: its term is
    added to the bands of both, so it makes the orientation undecided only where it can change a peak (stating every such sample
    undecided outright would discard about 2.4e-5 * 2 * (2 radius + 1)^2 of the keypoints: 1 - 5 %, above the cap of 2 % that
    the orientation stage is held to).  The third octave byte is undecided when (xi + 0.5) 255 lies within its band of a
    half-integer.
  * an IEEE operation on exact operands whose exact result is representable in float32 adds no band: differences of equal or
    nearly equal pixels (Sterbenz), sums that cancel, products with zero.  Plateaus and ties of the DoG thus stay exact: a
    Hessian row that is exactly zero gives det = 0 exactly, which Matx33f::solve answers with zeros.
  * angle wrap: a bin within its band of 0 or 36 maps to an angle near 0 or near 360; angles are compared on the circle.
  * a library keypoint that no decided reference keypoint explains is attributed to an undecided orientation when it shares that
    keypoint's octave field and position, or else to an undecided candidate of its octave within 6 pixels of where the walk stood
    (at most 5 steps; an offset that close to a half moves one pixel; the layer may move as well).  A candidate ends at one
    position: each undecided candidate explains the keypoints of one (octave field, x, y) only, nearest first.
  * the tested side's counters: as many candidates as stage 7 finds (exact: this observes `>=` on ties and every append path of
    the scan whether or not a tie survives the refinement), and as many refined candidates as stage 8 keeps, up to the undecided.
"""
import math

import numpy as np

from refimpl_orb import TRIG_ERR, U24, angle_dist, bgr2gray, fast_atan2_f64

F32 = np.float32
EXP_REL = 2e-7
BORDER = 5
MAX_STEPS = 5
ORI_BINS = 36
FLT_EPSILON = float(np.finfo(np.float32).eps)
BIG = float(F32((2 ** 31 - 1) // 3))
KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
REJECT_REASONS = ("layer", "border", "steps", "contrast", "edge_det", "edge_ratio")      # `overflow` needs |offset| > 7e8


def params(n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6):
    return dict(n_octave_layers=int(n_octave_layers), contrast_threshold=float(contrast_threshold), edge_threshold=float(edge_threshold),
                sigma=float(sigma))


# ------------------------------------------------------------------------------------------------ stage 3
def gaussian_ksize(sigma):
    return int(np.rint(8.0 * sigma + 1.0)) | 1


def gaussian_taps(sigma):
    n = gaussian_ksize(sigma)
    x = np.arange(n, dtype=np.float64) - (n - 1) * 0.5
    t = np.exp(-(x * x) / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(F32)


def base_sigma(p):
    return float(np.sqrt(np.maximum(F32(p["sigma"] * p["sigma"]) - F32(0.5) * F32(0.5) * F32(4), F32(0.01))))


def incremental_sigmas(p):
    nl, s = p["n_octave_layers"], p["sigma"]
    k = 2.0 ** (1.0 / nl)
    return [s] + [math.sqrt((s * k ** i) ** 2 - (s * k ** (i - 1)) ** 2) for i in range(1, nl + 3)]


def max_ksize(p):
    return max([gaussian_ksize(base_sigma(p))] + [gaussian_ksize(s) for s in incremental_sigmas(p)[1:]])


def num_octaves(w, h):
    return int(np.rint(math.log2(min(2 * w, 2 * h)) - 2.0)) + 1


def octave_sizes(w, h):
    out, cw, ch = [], 2 * w, 2 * h
    for _ in range(num_octaves(w, h)):
        out.append((cw, ch))
        cw, ch = cw // 2, ch // 2
        if cw < 1 or ch < 1:
            break
    return out


# ------------------------------------------------------------------------------------------------ stages 2, 4
def upsample2x(gray):
    def axis(a):
        q = np.concatenate([a[..., :1], a, a[..., -1:]], -1)
        out = np.empty(a.shape[:-1] + (2 * a.shape[-1],))
        out[..., 0::2] = 0.25 * q[..., :-2] + 0.75 * q[..., 1:-1]
        out[..., 1::2] = 0.75 * q[..., 1:-1] + 0.25 * q[..., 2:]
        return out
    out = axis(axis(gray.astype(np.float64)).T).T
    assert np.array_equal(out, out.astype(F32))
    return out.astype(F32)


def reflect101(p, n):
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * (n - 1))
    return np.where(q < n, q, 2 * (n - 1) - q)


def _pass(a, e, taps):
    """One pass along the last axis: (value, band) of the float32 sequential sum of the taps over (a, e)."""
    n, ln = len(taps), a.shape[-1]
    idx = reflect101(np.arange(-(n // 2), ln + n // 2), ln)
    pa, pe = a[..., idx], e[..., idx]
    v = np.zeros(a.shape)
    s = np.zeros(a.shape)
    pe_sum = np.zeros(a.shape)
    for k, t in enumerate(taps.astype(np.float64)):
        v += t * pa[..., k:k + ln]
        s += t * (np.abs(pa[..., k:k + ln]) + pe[..., k:k + ln])
        pe_sum += t * pe[..., k:k + ln]
    return v, pe_sum + (n + 1) * U24 * s


def blur(prev, sigma):
    """GaussianBlur(prev, sigma) of a given float32 image -> (value float64, band)."""
    taps = gaussian_taps(sigma)
    a = prev.astype(np.float64)
    v, e = _pass(a, np.zeros_like(a), taps)
    v, e = _pass(v.T, e.T, taps)
    return v.T, e.T


# ------------------------------------------------------------------------------------------------ banded float32 arithmetic
class B:
    """value (float64) and a first-order bound on the deviation of the float32 evaluation; every operation adds u |result|."""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, B) else B(x)

    def _r(self, v, e, exact_in):
        # an IEEE operation on exact operands whose exact result is a float32 commits no error (ties, plateaus, Sterbenz differences)
        with np.errstate(over="ignore"):
            free = exact_in & (v == v.astype(F32).astype(np.float64))
        return B(v, e + np.where(free, 0.0, U24 * np.abs(v)))

    def __add__(self, o):
        o = B.of(o)
        return self._r(self.v + o.v, self.e + o.e, (self.e == 0) & (o.e == 0))
    __radd__ = __add__

    def __sub__(self, o):
        o = B.of(o)
        return self._r(self.v - o.v, self.e + o.e, (self.e == 0) & (o.e == 0))

    def __rsub__(self, o):
        return B.of(o) - self

    def __mul__(self, o):
        o = B.of(o)
        return self._r(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e, (self.e == 0) & (o.e == 0))
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = B.of(o)
        q = self.v / o.v
        return self._r(q, (self.e + np.abs(q) * o.e) / np.abs(o.v), np.zeros(np.shape(q), bool))

    def __neg__(self):
        return B(-self.v, self.e)

    def exact_scale(self, s):
        return B(self.v * s, self.e * abs(s))

    def abs(self):
        return B(np.abs(self.v), self.e)

    def sqrt(self):
        r = np.sqrt(self.v)
        return self._r(r, np.where(r > 0, self.e / np.maximum(2 * r, 1e-300), np.sqrt(self.e)), np.zeros(np.shape(r), bool))

    def exp(self):
        r = np.exp(self.v)
        return B(r, r * (self.e + EXP_REL))

    def __getitem__(self, i):
        return B(self.v[i], self.e[i])


def tri(m, e, strict=True):
    """The branch `m > 0` (strict) or `m >= 0`: 1 true, 0 false, -1 inside the band."""
    out = np.where(m > e, 1, np.where(m < -e, 0, -1))
    exact = (e == 0)
    return np.where(exact, ((m > 0) if strict else (m >= 0)).astype(int), out)


def near_half(v, e):
    """cvRound(v) could go either way: v within e of a half-integer (e = 0: exact, half to even as cvRound)."""
    return (np.abs(v - np.floor(v) - 0.5) <= e) & (e > 0)


# ------------------------------------------------------------------------------------------------ stage 7
def contrast_scan_threshold(p):
    return math.floor(0.5 * p["contrast_threshold"] / p["n_octave_layers"] * 255)


def candidates(dog, p):
    """dog: (nl + 2, h, w) float32 of one octave -> int array of (layer, r, c)."""
    nl = p["n_octave_layers"]
    L, h, w = dog.shape
    if h <= 2 * BORDER or w <= 2 * BORDER:
        return np.zeros((0, 3), np.int64)
    thr = F32(contrast_scan_threshold(p))
    core = dog[1:nl + 1, BORDER:h - BORDER, BORDER:w - BORDER]
    nb = [dog[1 + dl:nl + 1 + dl, BORDER + dr:h - BORDER + dr, BORDER + dc:w - BORDER + dc]
          for dl in (-1, 0, 1) for dr in (-1, 0, 1) for dc in (-1, 0, 1)]
    hi, lo = np.maximum.reduce(nb), np.minimum.reduce(nb)
    ext = (np.abs(core) > thr) & np.where(core > 0, core >= hi, core <= lo)
    out = np.argwhere(ext)
    out[:, 0] += 1
    out[:, 1:] += BORDER
    return out


# ------------------------------------------------------------------------------------------------ stages 8, 9
IMG_SCALE = float(F32(1.0) / F32(255))
D1, D2, DX = IMG_SCALE * 0.5, IMG_SCALE, IMG_SCALE * 0.25


def _derivatives(dog, l, r, c):
    d = lambda dl, dr, dc: B(dog[l + dl, r + dr, c + dc].astype(np.float64))
    g = [(d(0, 0, 1) - d(0, 0, -1)) * D1, (d(0, 1, 0) - d(0, -1, 0)) * D1, (d(1, 0, 0) - d(-1, 0, 0)) * D1]
    v = d(0, 0, 0)
    v2 = v.exact_scale(2.0)
    dxx = (d(0, 0, 1) + d(0, 0, -1) - v2) * D2
    dyy = (d(0, 1, 0) + d(0, -1, 0) - v2) * D2
    dss = (d(1, 0, 0) + d(-1, 0, 0) - v2) * D2
    dxy = (d(0, 1, 1) - d(0, 1, -1) - d(0, -1, 1) + d(0, -1, -1)) * DX
    dxs = (d(1, 0, 1) - d(1, 0, -1) - d(-1, 0, 1) + d(-1, 0, -1)) * DX
    dys = (d(1, 1, 0) - d(1, -1, 0) - d(-1, 1, 0) + d(-1, -1, 0)) * DX
    return v, g, (dxx, dyy, dss, dxy, dxs, dys)


def _solve(g, hs):
    """x with H x = g: value by numpy.linalg.solve, band through the closed form of Matx33f::solve.  -> (x[3], det)."""
    dxx, dyy, dss, dxy, dxs, dys = hs
    a = [[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]]
    m = lambda i, j, k, l: a[i][j] * a[k][l]
    det = a[0][0] * (m(1, 1, 2, 2) - m(1, 2, 2, 1)) - a[0][1] * (m(1, 0, 2, 2) - m(1, 2, 2, 0)) + a[0][2] * (m(1, 0, 2, 1) - m(1, 1, 2, 0))
    b = g
    num = [b[0] * (m(1, 1, 2, 2) - m(1, 2, 2, 1)) - a[0][1] * (b[1] * a[2][2] - a[1][2] * b[2]) + a[0][2] * (b[1] * a[2][1] - a[1][1] * b[2]),
           a[0][0] * (b[1] * a[2][2] - a[1][2] * b[2]) - b[0] * (m(1, 0, 2, 2) - m(1, 2, 2, 0)) + a[0][2] * (a[1][0] * b[2] - b[1] * a[2][0]),
           a[0][0] * (a[1][1] * b[2] - b[1] * a[2][1]) - a[0][1] * (a[1][0] * b[2] - b[1] * a[2][0]) + b[0] * (m(1, 0, 2, 1) - m(1, 1, 2, 0))]
    ok = np.abs(det.v) > det.e
    H = np.stack([np.stack([a[i][j].v for j in range(3)], -1) for i in range(3)], -2)
    H = np.where(ok[:, None, None], H, np.eye(3))
    x = np.linalg.solve(H, np.stack([q.v for q in g], -1)[..., None])[..., 0]
    inv = B(1.0) / B(np.where(ok, det.v, 1.0), np.where(ok, det.e, 0.0))
    out = []
    for i in range(3):
        band = (inv * num[i]).e
        out.append(B(np.where(ok, x[:, i], 0.0), np.where(ok, band, 0.0)))
    return out, det


def refine(dog, cand, p, octv):
    """adjustLocalExtrema for all candidates of one octave -> dict of arrays (status, reason, final layer / r / c, banded fields)."""
    nl = p["n_octave_layers"]
    _, h, w = dog.shape
    n = len(cand)
    status = np.array(["active"] * n, dtype=object)          # active / kept / rejected / undecided
    reason = np.array([""] * n, dtype=object)
    l, r, c = cand[:, 0].copy(), cand[:, 1].copy(), cand[:, 2].copy()
    stood = cand.copy()
    X = [np.zeros(n) for _ in range(3)]
    XE = [np.zeros(n) for _ in range(3)]
    conv = np.zeros(n, bool)

    def settle(ix, st, why):
        status[ix] = st
        reason[ix] = why

    for _ in range(MAX_STEPS):
        act = np.nonzero((status == "active") & ~conv)[0]
        if not len(act):
            break
        _, g, hs = _derivatives(dog, l[act], r[act], c[act])
        sol, det = _solve(g, hs)
        x = [-s for s in sol]                                # xc, xr, xi
        sing = (np.abs(det.v) <= det.e) & (det.e > 0)
        t = [tri(0.5 - np.abs(q.v), q.e) for q in x]
        all_in = (t[0] == 1) & (t[1] == 1) & (t[2] == 1)
        some_out = (t[0] == 0) | (t[1] == 0) | (t[2] == 0)
        und = ~sing & ~all_in & ~some_out
        settle(act[sing], "undecided", "singular")
        settle(act[und], "undecided", "converge")
        done = ~sing & all_in
        for k in range(3):
            X[k][act[done]] = x[k].v[done]
            XE[k][act[done]] = x[k].e[done]
        conv[act[done]] = True
        mv = ~sing & ~all_in & some_out
        big = [tri(np.abs(q.v) - BIG, q.e) for q in x]
        over = mv & ((big[0] == 1) | (big[1] == 1) | (big[2] == 1))
        maybe_over = mv & ~over & ((big[0] == -1) | (big[1] == -1) | (big[2] == -1))
        settle(act[over], "rejected", "overflow")
        settle(act[maybe_over], "undecided", "overflow")
        mv &= ~over & ~maybe_over
        amb = mv & (near_half(x[0].v, x[0].e) | near_half(x[1].v, x[1].e) | near_half(x[2].v, x[2].e))
        settle(act[amb], "undecided", "round")
        mv &= ~amb
        ix = act[mv]
        c[ix] += np.rint(x[0].v[mv].astype(F32)).astype(np.int64)
        r[ix] += np.rint(x[1].v[mv].astype(F32)).astype(np.int64)
        l[ix] += np.rint(x[2].v[mv].astype(F32)).astype(np.int64)
        out_l = (l[ix] < 1) | (l[ix] > nl)
        out_b = (c[ix] < BORDER) | (c[ix] >= w - BORDER) | (r[ix] < BORDER) | (r[ix] >= h - BORDER)
        settle(ix[out_l], "rejected", "layer")
        settle(ix[~out_l & out_b], "rejected", "border")
        keep = ~out_l & ~out_b
        stood[ix[keep]] = np.stack([l[ix[keep]], r[ix[keep]], c[ix[keep]]], -1)
    settle(np.nonzero((status == "active") & ~conv)[0], "rejected", "steps")

    res = dict(status=status, reason=reason, layer=l, r=r, c=c, stood=stood, octv=octv, fields=None)
    ix = np.nonzero((status == "active") & conv)[0]
    if not len(ix):
        status[status == "active"] = "rejected"
        return res
    v, g, hs = _derivatives(dog, l[ix], r[ix], c[ix])
    xc, xr, xi = (B(X[k][ix], XE[k][ix]) for k in range(3))
    tdot = (g[0] * xc + g[1] * xr) + g[2] * xi
    contr = v * IMG_SCALE + tdot.exact_scale(0.5)
    lhs = contr.abs() * float(nl)
    tc = tri(float(F32(p["contrast_threshold"])) - lhs.v, lhs.e)            # |contr| nl < thr -> reject
    dxx, dyy, _, dxy, _, _ = hs
    trc, det2 = dxx + dyy, dxx * dyy - dxy * dxy
    td = tri(det2.v, det2.e)                                                # det > 0 keeps
    et = float(F32(p["edge_threshold"]))
    et1 = float(F32(et) + F32(1))
    el, er = trc * trc * et, B(float(F32(et1) * F32(et1))) * det2
    te = tri(er.v - el.v, el.e + er.e)                                      # tr^2 e < (e + 1)^2 det keeps
    for k, i in enumerate(ix):
        if tc[k] == 1:
            status[i], reason[i] = "rejected", "contrast"
        elif tc[k] == -1:
            status[i], reason[i] = "undecided", "contrast"
        elif td[k] == 0:
            status[i], reason[i] = "rejected", "edge_det"
        elif td[k] == -1 or te[k] == -1:
            status[i], reason[i] = "undecided", "edge"
        elif te[k] == 0:
            status[i], reason[i] = "rejected", "edge_ratio"
        else:
            status[i] = "kept"
    kept = status[ix] == "kept"
    ki = ix[kept]
    xc, xr, xi, contr = xc[kept], xr[kept], xi[kept], contr[kept]
    sc = float(2 ** octv)
    px = (B(c[ki].astype(np.float64)) + xc).exact_scale(sc)
    py = (B(r[ki].astype(np.float64)) + xr).exact_scale(sc)
    ex = ((B(l[ki].astype(np.float64)) + xi) / float(nl)) * float(F32(math.log(2.0)))
    size = (B(float(F32(p["sigma"]))) * ex.exp()).exact_scale(sc * 2.0)
    size = B(size.v, size.e + 2 * U24 * size.v)
    q = (xi + 0.5) * 255.0
    res["fields"] = dict(index=ki, x=px, y=py, size=size, response=contr.abs(), layer=l[ki], r=r[ki], c=c[ki],
                         byte=np.rint(q.v).astype(np.int64), byte_undecided=near_half(q.v, q.e))
    return res


# ------------------------------------------------------------------------------------------------ stage 10
def orientations(img, r, c, size, octv):
    """Orientation histogram of one refined keypoint on its Gaussian level.  size: banded raw size (one element).
    -> (list of (peak bin j, angle value, angle band), reason or None)."""
    h, w = img.shape
    n = ORI_BINS
    scl = size.exact_scale(0.5 / 2 ** octv)
    rad = scl * 4.5
    if near_half(rad.v, rad.e):
        return [], "radius"
    radius = int(np.rint(F32(rad.v)))
    sig = scl * 1.5
    escale = B(-1.0) / (sig * sig).exact_scale(2.0)
    ys = np.arange(max(r - radius, 1), min(r + radius, h - 2) + 1)
    xs = np.arange(max(c - radius, 1), min(c + radius, w - 2) + 1)
    if not len(ys) or not len(xs):
        return [], None
    Y, Xg = np.meshgrid(ys, xs, indexing="ij")
    dx = (img[Y, Xg + 1] - img[Y, Xg - 1]).astype(np.float64)
    dy = (img[Y - 1, Xg] - img[Y + 1, Xg]).astype(np.float64)
    d2 = ((Y - r) ** 2 + (Xg - c) ** 2).astype(np.float64)
    wgt = (B(d2) * B(float(escale.v), float(escale.e))).exp()
    mag = (B(dx) * B(dx) + B(dy) * B(dy)).sqrt()
    ori, oband = fast_atan2_f64(dy, dx)
    arg = B(ori, oband) * float(F32(n) / F32(360))
    live = mag.v > 0
    b = np.rint(arg.v).astype(np.int64)
    term = wgt * mag
    # a sample whose bin argument lies within its band of a half-integer may fall into either of the two bins: its whole term
    # enters the band of both (the histogram value keeps it in the nearer one)
    amb = near_half(arg.v, arg.e) & live
    other = np.where(arg.v >= b, b + 1, b - 1) % n
    b = b % n
    raw = np.bincount(b.ravel(), term.v.ravel(), n)
    cnt = np.bincount(b.ravel(), live.ravel().astype(np.float64), n) + np.bincount(other[amb], None, n)
    swing = np.bincount(b[amb], term.v[amb] + term.e[amb], n) + np.bincount(other[amb], term.v[amb] + term.e[amb], n)
    raw_e = np.bincount(b.ravel(), term.e.ravel(), n) + cnt * U24 * (raw + swing) + swing
    T = B(raw, raw_e)
    sh = lambda k: B(np.roll(T.v, k), np.roll(T.e, k))
    hist = (sh(2) + sh(-2)) * (1.0 / 16) + (sh(1) + sh(-1)) * (4.0 / 16) + T * (6.0 / 16)
    mx = B(hist.v.max(), hist.e.max()) * float(F32(0.8))
    L, R = B(np.roll(hist.v, 1), np.roll(hist.e, 1)), B(np.roll(hist.v, -1), np.roll(hist.e, -1))
    t1, t2, t3 = tri(hist.v - L.v, hist.e + L.e), tri(hist.v - R.v, hist.e + R.e), tri(hist.v - mx.v, hist.e + mx.e, strict=False)
    no = (t1 == 0) | (t2 == 0) | (t3 == 0)
    if np.any(~no & ((t1 == -1) | (t2 == -1) | (t3 == -1))):
        return [], "peak"
    out = []
    for j in np.nonzero(~no)[0]:
        hl, hj, hr = L[j], hist[j], R[j]
        bn = B(float(j)) + ((hl - hr) * 0.5) / (hl - hj.exact_scale(2.0) + hr)
        bv = bn.v + n if bn.v < 0 else (bn.v - n if bn.v >= n else bn.v)
        ang = 360.0 - 10.0 * bv
        out.append((int(j), float(ang), float(10.0 * bn.e + 3 * U24 * 360.0)))
    return out, None


# ------------------------------------------------------------------------------------------------ stages 7 - 11 on a given pyramid
def detect(pyr, p):
    """pyr: dict(gauss=[(nl + 3, h, w) per octave], dog=[(nl + 2, h, w) per octave]) of the tested side.
    -> dict(kps: list of decided reference keypoints (final coordinates, banded), undecided: list of (octv, layer, r, c, reason),
            undecided_orient: list of keypoints without angle, report)."""
    nl = p["n_octave_layers"]
    kps, und, und_ori = [], [], []
    rep = dict(candidates=0, refined=0, kept=0, rejected={}, undecided={}, undecided_orient={}, byte_undecided=0, per_tile_max=0)
    for o, dog in enumerate(pyr["dog"]):
        cand = candidates(dog, p)
        rep["candidates"] += len(cand)
        if o == 0 and len(cand):
            tiles = ((cand[:, 1] - BORDER) // 32) * 4096 + (cand[:, 2] - BORDER) // 256
            rep["per_tile_max"] = int(np.bincount(tiles).max())
        if not len(cand):
            continue
        res = refine(dog, cand, p, o)
        rep["refined"] += int((res["status"] == "kept").sum())          # before stage 11: two walks to one position count twice
        for st, key in (("rejected", "rejected"), ("undecided", "undecided")):
            for why in res["reason"][res["status"] == st]:
                rep[key][why] = rep[key].get(why, 0) + 1
        for i in np.nonzero(res["status"] == "undecided")[0]:
            und.append((o,) + tuple(int(v) for v in res["stood"][i]) + (res["reason"][i],))
        f = res["fields"]
        if f is None:
            continue
        seen = set()
        for k in range(len(f["index"])):
            key = (int(f["layer"][k]), int(f["r"][k]), int(f["c"][k]))
            if key in seen:                                   # stage 11: the same final position gives the same keypoints
                continue
            seen.add(key)
            rep["kept"] += 1
            base = dict(octv=o, layer=key[0], r=key[1], c=key[2],
                        x=float(f["x"].v[k]) * 0.5, xe=float(f["x"].e[k]) * 0.5, y=float(f["y"].v[k]) * 0.5, ye=float(f["y"].e[k]) * 0.5,
                        size=float(f["size"].v[k]) * 0.5, size_e=float(f["size"].e[k]) * 0.5,
                        response=float(f["response"].v[k]), response_e=float(f["response"].e[k]),
                        byte=int(f["byte"][k]), byte_undecided=bool(f["byte_undecided"][k]))
            base["octave"] = ((o - 1) & 255) | (key[0] << 8) | (base["byte"] << 16)
            rep["byte_undecided"] += base["byte_undecided"]
            peaks, why = orientations(pyr["gauss"][o][key[0]], key[1], key[2], f["size"][k], o)
            if why:
                rep["undecided_orient"][why] = rep["undecided_orient"].get(why, 0) + 1
                und_ori.append(base)
                continue
            for j, ang, band in peaks:
                kps.append(dict(base, peak=j, angle=ang, angle_e=band))
    rep["keypoints"] = len(kps)
    return dict(kps=kps, undecided=und, undecided_orient=und_ori, report=rep)


def kp_order_key(k):
    return np.lexsort((-k["octave"].astype(np.int64), -k["response"].astype(np.float64), k["angle"], -k["size"].astype(np.float64), k["y"], k["x"]))


def order_errors(kps):
    """Strictly increasing under KeyPoint_LessThan; no two entries share (x, y, size, angle)."""
    errs = []
    if len(kps) < 2:
        return errs
    if not np.array_equal(kp_order_key(kps), np.arange(len(kps))):
        errs.append("not in KeyPoint_LessThan order")
    a, b = kps[:-1], kps[1:]
    same = (a["x"] == b["x"]) & (a["y"] == b["y"]) & (a["size"] == b["size"]) & (a["angle"] == b["angle"])
    if same.any():
        errs.append("%d duplicated keypoints" % same.sum())
    return errs


# ------------------------------------------------------------------------------------------------ stage 12
def unpack_octave(field):
    o = field & 255
    return (o if o < 128 else o - 256), (field >> 8) & 255


def descriptor(img, x, y, size, angle, field):
    """-> (unrounded scaled values (128,), bands (128,)) of calcSIFTDescriptor for the given float32 keypoint on its level."""
    h, w = img.shape
    d, n = 4, 8
    octv, _ = unpack_octave(int(field))
    scale = F32(2.0 ** -octv)
    ptx, pty, sz = F32(x) * scale, F32(y) * scale, F32(size) * scale
    px, py = int(np.rint(ptx)), int(np.rint(pty))
    ori = F32(360) - F32(angle)
    if abs(ori - F32(360)) < FLT_EPSILON:
        ori = F32(0)
    scl = sz * F32(0.5)
    hw32 = F32(3) * scl
    radius = int(np.rint(hw32 * F32(1.4142135623730951) * F32(d + 1) * F32(0.5)))
    radius = min(radius, int(math.sqrt(float(w) * w + float(h) * h)))
    hw = float(hw32)
    rad = B(float(ori) * float(F32(math.pi / 180)))
    rad = B(rad.v, U24 * abs(rad.v))
    ct = B(np.cos(rad.v), TRIG_ERR + abs(np.sin(rad.v)) * rad.e) / hw
    st = B(np.sin(rad.v), TRIG_ERR + abs(np.cos(rad.v)) * rad.e) / hw
    ii, jj = np.meshgrid(np.arange(-radius, radius + 1), np.arange(-radius, radius + 1), indexing="ij")
    R, Cc = py + ii, px + jj
    inside = (R > 0) & (R < h - 1) & (Cc > 0) & (Cc < w - 1)
    ii, jj, R, Cc = ii[inside].astype(np.float64), jj[inside].astype(np.float64), R[inside], Cc[inside]
    c_rot = B(jj) * ct - B(ii) * st
    r_rot = B(jj) * st + B(ii) * ct
    rbin, cbin = r_rot + 1.5, c_rot + 1.5
    m = (rbin.v > -1) & (rbin.v < d) & (cbin.v > -1) & (cbin.v < d)
    c_rot, r_rot, rbin, cbin, R, Cc = c_rot[m], r_rot[m], rbin[m], cbin[m], R[m], Cc[m]
    dx = (img[R, Cc + 1] - img[R, Cc - 1]).astype(np.float64)
    dy = (img[R - 1, Cc] - img[R + 1, Cc]).astype(np.float64)
    wgt = ((c_rot * c_rot + r_rot * r_rot) * (-1.0 / 8)).exp()
    a, aband = fast_atan2_f64(dy, dx)
    obin = (B(a, aband) - float(ori)) * float(F32(n) / F32(360))
    mag = (B(dx) * B(dx) + B(dy) * B(dy)).sqrt() * wgt
    hist = np.zeros((d + 2, d + 2, n))
    herr = np.zeros((d + 2, d + 2, n))
    hcnt = np.zeros((d + 2, d + 2, n))
    r0, c0, o0 = np.floor(rbin.v).astype(int), np.floor(cbin.v).astype(int), np.floor(obin.v).astype(int)
    fr, fc, fo = rbin.v - r0, cbin.v - c0, obin.v - o0
    live = (mag.v > 0).astype(np.float64)
    for dr in (0, 1):
        wr = fr if dr else 1 - fr
        for dc in (0, 1):
            wc = fc if dc else 1 - fc
            for do in (0, 1):
                wo = fo if do else 1 - fo
                idx = (r0 + 1 + dr, c0 + 1 + dc, (o0 + do) % n)
                np.add.at(hist, idx, mag.v * wr * wc * wo)
                # the value's own band, the three coordinates' bands (slope 1 along each axis), three products and differences
                np.add.at(herr, idx, mag.e * wr * wc * wo + mag.v * (rbin.e * wc * wo + cbin.e * wr * wo + obin.e * wr * wc + 6 * U24 * wr * wc * wo))
                np.add.at(hcnt, idx, live)
    hv = hist[1:d + 1, 1:d + 1].reshape(-1)
    he = (herr + (hcnt + 1) * U24 * hist)[1:d + 1, 1:d + 1].reshape(-1)
    ln = len(hv)
    nrm = math.sqrt(float(np.sum(hv * hv)))
    nrm_e = (float(np.sum(hv * he)) / nrm if nrm > 0 else float(np.sqrt(np.sum(he * he)))) + (ln + 2) * U24 * nrm
    thr, thr_e = nrm * float(F32(0.2)), nrm_e * 0.2 + U24 * nrm
    cv = np.minimum(hv, thr)
    ce = np.maximum(he, thr_e)
    root = math.sqrt(float(np.sum(cv * cv)))
    root_e = (float(np.sum(cv * ce)) / root if root > 0 else float(np.sqrt(np.sum(ce * ce)))) + (ln + 2) * U24 * root
    s = 512.0 / max(root, FLT_EPSILON)
    s_e = s * (root_e / max(root, FLT_EPSILON) + U24)
    val = cv * s
    return val, ce * s + cv * s_e + U24 * val


# ------------------------------------------------------------------------------------------------ comparisons
def _ratio(rep, stage, diff, band):
    """Record the largest |difference| / band of a stage; -> number of elements outside the band."""
    diff, band = np.asarray(diff, np.float64), np.asarray(band, np.float64)
    if diff.size == 0:
        return 0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(band > 0, diff / band, np.where(diff > 0, np.inf, 0.0))
    rep["ratio"][stage] = max(rep["ratio"].get(stage, 0.0), float(q.max()))
    return int((diff > band).sum())


def compare_scale_space(bgr, p, pyr, rep):
    """Stages 1 - 6: every Gaussian level inside the band of the blur of the tested side's own previous level, DoG exact."""
    errs = []
    nl = p["n_octave_layers"]
    h, w = bgr.shape[:2]
    sizes = octave_sizes(w, h)
    if len(pyr["gauss"]) != len(sizes):
        return ["%d octaves, expected %d" % (len(pyr["gauss"]), len(sizes))]
    sig = incremental_sigmas(p)
    base = upsample2x(bgr2gray(bgr))
    for o, (ow, oh) in enumerate(sizes):
        G, D = pyr["gauss"][o], pyr["dog"][o]
        if G.shape != (nl + 3, oh, ow) or D.shape != (nl + 2, oh, ow):
            return errs + ["octave %d has shape %s" % (o, G.shape)]
        for i in range(nl + 3):
            if i == 0 and o > 0:
                if not np.array_equal(G[0], pyr["gauss"][o - 1][nl][::2, ::2][:oh, :ow]):
                    errs.append("octave %d base is not the decimated level" % o)
                continue
            v, e = blur(base, base_sigma(p)) if i == 0 else blur(G[i - 1], sig[i])
            bad = _ratio(rep, "gauss", np.abs(G[i].astype(np.float64) - v), e)
            if bad:
                errs.append("gauss (%d, %d): %d pixels outside the band (largest ratio %.3g)" % (o, i, bad, rep["ratio"]["gauss"]))
        for i in range(nl + 2):
            if not np.array_equal((G[i + 1] - G[i]).view(np.uint32), D[i].view(np.uint32)):
                errs.append("dog (%d, %d) is not the float32 difference" % (o, i))
    return errs


def compare_keypoints(kps, det, rep):
    """Stages 7 - 11: decided reference keypoints all present with fields inside their bands, nothing beyond decided + undecided."""
    errs = order_errors(kps)
    kps = kps.astype([(n, "f8") for n in ("x", "y", "size", "angle", "response")] + [("octave", "i8")])      # differences in float64
    by_field = {}
    for i, f in enumerate(kps["octave"].tolist()):
        by_field.setdefault(f, []).append(i)
    used = np.zeros(len(kps), bool)
    missing = 0
    for k in det["kps"]:
        fields = [k["octave"]]
        if k["byte_undecided"]:
            fields += [k["octave"] + (1 << 16), k["octave"] - (1 << 16)]
        hit = None
        for f in fields:
            for i in by_field.get(f, ()):
                g = kps[i]
                if used[i] or abs(g["x"] - k["x"]) > k["xe"] or abs(g["y"] - k["y"]) > k["ye"]:
                    continue
                if angle_dist(g["angle"], k["angle"]) > k["angle_e"]:
                    continue
                hit = i
                break
            if hit is not None:
                break
        if hit is None:
            # a nearest entry, for the message and the ratios: same octave field and position, any angle
            near = [i for f in fields for i in by_field.get(f, ()) if abs(kps[i]["x"] - k["x"]) <= k["xe"] and abs(kps[i]["y"] - k["y"]) <= k["ye"]]
            if near:
                _ratio(rep, "angle", min(angle_dist(kps[i]["angle"], k["angle"]) for i in near), k["angle_e"])
            missing += 1
            if missing <= 3:
                errs.append("decided keypoint missing: octave %d layer %d r %d c %d angle %.4f (x %.4f y %.4f)" % (k["octv"], k["layer"], k["r"], k["c"], k["angle"], k["x"], k["y"]))
            continue
        used[hit] = True
        g = kps[hit]
        _ratio(rep, "pt", [abs(g["x"] - k["x"]), abs(g["y"] - k["y"])], [k["xe"], k["ye"]])
        _ratio(rep, "angle", angle_dist(g["angle"], k["angle"]), k["angle_e"])
        for name in ("size", "response"):
            if _ratio(rep, name, abs(float(g[name]) - k[name]), k[name + "_e"]):
                errs.append("%s of keypoint (%d, %d, %d, %d) outside its band: %.9g vs %.9g +- %.3g" % (name, k["octv"], k["layer"], k["r"], k["c"], g[name], k[name], k[name + "_e"]))
    if missing:
        errs.append("%d decided keypoints missing" % missing)
    # an undecided candidate ends at one final position at most: it explains the keypoints (one per histogram peak) of one
    # (octave field, x, y) and no more, so the unexplained positions can never outnumber the undecided candidates
    extra = 0
    spent = np.zeros(len(det["undecided"]), bool)
    at = {}
    for i in np.nonzero(~used)[0]:
        g = kps[i]
        octv, layer = unpack_octave(int(g["octave"]))
        if any(u["octv"] == octv + 1 and u["layer"] == layer and abs(g["x"] - u["x"]) <= u["xe"] and abs(g["y"] - u["y"]) <= u["ye"] for u in det["undecided_orient"]):
            continue
        at.setdefault((int(g["octave"]), float(g["x"]), float(g["y"])), []).append(i)
    for (field, x, y), members in at.items():
        o = unpack_octave(field)[0] + 1
        gx, gy = x * 2.0 / 2 ** o, y * 2.0 / 2 ** o
        near = [(max(abs(u[2] - gy), abs(u[3] - gx)), j) for j, u in enumerate(det["undecided"]) if not spent[j] and u[0] == o and abs(u[2] - gy) <= 6.5 and abs(u[3] - gx) <= 6.5]
        if near:
            spent[min(near)[1]] = True
            continue
        for i in members:
            g = kps[i]
            extra += 1
            if extra <= 3:
                errs.append("keypoint beyond the reference's set: x %.4f y %.4f size %.4f angle %.4f octave %#x" % (g["x"], g["y"], g["size"], g["angle"], g["octave"]))
    rep["forgiven"] = int(spent.sum())
    if extra:
        errs.append("%d keypoints beyond the decided and undecided set" % extra)
    return errs


def compare_counts(counts, rep):
    """The tested side's own counters (dict(candidates, refined)) against stages 7 and 8.  The candidate set is exact, so its size
    is; the candidates that the refinement keeps are the decided keeps and at most every undecided one besides."""
    errs = []
    if counts["candidates"] != rep["candidates"]:
        errs.append("%d candidates, the scan of the given DoG has %d" % (counts["candidates"], rep["candidates"]))
    und = sum(rep["undecided"].values())
    if not rep["refined"] <= counts["refined"] <= rep["refined"] + und:
        errs.append("%d candidates refined, expected %d .. %d" % (counts["refined"], rep["refined"], rep["refined"] + und))
    return errs


def compare_descriptors(kps, desc, pyr, rep):
    """Stage 12 on every given keypoint: |got - value| <= 0.5 + band on all 128 elements."""
    errs = []
    if desc.shape != (len(kps), 128):
        return ["descriptor shape %s" % (desc.shape,)]
    if len(kps) and not (np.array_equal(desc, np.rint(desc)) and desc.min() >= 0 and desc.max() <= 255):
        errs.append("descriptor values are not integers 0 .. 255")
    bad = 0
    for i, g in enumerate(kps):
        octv, layer = unpack_octave(int(g["octave"]))
        val, band = descriptor(pyr["gauss"][octv + 1][layer], g["x"], g["y"], g["size"], g["angle"], g["octave"])
        val = np.minimum(val, 255.0)
        diff = np.abs(desc[i].astype(np.float64) - val)
        n = _ratio(rep, "descriptor", np.maximum(diff - 0.5, 0.0), np.maximum(band, 1e-300))
        bad += n
        if n and len(errs) < 3:
            j = int(np.argmax(diff - band))
            errs.append("descriptor %d element %d: %g vs %.6f (band %.2e)" % (i, j, desc[i, j], val[j], band[j]))
    if bad:
        errs.append("%d descriptor elements outside 0.5 + band" % bad)
    return errs


def compare_all(bgr, p, pyr, kps, desc, counts):
    """The tested side's pyramid, counters, keypoints and descriptors against the reference -> dict(errors, report, detect)."""
    rep = dict(ratio={})
    errs = compare_scale_space(bgr, p, pyr, rep)
    det = detect(pyr, p)
    rep.update(det["report"])
    errs += compare_counts(counts, rep)
    errs += compare_keypoints(kps, det, rep)
    errs += compare_descriptors(kps, desc, pyr, rep)
    rep["output"] = len(kps)
    return dict(errors=errs, report=rep, detect=det)
