"""Plain numpy reference of ORB detect + describe (cv::ORB::detectAndCompute of OpenCV 4.x with WTA_K 2, firstLevel 0), written
from OpenCV's documented semantics.

Nothing here calls the oracle (oracle/mo_orb.c) or the product library: both are checked against these functions, so a misreading
of OpenCV that the kernels and the oracle share shows up as a disagreement with this module.  Where the oracle's C walks loops, the
stages here are written in another form (closed forms, 2-D convolutions, per-rotation array minima, sorting instead of histograms),
so that one slip cannot sit in both.

Semantics restated (OpenCV 4.x features2d/src/orb.cpp, fast.cpp, keypoint.cpp; imgproc color_rgb, resize, smooth; core RNG):
  * levels: scale_l = (float)pow(double(scaleFactor), l); size = cvRound(cols / scale_l) with the division in float32 and
    round-half-even.  A level of size zero is refused (cv::resize refuses an empty size).
  * budgets: factor = (float)(1 / scaleFactor); n = nfeatures (1 - factor) / (1 - (float)pow(factor, nlevels)) in float32;
    N_l = cvRound(n factor^l) for l < nlevels - 1 (n multiplied by factor in float32 each level), the last level takes
    max(nfeatures - sum, 0).
  * umax: orb.cpp's quarter-disc table, float32 where orb.cpp computes in float.
  * BGR -> gray: (B 3735 + G 19235 + R 9798 + 2^14) >> 15, the 15-bit coefficients of RGB2Gray<uchar> (color_rgb.simd.hpp).
    Reading, not pinned: older releases used the 14-bit triple 1868 / 9617 / 4899.  The oracle reads it the same way.
  * pyramid: each level is resize(previous level, INTER_LINEAR_EXACT): per output coordinate the source position
    (i + 0.5) / inv_scale - 0.5 in float64, offset floor(.), weight cvRound(frac * 256) (weight 256 on the edge sample where the
    position leaves [0, len - 1)), both passes in exact integers, one rounding (+ 2^15) >> 16 at the end.  An exact halving takes
    resizeAreaFast in OpenCV, which is (a + b + c + d + 2) >> 2: identical to the above with weights 128 / 128.
  * border: copyMakeBorder(BORDER_REFLECT_101 | BORDER_ISOLATED) of every level, border 32 here (OpenCV's is
    max(edgeThreshold, ceil(halfPatch sqrt 2), 3) + 1; no stage reads farther than 31 pixels out, and the ring's values do not
    depend on its width).  borderInterpolate is written as a closed form: period 2 (len - 1), folded.
  * FAST-9/16 (threshold t, nonmaxSuppression): pixels with 3 <= x < w - 3, 3 <= y < h - 3.  A pixel is a corner when some arc of
    9 consecutive circle pixels has every difference > t (brighter) or every difference < -t (darker); its score is the largest
    arc minimum of |difference| minus 1.  Strict 3 x 3 non-maximum suppression on the score map (0 off the corners).
  * runByImageBorder(edgeThreshold): keep edge <= x < w - edge, edge <= y < h - edge.
  * retainBest(n): n = 0 keeps nothing; otherwise everything >= the n-th best response is kept (ties at the cut kept:
    nth_element + partition).  First on the FAST score with n = 2 N_l (HARRIS_SCORE) or N_l (FAST_SCORE), then, for
    HARRIS_SCORE, on the Harris response with n = N_l.
  * Harris (HarrisResponses, block 7, k 0.04): Sobel-like integer gradients summed to integers a, b, c over the 7 x 7 block, then
    ((a b - c c) - (0.04 (a + b)) (a + b)) scale^4 with scale = 1 / (4 * 7 * 255), every operation in float32, no contraction.
  * angle (ICAngles on the un-blurred level): integer moments m01, m10 over the umax disc, then fastAtan2 (degrees, the
    7th-order polynomial of core/fast_math) -- evaluated here in float64.
  * blur: GaussianBlur(7 x 7, sigma 2, BORDER_REFLECT_101) of the level's ROI in the bordered pyramid: Q8 taps from
    getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED (derived below, asserted to be 18 34 48 56 48 34 18), the integer
    2-D sum, one rounding (+ 2^15) >> 16.  The border ring is not blurred.
  * pattern (patchSize != 31): makeRandomPattern, cv::RNG(0x34985739) multiply-with-carry (4164903690), 512 points, coordinates
    rng.uniform(-half, half + 1).  patchSize 31 takes the fixed bit_pattern_31_ table, which is not restated: it is refused.
  * rBRIEF: per bit, pixel (round(x cos - y sin), round(x sin + y cos)) of the two pattern points on the blurred level around
    (round(pt.x / scale), round(pt.y / scale)) -- the level coordinate itself -- bit = first < second.
  * keypoints: pt = level coordinate * scale_l (float32), size = patchSize * scale_l, octave l, response = Harris (or the FAST
    score).  Canonical order: level, response descending, y, x.

Error model of the float32 quantities (the bands; derived once here, not tuned to the tests), u = 2^-24, first order:
  * angle: c = min / max of |m10|, |m01| has one rounding (u c), c^2 another (3 u c^2 with c's), Horner over 4 coefficients 8 u,
    the coefficients themselves (float32 products of float32 constants) 3 u each; with T = sum_i |p_i c^i| <= 87.4 degrees the
    polynomial is within u (7 + 9 + 8 + 3) T, and the up to three reflections 90 - a, 180 - a, 360 - a add u 360 each:
    band_angle = u (27 T + 1080) <= 2.1e-4 degrees.  The moments are exact in float32 (|m| < 2^24, asserted).
  * rotated sample coordinates x cos - y sin: the angle band (in radians, times the radius |(x, y)| <= 28.3), the degree ->
    radian product (2 u |rad|), sin / cos (3e-7 absolute each, pinned by test_dev_math_cpu.py on the library's functions), two
    products and a difference (u each): band = |(x, y)| band_rad + (|x| + |y|) (3e-7 + 2 u |rad|) + u (|x c| + |y s|) + u |x'|.
    A bit whose four rounded coordinates include one within its band of a .5 boundary is undetermined; every other bit is
    compared exactly.
"""
import math

import numpy as np

BORDER = 32
MAX_LEVEL_FEATURES = 1920       # the library's per-level budget limit (include/mistitch.h)
U24 = 2.0 ** -24
TRIG_ERR = 3e-7                 # test_dev_math_cpu.py::test_trig_err_is_tied_to_the_library (the library's mis_sinf / mis_cosf)
F32 = np.float32
KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])

# FAST circle of radius 3, clockwise from (0, 3) -- positions k = 0 .. 15
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


# ------------------------------------------------------------------------------------------------ parameters
def params(nfeatures=4000, scale_factor=1.2, nlevels=8, edge_threshold=1, score_type=0, patch_size=40, fast_threshold=20):
    return dict(nfeatures=nfeatures, scale_factor=float(F32(scale_factor)), nlevels=nlevels, edge_threshold=edge_threshold,
                score_type=score_type, patch_size=patch_size, fast_threshold=fast_threshold)


def level_scales(p):
    return [F32(math.pow(p["scale_factor"], l)) for l in range(p["nlevels"])]


def level_sizes(p, w, h):
    """[(w_l, h_l)]: cvRound(float32(len) / scale_l), half to even."""
    return [(int(np.rint(F32(w) / s)), int(np.rint(F32(h) / s))) for s in level_scales(p)]


def level_budgets(p):
    factor = F32(1.0 / p["scale_factor"])
    nd = F32(p["nfeatures"]) * (F32(1) - factor) / (F32(1) - F32(math.pow(float(factor), p["nlevels"])))
    out = []
    for _ in range(p["nlevels"] - 1):
        out.append(int(np.rint(nd)))
        nd = nd * factor
    out.append(max(p["nfeatures"] - sum(out), 0))
    return out


def refused(p, w, h):
    """Why the library and the oracle refuse these parameters for a w x h frame (None when they accept them)."""
    if p["patch_size"] == 31:
        return "patch_size 31"
    if max(level_budgets(p)) > MAX_LEVEL_FEATURES:
        return "level budget"
    if min(min(s) for s in level_sizes(p, w, h)) < 1:
        return "empty level"
    return None


def umax_table(patch_size):
    hp = patch_size // 2
    u = [0] * (hp + 2)
    half = F32(hp) * F32(math.sqrt(2.0)) / F32(2)          # int * std::sqrt(2.f) / 2, float32
    vmax, vmin = math.floor(half + F32(1)), math.ceil(half)
    for v in range(vmax + 1):
        u[v] = int(np.rint(math.sqrt(float(hp * hp - v * v))))
    v0 = 0
    for v in range(hp, vmin - 1, -1):
        while u[v0] == u[v0 + 1]:
            v0 += 1
        u[v] = v0
        v0 += 1
    return np.array(u, np.int64)


class CvRNG:
    """cv::RNG: state' = (state mod 2^32) * 4164903690 + floor(state / 2^32), next() = state' mod 2^32."""

    def __init__(self, seed):
        self.state = seed or 0xFFFFFFFF

    def next(self):
        self.state = (self.state % 2 ** 32) * 4164903690 + self.state // 2 ** 32
        return self.state % 2 ** 32

    def uniform(self, a, b):
        # (int)(next() % (unsigned)(b - a) + (unsigned)a): two's complement wrap of the unsigned sum
        if a == b:
            return a
        v = (self.next() % (b - a) + a) % 2 ** 32
        return v - 2 ** 32 if v >= 2 ** 31 else v


def pattern(patch_size, npoints=512):
    assert patch_size != 31, "bit_pattern_31_ is not restated"
    rng, hp = CvRNG(0x34985739), patch_size // 2
    pts = []
    for _ in range(npoints):
        x = rng.uniform(-hp, hp + 1)
        y = rng.uniform(-hp, hp + 1)
        pts.append((x, y))
    return np.array(pts, np.int64)


def gaussian_taps_q8(ksize=7, sigma=2.0, bits=8):
    """getGaussianKernelBitExact (float64 in place of softdouble: no value lands near a rounding boundary) followed by
    getGaussianKernelFixedPoint_ED: error-diffused rounding of the outer taps, the centre takes what is left."""
    n2 = (ksize - 1) // 2
    scale2 = -0.125 / (sigma * sigma)
    vals = [math.exp((x * x) * scale2) for x in range(1 - ksize, 0, 2)]     # x = 2 (i - n2)
    s = 2.0 * sum(vals) + 1.0
    k = [v / s for v in vals]
    one = float(1 << bits)
    out = [0] * ksize
    err, tot = 0.0, 0
    for i in range(n2):
        adj = k[i] * one + err
        v = int(round(adj))                 # cvRound: half to even (Python's round)
        err = adj - v
        out[i] = out[ksize - 1 - i] = v
        tot += v
    out[n2] = int(one) - 2 * tot
    return out


# ------------------------------------------------------------------------------------------------ images
def bgr2gray(bgr):
    coef = np.array([3735, 19235, 9798], np.int64)
    return ((np.tensordot(bgr.astype(np.int64), coef, axes=([2], [0])) + (1 << 14)) >> 15).astype(np.uint8)


def _linear_exact_axis(dlen, slen):
    """(offsets, weight of offset + 1 in Q8) of one axis of resize INTER_LINEAR_EXACT."""
    pos = (np.arange(dlen, dtype=np.float64) + 0.5) * (1.0 / (dlen / slen)) - 0.5
    fl = np.floor(pos)
    inside = (fl >= 0) & (fl < slen - 1)
    ofs = np.where(fl < 0, 0, np.where(inside, fl, slen - 1)).astype(np.int64)
    wt = np.where(inside, np.rint((pos - fl) * 256.0), 0).astype(np.int64)
    return ofs, wt


def resize_linear_exact(src, dw, dh):
    sh, sw = src.shape
    xo, xw = _linear_exact_axis(dw, sw)
    yo, yw = _linear_exact_axis(dh, sh)
    s = src.astype(np.int64)
    x1 = np.minimum(xo + 1, sw - 1)
    y1 = np.minimum(yo + 1, sh - 1)
    hz = s[:, xo] * (256 - xw) + s[:, x1] * xw                          # Q8, exact
    v = hz[yo] * (256 - yw)[:, None] + hz[y1] * yw[:, None]            # Q16, exact
    return ((v + (1 << 15)) >> 16).astype(np.uint8)


def reflect101(p, n):
    """borderInterpolate(BORDER_REFLECT_101) in closed form: gfedcb|abcdefgh|gfedcba, folded as often as needed."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * (n - 1))
    return np.where(q >= n, 2 * (n - 1) - q, q)


def pad_reflect101(img, b=BORDER):
    h, w = img.shape
    return img[reflect101(np.arange(-b, h + b), h)][:, reflect101(np.arange(-b, w + b), w)]


def fast_scores(level, t):
    """FAST-9/16 score map of a level (0 where not a corner), by brute force over the 16 arcs."""
    h, w = level.shape
    sc = np.zeros((h, w), np.int64)
    if w < 7 or h < 7:
        return sc
    g = level.astype(np.int16)
    for r0 in range(3, h - 3, 256):                 # bands of rows: the (16, rows, w) differences of a 4K level stay small
        r1 = min(r0 + 256, h - 3)
        c = g[r0:r1, 3:w - 3]
        d = np.stack([g[r0 + dy:r1 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE]) - c[None]   # (16, rows, w - 6)
        ys, xs = np.nonzero(np.abs(d).max(axis=0) > t)     # necessary: some pixel of the circle differs by more than t
        if len(ys) == 0:
            continue
        dd = d[:, ys, xs].astype(np.int64)                 # (16, n)
        best = np.full(len(ys), -10 ** 6, np.int64)
        for s in range(16):
            arc = dd[[(s + j) % 16 for j in range(9)]]
            best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
        sc[ys + r0, xs + 3] = np.where(best > t, best - 1, 0)
    return sc


def nms_border(sc, edge):
    """Strict 3 x 3 maxima of the score map (neighbours off the map count 0), then runByImageBorder(edge)."""
    h, w = sc.shape
    p = np.zeros((h + 2, w + 2), np.int64)
    p[1:-1, 1:-1] = sc
    keep = sc > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= sc > p[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx]
    yy, xx = np.mgrid[0:h, 0:w]
    keep &= (xx >= edge) & (xx < w - edge) & (yy >= edge) & (yy < h - edge)
    return np.where(keep, sc, 0)


def retain_best(resp, n):
    """KeyPointsFilter::retainBest as a mask: all of them when n >= count, none when n == 0, else everything >= the n-th best."""
    resp = np.asarray(resp)
    if n >= len(resp):
        return np.ones(len(resp), bool)
    if n == 0:
        return np.zeros(len(resp), bool)
    cut = np.partition(resp, len(resp) - n)[len(resp) - n]
    return resp >= cut


def harris(padded, xs, ys):
    """HarrisResponses(block 7, k 0.04) at level coordinates (xs, ys) of a level padded by BORDER: float32 responses + (a, b, c)."""
    n = len(xs)
    if n == 0:
        return np.zeros(0, F32), np.zeros((3, 0), np.int64)
    o = np.arange(-4, 5)
    win = padded[(ys + BORDER)[:, None, None] + o[None, :, None], (xs + BORDER)[:, None, None] + o[None, None, :]].astype(np.int64)
    c_, l_, r_, u_, d_ = (slice(1, 8), slice(0, 7), slice(2, 9), slice(0, 7), slice(2, 9))
    ix = 2 * (win[:, c_, r_] - win[:, c_, l_]) + (win[:, u_, r_] - win[:, u_, l_]) + (win[:, d_, r_] - win[:, d_, l_])
    iy = 2 * (win[:, d_, c_] - win[:, u_, c_]) + (win[:, d_, l_] - win[:, u_, l_]) + (win[:, d_, r_] - win[:, u_, r_])
    a = (ix * ix).sum(axis=(1, 2))
    b = (iy * iy).sum(axis=(1, 2))
    c = (ix * iy).sum(axis=(1, 2))
    fa, fb, fc = a.astype(F32), b.astype(F32), c.astype(F32)
    scale = F32(1) / (F32(4 * 7) * F32(255))
    ssq = scale * scale * scale * scale
    s1 = fa * fb
    s2 = fc * fc
    apb = fa + fb
    s3 = (F32(0.04) * apb) * apb
    return ((s1 - s2) - s3) * ssq, np.stack([a, b, c])


ATAN_P = [0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128]


def fast_atan2_f64(y, x):
    """cv::fastAtan2 in float64 -> (degrees, band in degrees)."""
    y = np.asarray(y, np.float64)
    x = np.asarray(x, np.float64)
    ax, ay = np.abs(x), np.abs(y)
    steep = ax < ay
    num, den = np.where(steep, ax, ay), np.where(steep, ay, ax)
    c = np.divide(num, den + 2.220446049250313e-16)
    deg = 180.0 / math.pi
    terms = [p * deg * c ** (2 * i + 1) for i, p in enumerate(ATAN_P)]
    a = sum(terms)
    a = np.where(steep, 90.0 - a, a)
    a = np.where(x < 0, 180.0 - a, a)
    a = np.where(y < 0, 360.0 - a, a)
    band = U24 * (27.0 * sum(np.abs(t) for t in terms) + 1080.0)
    return a, band


def ic_moments(padded, xs, ys, patch_size, umax):
    """(m01, m10) of ICAngles: the disc |u| <= umax[|v|] (all of row 0 out to half_patch), integer sums as one masked product."""
    hp = patch_size // 2
    o = np.arange(-hp, hp + 1)
    vv, uu = np.meshgrid(o, o, indexing="ij")
    lim = np.where(vv == 0, hp, umax[np.minimum(np.abs(vv), len(umax) - 1)])
    mask = np.abs(uu) <= lim
    win = padded[(ys + BORDER)[:, None, None] + o[None, :, None], (xs + BORDER)[:, None, None] + o[None, None, :]].astype(np.int64)
    m01 = (win * (vv * mask)[None]).sum(axis=(1, 2))
    m10 = (win * (uu * mask)[None]).sum(axis=(1, 2))
    return m01, m10


def blur_level(padded, w, h, taps):
    """GaussianBlur 7 x 7 of the level's ROI in its bordered buffer (the 2-D integer sum of the outer product of the taps), the
    border ring left as it is."""
    k2 = np.outer(taps, taps).astype(np.int64)
    p = padded.astype(np.int64)
    acc = np.zeros((h, w), np.int64)
    for j in range(7):
        for i in range(7):
            acc += k2[j, i] * p[BORDER - 3 + j:BORDER - 3 + j + h, BORDER - 3 + i:BORDER - 3 + i + w]
    out = padded.copy()
    out[BORDER:BORDER + h, BORDER:BORDER + w] = ((acc + (1 << 15)) >> 16).astype(np.uint8)
    return out


def _round_band(v, band):
    """cvRound of v (half to even) and whether a value within band of v could round differently."""
    r = np.rint(v)
    frac = np.abs(v - np.floor(v) - 0.5)
    return r.astype(np.int64), frac <= band


def describe(blurred, xs, ys, angle_deg, angle_band, pat):
    """rBRIEF, WTA_K 2 -> (descriptors (n, 32) u8, undetermined bits (n, 256) bool)."""
    n = len(xs)
    if n == 0:
        return np.zeros((0, 32), np.uint8), np.zeros((0, 256), bool)
    rad = np.asarray(angle_deg, np.float64) * (math.pi / 180.0)
    rband = np.asarray(angle_band, np.float64) * (math.pi / 180.0)
    cs, sn = np.cos(rad)[:, None], np.sin(rad)[:, None]
    px, py = pat[:, 0].astype(np.float64)[None], pat[:, 1].astype(np.float64)[None]   # (1, 512)
    rx = px * cs - py * sn
    ry = px * sn + py * cs
    rad_, rb = np.abs(rad)[:, None], rband[:, None]
    base = np.hypot(px, py) * rb + (np.abs(px) + np.abs(py)) * (TRIG_ERR + 2 * U24 * rad_)
    bx = base + U24 * (np.abs(px * cs) + np.abs(py * sn)) + U24 * np.abs(rx)
    by = base + U24 * (np.abs(px * sn) + np.abs(py * cs)) + U24 * np.abs(ry)
    ix, ambx = _round_band(rx, bx)
    iy, amby = _round_band(ry, by)
    vals = blurred[(ys + BORDER)[:, None] + iy, (xs + BORDER)[:, None] + ix].astype(np.int64)     # (n, 512)
    bits = vals[:, 0::2] < vals[:, 1::2]                                                            # (n, 256)
    amb = ambx | amby
    undet = amb[:, 0::2] | amb[:, 1::2]
    desc = np.packbits(bits, axis=1, bitorder="little")            # bit k of byte b: test 8 b + k
    return desc, undet


# ------------------------------------------------------------------------------------------------ the whole path
def orb(bgr, p=None, stages=True):
    """The whole detect + describe path on one BGR u8 frame.

    -> dict: levels [(w, h)], budgets, gray [level images], nms [score maps after NMS + border], blur [bordered blurred levels]
    (when stages), kps (KP_DTYPE, canonical order), desc (n, 32), undet (n, 256) undetermined descriptor bits, angle_band (n,),
    and per level the counts (after NMS, after the FAST cut, final)."""
    p = p or params()
    h, w = bgr.shape[:2]
    why = refused(p, w, h)
    if why:
        raise ValueError("refused: " + why)
    sizes, scales, budgets = level_sizes(p, w, h), level_scales(p), level_budgets(p)
    taps = gaussian_taps_q8()
    assert taps == [18, 34, 48, 56, 48, 34, 18], taps
    um = umax_table(p["patch_size"])
    pat = pattern(p["patch_size"])
    t, edge, harris_score = p["fast_threshold"], p["edge_threshold"], p["score_type"] == 0
    out = dict(levels=sizes, budgets=budgets, gray=[], nms=[], blur=[], counts=[], taps=taps)
    kp_parts, desc_parts, und_parts, band_parts, ang_parts = [], [], [], [], []
    g = bgr2gray(bgr)
    for l, ((lw, lh), sc) in enumerate(zip(sizes, scales)):
        if l:
            g = resize_linear_exact(g, lw, lh)
        padded = pad_reflect101(g)
        nms = nms_border(fast_scores(g, t), edge)
        ys, xs = np.nonzero(nms)
        resp = nms[ys, xs].astype(F32)
        n0 = len(ys)
        N = budgets[l]
        keep = retain_best(resp, 2 * N if harris_score else N)
        xs, ys, resp = xs[keep], ys[keep], resp[keep]
        n1 = len(ys)
        if harris_score:
            resp, _ = harris(padded, xs, ys)
            keep = retain_best(resp, N)
            xs, ys, resp = xs[keep], ys[keep], resp[keep]
        order = np.lexsort((xs, ys, -resp.astype(np.float64)))
        xs, ys, resp = xs[order], ys[order], resp[order]
        m01, m10 = ic_moments(padded, xs, ys, p["patch_size"], um)
        assert np.all(np.abs(m01) < 2 ** 24) and np.all(np.abs(m10) < 2 ** 24)
        ang, aband = fast_atan2_f64(m01, m10)
        blurred = blur_level(padded, lw, lh, taps)
        desc, und = describe(blurred, xs, ys, ang, aband, pat)
        kp = np.zeros(len(xs), KP_DTYPE)
        kp["x"] = xs.astype(F32) * sc
        kp["y"] = ys.astype(F32) * sc
        kp["size"] = F32(p["patch_size"]) * sc
        kp["angle"] = ang.astype(F32)
        kp["response"] = resp
        kp["octave"] = l
        kp_parts.append(kp)
        desc_parts.append(desc)
        und_parts.append(und)
        band_parts.append(np.broadcast_to(np.asarray(aband, np.float64), ang.shape).reshape(-1))
        ang_parts.append(np.asarray(ang, np.float64).reshape(-1))
        out["counts"].append((n0, n1, len(xs)))
        if stages:
            out["gray"].append(g)
            out["nms"].append(nms.astype(np.uint8))
            out["blur"].append(blurred)
    out["kps"] = np.concatenate(kp_parts)
    out["angle64"] = np.concatenate(ang_parts)
    out["desc"] = np.concatenate(desc_parts).reshape(-1, 32)
    out["undet"] = np.concatenate(und_parts).reshape(-1, 256)
    out["angle_band"] = np.concatenate(band_parts)
    return out


# ------------------------------------------------------------------------------------------------ comparisons
def angle_dist(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 360.0
    return np.minimum(d, 360.0 - d)


def kp_sets_equal(got, ref):
    """Keypoints as sets per level: (x, y, octave, size, response) exactly.  -> list of mismatch descriptions (empty when equal)."""
    bad = []
    for l in sorted(set(ref["octave"].tolist()) | set(got["octave"].tolist())):
        g = got[got["octave"] == l]
        r = ref[ref["octave"] == l]
        key = lambda k: set(zip(k["x"].tolist(), k["y"].tolist(), k["size"].tolist(), k["response"].view(np.uint32).tolist()))
        gs, rs = key(g), key(r)
        if gs != rs:
            bad.append("level %d: %d kernel-only, %d reference-only (of %d / %d)" % (l, len(gs - rs), len(rs - gs), len(g), len(r)))
    return bad


def canonical_order_ok(kps):
    """Levels ascending, inside a level response descending, then y, then x."""
    if len(kps) < 2:
        return True
    key = np.lexsort((kps["x"], kps["y"], -kps["response"].astype(np.float64), kps["octave"]))
    return bool(np.all(key == np.arange(len(kps))))


def compare_features(kps, desc, ref):
    """A feature set (kernel or oracle) against the reference -> dict(errors=[...], undetermined_share, max_angle_band).

    Same keypoints in the same (canonical) order; angle within band; every determined descriptor bit exact."""
    errs = kp_sets_equal(kps, ref["kps"])
    rk = ref["kps"]
    if errs or len(kps) != len(rk):
        return dict(errors=errs or ["count %d vs %d" % (len(kps), len(rk))], undetermined_share=None, max_angle_band=None)
    if not canonical_order_ok(kps):
        errs.append("not in canonical order")
    for f in ("x", "y", "octave", "size"):
        if not np.array_equal(kps[f], rk[f]):
            errs.append("field %s differs in order" % f)
    if not np.array_equal(kps["response"].view(np.uint32), rk["response"].view(np.uint32)):
        errs.append("response bits differ")
    da = angle_dist(kps["angle"], ref["angle64"])
    over = da > ref["angle_band"]
    if over.any():
        i = int(np.argmax(da - ref["angle_band"]))
        errs.append("%d angles outside the band (worst #%d: %.7f vs %.9f, band %.2e)" % (over.sum(), i, kps["angle"][i], ref["angle64"][i],
                                                                                         ref["angle_band"][i]))
    gb = np.unpackbits(np.asarray(desc, np.uint8), axis=1, bitorder="little")
    rb = np.unpackbits(ref["desc"], axis=1, bitorder="little")
    wrong = (gb != rb) & ~ref["undet"]
    if wrong.any():
        errs.append("%d determined descriptor bits differ in %d keypoints" % (wrong.sum(), wrong.any(axis=1).sum()))
    share = float(ref["undet"].mean()) if len(rk) else 0.0
    return dict(errors=errs, undetermined_share=share, max_angle_band=float(ref["angle_band"].max()) if len(rk) else 0.0)
