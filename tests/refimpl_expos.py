"""Plain numpy / scipy reference of the step between warp and blend: cv::detail::BlocksGainCompensator (feed, gain maps, apply),
cv::detail::VoronoiSeamFinder and the seam-mask step of the compositing loop, written from OpenCV's documented semantics.

Nothing here calls the oracle (oracle/mo_expos.c, mo_imgops.c) or the product library: both are checked against these functions,
so a misreading of OpenCV that the kernels and the oracle share shows up as a disagreement with this module.  Where the oracle
walks loops (a double loop per block pair, a hand-written LU, a two-pass chamfer), the stages here are whole-array operations:
boolean masks and an exact integer-square table, numpy.linalg.solve, np.pad, scipy's distance transform and maximum filter.

Semantics restated (OpenCV 4.x stitching/src/exposure_compensate.cpp, stitching/src/seam_finders.cpp, imgproc/src/resize.cpp,
imgproc/src/distransform.cpp; the compositing loop of image_stitching.cpp):
  * block_grid (BlocksCompensator::feed): an image of W x H with requested blocks bw x bh has nx = ceil(W / bw) by
    ny = ceil(H / bh) blocks of ceil(W / nx) x ceil(H / ny) pixels, the last column and row clipped to the image; every block,
    in row-major order image after image, becomes one "image" of a GainCompensator, at its pano position.
  * overlap_stats (GainCompensator::singleFeed): for every pair of blocks i <= j (a block with itself included) whose pano
    rectangles intersect: intersect = (mask_i == 255) & (mask_j == 255) over the shared rectangle -- mask bytes other than 255
    do NOT count; N_ij = N_ji = max(1, count); I_ij = (sum over the intersection of the Euclidean norm of block i's BGR pixel)
    / N_ij in float64, and I_ji likewise from block j's pixels.  A count of 0 therefore gives N = 1, I = 0.  The norm is the
    correctly rounded float64 square root of the exact integer sum of squares, and the sum here is math.fsum (exactly rounded),
    so this side carries one rounding where a running float64 sum carries one per pixel (relative 1e-13 at most over a 64 x 64
    block: invisible after the float32 cast below).
  * gains (GainCompensator::gains with alpha = 0.01, beta = 100, Brown & Lowe): over the blocks that are not skipped,
        A_ii = sum_j beta N_ij + sum_{j != i} 2 alpha I_ij^2 N_ij,   A_ij = -2 alpha I_ij I_ji N_ij,   b_i = sum_j beta N_ij
    (j runs over the un-skipped blocks, j = i included in the beta sums), solved in float64; these are the normal equations of
        E(g) = sum_ij N_ij [alpha (g_i I_ij - g_j I_ji)^2 + beta (1 - g_i)^2]
    (test_refimpl_expos_cpu.py checks the minimum from E itself).  A skipped block has gain 1.
    The un-skip rule: the product and the oracle un-skip both blocks of every pair i != j whose RECTANGLES intersect, whatever
    the count (strict=False, the default here).
    NOT PINNED: the stricter reading -- only a pair with a non-zero intersect count un-skips (strict=True) -- cannot be ruled
    out offline (OpenCV is not available to run).  The two differ for a block all of whose overlaps are masked out: un-skipped,
    it adds its unit count N = 1 (with I = 0) to the beta sums of every block it meets, pulling those gains towards 1 by about
    beta / (beta N_ii) of their distance from 1.  That is observable: on the `three_way` scene the gain maps of the two readings
    differ by up to 3.6e-5 (about 600 x 2^-24; test_refimpl_expos_cpu.py prints the figure), far above the gain-map tolerance.
  * gain_maps: the gains of image k as an ny x nx float32 map, then nfilt passes of the separable [1/4 1/2 1/4] along x, then y,
    with BORDER_REFLECT_101 (np.pad "reflect"); an axis of length 1 is left alone (its reflected neighbours are the sample
    itself: 1/4 + 1/2 + 1/4 = 1).  The filter runs in float64 here.
    Tolerance (gain_map_tol): the statistics and the solve are float64 on both sides and differ by order 1e-13, which vanishes
    in the float32 cast (1 rounding, relative 2^-24).  A float32 pass computes (a + b) * 0.25f + c * 0.5f per axis: the
    products by 1/4 and 1/2 are exact, the two sums round, each by at most 2^-24 of a magnitude that never exceeds max|map|
    (the taps are a convex combination), and a convex filter does not amplify an earlier error.  So
        |got - ref| <= (1 + 4 nfilt) * 2^-24 * max|map|,
    max|map| taken over the reference map.  With nfilt = 0 that is the one rounding of the cast; all-ones maps are exact.
  * apply_candidates (BlocksCompensator::apply): the float32 gain map is resized to the image with INTER_LINEAR, then
    multiply(image, gains, image) saturates to 8 bits.  resize(): scale = 1 / (dsize / ssize) in float64 per axis; for the
    destination index x, fx = (float)((x + 0.5) * scale - 0.5), sx = floor(fx), fx -= sx; sx < 0 gives sx = 0, fx = 0;
    sx >= ssize - 1 gives sx = ssize - 1, fx = 0; the taps are sx and min(sx + 1, ssize - 1) with weights (1.f - fx) and fx.
    Those float32 fractions are semantics, not error; the interpolation and the product v * g run in float64 here.
    The float32 operations on the kernel's (and OpenCV's) path to one output value, each rounding by at most 2^-24 of a
    magnitude bounded by max|map| (the weights are in [0, 1] and sum to 1 within a rounding):
        1 - fx, 1 - fy                                   2   (counted although restated above: the band must not depend on it)
        row y0:  two products and their sum              3
        row y1:  two products and their sum              3   (the two rows enter with weights summing to 1; counted in full)
        column:  two products and their sum              3
        v * g                                            1   (relative to v * g: as an error of g it is 2^-24 g)
    -- 12 in all, so band = 12 * 2^-24 * max|map| on the gain, and a byte may be any of rint(v (g - band)) .. rint(v (g + band))
    (half to even, as cvRound), clipped to 0..255.  A 16SC3 image with values 0..255 takes the same values.
  * voronoi (PairwiseSeamFinder::run + VoronoiSeamFinder::findInPair, gap = 10): every pair i < j whose frames' rectangles
    intersect, in (i, j) order, each on the masks as the earlier pairs left them.  Both masks are cut over the shared rectangle
    grown by the gap on every side, zero outside their frame; collision = both != 0 -- every non-zero byte is valid here,
    unlike in the compensator; unique_k = submask_k with the collision cleared; d_k = the city-block distance to the nearest
    pixel of unique_k (distanceTransform(unique_k == 0, DIST_L1, 3), exact for L1); over the whole shared rectangle, where
    d_1 < d_2 frame j loses the pixel (its mask byte becomes 0), otherwise -- ties included -- frame i does.
    An empty unique mask has no nearest pixel: its distance map is one constant larger than every finite distance (EMPTY_DIST).
    NOT PINNED: OpenCV's distanceTransform caps at float((INT_MAX >> 2) * 2^-16) = 8192.0f, which is also what it returns for
    the empty case; a finite distance of 8192 or more would then tie with "empty" where here it is smaller.  No frame overlap
    at seam scale (~0.1 MP) comes near 8192 pixels, so the cap is restated as a comment only.
  * seam_mask_apply (image_stitching.cpp's dilate(masks_warped[i], dilated) / resize(dilated, seam_mask, mask_warped.size(),
    0, 0, INTER_LINEAR_EXACT) / mask_warped = seam_mask & mask_warped): a 3 x 3 dilate whose border never wins (maximum filter
    with constant 0), the exact fixed-point bilinear resize of refimpl_orb.resize_linear_exact, and a bytewise AND -- on the
    bytes, not on their truth values.
"""
import math

import numpy as np
from scipy import ndimage

import refimpl_orb

F32 = np.float32
U24 = 2.0 ** -24
ALPHA, BETA = 0.01, 100.0
GAP = 10
EMPTY_DIST = 1 << 29            # "no unique pixel": above every finite distance (OpenCV: 8192, see the docstring)
APPLY_OPS = 12                  # float32 roundings on the path to one applied value (docstring)

# exact sums of three squares up to 3 * 255^2 -> correctly rounded float64 norms
_NORM = np.sqrt(np.arange(3 * 255 * 255 + 1, dtype=np.float64))


# ------------------------------------------------------------------------------------------------ blocks
class Grid:
    """blocks: (nb, 5) int64 rows (pano x, pano y, w, h, image); shapes: per image (ny, nx)."""

    def __init__(self, blocks, shapes):
        self.blocks, self.shapes = blocks, shapes


def block_grid(corners, sizes, bw, bh):
    blocks, shapes = [], []
    for k, ((cx, cy), (W, H)) in enumerate(zip(corners, sizes)):
        nx, ny = -(-W // bw), -(-H // bh)
        aw, ah = -(-W // nx), -(-H // ny)
        ox, oy = np.meshgrid(np.arange(nx) * aw, np.arange(ny) * ah)              # row-major: y outer, x inner
        ox, oy = ox.ravel(), oy.ravel()
        blocks.append(np.stack([cx + ox, cy + oy, np.minimum(ox + aw, W) - ox, np.minimum(oy + ah, H) - oy, np.full(nx * ny, k)], axis=1))
        shapes.append((ny, nx))
    return Grid(np.concatenate(blocks).astype(np.int64), shapes)


def overlap_stats(corners, images, masks, grid):
    """-> (count, N, I): nb x nb arrays; count is the raw intersect count (-1 where the rectangles do not intersect)."""
    B = grid.blocks
    nb = len(B)
    count = np.full((nb, nb), -1, np.int64)
    N = np.zeros((nb, nb), np.int64)
    I = np.zeros((nb, nb), np.float64)
    norms = [_NORM[(np.asarray(im, np.int64) ** 2).sum(axis=2)] for im in images]
    valid = [np.asarray(m) == 255 for m in masks]
    x0 = np.maximum(B[:, None, 0], B[None, :, 0]); y0 = np.maximum(B[:, None, 1], B[None, :, 1])
    x1 = np.minimum(B[:, None, 0] + B[:, None, 2], B[None, :, 0] + B[None, :, 2])
    y1 = np.minimum(B[:, None, 1] + B[:, None, 3], B[None, :, 1] + B[None, :, 3])
    for i, j in zip(*np.nonzero(np.triu((x0 < x1) & (y0 < y1)))):
        a, b = B[i, 4], B[j, 4]
        sa = np.s_[y0[i, j] - corners[a][1]:y1[i, j] - corners[a][1], x0[i, j] - corners[a][0]:x1[i, j] - corners[a][0]]
        sb = np.s_[y0[i, j] - corners[b][1]:y1[i, j] - corners[b][1], x0[i, j] - corners[b][0]:x1[i, j] - corners[b][0]]
        inter = valid[a][sa] & valid[b][sb]
        c = int(inter.sum())
        count[i, j] = count[j, i] = c
        N[i, j] = N[j, i] = max(1, c)
        I[i, j] = math.fsum(norms[a][sa][inter]) / N[i, j]
        I[j, i] = math.fsum(norms[b][sb][inter]) / N[i, j]
    return count, N, I


def active_blocks(count, strict=False):
    """The blocks that enter the solve: those meeting another block (strict: with a non-zero intersect count)."""
    meet = (count > 0) if strict else (count >= 0)
    meet = meet & ~np.eye(len(count), dtype=bool)
    return meet.any(axis=1)


def gains(count, N, I, strict=False):
    act = np.nonzero(active_blocks(count, strict))[0]
    g = np.ones(len(count), np.float64)
    if len(act):
        Na, Ia = N[np.ix_(act, act)].astype(np.float64), I[np.ix_(act, act)]
        A = -2 * ALPHA * Ia * Ia.T * Na
        np.fill_diagonal(A, 0.0)
        off = Na - np.diag(np.diag(Na))
        A += np.diag(BETA * Na.sum(axis=1) + 2 * ALPHA * (Ia * Ia * off).sum(axis=1))
        g[act] = np.linalg.solve(A, BETA * Na.sum(axis=1))
    return g


def error_function(g, count, N, I, strict=False):
    """E(g) written out from the statistics (not from A and b), over the un-skipped blocks."""
    act = np.nonzero(active_blocks(count, strict))[0]
    e = []
    for i in act:
        for j in act:
            if N[i, j]:
                e.append(N[i, j] * (ALPHA * (g[i] * I[i, j] - g[j] * I[j, i]) ** 2 + BETA * (1 - g[i]) ** 2))
    return math.fsum(e)


def _smooth(m, axis):
    if m.shape[axis] == 1:
        return m
    pw = [(0, 0), (0, 0)]
    pw[axis] = (1, 1)
    p = np.pad(m, pw, mode="reflect")
    n = m.shape[axis]
    lo, mid, hi = (np.take(p, np.arange(k, k + n), axis=axis) for k in range(3))
    return 0.25 * lo + 0.5 * mid + 0.25 * hi


def gain_maps(g, grid, nfilt):
    """-> per image the (ny, nx) float64 map: float32 gains, smoothed nfilt times in float64."""
    out, q = [], 0
    for ny, nx in grid.shapes:
        m = np.asarray(g[q:q + ny * nx], np.float64).astype(F32).astype(np.float64).reshape(ny, nx)
        q += ny * nx
        for _ in range(nfilt):
            m = _smooth(_smooth(m, 1), 0)
        out.append(m)
    return out


def gain_map_tol(ref_map, nfilt):
    return (1 + 4 * nfilt) * U24 * float(np.abs(ref_map).max())


# ------------------------------------------------------------------------------------------------ apply
def _linear_axis(dlen, slen):
    """resize(INTER_LINEAR) of a float image: (tap, next tap, float32 weight of the tap, float32 weight of the next tap)."""
    scale = 1.0 / (dlen / slen)
    f = ((np.arange(dlen, dtype=np.float64) + 0.5) * scale - 0.5).astype(F32)
    s = np.floor(f)
    f = f - s                                    # float32
    s = s.astype(np.int64)
    f = np.where((s < 0) | (s >= slen - 1), F32(0), f)
    s = np.clip(s, 0, slen - 1)
    return s, np.minimum(s + 1, slen - 1), (F32(1) - f).astype(np.float64), f.astype(np.float64)


def resized_gain(gmap, w, h):
    """The float32 map `gmap` at the size of a w x h image, interpolated in float64."""
    m = np.asarray(gmap, np.float64)
    x0, x1, a0, a1 = _linear_axis(w, m.shape[1])
    y0, y1, b0, b1 = _linear_axis(h, m.shape[0])
    rows = m[:, x0] * a0 + m[:, x1] * a1
    return rows[y0] * b0[:, None] + rows[y1] * b1[:, None]


def apply_candidates(gmap, img):
    """-> (lo, hi), uint8 arrays of img's shape: the inclusive range an applied byte may take."""
    h, w = img.shape[:2]
    g = resized_gain(gmap, w, h)[:, :, None]
    band = APPLY_OPS * U24 * float(np.abs(np.asarray(gmap, np.float64)).max())
    v = img.astype(np.float64)
    lo = np.clip(np.rint(v * (g - band)), 0, 255).astype(np.uint8)
    hi = np.clip(np.rint(v * (g + band)), 0, 255).astype(np.uint8)
    return lo, hi


# ------------------------------------------------------------------------------------------------ seams
def l1_distance(feature):
    """City-block distance of every pixel to the nearest True pixel of `feature`; EMPTY_DIST everywhere when there is none."""
    if not feature.any():
        return np.full(feature.shape, EMPTY_DIST, np.int64)
    return ndimage.distance_transform_cdt(~feature, metric="taxicab").astype(np.int64)


def voronoi(corners, masks, gap=GAP):
    """-> the masks after VoronoiSeamFinder::find (copies)."""
    out = [np.array(m, np.uint8) for m in masks]
    n = len(out)
    for i in range(n - 1):
        for j in range(i + 1, n):
            (xi, yi), (xj, yj) = corners[i], corners[j]
            (hi, wi), (hj, wj) = out[i].shape, out[j].shape
            x0, y0, x1, y1 = max(xi, xj), max(yi, yj), min(xi + wi, xj + wj), min(yi + hi, yj + hj)
            if not (x0 < x1 and y0 < y1):
                continue
            sub = []
            for m, (cx, cy) in ((out[i], corners[i]), (out[j], corners[j])):
                # the frame on a canvas that holds the grown rectangle, then the cut: zero outside the frame
                px, py = x0 - gap - cx, y0 - gap - cy                      # grown rectangle's corner inside the frame (may be < 0)
                W, H = x1 - x0 + 2 * gap, y1 - y0 + 2 * gap
                big = np.pad(m, ((max(0, -py), max(0, py + H - m.shape[0])), (max(0, -px), max(0, px + W - m.shape[1]))))
                sub.append(big[max(0, py):max(0, py) + H, max(0, px):max(0, px) + W])
            collision = (sub[0] != 0) & (sub[1] != 0)
            d1 = l1_distance((sub[0] != 0) & ~collision)[gap:-gap, gap:-gap]
            d2 = l1_distance((sub[1] != 0) & ~collision)[gap:-gap, gap:-gap]
            seam = d1 < d2
            out[j][y0 - yj:y1 - yj, x0 - xj:x1 - xj][seam] = 0
            out[i][y0 - yi:y1 - yi, x0 - xi:x1 - xi][~seam] = 0
    return out


def seam_mask_apply(seam, mask):
    dil = ndimage.maximum_filter(np.asarray(seam, np.uint8), size=3, mode="constant", cval=0)
    return np.asarray(mask, np.uint8) & refimpl_orb.resize_linear_exact(dil, mask.shape[1], mask.shape[0])


# ------------------------------------------------------------------------------------------------ scenes
FRAME_GAINS = (0.72, 1.33, 0.95, 1.18)          # per frame, inside 0.7 .. 1.35: the compensator has something to find
PANO_ORIGIN = (128, 64)                         # pano (0, 0) inside the panorama array: room for negative corners
PARAMS = [(64, 64, 2), (32, 48, 0), (32, 48, 1), (17, 64, 3), (200, 200, 2)]


def _pano():
    rng = np.random.default_rng(20240)
    p = rng.integers(30, 180, (400, 800, 3)).astype(np.float64)
    return (p + np.roll(p, 1, 0) + np.roll(p, 1, 1)) / 3


_PANO = _pano()


def _frames(rects, mask_fn=None):
    """rects: (x, y, w, h) in pano coordinates -> (corners, images, masks); mask_fn(k, w, h) -> mask, default all 255."""
    corners, images, masks = [], [], []
    for k, (x, y, w, h) in enumerate(rects):
        ax, ay = x + PANO_ORIGIN[0], y + PANO_ORIGIN[1]
        assert ax >= 0 and ay >= 0 and ay + h <= _PANO.shape[0] and ax + w <= _PANO.shape[1]
        images.append(np.clip(_PANO[ay:ay + h, ax:ax + w] * FRAME_GAINS[k % 4], 0, 255).astype(np.uint8))
        masks.append(np.full((h, w), 255, np.uint8) if mask_fn is None else mask_fn(k, w, h))
        corners.append((x, y))
    return corners, images, masks


def _holes(k, w, h):
    """A slanted invalid wedge as warping leaves, plus a stray hole."""
    m = np.full((h, w), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    m[(xx + 2 * yy) < 40 + 7 * k] = 0
    m[h // 3:h // 3 + 11, w - 47 - 5 * k:w - 20 - 5 * k] = 0
    return m


def _masked_out(k, w, h):
    m = np.full((h, w), 255, np.uint8)
    if k == 0:
        m[:, 60:] = 0
    return m


def _byte_mask(k, w, h):
    rng = np.random.default_rng(77 + k)
    m = rng.integers(1, 256, (h, w)).astype(np.uint8)
    m[rng.random((h, w)) < 0.3] = 255
    m[:8] = 0
    return m


def _strip4():
    rng = np.random.default_rng(4)
    return [(70 * k + int(rng.integers(-3, 4)), int(rng.integers(-6, 7)), 130 + int(rng.integers(-4, 5)), 100 + int(rng.integers(-4, 5)))
            for k in range(4)]


SCENES = {
    "tiny": lambda: _frames([(0, 0, 40, 30), (25, 10, 37, 29)]),
    "disjoint": lambda: _frames([(0, 0, 100, 80), (200, 0, 90, 70)]),
    "single": lambda: _frames([(3, -4, 150, 100)]),
    "masked_out": lambda: _frames([(0, 0, 100, 80), (60, 5, 90, 70)], _masked_out),
    "three_way": lambda: _frames([(0, 0, 200, 150), (80, 20, 210, 140), (40, 70, 190, 160)], _holes),
    "strip4": lambda: _frames(_strip4(), _holes),
    "byte_masks": lambda: _frames([(0, 0, 150, 100), (70, 10, 140, 110)], _byte_mask),
    "contained": lambda: _frames([(0, 0, 300, 200), (100, 60, 80, 50)]),
    "identical": lambda: _frames([(5, 5, 90, 60), (5, 5, 90, 60)]),
    "thin_col": lambda: _frames([(-100, -50, 101, 90), (0, -40, 120, 70)]),
    "thin_row": lambda: _frames([(-10, -50, 101, 51), (0, 0, 120, 70)]),
    "wide": lambda: _frames([(0, 0, 300, 90), (20, 10, 300, 90)]),
}
# no block meets another's valid pixels (masked_out: the rectangles meet, every count is 0, so every I is 0 and the equations
# decouple into beta N g = beta N): every gain is exactly 1.0f
ALL_ONES = ("disjoint", "single", "masked_out")
# no pair of frames overlaps, or (masked_out) the shared rectangle is already zero in the frame that loses it: no mask changes
NO_SEAM = ("disjoint", "single", "masked_out")


def reference_maps(scene, bw, bh, nfilt, strict=False):
    """The whole feed of one scene -> (grid, gain maps)."""
    corners, images, masks = scene
    grid = block_grid(corners, [(m.shape[1], m.shape[0]) for m in masks], bw, bh)
    count, N, I = overlap_stats(corners, images, masks, grid)
    return grid, gain_maps(gains(count, N, I, strict), grid, nfilt)


# seam_mask_apply geometries: (seam h, w) -> (mask h, w)
SEAM_GEOMETRIES = [((37, 53), (211, 307)), ((211, 307), (37, 53)), ((37, 53), (37, 53)), ((37, 53), (9, 1)), ((37, 53), (9, 2)),
                   ((37, 53), (9, 3)), ((37, 53), (9, 5)), ((1, 1), (6, 7))]


def seam_case(geometry, byte_values=False):
    """A ragged seam mask with isolated zero pixels (bytes 1..254 instead of 255 when byte_values) and a compose mask with zero
    columns and scattered zeros."""
    (sh, sw), (mh, mw) = geometry
    rng = np.random.default_rng(sh * 1000 + sw + 7 * mh + mw)
    yy, xx = np.mgrid[0:sh, 0:sw]
    seam = ((xx >= (yy // 5) % 4) & (xx < sw - (yy // 3) % 5) & (yy < sh - (xx // 7) % 3)) | (sh * sw == 1)
    seam = np.where(seam, 255, 0).astype(np.uint8)
    seam[rng.random((sh, sw)) < 0.03] = 0
    if sh * sw > 1:
        seam[sh // 4:sh // 4 + 4, sw // 3:sw // 3 + 6] = 0           # a hole the dilate cannot close
        seam[sh // 2 - 2:sh // 2 + 4] = 0                            # and a band that every mask width samples
    if byte_values:
        seam = np.where(seam != 0, rng.integers(1, 255, (sh, sw)), 0).astype(np.uint8)
    mask = np.full((mh, mw), 255, np.uint8)
    mask[rng.random((mh, mw)) < 0.05] = 0
    if mw > 8:
        mask[:, mw // 4:mw // 4 + 3] = 0
    if byte_values:
        mask = np.where(mask != 0, rng.integers(1, 256, (mh, mw)), 0).astype(np.uint8)
    return seam, mask
