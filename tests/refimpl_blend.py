"""Plain numpy reference of cv::detail::Blender, FeatherBlender and MultiBandBlender (OpenCV 4.x, CV_32F weights) and of the
reference program's blender sizing, written from OpenCV's documented semantics.

Nothing here calls the oracle (oracle/mo_blend.c) or the product library: both are checked against these functions, so a misreading
of OpenCV that the kernels and the oracle share shows up as a disagreement with this module.  Where the oracle walks loops, the
stages here are whole-array operations (np.pad, strided slices, integer / float32 array arithmetic, scipy's distance transform).

Semantics restated (OpenCV 4.x stitching/src/blenders.cpp, imgproc/src/pyramids.cpp, imgproc/src/distransform.cpp; the sizing of
image_stitching.cpp's main()):
  * result_roi(corners, sizes): the bounding box of all frames.
  * blend_config: blend_width = sqrt((float)(w h)) * strength / 100.f, all float32 (sqrt of a float is the float overload);
    blend_width < 1 means no blending (Blender::NO); bands = (int)(ceil(log(blend_width) / log(2.)) - 1.), where log of the
    float blend_width is the float overload (logf, correctly rounded here) and only the division is in float64 -- at a
    blend_width of exactly 2^k that gives k bands, not k - 1; sharpness = 1.f / blend_width.
  * MultiBandBlender::prepare: bands = min(requested, (int)ceil(log(max_len) / log(2.0))), max_len = max(w, h) of the roi, in
    float64 exactly as written; the roi is padded on the right / bottom to multiples of 2^bands; level l + 1 has
    ((n + 1) / 2) rows and columns of level l (exact halves, by the padding).  Accumulators start at zero.
  * feed tile (feed_tile): gap = 3 * 2^bands; [tl - gap, br + gap) clamped to the padded roi; the top-left snapped down to a
    multiple of 2^bands relative to the roi; the size rounded up to a multiple of 2^bands; the tile shifted back (left / up) by
    what its bottom-right overshoots the padded roi; margins top / left / bottom / right around the frame.  The roi being padded
    to multiples of 2^bands, that shift-back is never taken inside a blender (test_feed_tile_invariants asserts it).
  * Laplacian pyramid of the tile: copyMakeBorder(BORDER_REFLECT) of the 16SC3 frame (np.pad "symmetric": edge pixel repeated,
    folded as many times as the margins need); G_{l+1} = pyrDown(G_l): [1 4 6 4 1] x [1 4 6 4 1] with BORDER_REFLECT_101,
    (v + 128) >> 8 in integers; L_l = saturate_cast<short>(G_l - pyrUp(G_{l+1})), L_bands = G_bands.  pyrUp (s16): even outputs
    s[x-1] + 6 s[x] + s[x+1], odd outputs 4 (s[x] + s[x+1]), rows and columns alike; the left / top neighbour of sample 0 is
    sample 1 (REFLECT_101; sample 0 itself when the length is 1), the right / bottom neighbour of the last sample is that sample;
    (v + 32) >> 6.  Inside a blender every pyrDown halves exactly and every pyrUp doubles exactly: asserted, the odd-size
    branches of pyramids.cpp are not restated.
  * weights: mask.convertTo(CV_32F, 1/255.) = mask * (float)(1/255.) in float32, copyMakeBorder(BORDER_CONSTANT 0) to the tile;
    W_{l+1} = pyrDown(W_l) in float32: per row ((s[2x] * 6 + (s[2x-1] + s[2x+1]) * 4) + s[2x-2]) + s[2x+2], then the same over
    the five row sums, then * (1/256), one float32 rounding per operation (numpy does not contract).
    NOT PINNED: this association is the one reading that cannot be settled offline.  pyramids.cpp states the kernel, not the
    order of the float additions, and SIMD builds of OpenCV may associate differently.  The oracle and the library
    use the same order; DESIGN.md section 2 lists it as parity-unpinned.
  * accumulate (every level l, the tile rectangle with its corner and far corner halved by integer division per level):
    dst = (short)(dst + (short)((float)L * W)) -- the float product truncated toward zero, the 16-bit sum wrapping -- and
    wsum = wsum + W in float32, in feed order.
  * blend: every level normalised, L = (short)((float)L / (wsum + 1e-5f)) (truncation; the quotient always fits 16 bits,
    asserted); collapsed from the coarsest level, G_l = saturate_cast<short>(pyrUp(G_{l+1}) + L_l); cropped to the un-padded roi
    (dst_roi_final_); mask = wsum_0 > 1e-5f ? 255 : 0; the image is zero outside the mask.  blend_columns(x0, x1) is columns
    x0 .. min(x1, width) - 1 of that result.
  * FeatherBlender: createWeightMap = distanceTransform(mask, DIST_L1, 3) -- the exact city-block distance to the nearest zero
    pixel, as float32 of (int distance << 16) capped at DIST_MAX = INT_MAX >> 2, times 2^-16: every distance above 8192, and the
    "no zero anywhere" of a frame without zeros, becomes 8192.0f -- then multiply by sharpness (float32) and THRESH_TRUNC at 1:
    W = min(1, (float)d * sharpness).  Accumulated at level 0 as above (no pyramid); blend = normalise, crop, mask as above.
  * Blender (plain): where mask != 0 the frame's pixel overwrites the panorama's (the later frame wins), the panorama mask is
    OR-ed with the frame's mask bytes; blend: the image zero where the OR-ed mask is 0, and the mask returned is that OR (its
    bytes, not 255).
"""
import math

import numpy as np

BLEND_NO, BLEND_FEATHER, BLEND_MULTI_BAND = 0, 1, 2
F32 = np.float32
WEIGHT_EPS = F32(1e-5)
INV255 = F32(1.0 / 255.0)
INV256 = F32(1.0 / 256.0)
DIST_CAP = 8192                 # float((INT_MAX >> 2) * 2^-16) = 8192.0f


# ------------------------------------------------------------------------------------------------ sizing
def result_roi(corners, sizes):
    c = np.asarray(corners, np.int64).reshape(-1, 2)
    s = np.asarray(sizes, np.int64).reshape(-1, 2)
    tl, br = c.min(axis=0), (c + s).max(axis=0)
    return int(tl[0]), int(tl[1]), int(br[0] - tl[0]), int(br[1] - tl[1])


def blend_config(btype, strength, w, h):
    """image_stitching.cpp's blender sizing -> (type, bands, sharpness)."""
    bw = F32(np.sqrt(F32(w * h))) * F32(strength) / F32(100)
    if bw < F32(1):
        return BLEND_NO, 0, 0.0
    if btype == BLEND_MULTI_BAND:
        log_bw = float(F32(math.log(float(bw))))          # logf(blend_width): float32, correctly rounded
        return btype, int(math.ceil(log_bw / math.log(2.0)) - 1.0), 0.0
    if btype == BLEND_FEATHER:
        return btype, 0, float(F32(1) / bw)
    return btype, 0, 0.0


def band_crop(requested, w, h):
    return min(requested, int(math.ceil(math.log(float(max(w, h))) / math.log(2.0))))


def feed_tile(roi, nb, tl, size):
    """MultiBandBlender::feed's tile -> (x, y, width, height, (top, left, bottom, right)); roi = the padded (x, y, w, h)."""
    q = 2 ** nb
    gap = 3 * q
    rx, ry, rw, rh = roi
    (fx, fy), (fw, fh) = tl, size
    lo = np.maximum([rx, ry], [fx - gap, fy - gap])
    hi = np.minimum([rx + rw, ry + rh], [fx + fw + gap, fy + fh + gap])
    lo = np.array([rx, ry]) + (lo - [rx, ry]) // q * q
    ext = -(-(hi - lo) // q) * q
    lo = lo - np.maximum(lo + ext - [rx + rw, ry + rh], 0)
    x, y = int(lo[0]), int(lo[1])
    W, H = int(ext[0]), int(ext[1])
    return x, y, W, H, (fy - y, fx - x, y + H - fy - fh, x + W - fx - fw)


# ------------------------------------------------------------------------------------------------ pyramids
def _pad101(a, axis, n):
    """BORDER_REFLECT_101 by n samples on both ends of `axis` (np.pad "reflect"; a length-1 axis repeats its sample)."""
    if a.shape[axis] == 1:
        return np.repeat(a, 2 * n + 1, axis=axis)
    pw = [(0, 0)] * a.ndim
    pw[axis] = (n, n)
    return np.pad(a, pw, mode="reflect")


def _take(a, axis, start, stop, step=1):
    sl = [slice(None)] * a.ndim
    sl[axis] = slice(start, stop, step)
    return a[tuple(sl)]


def pyr_down_s16(g):
    """[h, w, 3] int16, h and w even -> [h / 2, w / 2, 3]."""
    h, w = g.shape[:2]
    assert h % 2 == 0 and w % 2 == 0, "a blender's pyrDown halves exactly"
    v = g.astype(np.int32)
    for axis, n in ((0, h // 2), (1, w // 2)):
        p = _pad101(v, axis, 2)
        t = [_take(p, axis, k, k + 2 * n, 2) for k in range(5)]
        v = 6 * t[2] + 4 * (t[1] + t[3]) + t[0] + t[4]
    return ((v + 128) >> 8).astype(np.int16)


def pyr_down_f32(wm):
    """[h, w] float32, h and w even -> [h / 2, w / 2]: rows, then columns, then * 1/256, in the stated order."""
    h, w = wm.shape
    assert h % 2 == 0 and w % 2 == 0 and wm.dtype == F32
    v = wm
    for axis, n in ((1, w // 2), (0, h // 2)):
        p = _pad101(v, axis, 2)
        t = [_take(p, axis, k, k + 2 * n, 2) for k in range(5)]
        v = ((t[2] * F32(6) + (t[1] + t[3]) * F32(4)) + t[0]) + t[4]
    return v * INV256


def pyr_up_s16(c):
    """[h, w, 3] int16 -> [2h, 2w, 3]."""
    v = c.astype(np.int32)
    for axis in (0, 1):
        n = v.shape[axis]
        left = _take(v, axis, 1, 2) if n > 1 else _take(v, axis, 0, 1)
        p = np.concatenate([left, v, _take(v, axis, n - 1, n)], axis=axis)
        prev, cur, nxt = _take(p, axis, 0, n), _take(p, axis, 1, n + 1), _take(p, axis, 2, n + 2)
        even, odd = prev + 6 * cur + nxt, 4 * (cur + nxt)
        v = np.stack([even, odd], axis=axis + 1).reshape(v.shape[:axis] + (2 * n,) + v.shape[axis + 1:])
    return ((v + 32) >> 6).astype(np.int16)


def sat16(v):
    return np.clip(v, -32768, 32767).astype(np.int16)


def laplace_pyr(tile, nb):
    """Laplacian pyramid (int16) of a reflect-padded tile."""
    g = [tile.astype(np.int16)]
    for _ in range(nb):
        g.append(pyr_down_s16(g[-1]))
    return [sat16(g[l].astype(np.int32) - pyr_up_s16(g[l + 1])) for l in range(nb)] + [g[nb]]


def weight_pyr(mask, pads, nb):
    top, left, bottom, right = pads
    w0 = np.pad(mask.astype(F32) * INV255, ((top, bottom), (left, right)), mode="constant")
    out = [w0]
    for _ in range(nb):
        out.append(pyr_down_f32(out[-1]))
    return out


# ------------------------------------------------------------------------------------------------ feather weights
def l1_distance(mask):
    """distanceTransform(mask, DIST_L1, 3) as integers capped at 8192 (no zero anywhere: 8192)."""
    m = np.asarray(mask) != 0
    try:
        from scipy import ndimage
        d = ndimage.distance_transform_cdt(m, metric="taxicab").astype(np.int64)
    except ImportError:
        d = _l1_distance_separable(m)
    d[d < 0] = DIST_CAP
    return np.minimum(d, DIST_CAP)


def _l1_distance_separable(m):
    """min over y' of |y - y'| + (distance to the nearest zero of row y' at x): exact, without scipy."""
    h, w = m.shape
    big = 1 << 40
    xs = np.arange(w)
    row = np.full((h, w), big, np.int64)
    for y in range(h):
        z = np.flatnonzero(~m[y])
        if z.size:
            k = np.clip(np.searchsorted(z, xs), 1, z.size) - 1
            k2 = np.minimum(k + 1, z.size - 1)
            row[y] = np.minimum(np.abs(xs - z[k]), np.abs(xs - z[k2]))
    ys = np.arange(h)
    d = np.min(row[None, :, :] + np.abs(ys[:, None] - ys[None, :])[:, :, None], axis=1) if h * h * w <= 1 << 26 else \
        np.stack([np.min(row + np.abs(ys - y)[:, None], axis=0) for y in range(h)])
    d[d >= big] = -1
    return d


def feather_weights(mask, sharpness):
    return np.minimum(l1_distance(mask).astype(F32) * F32(sharpness), F32(1))


# ------------------------------------------------------------------------------------------------ blenders
class Blender:
    """Blender / FeatherBlender / MultiBandBlender after prepare(corners, sizes)."""

    def __init__(self, btype, num_bands=5, sharpness=0.02):
        self.type, self.requested, self.sharpness = btype, num_bands, F32(sharpness)

    def prepare(self, corners, sizes):
        x, y, w, h = result_roi(corners, sizes)
        self.final = (w, h)
        self.nb = 0
        if self.type == BLEND_MULTI_BAND:
            self.nb = band_crop(self.requested, w, h)
            q = 2 ** self.nb
            w, h = -(-w // q) * q, -(-h // q) * q
        self.roi = (x, y, w, h)
        self.lap = [np.zeros((h >> l, w >> l, 3), np.int16) for l in range(self.nb + 1)]
        self.wgt = [np.zeros((h >> l, w >> l), F32) for l in range(self.nb + 1)]
        self.mask = np.zeros((h, w), np.uint8)
        for l in range(self.nb + 1):
            assert self.lap[l].shape[:2] == (-(-h // 2 ** l), -(-w // 2 ** l))
        return self

    def tile(self, tl, size):
        return feed_tile(self.roi, self.nb, tl, size)

    def _add(self, l, y0, x0, src, wm):
        h, w = wm.shape
        d = self.lap[l][y0:y0 + h, x0:x0 + w]
        c = np.trunc(src.astype(F32) * wm[:, :, None]).astype(np.int32)
        d[...] = (d.astype(np.int32) + c).astype(np.int16)
        self.wgt[l][y0:y0 + h, x0:x0 + w] += wm

    def feed(self, img, mask, tl):
        img, mask = np.asarray(img, np.int16), np.asarray(mask, np.uint8)
        h, w = mask.shape
        rx, ry = self.roi[:2]
        dx, dy = tl[0] - rx, tl[1] - ry
        assert dx >= 0 and dy >= 0 and dx + w <= self.final[0] and dy + h <= self.final[1], "frame outside the roi"
        if self.type == BLEND_NO:
            m = mask != 0
            self.lap[0][dy:dy + h, dx:dx + w][m] = img[m]
            self.mask[dy:dy + h, dx:dx + w] |= mask
        elif self.type == BLEND_FEATHER:
            self._add(0, dy, dx, img, feather_weights(mask, self.sharpness))
        else:
            x, y, W, H, pads = self.tile(tl, (w, h))
            top, left, bottom, right = pads
            assert min(pads) >= 0 and W % 2 ** self.nb == 0 and H % 2 ** self.nb == 0
            tile = np.pad(img, ((top, bottom), (left, right), (0, 0)), mode="symmetric")
            laps, wps = laplace_pyr(tile, self.nb), weight_pyr(mask, pads, self.nb)
            x0, y0 = x - rx, y - ry
            for l in range(self.nb + 1):
                self._add(l, y0, x0, laps[l], wps[l])
                x0, y0 = x0 // 2, y0 // 2
        return self

    def levels(self):
        return [(self.lap[l].copy(), self.wgt[l].copy()) for l in range(self.nb + 1)]

    def blend(self):
        fw, fh = self.final
        if self.type == BLEND_NO:
            m = self.mask[:fh, :fw]
            return np.where(m[:, :, None] != 0, self.lap[0][:fh, :fw], 0).astype(np.int16), m.copy()
        norm = []
        for lap, wgt in zip(self.lap, self.wgt):
            q = np.trunc(lap.astype(F32) / (wgt + WEIGHT_EPS)[:, :, None])
            assert np.all(np.abs(q) <= 32767), "a normalised sum outside 16 bits"
            norm.append(q.astype(np.int16))
        cur = norm[-1]
        for l in range(self.nb - 1, -1, -1):
            up = pyr_up_s16(cur)
            assert up.shape == norm[l].shape, "a blender's pyrUp doubles exactly"
            cur = sat16(up.astype(np.int32) + norm[l])
        m = self.wgt[0][:fh, :fw] > WEIGHT_EPS
        return np.where(m[:, :, None], cur[:fh, :fw], 0).astype(np.int16), (m * 255).astype(np.uint8)

    def blend_columns(self, x0, x1, full=None):
        img, m = self.blend() if full is None else full
        x1 = min(x1, self.final[0])
        return img[:, x0:x1], m[:, x0:x1]


def blend_frames(btype, frames, num_bands=5, sharpness=0.02):
    """frames: [(int16 image, uint8 mask, (x, y))] -> the prepared-and-fed reference Blender."""
    b = Blender(btype, num_bands, sharpness).prepare([f[2] for f in frames], [(f[1].shape[1], f[1].shape[0]) for f in frames])
    for img, mask, tl in frames:
        b.feed(img, mask, tl)
    return b
