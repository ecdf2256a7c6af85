"""Plain numpy references of the image operators either side of the hot path, written from OpenCV's semantics:
cv::resize(..., INTER_LINEAR_EXACT) on 8-bit images of 1 or 3 channels, and cv::rotate.

Nothing here calls the oracle (oracle/mo_imgops.c) or the product library (csrc/imgops.hip): both are checked against these
functions, so a misreading the two share shows up as a disagreement with this module.

resize: the destination size is cvRound(size * f) (half to even) when it is not given, and inv_scale = f; given a size,
inv_scale = dsize / ssize.  Destination index i samples the source at (i + 0.5) * (1 / inv_scale) - 0.5, in float64.  Inside
[0, len - 1) the two neighbouring samples are weighted 256 - w and w with w = rint(frac * 256) (8.8 fixed point, ties to even);
outside, the edge sample alone.  The horizontal pass comes first and fits 16 bits (255 * 256 at most: asserted), then the
vertical pass with one rounding, (v + 2^15) >> 16.
"""
import numpy as np

ROTATE_90_CLOCKWISE, ROTATE_180, ROTATE_90_COUNTERCLOCKWISE = 0, 1, 2


def cv_round(v):
    return int(np.rint(np.float64(v)))


def axis_table(slen, dlen, inv_scale):
    """-> (i0, i1, w): destination index d takes sample i0[d] with weight 256 - w[d] and i1[d] with weight w[d]."""
    scale = 1.0 / np.float64(inv_scale)
    pos = (np.arange(dlen, dtype=np.float64) + 0.5) * scale - 0.5
    fl = np.floor(pos)
    w = np.rint((pos - fl) * 256.0).astype(np.int64)
    i0 = fl.astype(np.int64)
    low, high = pos < 0, pos >= slen - 1
    i0[low], w[low] = 0, 0
    i0[high], w[high] = slen - 1, 0
    return i0, np.minimum(i0 + 1, slen - 1), w


def geometry(sw, sh, dsize=None, fx=0.0, fy=0.0):
    """-> (dw, dh, inv_scale_x, inv_scale_y) as cv::resize derives them"""
    if dsize:
        dw, dh = int(dsize[0]), int(dsize[1])
        return dw, dh, np.float64(dw) / np.float64(sw), np.float64(dh) / np.float64(sh)
    return cv_round(sw * np.float64(fx)), cv_round(sh * np.float64(fy)), np.float64(fx), np.float64(fy)


def resize_linear_exact(src, dsize=None, fx=0, fy=0):
    src = np.asarray(src)
    assert src.dtype == np.uint8 and (src.ndim == 2 or (src.ndim == 3 and src.shape[2] in (1, 3)))
    sh, sw = src.shape[:2]
    dw, dh, ix, iy = geometry(sw, sh, dsize, fx, fy)
    assert dw > 0 and dh > 0
    x0, x1, wx = axis_table(sw, dw, ix)
    y0, y1, wy = axis_table(sh, dh, iy)
    s = src.astype(np.int64)
    wxb = wx.reshape((1, dw) + (1,) * (src.ndim - 2))
    h = s[:, x0] * (256 - wxb) + s[:, x1] * wxb
    assert h.max() < 1 << 16
    wyb = wy.reshape((dh, 1) + (1,) * (src.ndim - 2))
    v = h[y0] * (256 - wyb) + h[y1] * wyb
    out = (v + (1 << 15)) >> 16
    assert out.max() <= 255
    return out.astype(np.uint8)


def rotate(src, code):
    """cv::rotate: 0 = 90 degrees clockwise, 1 = 180, 2 = 90 counter-clockwise"""
    return np.ascontiguousarray(np.rot90(np.asarray(src), {0: -1, 1: 2, 2: 1}[code], axes=(0, 1)))


# ------------------------------------------------------------------------------------------------ the cases both test files use
SRC_W = (1, 2, 3, 4, 5, 7, 8, 13, 16, 17, 20, 64)
SRC_H = (1, 2, 3, 9)
DST_W = (1, 2, 3, 4, 5, 6, 7, 8, 9, 64, 65, 255, 256, 257)
DST_H = (1, 2, 7, 8, 9, 17)
# (source h, w, fx, fy): 0.5 on odd sizes (5 -> 2, 7 -> 4, 3 -> 2: cvRound's ties), the factors of the jobs' kind, 256 (every
# interior weight a tie), 1.  77 x 132 and 76 x 133 at 0.5: called by size straight afterwards, one axis keeps its scale (exactly 2)
# and the other does not (77 / 38, 133 / 66) -- the two halves of the table cache's key, one at a time
BY_FACTOR = [(5, 7, 0.5, 0.5), (3, 5, 0.5, 0.5), (7, 3, 0.5, 0.5), (77, 133, 0.5, 0.5), (77, 132, 0.5, 0.5), (76, 133, 0.5, 0.5), (31, 47, 1.0 / 3.0, 1.0 / 3.0), (90, 150, 0.08, 0.08),
             (23, 37, 1.7, 1.7), (50, 90, 1.7, 2.3), (9, 13, 2.0, 2.0), (3, 4, 256.0, 256.0), (33, 65, 1.0, 1.0)]
ROTATE_SIZES = [(1, 1), (300, 1), (1, 300), (3, 255), (3, 256), (3, 257), (161, 97)]        # (h, w)


def image(h, w, c, kind, seed=0):
    """kind: "rand", "ramp" (a different value in every byte up to wrap-around: misplaced pixels and channels show), "full" (255)"""
    shape = (h, w) if c == 1 else (h, w, c)
    if kind == "full":
        return np.full(shape, 255, np.uint8)
    if kind == "ramp":
        return (np.arange(h * w * c, dtype=np.int64) * 7 % 251).astype(np.uint8).reshape(shape)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def sweep():
    """-> [(sw, sh, dw, dh)]: the smallest geometries at which the kernels branch (the ragged four-pixel group, a row pair with
    one row, the second x block of the single kernel, sources narrower than a dword group)"""
    return [(sw, sh, dw, dh) for sw in SRC_W for sh in SRC_H for dw in DST_W for dh in DST_H]
