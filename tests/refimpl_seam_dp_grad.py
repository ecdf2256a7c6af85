"""Plain numpy reference of cv::detail::DpSeamFinder(DpSeamFinder::COLOR_GRAD) ("dp_colorgrad", image_stitching.cpp:1057-1058): the
gradient planes of DpSeamFinder::computeGradients and `find` with the COLOR_GRAD branch of DpSeamFinder::computeCosts.  Everything
but the cost step is refimpl_seam_dp.py (imported, not edited); nothing here calls the oracle or the product library.

The gradients (whole-array float32 operations, each rounded; the product's kernel, csrc/seam_grad.hip, performs the same ones):
    g           = (B * 0.114f + G * 0.587f) + R * 0.299f                                    cvtColor(BGR2GRAY) on CV_32F
    gradx(y, x) = (d(y - 1, x) + 2 d(y, x)) + d(y + 1, x),   d(y, x) = g(y, x + 1) - g(y, x - 1)        Sobel(gray, CV_32F, 1, 0)
    grady(y, x) = s(y + 1, x) - s(y - 1, x),                 s(y, x) = (g(y, x - 1) + 2 g(y, x)) + g(y, x + 1)   Sobel(gray, CV_32F, 0, 1)
with BORDER_REFLECT_101 (index -1 is 1, index n is n - 2; a dimension of length 1 reflects to index 0), per whole image.
PARITY UNPINNED: the association of the three-term sums and the absence of FMA in OpenCV's grey conversion are recalled, not
observed.  `gradients64` is the same filter in float64, the ground truth of the rounding bound.

The costs (float32): with costColor the COLOR cost of the cut,
    costV(y, x) = costColor / ((((|gradx1(y, x)| + |gradx1(y, x - 1)|) + |gradx2(y, x)|) + |gradx2(y, x - 1)|) + 1.f)
    costH(y, x) = costColor / ((((|grady1(y, x)| + |grady1(y - 1, x)|) + |grady2(y, x)|) + |grady2(y - 1, x)|) + 1.f)
each image's plane read at the pixel's position in that image; the bad-region cost is not divided.  The costs are no longer
half-integers, so float32 is the only dynamic programme (refimpl_seam_dp's dp="float32", additions associated as written).
"""
import collections

import numpy as np

import refimpl_seam_dp as rs

F32 = np.float32
WB, WG, WR = F32(0.114), F32(0.587), F32(0.299)


def reflect101(p, n):
    """BORDER_REFLECT_101 for p in [-1, n]: one fold."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    return np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))


def _sobel(g, two):
    h, w = g.shape
    gp = g[reflect101(np.arange(-1, h + 1), h)][:, reflect101(np.arange(-1, w + 1), w)]
    d = gp[:, 2:] - gp[:, :-2]                                  # the row pass, on the h + 2 rows
    s = (gp[:, :-2] + two * gp[:, 1:-1]) + gp[:, 2:]
    return (d[:-2] + two * d[1:-1]) + d[2:], s[2:] - s[:-2]     # the column pass


def gradients(image):
    """8UC3 (B, G, R) -> (gradx, grady), float32, the operation order of the module docstring."""
    f = np.asarray(image).astype(F32)
    g = (f[..., 0] * WB + f[..., 1] * WG) + f[..., 2] * WR
    gx, gy = _sobel(g, F32(2))
    assert g.dtype == gx.dtype == gy.dtype == F32
    return gx, gy


def gradients64(image):
    """The same filter in float64 (the float32 weights, converted exactly)."""
    f = np.asarray(image).astype(np.float64)
    g = (f[..., 0] * float(WB) + f[..., 1] * float(WG)) + f[..., 2] * float(WR)
    return _sobel(g, 2.0)


class _PairGrad(rs._Pair):
    def __init__(self, grads1, grads2, *args):
        super().__init__(*args)
        self.G = []
        for (gx, gy), sl in ((grads1, self.s1), (grads2, self.s2)):
            px = np.zeros((self.uh, self.uw), F32); px[sl] = gx
            py = np.zeros((self.uh, self.uw), F32); py[sl] = gy
            self.G.append((px, py))

    # computeCosts, COLOR_GRAD: float32, returned DOUBLED (exact), because refimpl_seam_dp._dp halves what it is given
    def costs(self, L, box):
        y0, y1, x0, x1 = box
        c2v, c2h = super().costs(L, box)                         # the doubled COLOR costs over the box, the bad cost where not ok
        (gx1, gy1), (gx2, gy2) = self.G
        a = np.abs
        dv = np.ones((self.uh, self.uw), F32)
        dv[:, 1:] = (((a(gx1[:, 1:]) + a(gx1[:, :-1])) + a(gx2[:, 1:])) + a(gx2[:, :-1])) + F32(1)
        okv = np.zeros((self.uh, self.uw), bool)
        okv[:, 1:] = L[:, 1:] & L[:, :-1]
        dh = np.ones((self.uh, self.uw), F32)
        dh[1:, :] = (((a(gy1[1:, :]) + a(gy1[:-1, :])) + a(gy2[1:, :])) + a(gy2[:-1, :])) + F32(1)
        okh = np.zeros((self.uh, self.uw), bool)
        okh[1:, :] = L[1:, :] & L[:-1, :]
        out = []
        for c2, den, ok in ((c2v, dv, okv), (c2h, dh, okh)):
            color = c2.astype(F32) / F32(2)
            den, ok = den[y0:y1, x0:x1], ok[y0:y1, x0:x1]
            cost = np.where(ok, color / den, color)
            assert cost.dtype == F32
            out.append(F32(2) * cost)
        return out[0], out[1]


def find(images, corners, masks, *, tie_order="reversed", trace=None, seams=None):
    """DpSeamFinder(COLOR_GRAD)::find; arguments and result as refimpl_seam_dp.find."""
    trace = collections.Counter() if trace is None else trace
    seams = [] if seams is None else seams
    out = [np.array(m, np.uint8) for m in masks]
    n = len(out)
    if n == 0:
        return out
    grads = [gradients(i) for i in images]
    sizes = [(m.shape[1], m.shape[0]) for m in out]
    pairs, _ = rs.pair_order(corners, sizes, tie_order)
    for i, j in pairs:
        (x1, y1), (x2, y2), (w1, h1), (w2, h2) = corners[i], corners[j], sizes[i], sizes[j]
        if max(x1, x2) >= min(x1 + w1, x2 + w2) or max(y1, y2) >= min(y1 + h1, y2 + h2):
            continue
        _PairGrad(grads[i], grads[j], np.asarray(images[i], np.int64), np.asarray(images[j], np.int64), corners[i], corners[j], out[i], out[j],
                  "float32", False, trace, seams, "pair (%d, %d)" % (i, j)).run(out[i], out[j])
    return out


def edge_scene():
    """Two overlapping textured frames with a strong vertical edge inside the overlap, wavy so that no straight cut follows it:
    COLOR cuts where the frames' noise happens to agree, COLOR_GRAD along the edge (its cuts cost 1 / gradient there)."""
    w, h = 56, 40
    images, corners, masks = [], [(0, 0), (24, 3)], []
    for k, (cx, cy) in enumerate(corners):
        rng = np.random.default_rng(5700 + k)
        y, x = np.mgrid[0:h, 0:w]
        gx, gy = x + cx, y + cy
        v = np.stack([90 + 0.6 * gx + 0.4 * gy, 120 - 0.5 * gx + 0.3 * gy, 100 + 0.2 * gx - 0.4 * gy], -1)
        v += 90 * (gx > 40 + 5 * np.sin(gy / 4.0))[..., None]
        v += rng.integers(-12, 13, v.shape)
        images.append(np.clip(np.rint(v), 0, 255).astype(np.uint8))
        masks.append(np.full((h, w), 255, np.uint8))
    return images, corners, masks
