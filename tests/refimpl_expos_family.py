"""Plain numpy reference of the other members of cv::detail::ExposureCompensator's family -- GainCompensator, ChannelsCompensator,
BlocksChannelsCompensator -- and of nr_feeds > 1 for all of them, on top of tests/refimpl_expos.py (imported, left unchanged).

Semantics restated [OpenCV-upstream, recalled] (OpenCV 4.x stitching/src/exposure_compensate.cpp):
  * GainCompensator::singleFeed: refimpl_expos.overlap_stats over whole FRAMES -- the block grid with an oversized block, one
    block per frame (frame_grid).  Three-channel images: I_ij = sum norm(BGR_i) / N_ij (math.fsum: exactly rounded); one-channel
    images (the channels of ChannelsCompensator): I_ij = sum value_i / N_ij, an integer sum (channel_stats).  The normal
    equations and the un-skip rule are refimpl_expos.gains, unchanged.  The similarity threshold stays at 1: no similarity masks.
  * GainCompensator::feed with nr_feeds: for feed k > 0 every image is first multiplied in place by the gain of feed k - 1,
    cv::multiply(8U image, double scalar), which works in float32: saturate_cast<uchar>(cvRound((float)v * (float)g))
    (apply_scalar); after each feed accumulated *= gains; the result is the accumulated product.
  * ChannelsCompensator: one GainCompensator with the same nr_feeds per channel of the split image; gains[i][c].
  * BlocksCompensator<Compensator>: the inner compensator over the block grid, nr_feeds forwarded to it: between feeds the
    UNSMOOTHED per-block scalar gains multiply each block's pixels.  BlocksChannelsCompensator: a three-channel float32 map of
    (float)gains[block][c], each channel smoothed and resized as BlocksGainCompensator's one map is.

Tolerances.
  * gains (gain_tol): product and reference solve the same symmetric positive definite system A g = b in float64 from bit-equal
    statistics (the sums are exact on both sides); a backward-stable solve of n unknowns leaves a relative error of order
    n * cond_2(A) * 2^-53 in each, so |g - g_ref| <= 4 n cond_2(A_ref) 2^-52 max|g_ref| covers the two of them.
  * accumulated gains after k feeds (accumulated_tol): a product of k factors, each within its own feed's bound, and k - 1 float64
    multiplications: max|acc_ref| * (sum_f tol_f / min|g_f| + k 2^-53).  This needs every feed to see the same images on both
    sides, i.e. (float)g equal on both sides for every intermediate gain: the DECIDEDNESS condition (float32_margin): each
    intermediate reference gain is further from the nearest float32 rounding boundary than its tolerance.  The scenes are chosen
    so that the reference alone satisfies it (test_refimpl_expos_family_cpu.py asserts it).
"""
import math

import numpy as np

import refimpl_expos as rx

F32 = np.float32
U52, U53 = 2.0 ** -52, 2.0 ** -53
OVERSIZED = 1 << 20                     # a block no frame exceeds: one block per frame
TYPES = ("gain", "gain_blocks", "channels", "channels_blocks")


def is_blocks(kind):
    return kind.endswith("_blocks")


def is_channels(kind):
    return kind.startswith("channels")


def frame_grid(corners, sizes):
    g = rx.block_grid(corners, sizes, OVERSIZED, OVERSIZED)
    assert len(g.blocks) == len(sizes)
    return g


def channel_stats(corners, images, masks, grid, ch):
    """overlap_stats of one-channel images: channel `ch` of every image.  Integer sums, so I is one correctly rounded division."""
    B = grid.blocks
    nb = len(B)
    count = np.full((nb, nb), -1, np.int64)
    N = np.zeros((nb, nb), np.int64)
    I = np.zeros((nb, nb), np.float64)
    for i in range(nb):
        for j in range(i, nb):
            x0, y0 = max(B[i, 0], B[j, 0]), max(B[i, 1], B[j, 1])
            x1, y1 = min(B[i, 0] + B[i, 2], B[j, 0] + B[j, 2]), min(B[i, 1] + B[i, 3], B[j, 1] + B[j, 3])
            if not (x0 < x1 and y0 < y1):
                continue
            a, b = B[i, 4], B[j, 4]
            cut = lambda arr, k: arr[y0 - corners[k][1]:y1 - corners[k][1], x0 - corners[k][0]:x1 - corners[k][0]]
            inter = (cut(masks[a], a) == 255) & (cut(masks[b], b) == 255)
            c = int(inter.sum())
            count[i, j] = count[j, i] = c
            N[i, j] = N[j, i] = max(1, c)
            I[i, j] = int(cut(images[a], a)[..., ch][inter].astype(np.int64).sum()) / int(N[i, j])
            I[j, i] = int(cut(images[b], b)[..., ch][inter].astype(np.int64).sum()) / int(N[i, j])
    return count, N, I


def normal_matrix(count, N, I, strict=False):
    """A of refimpl_expos.gains' system over the active units, for its condition number."""
    act = np.nonzero(rx.active_blocks(count, strict))[0]
    Na, Ia = N[np.ix_(act, act)].astype(np.float64), I[np.ix_(act, act)]
    A = -2 * rx.ALPHA * Ia * Ia.T * Na
    np.fill_diagonal(A, 0.0)
    off = Na - np.diag(np.diag(Na))
    return A + np.diag(rx.BETA * Na.sum(axis=1) + 2 * rx.ALPHA * (Ia * Ia * off).sum(axis=1))


def gain_tol(count, N, I, g):
    A = normal_matrix(count, N, I)
    if not len(A):
        return 0.0
    return 4 * len(A) * float(np.linalg.cond(A, 2)) * U52 * float(np.abs(g).max())


def apply_scalar(img, g):
    """cv::multiply(8U, scalar) in float32: g a scalar or one gain per channel."""
    g32 = np.asarray(g, np.float64).astype(F32)
    return np.clip(np.rint(np.asarray(img).astype(F32) * g32), 0, 255).astype(np.asarray(img).dtype)


def float32_margin(g):
    """The relative distance of each float64 gain from the nearest float32 rounding boundary (the midpoints between (float)g and
    its two neighbours)."""
    g = np.asarray(g, np.float64)
    f = g.astype(F32)
    lo = (f.astype(np.float64) + np.nextafter(f, F32(-np.inf)).astype(np.float64)) / 2
    hi = (f.astype(np.float64) + np.nextafter(f, F32(np.inf)).astype(np.float64)) / 2
    return np.minimum(np.abs(g - lo), np.abs(hi - g)) / np.abs(g)


class Feed:
    """The result of feed(): grid; stats[f][c] = (count, N, I) of feed f, channel c; gains[f][c] = that feed's gains (one per
    unit); tol[f][c] = gain_tol of them; acc[c] = the accumulated gains."""


def feed(kind, scene, nr_feeds=1, bw=64, bh=64):
    corners, images, masks = scene
    images = [np.array(im) for im in images]                 # private copies: the scene is never altered
    sizes = [(m.shape[1], m.shape[0]) for m in masks]
    out = Feed()
    out.kind, out.nr_feeds = kind, nr_feeds
    out.grid = grid = rx.block_grid(corners, sizes, bw, bh) if is_blocks(kind) else frame_grid(corners, sizes)
    nc = 3 if is_channels(kind) else 1
    out.stats, out.gains, out.tol = [], [], []
    out.acc = [np.ones(len(grid.blocks)) for _ in range(nc)]
    for f in range(nr_feeds):
        if is_channels(kind):
            stats = [channel_stats(corners, images, masks, grid, c) for c in range(3)]
        else:
            stats = [rx.overlap_stats(corners, images, masks, grid)]
        g = [rx.gains(*s) for s in stats]
        out.stats.append(stats)
        out.gains.append(g)
        out.tol.append([gain_tol(*s, gc) for s, gc in zip(stats, g)])
        for c in range(nc):
            out.acc[c] = out.acc[c] * g[c]
        if f + 1 < nr_feeds:
            for u, (x, y, w, h, k) in enumerate(grid.blocks):
                cx, cy = corners[k]
                view = images[k][y - cy:y - cy + h, x - cx:x - cx + w]
                view[...] = apply_scalar(view, [g[c][u] for c in range(nc)] if nc == 3 else g[0][u])
    return out


def accumulated_tol(fd, c=0):
    rel = sum(fd.tol[f][c] / float(np.abs(fd.gains[f][c]).min()) for f in range(fd.nr_feeds))
    return float(np.abs(fd.acc[c]).max()) * (rel + fd.nr_feeds * U53)


def decidedness(fd):
    """-> (smallest relative float32 margin over the intermediate gains, the largest relative tolerance of one of them);
    (inf, 0) with one feed."""
    margin, tol = math.inf, 0.0
    for f in range(fd.nr_feeds - 1):
        for c, g in enumerate(fd.gains[f]):
            margin = min(margin, float(float32_margin(g).min()))
            tol = max(tol, fd.tol[f][c] / float(np.abs(g).min()))
    return margin, tol


def frame_gains(fd):
    """gains() of the frame types: (n, 3) float64 -- GainCompensator's gain three times, ChannelsCompensator's B, G, R."""
    assert not is_blocks(fd.kind)
    return np.stack([fd.acc[c if is_channels(fd.kind) else 0] for c in range(3)], axis=1)


def gain_maps(fd, nfilt):
    """The block types' maps per image: (ny, nx) for gain_blocks, (ny, nx, 3) for channels_blocks, float64 as rx.gain_maps."""
    assert is_blocks(fd.kind)
    per_channel = [rx.gain_maps(a, fd.grid, nfilt) for a in fd.acc]
    if not is_channels(fd.kind):
        return per_channel[0]
    return [np.stack([per_channel[c][k] for c in range(3)], axis=2) for k in range(len(fd.grid.shapes))]


# one pair of 422 x 237 frames: a 4K frame at seam scale (0.1 MP), so that a pair spans many row strips of the statistics kernel
SEAM_SCALE_4K = "seam_4k"


def scenes():
    s = dict(rx.SCENES)
    s[SEAM_SCALE_4K] = lambda: rx._frames([(0, 0, 422, 237), (131, 17, 422, 237)], rx._holes)
    return s
