"""GPU: the wide Hamming 2-NN (knn2_hamming_wide_kernel: 61-byte rows, AKAZE's 486-bit MLDB) against a numpy brute force, exactly:
mis_knn2 at the count edges, mis_match_all_pairs on planted correspondences against the matcher reference of tests/refimpl.py and
tests/refimpl_homography.py fed that brute force, the refusal of mixed widths, and the 32-byte path unchanged beside it."""
import ctypes as C

import numpy as np
import pytest

import refimpl as ri
import refimpl_homography as rh
from test_refimpl_match_gpu import _assert_knn2_equal, _keypoints, hamming_edge_sets

pytestmark = pytest.mark.gpu

WIDE = 61
E_INVALID = -1


def wide_rows(rng, n):
    """n random 486-bit rows: the top two bits of byte 60 are clear, as the finder writes them"""
    d = rng.integers(0, 256, (n, WIDE), dtype=np.uint8)
    d[:, 60] &= 0x3F
    return d


def knn2_bytes_exact(q, t, chunk=128):
    """Exact Hamming 2-NN of rows of any width: popcount of XOR byte by byte, (distance, index) order (refimpl._knn2_from_dist)."""
    q, t = np.ascontiguousarray(q, np.uint8), np.ascontiguousarray(t, np.uint8)
    nq, nt = len(q), len(t)
    idx = np.full((nq, 2), -1, np.int64)
    dist = np.full((nq, 2), -1, np.int64)
    for a in range(0, nq, chunk):
        d = np.bitwise_count(q[a:a + chunk, None, :] ^ t[None, :, :]).sum(-1, dtype=np.int64) if nt else np.zeros((min(chunk, nq - a), 0), np.int64)
        idx[a:a + chunk], dist[a:a + chunk] = ri._knn2_from_dist(d, nt)
    return idx.astype(np.int32), dist


def _upload(ctx, d, i=0, size=(640, 480), kps=None):
    import image_stitching_amd as isa
    return isa.ImageFeatures.upload(ctx, size, _keypoints(len(d), i, size) if kps is None else kps, d, i)


def _knn2_rc(ctx, q, t):
    fq, ft = _upload(ctx, q), _upload(ctx, t)
    idx = np.zeros((max(len(q), 1), 2), np.int32)
    dist = np.zeros((max(len(q), 1), 2), np.float32)
    rc = ctx.lib.mis_knn2(ctx.h, C.byref(fq.raw), C.byref(ft.raw), idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p))
    return rc, idx[:len(q)], dist[:len(q)]


@pytest.mark.parametrize("nq,nt", [(1, 1), (2, 2), (255, 256), (256, 257), (257, 255), (1000, 3), (3, 1000), (5, 0), (300, 129)])
def test_knn2_wide_vs_brute_force(ctx, nq, nt):
    rng = np.random.default_rng(100 * nq + nt)
    q, t = wide_rows(rng, nq), wide_rows(rng, nt)
    if nt >= 3:      # duplicate rows: ties go to the lower train index, across the 128-row tiles too
        t[-1] = t[0]
        t[nt // 2] = t[0]
        q[0] = t[0]
        if nq > 1:
            q[-1] = ~t[0]
            q[-1, 60] &= 0x3F      # distance 486 to the duplicates
    rc, idx, dist = _knn2_rc(ctx, q, t)
    assert rc == 0
    ridx, rdist = knn2_bytes_exact(q, t)
    _assert_knn2_equal(idx, dist, ridx, rdist.astype(np.float32))
    if nt >= 3:
        assert tuple(idx[0]) == (0, nt // 2) and tuple(dist[0]) == (0.0, 0.0)
        if nq > 1 and nt == 3:
            assert np.all(dist[-1] == 486.0)


def test_the_last_row_is_not_read_past_its_end(ctx):
    """The last train and the last query row end the descriptor block: with all bits set their distance to an all-clear row is 486
    only if the three zero-filled bytes of the sixteenth dword stay zero."""
    q = np.zeros((2, WIDE), np.uint8)
    t = np.full((3, WIDE), 0xFF, np.uint8)
    t[:, 60] = 0x3F
    rc, idx, dist = _knn2_rc(ctx, q, t)
    assert rc == 0 and np.all(dist == 486.0) and np.array_equal(idx, [[0, 1], [0, 1]])


def test_match_all_pairs_wide_vs_reference(ctx, monkeypatch):
    """Three frames of AKAZE-width sets with planted correspondences under a known homography: every pair's match list, inlier mask,
    inlier count and confidence equal the matcher reference's, which is fed the numpy brute force."""
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import KP_DTYPE
    monkeypatch.setattr(ri, "knn2_exact", lambda q, t: (lambda i, d: (i, d.astype(np.float32)))(*knn2_bytes_exact(q, t)))
    rng = np.random.default_rng(61)
    sizes = [(1000, 800)] * 3
    blocks = {(0, 1): rh.synth(71, 400, 60, lim=380.0, noise=0.3), (0, 2): rh.synth(72, 120, 40, lim=380.0, noise=0.3), (1, 2): rh.synth(73, 9, 2, lim=300.0)}
    xy, desc = [[] for _ in sizes], [[] for _ in sizes]
    for (i, j), (src, dst) in sorted(blocks.items()):
        codes = wide_rows(rng, len(src))      # one code a correspondence: random codes lie ~243 +- 11 bits apart
        for f, pts in ((i, src), (j, dst)):
            half = np.array([np.float32(sizes[f][0]) * np.float32(0.5), np.float32(sizes[f][1]) * np.float32(0.5)], np.float32)
            xy[f].append((np.asarray(pts, np.float32) + half).astype(np.float32))
            desc[f].append(codes)
    frames = []
    for f, size in enumerate(sizes):
        order = rng.permutation(sum(len(a) for a in xy[f]))
        frames.append(dict(size=size, xy=np.concatenate(xy[f])[order], desc=np.concatenate(desc[f])[order]))
    infos = {}
    for (i, j) in blocks:
        m = ri.best_of_2_nearest_matches(frames[i]["desc"], frames[j]["desc"], 0.65).astype(rh.DMATCH_DTYPE)
        assert len(m) == len(blocks[(i, j)][0]), (i, j, len(m))
        infos[(i, j)] = rh.matches_info(m, frames[i]["xy"], frames[i]["size"], frames[j]["xy"], frames[j]["size"])
        infos[(i, j)].matches = m
    assert infos[(0, 1)].is_decided and infos[(0, 2)].is_decided and infos[(0, 1)].has_H and infos[(0, 1)].num_inliers > 300
    feats = []
    for i, f in enumerate(frames):
        k = np.zeros(len(f["xy"]), KP_DTYPE)
        k["x"], k["y"] = f["xy"][:, 0], f["xy"][:, 1]
        feats.append(_upload(ctx, f["desc"], i, f["size"], k))
    pm = isa.BestOf2NearestMatcher(ctx, 0.65)(feats)
    entries = [dict(src=m.src_img_idx, dst=m.dst_img_idx, matches=m.matches, inliers_mask=m.inliers_mask, num_inliers=m.num_inliers, H=m.H, confidence=m.confidence)
               for m in pm]
    rh.check_batch(dict(frames=frames), infos, entries)


def test_mixed_widths_are_refused(ctx):
    import image_stitching_amd as isa
    rng = np.random.default_rng(5)
    a, b = wide_rows(rng, 40), rng.integers(0, 256, (40, 32), dtype=np.uint8)
    rc, _, _ = _knn2_rc(ctx, a, b)
    assert rc == E_INVALID and "32 and of 61" in ctx.lib.mis_last_error(ctx.h).decode()
    feats = [_upload(ctx, a, 0), _upload(ctx, b, 1), _upload(ctx, wide_rows(rng, 30), 2)]
    with pytest.raises(isa.MisError) as e:
        isa.BestOf2NearestMatcher(ctx, 0.65)(feats)
    assert e.value.code == E_INVALID


def test_the_32_byte_path_is_what_it_was(ctx):
    """A 32-byte call before and after wide calls on the same context: mis_knn2 equals the pinned reference bit for bit, and the
    all-pairs lists of 32-byte sets equal mis_knn2's neighbours put through the reference's ratio rule."""
    import image_stitching_amd as isa
    rng = np.random.default_rng(9)
    q, t = hamming_edge_sets(rng, 300, 700)

    def knn32():
        fq, ft = _upload(ctx, q), _upload(ctx, t)
        idx, dist = np.zeros((len(q), 2), np.int32), np.zeros((len(q), 2), np.float32)
        ctx.check(ctx.lib.mis_knn2(ctx.h, C.byref(fq.raw), C.byref(ft.raw), idx.ctypes.data_as(C.c_void_p), dist.ctypes.data_as(C.c_void_p)))
        return idx, dist
    before = knn32()
    assert _knn2_rc(ctx, wide_rows(rng, 50), wide_rows(rng, 60))[0] == 0
    after = knn32()
    assert np.array_equal(before[0], after[0]) and before[1].tobytes() == after[1].tobytes()
    _assert_knn2_equal(after[0], after[1], *ri.knn2_hamming_exact(q, t))
    pm = isa.BestOf2NearestMatcher(ctx, 0.32)([_upload(ctx, q, 0), _upload(ctx, t, 1)])
    ref = ri.best_of_2_nearest_matches(q, t, 0.32)
    assert np.array_equal(pm[1].matches, ref.astype(pm[1].matches.dtype))
