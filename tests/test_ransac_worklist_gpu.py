"""GPU parity of the RANSAC hypothesis work list (homography.hip): draw_kernel appends every phase's blocks of hypotheses to a
per-batch list, the persistent solve and count kernels drain it by ticket, and the last count workgroup empties it again.  Every
case compares isa.find_homography with the oracle bit for bit: H as u64, the mask and ok."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PHASE0 = 128        # hypotheses of the first RANSAC phase (homography.hip)
MAX_ITERS = [1, 4, 63, 64, 65, 127, 128, 129, 2000, 3000]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check(ctx, oracle_mod, src, dst, max_iters):
    import image_stitching_amd as isa
    ok_o, H_o, mask_o, iters_o = oracle_mod.find_homography_ransac(src, dst, max_iters=max_iters)
    ok_g, H_g, mask_g = isa.find_homography(ctx, src, dst, max_iters=max_iters)
    assert ok_g == ok_o, (max_iters, len(src))
    assert np.array_equal(mask_g, mask_o), (max_iters, len(src))
    if ok_o:
        assert np.array_equal(_bits(H_g), _bits(H_o)), (max_iters, len(src), H_g - H_o)
    return iters_o


def _projective(rng, n, outlier_frac, noise=0.4):
    H = np.array([[0.97, 0.03, 25.0], [-0.02, 1.03, -14.0], [2e-5, -1e-5, 1.0]])
    src = rng.uniform(-900, 900, (n, 2)).astype(np.float32)
    p = np.c_[src, np.ones(n)] @ H.T
    dst = (p[:, :2] / p[:, 2:] + rng.normal(0, noise, (n, 2))).astype(np.float32)
    no = int(n * outlier_frac)
    dst[:no] = rng.uniform(-900, 900, (no, 2)).astype(np.float32)
    return src, dst


def _noise(rng, n):
    return rng.uniform(-500, 500, (n, 2)).astype(np.float32), rng.uniform(-500, 500, (n, 2)).astype(np.float32)


@pytest.mark.parametrize("max_iters", MAX_ITERS)
def test_block_edges_small_n(ctx, oracle_mod, max_iters):
    """n = 3 and 4 never reach the list (no RANSAC); n = 5 does, clean and with one outlier."""
    rng = np.random.default_rng(500 + max_iters)
    for n in (3, 4, 5):
        _check(ctx, oracle_mod, *_projective(rng, n, 0.0), max_iters)
    _check(ctx, oracle_mod, *_projective(rng, 5, 0.2), max_iters)


@pytest.mark.parametrize("max_iters", MAX_ITERS)
def test_block_edges_outliers(ctx, oracle_mod, max_iters):
    """Half outliers: the adaptive count lands in phase 1 (a few hundred hypotheses) unless max_iters cuts it short."""
    rng = np.random.default_rng(600 + max_iters)
    _check(ctx, oracle_mod, *_projective(rng, 300, 0.5), max_iters)
    _check(ctx, oracle_mod, *_projective(rng, 40, 0.6), max_iters)


@pytest.mark.parametrize("max_iters", MAX_ITERS)
def test_pure_noise_fills_the_list(ctx, oracle_mod, max_iters):
    """No model: niters stays at max_iters, so every block of both phases is on the list."""
    rng = np.random.default_rng(700 + max_iters)
    it = _check(ctx, oracle_mod, *_noise(rng, 200), max_iters)
    assert it == max_iters


@pytest.mark.parametrize("max_iters", [4, 129, 2000])
def test_collinear_sources_leave_the_list_empty(ctx, oracle_mod, max_iters):
    """checkSubset rejects every subset: draw_fail, no hypothesis is listed."""
    rng = np.random.default_rng(800 + max_iters)
    for n in (5, 12, 50):
        x = rng.uniform(-100, 100, n).astype(np.float32)
        src = np.stack([x, 2 * x], 1).astype(np.float32)
        _check(ctx, oracle_mod, src, src + 1, max_iters)


def test_clean_set_finishes_in_phase0(ctx, oracle_mod):
    """A clean set converges within the first phase: the second phase's list is empty."""
    rng = np.random.default_rng(900)
    it = _check(ctx, oracle_mod, *_projective(rng, 600, 0.05), 2000)
    assert it <= PHASE0


def test_list_is_reset_between_calls(ctx, oracle_mod):
    """The same problem twice, then a larger list, then a smaller one: no call may see another's entries."""
    rng = np.random.default_rng(1000)
    mid = _projective(rng, 300, 0.5)
    big = _noise(rng, 400)
    small = _projective(rng, 60, 0.1)
    for src, dst, mi in (mid + (2000,), mid + (2000,), big + (3000,), small + (2000,), mid + (129,), big + (65,), small + (1,)):
        _check(ctx, oracle_mod, src, dst, mi)


def _feat_dict(kps, desc, size):
    return dict(img_w=size[0], img_h=size[1], xy=np.stack([kps["x"], kps["y"]], 1), desc=desc)


def test_matcher_batch_without_second_phase(ctx, oracle_mod):
    """Three strongly overlapping frames: every RANSAC problem of the matcher's first estimation finishes in phase 0, so the
    second phase's lists of the main and third chains are empty; every MatchesInfo field equals the oracle's."""
    import torch
    import synth
    import image_stitching_amd as isa
    w, h = 480, 270
    cams = [synth.make_camera(w, h, 60.0, y, p, r) for y, p, r in ((0, 0, 0), (6, 0.3, -0.2), (12, -0.2, 0.3))]
    frames = [synth.render_frame(c) for c in cams]
    finder = isa.OrbFeatureFinder(ctx, (w, h))
    feats = [isa.computeImageFeatures(finder, torch.from_numpy(f).cuda(), i) for i, f in enumerate(frames)]
    host = [f.download() for f in feats]
    pm = isa.BestOf2NearestMatcher(ctx, 0.32)(feats)
    st = np.zeros((16, 8), np.int32)
    n = ctx.lib.mis_debug_ransac_states(ctx.h, 0, st.ctypes.data_as(C.c_void_p), 16)
    st = st[:n]          # columns: n, mode, n_sub, iter, niters, draw_fail, done, max_good
    ransac = st[st[:, 1] == 2]
    assert len(ransac) > 0 and (ransac[:, 3] <= PHASE0).all(), st.tolist()
    ref = oracle_mod.match_all_pairs([_feat_dict(k, d, (w, h)) for k, d in host])
    assert len(pm) == 9
    for g, o in zip(pm, ref):
        assert g.src_img_idx == o["src_img_idx"] and g.dst_img_idx == o["dst_img_idx"]
        assert np.array_equal(g.matches, o["matches"].astype(g.matches.dtype))
        assert np.array_equal(g.inliers_mask, o["inliers_mask"])
        assert g.num_inliers == o["num_inliers"]
        assert (g.H is not None) == o["has_H"]
        if o["has_H"]:
            assert np.array_equal(_bits(g.H), _bits(o["H"]))
        assert g.confidence == o["confidence"]
