"""Unit tests of the independent estimateAffinePartial2D / AffineBestOf2NearestMatcher reference (tests/refimpl_affine.py) and of
the configuration rules around matcher_type.  No GPU."""
import math

import numpy as np
import pytest

import refimpl_affine as ra


# ------------------------------------------------------------------------------------------------ the reference itself
def test_planted_similarity_is_recovered():
    sim = (0.8, -0.35, 120.0, -64.0)
    src, dst = ra.synth(3, 400, 120, noise=0.2, sim=sim)
    est = ra.estimate_affine_partial(src, dst)
    assert est.is_decided and est.ok
    assert 270 <= est.mask.sum() <= 285                                       # the 280 planted ones, give or take a chance outlier
    assert np.abs(ra.params_of(est.Hstar) - np.array(sim)).max() < 0.05
    assert ra.cost(est.Hstar, est.inl_src, est.inl_dst) <= ra.cost(est.M_ransac, est.inl_src, est.inl_dst)
    # the least-squares solution is a stationary point: J^T r = 0 at the size of the data's rounding
    s, d = est.inl_src.astype(np.float64), est.inl_dst.astype(np.float64)
    a, b, tx, ty = ra.params_of(est.Hstar)
    rx, ry = a * s[:, 0] - b * s[:, 1] + tx - d[:, 0], b * s[:, 0] + a * s[:, 1] + ty - d[:, 1]
    g = np.array([(s[:, 0] * rx + s[:, 1] * ry).sum(), (-s[:, 1] * rx + s[:, 0] * ry).sum(), rx.sum(), ry.sum()])
    assert np.abs(g).max() < 1e-6


def test_two_points_map_both():
    src = np.array([[10.5, -3.25], [400.0, 77.0]], np.float32)
    dst = np.array([[-20.0, 31.5], [15.75, 640.0]], np.float32)
    est = ra.estimate_affine_partial(src, dst)
    assert est.is_decided and est.ok and est.iters == 0 and est.mask.tolist() == [1, 1] and est.Hstar is None
    M = est.M_ransac
    assert M[0, 0] == M[1, 1] and M[0, 1] == -M[1, 0]
    got = np.c_[src.astype(np.float64), np.ones(2)] @ M.T
    assert np.abs(got - dst).max() < 1e-9
    for n in (0, 1):
        e = ra.estimate_affine_partial(src[:n], dst[:n])
        assert e.is_decided and not e.ok and e.iters == 0


def test_coincident_points_give_a_model_without_inliers():
    p = np.array([5.0, 6.0], np.float32)
    assert ra.hypothesis_exact(p, (1.0, 2.0), p, (3.0, 4.0)) is None
    src = np.tile(p, (20, 1))
    dst = ra.synth(7, 20, 0)[1]
    sure, maybe = ra.inlier_intervals(None, src, dst, 9.0)
    assert not sure.any() and not maybe.any()
    est = ra.estimate_affine_partial(src, dst)
    assert est.is_decided and not est.ok and est.iters == 2000 and not est.mask.any()      # every subset is still an iteration
    e2 = ra.estimate_affine_partial(src[:2], dst[:2])
    assert e2.ok and e2.M_ransac is None and e2.mask.tolist() == [1, 1]                  # n == 2: runKernel's 1 / 0, no inlier test


def test_num_iters_table_with_exponent_2():
    assert ra.update_num_iters(0.99, 0.0, 2000) == (0, False)                   # ep = 0: denom = 1 - 1 < DBL_MIN
    assert ra.update_num_iters(0.99, 1.0, 2000) == (2000, False)                # ep = 1: log(1) = 0 >= 0
    assert ra.update_num_iters(0.99, 0.5, 2000)[0] == round(math.log(0.01) / math.log(1 - 0.5 ** 2)) == 16
    assert ra.update_num_iters(0.995, 0.5, 2000)[0] == 18                       # (exponent 4 gives 82, confidence 0.995 gives 18)
    assert ra.update_num_iters(0.99, 0.5, 10)[0] == 10                          # never above the current niters
    assert ra.update_num_iters(0.99, 286 / 300, 2000)[0] == 2000                # 14 inliers of 300: 2112 > 2000
    assert ra.update_num_iters(0.99, 0.3, 2000)[0] == round(math.log(0.01) / math.log(1 - 0.7 ** 2)) == 7
    assert ra.update_num_iters(1.0, 0.5, 2000)[0] == 2000                       # p = 1: log(DBL_MIN) / log(3/4) = 2463 > 2000
    assert ra.update_num_iters(2.0, -1.0, 10) == (0, False)                     # clamped to p = 1, ep = 0
    for (n, no, seed, iters) in ra.ITER_REGIMES:
        assert iters == 2000 or ra.update_num_iters(0.99, no / n, 2000)[0] == iters, (n, no)


def test_the_bar_is_one_and_a_model_needs_two_inliers():
    """Three points in general position: every subset's model holds its own two points only; 2 > max(0, 1), so a model exists
    with exactly two inliers, and niters = log(0.01) / log(1 - (2/3)^2) = 8."""
    src = np.array([[0, 0], [100, 0], [0, 100]], np.float32)
    dst = np.array([[0, 0], [100, 0], [500, 500]], np.float32)
    est = ra.estimate_affine_partial(src, dst)
    assert est.is_decided and est.ok and est.mask.sum() == 2 and est.iters == 8


@pytest.mark.parametrize("family", sorted(ra.FAMILIES))
def test_families_are_decided(family):
    cases = ra.FAMILIES[family]()
    ests = [ra.replay(c) for c in cases]
    for c, e in zip(cases, ests):
        ra.check_expectations(c, e)
    ra.family_gate(family, ests)


def test_matches_info_reading():
    rng = np.random.default_rng(1)
    xy = rng.uniform(0, 1000, (300, 2)).astype(np.float32)
    m = np.zeros(300, ra.DMATCH_DTYPE)
    m["query_idx"] = m["train_idx"] = np.arange(300)
    info = ra.matches_info(m, xy, xy)
    assert info.has_H and info.num_inliers == 300 and info.confidence == 300 / 98.0 > 3      # identical frames: NOT zeroed
    assert not ra.matches_info(m[:5], xy, xy).has_H and ra.matches_info(m[:5], xy, xy).est is None      # below thresh1
    # the points are taken as they are: a shift of one frame's keypoints is a translation of the model, not of the centre
    info2 = ra.matches_info(m, xy, xy + np.float32(64))
    assert info2.num_inliers == 300 and np.abs(ra.params_of(info2.est.Hstar) - (1, 0, 64, 64)).max() < 1e-6


# ------------------------------------------------------------------------------------------------ the configuration rules
def test_presets_default_to_homography():
    from image_stitching_amd.stitching import StitchConfig, check_matcher_config
    assert StitchConfig().matcher_type == "homography" and StitchConfig.hot_path().matcher_type == "homography"
    assert StitchConfig.reference().matcher_type == "homography"
    assert check_matcher_config(StitchConfig.hot_path(matcher_type="affine")) == "affine"


@pytest.mark.parametrize("bad", ["nonsense", "Affine", "", None, 1])
def test_unknown_matcher_type_is_refused_by_name(bad):
    """ctx None: anything that touched the device would fail otherwise than by ValueError"""
    from image_stitching_amd.distributed import HipEngine, StitchJob
    from image_stitching_amd.stitching import StitchConfig, Stitcher, check_matcher_config, make_matcher
    cfg = StitchConfig(matcher_type=bad)
    for make in (lambda: check_matcher_config(cfg), lambda: make_matcher(None, cfg), lambda: Stitcher(None, (640, 360), cfg),
                 lambda: HipEngine(None, (640, 360), cfg), lambda: StitchJob(None, (640, 360), [], config=cfg)):
        with pytest.raises(ValueError, match="matcher_type"):
            make()


def test_affine_with_a_range_width_is_refused_by_name():
    from image_stitching_amd.distributed import HipEngine, StitchJob
    from image_stitching_amd.stitching import StitchConfig, check_matcher_config
    cfg = StitchConfig.hot_path(matcher_type="affine", range_width=3)
    for make in (lambda: check_matcher_config(cfg), lambda: HipEngine(None, (640, 360), cfg), lambda: StitchJob(None, (640, 360), [], config=cfg)):
        with pytest.raises(ValueError, match="range_width"):
            make()


def test_full_affine_is_refused_by_name():
    from image_stitching_amd import AffineBestOf2NearestMatcher
    with pytest.raises(NotImplementedError, match="full_affine"):
        AffineBestOf2NearestMatcher(None, full_affine=True)


def test_job_refuses_an_engine_of_another_matcher_type():
    import synth
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    from oracle_engine import OracleEngine
    cams = [synth.make_camera(640, 360, 60.0, 13.0 * i) for i in range(4)]
    cfg = StitchConfig.hot_path(matcher_type="affine")
    with pytest.raises(NotImplementedError, match="matcher_type"):
        StitchJob(None, (640, 360), cams, engine=OracleEngine((640, 360)), config=cfg)      # declares none: "homography"
    StitchJob(None, (640, 360), cams, engine=OracleEngine((640, 360)), config=StitchConfig.hot_path())

    class Declared:
        warp_type = "spherical"
        matcher_type = "affine"
    assert StitchJob(None, (640, 360), cams, engine=Declared(), config=cfg).cfg.matcher_type == "affine"
    with pytest.raises(NotImplementedError, match="matcher_type"):
        StitchJob(None, (640, 360), cams, engine=Declared(), config=StitchConfig.hot_path())


def test_abi_declares_the_model_entries():
    from image_stitching_amd import _capi
    assert (_capi.MATCH_HOMOGRAPHY, _capi.MATCH_AFFINE_PARTIAL) == (0, 1)
    for name in ("mis_match_affine_default_params", "mis_match_pairs_model", "mis_estimate_affine_partial"):
        assert name in _capi.PROTOTYPES and name in _capi.header_functions()
