"""The oracle's findHomography and pair matcher held to the independent reference of tests/refimpl_homography.py on every input
family of that file, and unit tests of the reference itself.  No GPU.  A case the reference does not decide is reported (run
with -s) and left out of the comparisons; family_gate caps how many such cases a family may have."""
import math
from fractions import Fraction

import numpy as np
import pytest

import refimpl_homography as rh


# ------------------------------------------------------------------------------------------------ the reference itself
def test_rng_stream_by_hand():
    """state0 = 2^64 - 1 has low and high word 2^32 - 1, so state1 = A * (2^32 - 1) + (2^32 - 1) = (A + 1) * 2^32 - (A + 1):
    high word A, low word 2^32 - (A + 1) = 130063605.  The next two follow from the recurrence low * A + high."""
    A = 4164903690
    x1 = 2 ** 32 - (A + 1)
    assert x1 == 130063605
    s2 = x1 * A + A
    s3 = (s2 % 2 ** 32) * A + (s2 >> 32)
    r = rh.Rng()
    assert [r.next() for _ in range(3)] == [x1, s2 % 2 ** 32, s3 % 2 ** 32] and r.draws == 3
    r = rh.Rng()
    assert r.uniform(0, 7) == x1 % 7 and r.uniform(5, 5) == 5 and r.draws == 1
    assert rh.Rng(0).state == 0xFFFFFFFF


def test_num_iters_formula():
    assert rh.update_num_iters(0.995, 0.0, 2000) == (0, False)                  # ep = 0: denom = 1 - 1 = 0 < DBL_MIN
    assert rh.update_num_iters(0.995, 1.0, 2000) == (2000, False)               # ep = 1: log(1) = 0 >= 0
    assert rh.update_num_iters(1.0, 0.5, 2000)[0] == 2000                       # p = 1: num = log(DBL_MIN) ~ -708, / log(15/16) > 2000
    assert rh.update_num_iters(1.0, 0.01, 2000)[0] == round(math.log(rh.DBL_MIN) / math.log(1 - 0.99 ** 4))
    assert rh.update_num_iters(0.995, 0.5, 2000)[0] == round(math.log(0.005) / math.log(1 - 0.5 ** 4)) == 82
    assert rh.update_num_iters(0.995, 0.5, 50)[0] == 50                         # never above the current niters
    assert rh.update_num_iters(2.0, -1.0, 10) == (0, False)                     # clamped to p = 1, ep = 0


def test_exact_zero_orientation_is_decided():
    """Three exactly collinear points make one determinant exactly 0: 0 * x < 0 is false, nothing is near a boundary; a float64
    LU of the same matrix may return +-1e-13 instead."""
    s = np.array([[0.1, 0.2], [0.3, 0.6], [0.7, 1.4], [5, -3]], np.float32)
    s[:3, 1] = s[:3, 0] * np.float32(2)                                         # exact in float32
    d = np.array([[1, 1], [4, 2], [3, 7], [-2, 5]], np.float32)
    det, mag = rh.det3_exact(s[0], s[1], s[2])
    assert det == 0 and mag > 0
    neg, near = rh.orientation_negative_exact(s, d)
    assert not near
    signs = [np.sign(float(rh.det3_exact(*s[list(t)])[0] * rh.det3_exact(*d[list(t)])[0])) for t in rh._TRIPLES]
    assert signs[0] == 0 and neg == sum(v < 0 for v in signs)
    # a determinant that is not zero but within a few ulps of its terms is reported, not decided: det = 1 among terms of 6e14
    s3 = np.array([[1e7, 1e7], [1e7 + 1, 1e7 + 1], [1e7 + 2, 1e7 + 3], [0, 5]], np.float32)
    d3, m3 = rh.det3_exact(s3[0], s3[1], s3[2])
    assert isinstance(d3, Fraction) and d3 == 1 and m3 > 5e14
    assert rh.orientation_negative_exact(s3, d)[1] is True
    assert rh.check_subset_exact(s3, d)[1] is not None                          # reported with its reason
    # collinearity: only the triples that contain the last point count
    assert rh.have_collinear_exact(np.array([[0, 0], [1, 2], [5, 5], [3, 6]], np.float32)) == (True, False)
    assert rh.have_collinear_exact(np.array([[0, 0], [1, 2], [3, 6], [5, 5]], np.float32)) == (False, False)
    assert rh.have_collinear_exact(np.array([[0, 0], [1, 2], [1, 2], [5, 5]], np.float32)) == (True, False)   # two equal points


def test_four_point_model_reproduces_a_known_homography():
    H = np.array([[1.2, -0.1, 30.0], [0.2, 0.9, -12.0], [3e-4, -2e-4, 1.0]])
    s = np.array([[-200, -100], [250, -120], [230, 180], [-190, 160]], np.float64)
    d = rh._apply(H, s)
    G = rh.homography_4pt(s, d)
    assert np.abs(G - H).max() < 1e-9 * 30
    assert rh.subset_sv_ratio(s, d) > 1e-3
    # three collinear points plus one: a family of homographies, flagged by the singular values
    s[2] = 2 * s[1] - s[0]
    assert rh.subset_sv_ratio(s, rh._apply(H, s)) < 1e-9
    # the tail's fixed point on noise-free data is the map itself (up to the float32 rounding of the points)
    src, dst = rh.synth(3, 200, 0, noise=0.0)
    H0 = rh.dlt_normalized_svd(src, dst)
    Hs, steps = rh.gauss_newton(H0, src, dst)
    assert np.abs(Hs - np.array(rh.H_BASE)).max() < 1e-5 and rh.converged_fast(steps)


# ------------------------------------------------------------------------------------------------ oracle against the reference
@pytest.mark.parametrize("family", sorted(rh.FAMILIES))
def test_oracle_find_homography_vs_reference(oracle_mod, family):
    cases = rh.FAMILIES[family]()
    ests = [rh.replay(c) for c in cases]
    for c, e in zip(cases, ests):
        rh.check_expectations(c, e)
        if not e.is_decided:
            print("UNDECIDED %s / %s: %s" % (family, c["name"], e.decided))
    decided, weak = rh.family_gate(family, ests)
    worst, near, worst_near = 0.0, 0, 0.0
    for c, e in zip(cases, ests):
        if not e.is_decided:
            continue
        ok, H, mask, iters = oracle_mod.find_homography_ransac(c["src"], c["dst"], **c["kw"])
        try:
            res = rh.check_estimate(e, ok, H, mask, iters)
        except AssertionError as err:
            raise AssertionError("%s / %s: %s" % (family, c["name"], err)) from err
        if res["kind"] == "params" and e.n > 4:
            worst = max(worst, res["dH"])
        if res["kind"] == "near start":
            near, worst_near = near + 1, max(worst_near, res["dH"])
    print("family %s: %d cases, %d decided, %d cost-only or near start, max |H - H*| = %.3g (bound %.3g); %d near start, max |H - H*| = %.3g"
          % (family, len(cases), decided, weak, worst, 2 * rh.FLT_EPSILON, near, worst_near))


def test_oracle_matches_info_vs_reference(oracle_mod):
    """Six frames in one oracle call (the batch of the GPU test): every MatchesInfo field of every pair, both directions."""
    batch = rh.matcher_batch()
    infos = rh.batch_reference(batch)
    rh.batch_gate(batch, infos)
    feats = [dict(img_w=f["size"][0], img_h=f["size"][1], xy=f["xy"], desc=f["desc"]) for f in batch["frames"]]
    got = oracle_mod.match_all_pairs(feats)
    n = len(feats)
    entries = [dict(matches=g["matches"], inliers_mask=g["inliers_mask"], num_inliers=g["num_inliers"], H=g["H"] if g["has_H"] else None,
                    confidence=g["confidence"], src=g["src_img_idx"], dst=g["dst_img_idx"]) for g in got]
    worst = rh.check_batch(batch, infos, entries)
    for (i, j), info in infos.items():                                          # the oracle exposes both iteration counts
        if info.is_decided:
            its = got[i * n + j]["ransac_iters"]
            assert its[0] == (info.first.iters if info.first else 0), (i, j, its)
            assert its[1] == (info.second.iters if info.second else 0), (i, j, its)
    print("matcher batch: %d pairs, %d decided, max |H - H*| = %.3g" % (len(infos), sum(v.is_decided for v in infos.values()), worst))
