"""The affine-partial bundle adjuster's host twin (tests/harness/ba_affine_host_harness.cpp: ba_affine.h with loops for kernels,
the library's solver) and the affine estimator against the float64 reference of tests/refimpl_affine_family.py; the reference's
own Jacobian and gauge; the Python entry points."""
import numpy as np
import pytest

import ba_affine_twin as twin
import refimpl_affine_family as ra
import refimpl_motion as rm


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    lib = twin.build(tmp_path_factory.mktemp("ba_affine"))
    if lib is None:
        pytest.skip("no hipcc: the host twin cannot be built")
    return lib


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_jacobian_is_the_derivative_and_the_cost_sees_relative_transforms_only():
    s, tab, ref = ra.get_ba_scene("chain4-255", 0.5)
    P, obs = ref["P"], ref["obs"]
    every = [(c, k) for c in range(s["n"]) for k in range(4)]
    J = ra.ba_jacobian(P, obs, every)
    for q, (c, k) in enumerate(every):
        h = 1e-6 * max(1.0, abs(P[c, k]))
        Pp, Pm = P.copy(), P.copy()
        Pp[c, k] += h
        Pm[c, k] -= h
        num = (ra.ba_residuals(Pp, obs) - ra.ba_residuals(Pm, obs)) / (2 * h)
        assert np.abs(num - J[:, q]).max() <= 1e-6 * max(1.0, np.abs(J[:, q]).max()), (c, k)
    # a common left factor changes nothing: S(G H_c) = S(H_c)
    G = ra.mat_of(ra.params_of(ra.similarity(33.0, 1.7, -40.0, 12.0)))
    Q = np.array([ra.params_of(G @ ra.mat_of(p)) for p in P])
    assert abs(ra.ba_cost(Q, obs) - ra.ba_cost(P, obs)) <= 1e-9 * max(1.0, ra.ba_cost(P, obs))
    assert abs(ra.ba_cost(ref["out"], obs) - ra.ba_cost(P, obs)) <= 1e-9 * max(1.0, ref["S"])
    assert np.abs(ref["out"][ref["centre"]] - [1, 0, 0, 0]).max() < 1e-12
    # at the truth, noise-free keypoints cost their float32 rounding only
    s0, _, ref0 = ra.get_ba_scene("chain4-255", 0.0)
    assert ra.ba_cost(s0["truth"], ref0["obs"]) < 1e-5 and ref0["S"] <= ra.ba_cost(s0["truth"], ref0["obs"])


# ------------------------------------------------------------------------------------------------ the twin against the reference
@pytest.mark.parametrize("name,sigma", ra.BA_CASES)
def test_twin_reaches_the_reference_minimum(harness, name, sigma):
    s, tab, ref = ra.get_ba_scene(name, sigma)
    rc, got = twin.run(harness, s["n"], s["xy"], tab, s["start"], ra.BA_THR, size=(ra.BA_W, ra.BA_H))
    assert rc == 0
    P0 = np.array([ra.params_of(c["R"]) for c in s["start"]])
    res = ra.check_ba_affine(ref, got)
    print("\n    %s s%g: start cost %.3f  S* %.6g  excess %+.3e  /E %+.2e  parameters / bound %.3f  cond %.3g" % (
        name, sigma, ra.ba_cost(P0, ref["obs"]), ref["S"], res["excess"], res["over_E"], res["par_ratio"], ref["cond"]))
    assert ra.ba_cost(P0, ref["obs"]) > 100 * max(ref["S"], 1.0)        # the start is far from the minimum


def test_twin_edge_rules(harness):
    """An edge at confidence == conf_thresh is not an edge (its corrupt matches do not move the result); a masked-out match is
    not read (its indices lie far outside the features); a camera with a = b = 0 (D = 0) stays finite; out-of-range indices of an
    inlier are refused."""
    d = ra.BA_SCENES["chain4-255"]
    thr = float(np.float32(ra.BA_THR))
    s = ra.make_ba_scene("rules", d["sims"], d["edges"], 0.5, 7, counts=d["counts"], conf={(0, 2): thr}, corrupt=[(0, 2)], wild_masked=[(1, 2)])
    tab = rm.table(s)
    ref = ra.reference_ba_affine(s, tab, ra.BA_THR)
    assert ref["n_obs"] == 255 - 30
    rc, got = twin.run(harness, s["n"], s["xy"], tab, s["start"], ra.BA_THR, size=(ra.BA_W, ra.BA_H))
    assert rc == 0
    ra.check_ba_affine(ref, got)
    zero = [dict(c) for c in s["start"]]
    zero[3] = dict(zero[3], R=np.array([[0, 0, 5], [0, 0, 7], [0, 0, 1]], np.float32))
    rc, got = twin.run(harness, s["n"], s["xy"], tab, zero, ra.BA_THR, size=(ra.BA_W, ra.BA_H))
    assert rc == 0 and all(np.isfinite(g["R"]).all() for g in got)
    bad = [dict(e) for e in tab]
    k = 1 * s["n"] + 2
    mm = bad[k]["matches"].copy()
    mm["train_idx"][5] = len(s["xy"][2])
    bad[k]["matches"] = mm
    rc, _ = twin.run(harness, s["n"], s["xy"], bad, s["start"], ra.BA_THR, size=(ra.BA_W, ra.BA_H))
    assert rc == -1


# ------------------------------------------------------------------------------------------------ the estimator
def _entries(s):
    return [(e["i"], e["j"], e["matches"], e["inliers_mask"], e["num_inliers"], e["has_H"], e["H"], e["confidence"]) for e in s["entries"]]


def _check_estimate(cams, n, tab, tree_only=None):
    centre, want = ra.reference_estimate(n, tab)
    for c, w in zip(cams, want):
        assert (c["focal"], c["aspect"], c["ppx"], c["ppy"]) == (1.0, 1.0, 0.0, 0.0) and not c["t"].any()
        assert np.array_equal(c["R"], rm.f32(c["R"]))
        assert np.abs(c["R"] - w).max() <= 4 * 2.0 ** -24 * max(1.0, np.abs(w).max()), (c["R"], w)
    assert np.array_equal(cams[centre]["R"], np.eye(3))
    return centre, want


def test_estimator_chains_exact_transforms_along_the_tree(harness):
    """Every pair carries its exact H: R_i^-1 R_j = H_ij to rounding for every pair, tree edge or not; the library's entry, its
    Python wrapper and the twin give the same bits."""
    import image_stitching_amd as isa
    for name in ra.BA_SCENES:
        s, tab, _ = ra.get_ba_scene(name, 0.0)
        n = s["n"]
        pm = isa.stitching.PairwiseMatches.from_entries(None, n, _entries(s))
        cams = isa.estimate_affine_cameras(pm)
        _check_estimate(cams, n, tab)
        assert twin.same_bits(cams, twin.estimate(harness, n, tab))
        for e in s["entries"]:
            rel = np.linalg.inv(cams[e["i"]]["R"]) @ cams[e["j"]]["R"]
            assert np.abs(rel - e["H"]).max() <= 1e-5 * max(1.0, np.abs(e["H"]).max()), (name, e["i"], e["j"])


def test_estimator_honours_tree_edges_only():
    """A cycle whose weakest edge carries an H inconsistent with the others: the spanning tree leaves it out and the cameras are
    those of the consistent edges."""
    import image_stitching_amd as isa
    d = ra.BA_SCENES["chain3"]
    s = ra.make_ba_scene("cycle", d["sims"], d["edges"], 0.0, 3, counts=d["counts"])
    weakest = min(s["entries"], key=lambda e: e["num_inliers"])
    assert (weakest["i"], weakest["j"]) == (0, 1)
    weakest["H"] = ra.mat_of(ra.params_of(ra.similarity(40.0, 1.3, -77.0, 50.0)))
    tab = rm.table(s)
    cams = isa.estimate_affine_cameras(isa.stitching.PairwiseMatches.from_entries(None, 3, _entries(s)))
    centre, want = _check_estimate(cams, 3, tab)
    truth = [ra.mat_of(p) for p in s["truth"]]
    for c in range(3):
        assert np.abs(cams[c]["R"] - np.linalg.inv(truth[centre]) @ truth[c]).max() <= 1e-4
    rel = np.linalg.inv(cams[0]["R"]) @ cams[1]["R"]
    assert np.abs(rel - weakest["H"]).max() > 1.0


def test_python_entry_points_exist():
    import image_stitching_amd as isa
    assert callable(isa.bundle_adjust_affine_partial) and callable(isa.estimate_affine_cameras)
    with pytest.raises(TypeError):
        isa.estimate_affine_cameras([])
