"""The oracle (oracle/mo_*.c) against the float64 / exact-integer numpy references of tests/refimpl.py, at the warp's and the
matchers' edge regimes.  The GPU tests compare the kernels with the oracle bit for bit; this pins the oracle itself to
OpenCV's documented semantics, independently of how it was written."""
import math

import numpy as np
import pytest

import refimpl as ri
import test_refimpl_match_gpu as mreg


def test_reflect_and_round_closed_forms():
    # BORDER_REFLECT: fedcba|abcdefgh|hgfedcb, folded as often as needed; lengths 1 and 2
    assert [ri.reflect(p, 3) for p in range(-7, 10)] == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2]
    assert [ri.reflect(p, 2) for p in range(-5, 6)] == [0, 0, 1, 1, 0, 0, 1, 1, 0, 0, 1]
    assert {ri.reflect(p, 1) for p in range(-40000, 40000, 7)} == {0}
    assert list(ri.cv_round(np.array([0.5, 1.5, 2.5, -0.5, -1.5, 2.0 ** 31, -2.0 ** 31 - 1, np.nan]))) == \
        [0, 2, 2, 0, -2, -2 ** 31, -2 ** 31, -2 ** 31]


def test_band_model_stays_below_2e_minus_8_on_the_source():
    """delta <= 2^-8 px wherever the map lands on the source frame.  The 4K frame at scale = f (3325) is the exception: the
    pinned 3e-7 trig error times the focal length alone is 1e-3 px there, and the bound reaches 5.3e-3 px at its corners
    (<= 2^-7 is asserted)."""
    cases = [(w, h, m, g) for (w, h), ms in ri.WARP_SOURCES for m in ms for g in ri.WARP_GEOMS[:2]]
    cases += [(3840, 2160, 1.0, ("4k", 60.0, 15.0, 0.3, -0.2)), (333, 217, 1.0, ri.WARP_GEOMS[-1])]
    for w, h, m, (name, hfov, yaw, pitch, roll) in cases:
        K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, m, seam=m < 1)
        r = ri.warp_roi_f64(scale, w, h, K, R)
        roi = (min(r["tl_x"]), min(r["tl_y"]), max(r["br_x"]) - min(r["tl_x"]) + 1, max(r["br_y"]) - min(r["tl_y"]) + 1)
        maps = ri.spherical_backward_f64(K, R, scale, roi)
        on = (maps["z"] > 0) & (maps["x"] >= -1) & (maps["x"] <= w) & (maps["y"] >= -1) & (maps["y"] <= h)
        assert on.any()
        assert max(maps["dx"][on].max(), maps["dy"][on].max()) <= 2.0 ** (-7 if w > 2000 else -8), (w, h, m, name)


def _oracle_warp_vs_reference(oracle_mod, img, K, R, scale, tag):
    o = oracle_mod
    h, w = img.shape[:2]
    roi = o.warp_roi(scale, w, h, K, R)
    assert ri.roi_matches(roi, ri.warp_roi_f64(scale, w, h, K, R)), (tag, roi)
    maps = ri.spherical_backward_f64(K, R, scale, roi)
    lin, tl = o.warp_spherical(img, scale, K, R)
    assert tl == roi[:2]
    bad, nb, nu = ri.check_candidates(lin, *ri.remap_linear_reflect_candidates(img, maps))
    assert not bad.any(), (tag, "linear", int(bad.sum()), np.argwhere(bad)[0])
    ones = np.full((h, w), 255, np.uint8)
    msk, _ = o.warp_spherical(ones, scale, K, R, o.INTER_NEAREST, o.BORDER_CONSTANT)
    bad, nbm, num = ri.check_candidates(msk, *ri.remap_nearest_constant_candidates(ones, maps))
    assert not bad.any(), (tag, "mask", int(bad.sum()), np.argwhere(bad)[0])
    g = img if img.ndim == 2 else img[:, :, 1]
    near, _ = o.warp_spherical(g, scale, K, R, o.INTER_NEAREST, o.BORDER_CONSTANT)
    bad, _, _ = ri.check_candidates(near, *ri.remap_nearest_constant_candidates(g, maps))
    assert not bad.any(), (tag, "nearest", int(bad.sum()))
    return nb / lin.shape[0] / lin.shape[1]


def _warp_cases():
    for (w, h), mults in ri.WARP_SOURCES:
        for m in mults:
            yield pytest.param(w, h, m, id="%dx%d-s%g" % (w, h, m))
    yield pytest.param(333, 217, 0.37, id="333x217-s0.37")


@pytest.mark.parametrize("w,h,mult", list(_warp_cases()))
def test_oracle_warp_vs_float64_reference(oracle_mod, w, h, mult):
    shares = []
    for k, (name, hfov, yaw, pitch, roll) in enumerate(ri.WARP_GEOMS):
        K, R, scale = ri.camera(w, h, hfov, yaw, pitch, roll, mult, seam=mult < 1)
        for kind in ("rand", "full", "zero") if k < 3 else ("rand",):
            img = ri.content(kind, (h, w, 3), seed=k)
            shares.append(_oracle_warp_vs_reference(oracle_mod, img, K, R, scale, (name, kind)))
    print("%dx%d s%g: largest in-band share %.2f %%" % (w, h, mult, 100 * max(shares)))


def test_oracle_warp_4k_vs_float64_reference(oracle_mod):
    w, h = 3840, 2160
    K, R, scale = ri.camera(w, h, 60.0, 15.0, 0.3, -0.2)
    share = _oracle_warp_vs_reference(oracle_mod, ri.content("rand", (h, w, 3), seed=4), K, R, scale, "4k")
    print("4K: in-band share %.2f %%" % (100 * share))


def _fd(d):
    return dict(img_w=640, img_h=480, xy=np.zeros((len(d), 2), np.float32), desc=d)


@pytest.mark.parametrize("nt", mreg.HM_TRAINS)
def test_oracle_hamming_knn2_and_matches_vs_exact(oracle_mod, nt):
    rng = np.random.default_rng(nt)
    for nq in mreg.QUERIES:
        for gen in (mreg.hamming_far_sets, mreg.hamming_edge_sets):
            q, t = gen(rng, nq, nt)
            oi, od = oracle_mod.knn2_hamming(q, t)
            ridx, rdist = ri.knn2_hamming_exact(q, t)
            have = ridx >= 0
            assert np.array_equal(oi, ridx) and np.array_equal(od[have], rdist[have])
    for gen in (mreg.hamming_far_sets, mreg.hamming_edge_sets):
        q, t = gen(rng, 257 + 255, nt)
        sets = [q[:257], t, q[257:]]
        out = oracle_mod.match_all_pairs([_fd(d) for d in sets])
        for i, j in ((0, 1), (0, 2), (1, 2)):
            ref = ri.best_of_2_nearest_matches(sets[i], sets[j], 0.32)
            assert np.array_equal(out[i * 3 + j]["matches"], ref.astype(out[0]["matches"].dtype)), (gen.__name__, i, j)


@pytest.mark.parametrize("cols", [1, 2, 64, 100, 127, 128])
def test_oracle_l2_knn2_and_matches_vs_exact(oracle_mod, cols):
    rng = np.random.default_rng(cols)
    q, t = mreg.l2_sets(rng, 120, 300, cols)
    oi, od = oracle_mod.knn2_l2(q, t)
    ridx, rdist = ri.knn2_l2_exact(q, t)
    assert np.array_equal(oi, ridx) and np.array_equal(od.view(np.uint32), rdist.view(np.uint32))
    for conf in (0.32, 0.65):
        ref = ri.best_of_2_nearest_matches(q, t, conf)
        got = oracle_mod.match_pair(_fd(q), _fd(t), oracle_mod.match_default_params(match_conf=conf))["matches"]
        assert np.array_equal(got, ref.astype(got.dtype))
    z, f = np.zeros((3, cols), np.float32), np.full((2, cols), 255.0, np.float32)
    oi, od = oracle_mod.knn2_l2(z, f)
    assert od[0, 0] == np.float32(math.sqrt(cols * 255.0 ** 2)) and list(oi[0]) == [0, 1]


def test_ratio_boundary_is_strict():
    """17 vs 25 at conf 0.32: float32(0.68) * 25 rounds to 17.0, and 17 < 17 is false."""
    assert not np.float32(17) < (np.float32(1) - np.float32(0.32)) * np.float32(25)
    q = np.zeros((1, 32), np.uint8)
    t = np.zeros((2, 32), np.uint8)
    t[0, :2] = 0xff; t[0, 2] = 0x01          # 17 bits
    t[1, :3] = 0xff; t[1, 3] = 0x01          # 25 bits
    assert len(ri.best_of_2_nearest_matches(q, t, 0.32)) == 0
    assert len(ri.best_of_2_nearest_matches(q, t, 0.31)) == 1


def test_oracle_refuses_mixed_descriptor_widths(oracle_mod):
    rng = np.random.default_rng(3)
    a = rng.integers(0, 256, (20, 64)).astype(np.float32)
    b = rng.integers(0, 256, (30, 128)).astype(np.float32)
    with pytest.raises(ValueError):
        oracle_mod.match_all_pairs([_fd(a), _fd(b)])
    with pytest.raises(ValueError):
        oracle_mod.match_pair(_fd(a), _fd(b))
    with pytest.raises(ValueError):
        oracle_mod.match_all_pairs([_fd(a), _fd(rng.integers(0, 256, (10, 32), dtype=np.uint8))])
    out = oracle_mod.match_all_pairs([_fd(a), _fd(np.zeros((0, 128), np.float32)), _fd(a[::-1].copy())])   # empty frames do not count
    assert np.array_equal(out[2]["matches"], ri.best_of_2_nearest_matches(a, a[::-1], 0.32).astype(out[2]["matches"].dtype))
