"""The speculative drawing of the second RANSAC phase's subsets (homography.hip, DRAW_SPEC): while the first phase of the
matcher's first estimation is solved, the subsets of the few-match problems (PHASE0 < B4(n) < max_iters, n <= 17 at the defaults)
are drawn up to B4(n) on another stream, and the second phase's draw adopts them.  One matcher call holds every path of that:
speculated and adopted whole, adopted and continued past the chunk budget, discarded, given up, outside the class.  Every pair is
held to the independent reference tests/refimpl_homography.py, whose replay also says, before anything runs on the device, that
each pair is in the regime it was built for."""
import ctypes as C

import numpy as np
import pytest

import refimpl_homography as rh

pytestmark = pytest.mark.gpu

SIZE = (1920, 1080)


def _few(seed, n, inliers):
    return rh.synth(seed, n, n - inliers, lim=300.0, noise=0.3)


# (name, correspondences, iterations of the reference's replay).  Seeds: the replay of the pair, centred as the matcher centres
# it, is decided and runs the wanted count (recipe: the comment above rh.ITER_REGIMES); the counts of cases 1 - 6 are
# B4(n) = update_num_iters(0.995, (n - 4) / n, 2000), those of 4 and 7 the same with 5 and 9 inliers.
CASES = (
    ("n9 four inliers", lambda: _few(1, 9, 4), 133),             # first count past the phase boundary: five speculated subsets
    ("n12 four inliers", lambda: _few(1, 12, 4), 427),           # the typical pair without an overlap
    ("n15 four inliers", lambda: _few(1, 15, 4), 1045),          # 6 - 7 chunks of the stream: at the chunk budget
    ("n15 five inliers", lambda: _few(1, 15, 5), 427),           # the loop ends well inside the speculated 1045
    ("n17 four inliers", lambda: _few(2, 17, 4), 1726),          # top of the class, past the chunk budget: the regular draw continues
    ("n18 four inliers", lambda: _few(1, 18, 4), 2000),          # first n outside the class
    ("n12 nine inliers", lambda: _few(1, 12, 9), 14),            # finishes in the first phase: the speculation is discarded
    ("heap n17", lambda: rh._heap(2, 13, 4), 1726),              # nearly every attempt rejected: budget spent at once, past the RNG table
    ("heap n16 no subset", lambda: rh._heap(1, 14, 2), 0),       # getSubset gives up at iteration 0, inside the class
    ("n400", lambda: rh.synth(3, 400, 280, noise=0.3), 651),     # a large problem in the same second-phase work list
)
K_N15_5, K_N18, K_GIVE_UP = 3, 5, 8


def _pair_index(n_frames, i, j):
    return sum(n_frames - 1 - a for a in range(i)) + (j - i - 1)


def _build_batch():
    """Pair k owns frames 2k and 2k + 1: one random 256-bit code per correspondence, listed in the same order in both frames, so
    the match list keeps the generator's order; any other two frames share no code.  -> (batch, infos) with the reference's
    PairInfo (and .matches) of the ten pairs, regimes asserted."""
    import refimpl
    rng = np.random.default_rng(70)
    half = np.array([np.float32(SIZE[0]) * np.float32(0.5), np.float32(SIZE[1]) * np.float32(0.5)], np.float32)
    frames = []
    for _, make, _ in CASES:
        src, dst = make()
        codes = rng.integers(0, 256, (len(src), 32), dtype=np.uint8)
        for pts in (src, dst):
            frames.append(dict(size=SIZE, xy=(np.asarray(pts, np.float32) + half).astype(np.float32), desc=codes))
    infos = {}
    for k, (name, _, iters) in enumerate(CASES):
        a, b = frames[2 * k], frames[2 * k + 1]
        m = refimpl.best_of_2_nearest_matches(a["desc"], b["desc"], 0.32).astype(rh.DMATCH_DTYPE)
        assert np.array_equal(m["query_idx"], np.arange(len(a["xy"]))) and np.array_equal(m["train_idx"], m["query_idx"]), name
        info = rh.matches_info(m, a["xy"], a["size"], b["xy"], b["size"])
        info.matches = m
        infos[(2 * k, 2 * k + 1)] = info
        # the regime, on the reference alone
        assert info.first is not None and info.first.iters == iters, (name, info.first.iters, info.first.decided)
    und = [k for k, v in infos.items() if not v.is_decided]
    weak = [k for k, v in infos.items() if v.is_decided and v.has_H and v.final.n > 4 and (not v.final.fast or v.final.near_start)]
    assert len(und) + len(weak) <= 0.10 * len(infos), ("undecided", [(k, infos[k].decided) for k in und], "cost only", weak)
    heap, give_up, early = infos[(14, 15)], infos[(16, 17)], infos[(12, 13)]
    assert heap.first.draws > 1000000                                         # far past the RNG table (131072 positions)
    assert give_up.is_decided and not give_up.has_H and give_up.first.draws >= 40000 and not give_up.mask.any()
    assert early.second is not None and infos[(18, 19)].second is not None    # the inlier-only estimation runs on the side chain
    for k in (0, 1, 2, 4, 5):
        assert infos[(2 * k, 2 * k + 1)].num_inliers <= 5 and infos[(2 * k, 2 * k + 1)].second is None, CASES[k][0]
    return dict(frames=frames), infos


@pytest.fixture(scope="module")
def spec_batch():
    return _build_batch()


def _entries(pm):
    return [dict(src=m.src_img_idx, dst=m.dst_img_idx, matches=m.matches, inliers_mask=m.inliers_mask, num_inliers=m.num_inliers, H=m.H,
                 confidence=m.confidence) for m in pm]


def _upload(ctx, batch):
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import KP_DTYPE
    feats = []
    for i, f in enumerate(batch["frames"]):
        k = np.zeros(len(f["xy"]), KP_DTYPE)
        k["x"], k["y"] = f["xy"][:, 0], f["xy"][:, 1]
        feats.append(isa.ImageFeatures.upload(ctx, f["size"], k, f["desc"], i))
    return feats


def _same(a, b):
    if (a["src"], a["dst"], a["num_inliers"], a["confidence"]) != (b["src"], b["dst"], b["num_inliers"], b["confidence"]):
        return False
    if np.asarray(a["matches"]).tobytes() != np.asarray(b["matches"]).tobytes():
        return False
    if np.asarray(a["inliers_mask"]).tobytes() != np.asarray(b["inliers_mask"]).tobytes() or (a["H"] is None) != (b["H"] is None):
        return False
    return a["H"] is None or np.asarray(a["H"], np.float64).tobytes() == np.asarray(b["H"], np.float64).tobytes()


def _href(info):
    return info.final.Hstar if info.final.Hstar is not None else info.final.H4


def _check_pairs(batch, infos, entries):
    """rh.check_batch over the ten pairs.  It holds the product of a pair's H with its mirrored entry's to the identity within
    1e-9 and, for that bound to mean something, asserts cond(H*) < 1e4 on the reference.  With four inliers the best model is the
    first four-point subset the loop tried -- four arbitrary matches --, and the reference's H* of such a pair has a condition
    number of 2e4 to 9e6 (cases 2, 3, 5, 6 and 8).  Those pairs get the same checks, field by field, with the bound of the
    product scaled by the condition number: 1e-13 cond(H*), which is check_batch's own 1e-9 at its limit of 1e4 (the error of a
    3 x 3 inverse in float64 grows with cond(H) eps)."""
    n = len(batch["frames"])
    ill = {k: v for k, v in infos.items() if v.is_decided and v.has_H and np.linalg.cond(_href(v)) >= 1e4}
    worst = rh.check_batch(batch, {k: v for k, v in infos.items() if k not in ill}, entries)
    for (i, j), info in ill.items():
        a, b = entries[i * n + j], entries[j * n + i]
        assert (a["src"], a["dst"], b["src"], b["dst"]) == (i, j, j, i)
        got, back = np.asarray(a["matches"]), np.asarray(b["matches"])
        for fld in ("query_idx", "train_idx", "img_idx", "distance"):
            assert np.array_equal(got[fld], info.matches[fld]), (i, j, fld)
        assert np.array_equal(back["query_idx"], got["train_idx"]) and np.array_equal(back["train_idx"], got["query_idx"])
        for e in (a, b):
            assert np.asarray(e["inliers_mask"], np.uint8).tobytes() == info.mask.tobytes(), (i, j)
            assert e["num_inliers"] == info.num_inliers, (i, j, e["num_inliers"], info.num_inliers)
            assert e["confidence"] == info.confidence, (i, j, e["confidence"], info.confidence)
            assert e["H"] is not None, (i, j)
        H = np.asarray(a["H"], np.float64).reshape(3, 3)
        assert np.isfinite(H).all() and abs(H[2, 2] - 1.0) <= rh.DBL_EPSILON
        try:
            res = rh.check_tail(info.final, H)
        except AssertionError as err:
            raise AssertionError("pair (%d, %d): %s" % (i, j, err)) from err
        if res["kind"] == "params":
            worst = max(worst, res["dH"])
        P = np.asarray(b["H"], np.float64).reshape(3, 3) @ H
        assert np.abs(P / P[2, 2] - np.eye(3)).max() <= 1e-13 * np.linalg.cond(_href(info)), (i, j, P)
    return worst


def test_pairs_of_every_drawing_path_vs_reference(ctx, spec_batch):
    """Every MatchesInfo field of the ten pairs and of their mirrored entries against the reference; the other 180 pairs of
    the call have no match."""
    import image_stitching_amd as isa
    batch, infos = spec_batch
    entries = _entries(isa.BestOf2NearestMatcher(ctx, 0.32)(_upload(ctx, batch)))
    n = len(batch["frames"])
    assert len(entries) == n * n
    worst = _check_pairs(batch, infos, entries)
    print("speculative draw batch: %d pairs, %d decided, max |H - H*| = %.3g" % (len(infos), sum(v.is_decided for v in infos.values()), worst))
    for i in range(n):
        for j in range(n):
            if i != j and (min(i, j), max(i, j)) not in infos:
                e = entries[i * n + j]
                assert len(e["matches"]) == 0 and e["H"] is None and e["num_inliers"] == 0, (i, j)


def test_speculation_is_in_effect_and_harmless(ctx, spec_batch):
    """The same call twice gives the same bytes, and the states of the first estimation's batch show what was drawn: the whole
    B4(15) = 1045 subsets for a loop that ends at 427 (drawing behind the replay stops at niters), exactly niters outside the
    class, nothing where getSubset gave up at once."""
    import image_stitching_amd as isa
    batch, infos = spec_batch
    feats = _upload(ctx, batch)
    matcher = isa.BestOf2NearestMatcher(ctx, 0.32)
    first, second = _entries(matcher(feats)), _entries(matcher(feats))
    assert len(first) == len(second) and all(_same(a, b) for a, b in zip(first, second))
    n = len(batch["frames"])
    st = np.zeros((256, 8), np.int32)
    got = ctx.lib.mis_debug_ransac_states(ctx.h, 0, st.ctypes.data_as(C.c_void_p), 256)
    assert got == n * (n - 1) // 2
    row = lambda k: dict(zip(("n", "mode", "n_sub", "iter", "niters", "draw_fail", "done", "max_good"), st[_pair_index(n, 2 * k, 2 * k + 1)].tolist()))
    for k, (name, _, iters) in enumerate(CASES):
        r = row(k)
        assert r["n"] == len(batch["frames"][2 * k]["xy"]) and r["mode"] == 2 and r["done"] == 1 and r["iter"] == iters, (name, r)
    r = row(K_N15_5)
    assert r["iter"] == r["niters"] == 427 and r["n_sub"] > r["niters"], r
    r = row(K_N18)
    assert r["n_sub"] == r["niters"] == 2000, r
    r = row(K_GIVE_UP)
    assert r["draw_fail"] == 1 and r["n_sub"] == 0, r
