"""estimate_affine_partial and the MatchesInfo of AffineBestOf2NearestMatcher (HIP) held to the independent reference of
tests/refimpl_affine.py.  A case the reference does not decide is reported (run with -s) and left out of the comparisons;
family_gate / batch_gate cap how many such cases there may be."""
import numpy as np
import pytest

import refimpl_affine as ra

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", sorted(ra.FAMILIES))
def test_estimate_affine_partial_vs_reference(ctx, family):
    import image_stitching_amd as isa
    cases = ra.FAMILIES[family]()
    ests = [ra.replay(c) for c in cases]
    for c, e in zip(cases, ests):
        ra.check_expectations(c, e)
        if not e.is_decided:
            print("UNDECIDED %s / %s: %s" % (family, c["name"], e.decided))
    decided, weak = ra.family_gate(family, ests)
    worst = worst_ransac = 0.0
    for c, e in zip(cases, ests):
        if not e.is_decided:
            continue
        ok, M, mask = isa.estimate_affine_partial(ctx, c["src"], c["dst"], **c["kw"])
        try:
            res = ra.check_estimate(e, ok, M, mask)
        except AssertionError as err:
            raise AssertionError("%s / %s: %s" % (family, c["name"], err)) from err
        if res["kind"] in ("params", "near start"):
            worst = max(worst, res["dH"])
        if res["kind"] == "ransac":
            worst_ransac = max(worst_ransac, res["dH"])
    print("family %s: %d cases, %d decided, %d near start, max |M - H*| = %.3g (bound %.3g), max |M - M_ransac| = %.3g"
          % (family, len(cases), decided, weak, worst, 2 * ra.FLT_EPSILON, worst_ransac))


def _entries(pm):
    return [dict(src=m.src_img_idx, dst=m.dst_img_idx, matches=m.matches, inliers_mask=m.inliers_mask, num_inliers=m.num_inliers, H=m.H,
                 confidence=m.confidence) for m in pm]


def _same(o, s):
    assert (o["src"], o["dst"], o["num_inliers"], o["confidence"]) == (s["src"], s["dst"], s["num_inliers"], s["confidence"])
    assert np.asarray(o["matches"]).tobytes() == np.asarray(s["matches"]).tobytes()
    assert np.asarray(o["inliers_mask"]).tobytes() == np.asarray(s["inliers_mask"]).tobytes()
    assert (o["H"] is None) == (s["H"] is None)
    if s["H"] is not None:
        assert np.asarray(o["H"], np.float64).tobytes() == np.asarray(s["H"], np.float64).tobytes()


@pytest.fixture(scope="module")
def batch():
    b = ra.matcher_batch()
    infos = ra.batch_reference(b)
    ra.batch_gate(b, infos)
    return b, infos


def _upload(ctx, b):
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import KP_DTYPE
    feats = []
    for i, f in enumerate(b["frames"]):
        k = np.zeros(len(f["xy"]), KP_DTYPE)
        k["x"], k["y"] = f["xy"][:, 0], f["xy"][:, 1]
        feats.append(isa.ImageFeatures.upload(ctx, f["size"], k, f["desc"], i))
    return feats


def test_matches_info_batch_vs_reference(ctx, batch):
    """Six frames in ONE matcher call: pairs of 5, 6, 100 and 2500 matches share the work list and both phases.  Every
    MatchesInfo field of every pair and of its mirror; the same call over three ranks (the union equals the single call bit for
    bit) and with a pair mask (unselected entries stay default)."""
    import image_stitching_amd as isa
    b, infos = batch
    feats = _upload(ctx, b)
    matcher = isa.AffineBestOf2NearestMatcher(ctx)
    single = _entries(matcher(feats))
    n = len(feats)
    assert len(single) == n * n
    worst = ra.check_batch(b, infos, single)
    print("affine matcher batch: %d pairs, %d decided, max |M - H*| = %.3g" % (len(infos), sum(v.is_decided for v in infos.values()), worst))
    # identical frames: n / (8 + 0.3 n) > 3 is kept; the homography matcher on the same features zeroes it
    e05 = single[0 * n + 5]
    assert e05["num_inliers"] == 300 and e05["confidence"] == 300 / (8 + 0.3 * 300) > 3
    h05 = _entries(isa.BestOf2NearestMatcher(ctx, 0.3)(feats))[0 * n + 5]
    assert h05["num_inliers"] == 300 and h05["confidence"] == 0.0
    parts = [_entries(matcher(feats, rank=r, world_size=3)) for r in range(3)]
    for k in range(n * n):
        owners = [p[k] for p in parts if p[k]["src"] >= 0]
        if single[k]["src"] < 0:
            assert not owners
            continue
        assert len(owners) == 1, k
        _same(owners[0], single[k])
    mask = np.zeros((n, n), np.uint8)
    chosen = ((0, 3), (0, 5), (1, 4), (2, 4))
    for i, j in chosen:
        mask[i, j] = 1
    masked = _entries(matcher(feats, mask=mask))
    for i in range(n):
        for j in range(n):
            k = i * n + j
            if (min(i, j), max(i, j)) in chosen and i != j:
                _same(masked[k], single[k])
            else:
                assert masked[k]["src"] == -1 and len(masked[k]["matches"]) == 0 and masked[k]["H"] is None and masked[k]["confidence"] == 0


def test_old_entry_points_are_unchanged_by_an_affine_call(ctx, batch):
    """The workspaces are shared between the models: the homography entries return byte-identical results before and after one
    affine call on the same context, and so does the affine one around a homography call."""
    import image_stitching_amd as isa
    b, _ = batch
    feats = _upload(ctx, b)
    n = len(feats)
    homo, aff = isa.BestOf2NearestMatcher(ctx, 0.3), isa.AffineBestOf2NearestMatcher(ctx)
    src, dst = ra.synth(5, 700, 300)
    before = _entries(homo(feats))
    before_sel = _entries(isa.BestOf2NearestRangeMatcher(ctx, 3, 0.3)(feats))
    before_sh = _entries(homo(feats, rank=1, world_size=2))
    fh0 = isa.find_homography(ctx, src, dst)
    a0 = _entries(aff(feats))
    fa0 = isa.estimate_affine_partial(ctx, src, dst)
    after = _entries(homo(feats))
    after_sel = _entries(isa.BestOf2NearestRangeMatcher(ctx, 3, 0.3)(feats))
    after_sh = _entries(homo(feats, rank=1, world_size=2))
    fh1 = isa.find_homography(ctx, src, dst)
    a1 = _entries(aff(feats))
    fa1 = isa.estimate_affine_partial(ctx, src, dst)
    for x, y in ((before, after), (before_sel, after_sel), (before_sh, after_sh), (a0, a1)):
        for k in range(n * n):
            _same(x[k], y[k])
    for x, y in ((fh0, fh1), (fa0, fa1)):
        assert x[0] == y[0] and x[1].tobytes() == y[1].tobytes() and x[2].tobytes() == y[2].tobytes()


def test_unknown_model_is_unsupported(ctx, batch):
    import ctypes as C
    from image_stitching_amd import _capi as capi
    b, _ = batch
    feats = _upload(ctx, b)[:2]
    arr = (capi.MisFeatures * 2)()
    for k, f in enumerate(feats):
        C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
    p = capi.MisMatchParams()
    ctx.lib.mis_match_affine_default_params(C.byref(p))
    assert (p.ransac_thresh, p.max_iters, p.confidence, p.num_matches_thresh1) == (3.0, 2000, 0.99, 6)
    mis = (capi.MisMatchesInfo * 4)()
    assert ctx.lib.mis_match_pairs_model(ctx.h, arr, 2, C.byref(p), 2, None, -1, 0, 1, mis) == -6      # MIS_E_UNSUPPORTED
    assert ctx.lib.mis_match_pairs_model(ctx.h, arr, 2, C.byref(p), capi.MATCH_AFFINE_PARTIAL, None, -1, 0, 1, mis) == 0
    ctx.lib.mis_matches_free(mis, 4)
