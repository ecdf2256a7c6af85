"""findHomography and the MatchesInfo of BestOf2NearestMatcher (HIP) held to the independent reference of
tests/refimpl_homography.py: the same input families and the same assertions as tests/test_refimpl_homography_cpu.py applies to
the oracle.  The oracle takes no part here.  A case the reference does not decide is reported (run with -s) and left out of the
comparisons; family_gate / batch_gate cap how many such cases there may be."""
import numpy as np
import pytest

import refimpl_homography as rh

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", sorted(rh.FAMILIES))
def test_find_homography_vs_reference(ctx, family):
    import image_stitching_amd as isa
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
        ok, H, mask = isa.find_homography(ctx, c["src"], c["dst"], **c["kw"])
        try:
            res = rh.check_estimate(e, ok, H, mask)
        except AssertionError as err:
            raise AssertionError("%s / %s: %s" % (family, c["name"], err)) from err
        if res["kind"] == "params" and e.n > 4:
            worst = max(worst, res["dH"])
        if res["kind"] == "near start":
            near, worst_near = near + 1, max(worst_near, res["dH"])
    print("family %s: %d cases, %d decided, %d cost-only or near start, max |H - H*| = %.3g (bound %.3g); %d near start, max |H - H*| = %.3g"
          % (family, len(cases), decided, weak, worst, 2 * rh.FLT_EPSILON, near, worst_near))


def _entries(pm):
    return [dict(src=m.src_img_idx, dst=m.dst_img_idx, matches=m.matches, inliers_mask=m.inliers_mask, num_inliers=m.num_inliers, H=m.H,
                 confidence=m.confidence) for m in pm]


def test_matches_info_batch_vs_reference(ctx):
    """Six frames in ONE matcher call: pairs of 5 to 2500 matches share the work list, both phases and the side chain.  Every
    MatchesInfo field of every pair and of its mirrored entry; then the same features through the sharded entry point over three
    ranks, whose union must equal the single call bit for bit."""
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import KP_DTYPE
    batch = rh.matcher_batch()
    infos = rh.batch_reference(batch)
    rh.batch_gate(batch, infos)
    feats = []
    for i, f in enumerate(batch["frames"]):
        k = np.zeros(len(f["xy"]), KP_DTYPE)
        k["x"], k["y"] = f["xy"][:, 0], f["xy"][:, 1]
        feats.append(isa.ImageFeatures.upload(ctx, f["size"], k, f["desc"], i))
    matcher = isa.BestOf2NearestMatcher(ctx, 0.32)
    single = _entries(matcher(feats))
    n = len(feats)
    assert len(single) == n * n
    worst = rh.check_batch(batch, infos, single)
    print("matcher batch: %d pairs, %d decided, max |H - H*| = %.3g" % (len(infos), sum(v.is_decided for v in infos.values()), worst))
    parts = [_entries(matcher(feats, rank=r, world_size=3)) for r in range(3)]
    for k in range(n * n):
        owners = [p[k] for p in parts if p[k]["src"] >= 0]
        if single[k]["src"] < 0:
            assert not owners
            continue
        assert len(owners) == 1, k
        o, s = owners[0], single[k]
        assert (o["src"], o["dst"], o["num_inliers"], o["confidence"]) == (s["src"], s["dst"], s["num_inliers"], s["confidence"])
        assert np.asarray(o["matches"]).tobytes() == np.asarray(s["matches"]).tobytes()
        assert np.asarray(o["inliers_mask"]).tobytes() == np.asarray(s["inliers_mask"]).tobytes()
        assert (o["H"] is None) == (s["H"] is None)
        if s["H"] is not None:
            assert np.asarray(o["H"], np.float64).tobytes() == np.asarray(s["H"], np.float64).tobytes()
