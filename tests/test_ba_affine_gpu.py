"""The affine-partial bundle adjuster through the GPU entry point (device keypoints from ImageFeatures.upload, tables from
PairwiseMatches.from_entries; the kernels of csrc/ba_eval_device.h over ba_affine.h) against the independent reading of
tests/refimpl_affine_family.py, and bit for bit against the host twin of tests/harness/ba_affine_host_harness.cpp: the same
arithmetic header in plain loops on the CPU.  Scenes of 3 - 6 cameras, noise-free and with 0.5 px keypoint noise, from perturbed
similarities; inlier counts on the kernels' edges (1, 31, 32, 33 per edge; 255, 256, 257 in total)."""
import numpy as np
import pytest

import ba_affine_twin as twin
import refimpl_affine_family as ra
import refimpl_motion as rm

pytestmark = pytest.mark.gpu
SIZE = (ra.BA_W, ra.BA_H)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    lib = twin.build(tmp_path_factory.mktemp("baaffine"))
    assert lib is not None, "hipcc is needed for the host twin"
    return lib


def _entries(scene, edit=None):
    out = []
    for e in scene["entries"]:
        mm = e["matches"].copy()
        if edit:
            edit(e["i"], e["j"], mm)
        out.append((e["i"], e["j"], mm, e["inliers_mask"], e["num_inliers"], e["has_H"], e["H"], e["confidence"]))
    return out


def _device_side(ctx, scene, edit=None):
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import KP_DTYPE, PairwiseMatches
    feats = []
    for i, xy in enumerate(scene["xy"]):
        kp = np.zeros(len(xy), KP_DTYPE)
        kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
        feats.append(isa.ImageFeatures.upload(ctx, SIZE, kp, np.zeros((len(xy), 32), np.uint8), img_idx=i))
    return feats, PairwiseMatches.from_entries(ctx, scene["n"], _entries(scene, edit))


@pytest.mark.parametrize("name,sigma", ra.BA_CASES)
def test_adjustment_reaches_the_reference_minimum_and_equals_the_twin(ctx, harness, name, sigma):
    import image_stitching_amd as isa
    scene, tab, ref = ra.get_ba_scene(name, sigma)
    feats, pm = _device_side(ctx, scene)
    got = isa.bundle_adjust_affine_partial(ctx, feats, pm, scene["start"], conf_thresh=ra.BA_THR)
    res = ra.check_ba_affine(ref, got)
    print("\n    device %s s%g: %d observations  S* %.6g  excess %+.3e  /E %+.2e  parameters / bound %.3f  cond %.3g" % (
        name, sigma, ref["n_obs"], ref["S"], res["excess"], res["over_E"], res["par_ratio"], ref["cond"]))
    rc, want = twin.run(harness, scene["n"], scene["xy"], tab, scene["start"], ra.BA_THR, size=SIZE)
    assert rc == 0
    assert twin.same_bits(got, want), "the device and the host twin differ in some bit"
    assert twin.same_bits(got, isa.bundle_adjust_affine_partial(ctx, feats, pm, scene["start"], conf_thresh=ra.BA_THR)), "two calls differ"


def test_edge_rules_on_the_device(ctx, harness):
    """An edge at confidence == conf_thresh is not an edge (its corrupt matches do not move the result); a masked-out match is
    not read (its indices lie far outside the features); the result is the twin's."""
    import image_stitching_amd as isa
    d = ra.BA_SCENES["chain4-255"]
    thr = float(np.float32(ra.BA_THR))
    scene = ra.make_ba_scene("rules", d["sims"], d["edges"], 0.5, 7, counts=d["counts"], conf={(0, 2): thr}, corrupt=[(0, 2)], wild_masked=[(1, 2)])
    tab = rm.table(scene)
    ref = ra.reference_ba_affine(scene, tab, ra.BA_THR)
    assert ref["n_obs"] == 255 - 30
    feats, pm = _device_side(ctx, scene)
    got = isa.bundle_adjust_affine_partial(ctx, feats, pm, scene["start"], conf_thresh=ra.BA_THR)
    ra.check_ba_affine(ref, got)
    rc, want = twin.run(harness, scene["n"], scene["xy"], tab, scene["start"], ra.BA_THR, size=SIZE)
    assert rc == 0 and twin.same_bits(got, want)


def test_degenerate_camera_stays_finite(ctx, harness):
    """A camera with a = b = 0: invertAffineTransform's D = 0 gives the zero inverse, not a division by zero; every returned
    value is finite and the device follows the twin."""
    import image_stitching_amd as isa
    scene, tab, _ = ra.get_ba_scene("chain4-255", 0.5)
    start = [dict(c) for c in scene["start"]]
    start[3] = dict(start[3], R=np.array([[0, 0, 5], [0, 0, 7], [0, 0, 1]], np.float32))
    feats, pm = _device_side(ctx, scene)
    got = isa.bundle_adjust_affine_partial(ctx, feats, pm, start, conf_thresh=ra.BA_THR)
    assert all(np.isfinite(g["R"]).all() for g in got)
    rc, want = twin.run(harness, scene["n"], scene["xy"], tab, start, ra.BA_THR, size=SIZE)
    assert rc == 0 and twin.same_bits(got, want)


def test_out_of_range_indices_are_refused_and_the_context_stays_usable(ctx):
    import image_stitching_amd as isa
    scene, tab, ref = ra.get_ba_scene("chain3", 0.5)
    for field, cam in (("query_idx", 1), ("train_idx", 2)):
        def edit(i, j, mm, field=field, cam=cam):
            if (i, j) == (1, 2):
                mm[field][7] = len(scene["xy"][cam])
        feats, pm = _device_side(ctx, scene, edit)
        with pytest.raises(isa.MisError, match="exceed the feature counts") as ei:
            isa.bundle_adjust_affine_partial(ctx, feats, pm, scene["start"], conf_thresh=ra.BA_THR)
        assert ei.value.code == -1      # MIS_E_INVALID
    with pytest.raises(isa.MisError):
        def neg(i, j, mm):
            if (i, j) == (0, 2):
                mm["query_idx"][0] = -1
        feats, pm = _device_side(ctx, scene, neg)
        isa.bundle_adjust_affine_partial(ctx, feats, pm, scene["start"], conf_thresh=ra.BA_THR)
    feats, pm = _device_side(ctx, scene)
    ra.check_ba_affine(ref, isa.bundle_adjust_affine_partial(ctx, feats, pm, scene["start"], conf_thresh=ra.BA_THR))
