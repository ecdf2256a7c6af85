"""The ray bundle adjuster through the GPU entry point (device keypoints, PairwiseMatches; the kernels of csrc/motion_ray.hip)
against the independent reading of tests/refimpl_motion_ray.py, and bit for bit against the host twin of
tests/harness/ba_ray_host_harness.cpp: the same arithmetic header in plain loops on the CPU."""
import numpy as np
import pytest

import ba_ray_twin as twin
import refimpl_motion as rm
import refimpl_motion_ray as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    lib = twin.build(tmp_path_factory.mktemp("baray"))
    assert lib is not None, "hipcc is needed for the host twin"
    return lib


def _device_side(ctx, scene):
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import KP_DTYPE, PairwiseMatches
    feats = []
    for i, xy in enumerate(scene["xy"]):
        kp = np.zeros(len(xy), KP_DTYPE)
        kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
        feats.append(isa.ImageFeatures.upload(ctx, (rm.W, rm.H), kp, np.zeros((len(xy), 32), np.uint8), img_idx=i))
    return feats, PairwiseMatches.from_entries(ctx, scene["n"], _entries(scene))


def _entries(scene, edit=None):
    out = []
    for e in scene["entries"]:
        mm = e["matches"].copy()
        if edit and (e["i"], e["j"]) == (0, 1):
            edit(mm)
        out.append((e["i"], e["j"], mm, e["inliers_mask"], e["num_inliers"], e["has_H"], e["H"], e["confidence"]))
    return out


@pytest.fixture(scope="module")
def device_scenes(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _device_side(ctx, rr.get_ray_scene(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name,eligible", rr.RAY_CASES, ids=[c[0] for c in rr.RAY_CASES])
def test_ray_adjustment_reaches_the_reference_minimum_and_equals_the_twin(ctx, harness, device_scenes, name, eligible):
    import image_stitching_amd as isa
    scene = rr.get_ray_scene(name)
    feats, pm = device_scenes(name)
    ref = rr.get_ray_reference(name)
    got = isa.bundle_adjust_ray(ctx, feats, pm, scene["start"], conf_thresh=rm.THR)
    print()
    twin.report("    device", name, rr.check_ba_ray(ref, got, eligible), "  %d observations" % ref["n_obs"])
    rc, want = twin.run(harness, scene["n"], scene["xy"], rm.table(scene), scene["start"], rm.THR)
    assert rc == 0
    rr.check_ba_ray(ref, want, eligible)
    assert twin.same_bits(got, want), "the device and the host twin differ in some bit"
    assert twin.same_bits(got, isa.bundle_adjust_ray(ctx, feats, pm, scene["start"], conf_thresh=rm.THR)), "two calls differ"


def test_principal_point_and_aspect_are_not_read(ctx, device_scenes):
    import image_stitching_amd as isa
    scene = rr.get_ray_scene("chain5")
    feats, pm = device_scenes("chain5")
    shifted = rr.shifted_start(scene)
    a = isa.bundle_adjust_ray(ctx, feats, pm, scene["start"], conf_thresh=rm.THR)
    b = isa.bundle_adjust_ray(ctx, feats, pm, shifted, conf_thresh=rm.THR)
    assert twin.same_bits(a, b)
    for g, s in zip(b, shifted):
        assert all(np.array_equal(rm._bits(g[k]), rm._bits(s[k])) for k in rr.FIXED)


def test_refused_input_leaves_the_context_usable(ctx, device_scenes):
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import PairwiseMatches
    scene = rr.get_ray_scene("chain5")
    feats, pm = device_scenes("chain5")
    first = isa.bundle_adjust_ray(ctx, feats, pm, scene["start"], conf_thresh=rm.THR)
    with pytest.raises(isa.MisError):
        isa.bundle_adjust_ray(ctx, feats, pm, scene["start"], conf_thresh=1e9)                  # no pair above the threshold

    def past_the_end(mm):
        mm["train_idx"][3] = len(scene["xy"][1])                                                # one past the last keypoint of image 1

    def negative(mm):
        mm["query_idx"][5] = -1
    for edit in (past_the_end, negative):
        with pytest.raises(isa.MisError):
            isa.bundle_adjust_ray(ctx, feats, PairwiseMatches.from_entries(ctx, scene["n"], _entries(scene, edit)), scene["start"], conf_thresh=rm.THR)
        assert twin.same_bits(first, isa.bundle_adjust_ray(ctx, feats, pm, scene["start"], conf_thresh=rm.THR))


def test_features_of_a_detect_batch_call(ctx, harness):
    """Device keypoints written by the ORB kernels (not uploaded), matches of the matcher: the same assertions, and the twin's bits."""
    import torch
    import synth
    import image_stitching_amd as isa
    w, h, n = rm.W, rm.H, 5
    cams = [synth.make_camera(w, h, 60.0, 11.0 * i - 22.0, 2.5 * ((i % 3) - 1), 1.5 * ((i % 2) - 0.5)) for i in range(n)]
    feats = isa.OrbFeatureFinder(ctx, (w, h)).detect_batch([torch.from_numpy(synth.render_frame(c)).cuda() for c in cams])
    pm = isa.BestOf2NearestMatcher(ctx, 0.32)(feats)
    rng = np.random.default_rng(31)
    start = [dict(focal=float(c["K"][0, 0]), aspect=1.0, ppx=float(c["K"][0, 2]), ppy=float(c["K"][1, 2]),
                  R=rm.f32(rm.rot_yxz(*rng.normal(0, 0.5, 3)) @ c["R"])) for c in cams]
    xy = [np.stack([k["x"], k["y"]], 1).astype(np.float32) for k, _ in (f.download() for f in feats)]
    tab = [dict(src_img_idx=m.src_img_idx, dst_img_idx=m.dst_img_idx, matches=m.matches, inliers_mask=m.inliers_mask, num_inliers=m.num_inliers,
                has_H=1 if m.H is not None else 0, H=m.H, confidence=m.confidence) for m in pm]
    ref = rr.reference_ba_ray(dict(name="orb", n=n, xy=xy, start=start), tab, rm.THR)
    assert ref is not None and len(ref["obs"]) >= n - 1 and ref["cond"] <= rm.COND_CAP
    got = isa.bundle_adjust_ray(ctx, feats, pm, start, conf_thresh=rm.THR)
    print()
    twin.report("    device", "orb", rr.check_ba_ray(ref, got, True), "  %d observations" % ref["n_obs"])
    rc, want = twin.run(harness, n, xy, tab, start, rm.THR)
    assert rc == 0 and twin.same_bits(got, want)
