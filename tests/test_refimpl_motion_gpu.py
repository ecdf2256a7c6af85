"""Camera refinement through the GPU entry point (device keypoints, PairwiseMatches) against the independent reading of
tests/refimpl_motion.py: the case list and the assertions of test_refimpl_motion_cpu.py on isa.bundle_adjust_reproj, plus
bit-equality with the oracle, plus one case whose device features come from an ORB detect_batch call."""
import numpy as np
import pytest

import refimpl_motion as rm

pytestmark = pytest.mark.gpu


def _device_side(ctx, scene):
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import KP_DTYPE, PairwiseMatches
    feats = []
    for i, xy in enumerate(scene["xy"]):
        kp = np.zeros(len(xy), KP_DTYPE)
        kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
        feats.append(isa.ImageFeatures.upload(ctx, (rm.W, rm.H), kp, np.zeros((len(xy), 32), np.uint8), img_idx=i))
    pm = PairwiseMatches.from_entries(ctx, scene["n"], [(e["i"], e["j"], e["matches"], e["inliers_mask"], e["num_inliers"], e["has_H"], e["H"], e["confidence"])
                                                        for e in scene["entries"]])
    return feats, pm


def _oracle(oracle, scene, tab, start, mask):
    ofe = [dict(img_w=rm.W, img_h=rm.H, xy=xy, desc=np.zeros((len(xy), 32), np.uint8)) for xy in scene["xy"]]
    return oracle.bundle_adjust_reproj(ofe, tab, start, rm.THR, mask)[0]


def _same_bits(a, b):
    return all(np.array_equal(rm._bits(x["R"]), rm._bits(y["R"])) and all(np.array_equal(rm._bits(x[k]), rm._bits(y[k])) for k in rm.INTR) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def device_scenes(ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _device_side(ctx, rm.get_scene(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name,mask,eligible", rm.BA_CASES, ids=["%s-%s%s" % (n, m, "" if e else "-cost-only") for n, m, e in rm.BA_CASES])
def test_bundle_adjustment_reaches_the_reference_minimum(ctx, oracle_mod, device_scenes, name, mask, eligible):
    import image_stitching_amd as isa
    scene = rm.get_scene(name)
    feats, pm = device_scenes(name)
    ref = rm.get_reference(name, mask)
    got = isa.bundle_adjust_reproj(ctx, feats, pm, scene["start"], conf_thresh=rm.THR, refine_mask=mask)
    res = rm.check_ba(ref, got, eligible)
    print("\n    %s %s excess %+.3e  /Y %+.3f  /E %+.2e  parameters / bound %s" % (name, mask, res["excess"], res["over_Y"], res["over_E"],
                                                                               "cost only" if res["par_ratio"] is None else "%.3f" % res["par_ratio"]))
    assert _same_bits(got, _oracle(oracle_mod, scene, rm.table(scene), scene["start"], mask))


def test_skew_position_and_refused_input(ctx, device_scenes):
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import PairwiseMatches
    scene = rm.get_scene("chain5")
    feats, pm = device_scenes("chain5")
    a = isa.bundle_adjust_reproj(ctx, feats, pm, scene["start"], conf_thresh=rm.THR, refine_mask="xxxxx")
    b = isa.bundle_adjust_reproj(ctx, feats, pm, scene["start"], conf_thresh=rm.THR, refine_mask="x_xxx")
    assert _same_bits(a, b)
    with pytest.raises(isa.MisError):
        isa.bundle_adjust_reproj(ctx, feats, pm, scene["start"], conf_thresh=1e9)                  # no pair above the threshold
    entries = []
    for e in scene["entries"]:
        mm = e["matches"].copy()
        if (e["i"], e["j"]) == (0, 1):
            mm["train_idx"][3] = len(scene["xy"][1])                                              # one past the last keypoint of image 1
        entries.append((e["i"], e["j"], mm, e["inliers_mask"], e["num_inliers"], e["has_H"], e["H"], e["confidence"]))
    with pytest.raises(isa.MisError):
        isa.bundle_adjust_reproj(ctx, feats, PairwiseMatches.from_entries(ctx, scene["n"], entries), scene["start"], conf_thresh=rm.THR)


def test_features_of_a_detect_batch_call(ctx, oracle_mod):
    """Device keypoints written by the ORB kernels (not uploaded), matches of the matcher: the same cost assertions, rotations only."""
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
    scene = dict(name="orb", n=n, xy=xy, start=start)
    ref = rm.reference_ba(scene, tab, rm.THR, "_____")
    assert ref is not None and len(ref["obs"]) >= n - 1 and ref["cond"] <= rm.COND_CAP
    got = isa.bundle_adjust_reproj(ctx, feats, pm, start, conf_thresh=rm.THR, refine_mask="_____")
    res = rm.check_ba(ref, got, True)
    print("\n    orb _____ %d observations, excess %+.3e  /Y %+.3f  /E %+.2e  parameters / bound %.3f" % (ref["n_obs"], res["excess"], res["over_Y"], res["over_E"], res["par_ratio"]))
    ofe = [dict(img_w=w, img_h=h, xy=p, desc=np.zeros((len(p), 32), np.uint8)) for p in xy]
    assert _same_bits(got, oracle_mod.bundle_adjust_reproj(ofe, tab, start, rm.THR, "_____")[0])
