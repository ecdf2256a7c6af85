"""GPU: features_type = "akaze" through the jobs, on four frames of the synthetic sweep at 400 x 225: the smallest size, enlarging
from 320 x 180 in steps of 80 columns, at which both jobs keep all four frames (at 320 x 180 the AKAZE job finds 70 to 89 keypoints
a frame -- its borders are 28 to 57 level pixels -- no pair passes, and frame 0 is kept alone; at 400 x 225 it finds 205 to 232 with
12 to 18 inliers between neighbours; the ORB job keeps all four at both).  Composition is camera-driven, so with supplied cameras the AKAZE job's panorama equals the ORB job's bit for
bit as soon as both keep the same frames; and an ORB job's features and matches do not change by an AKAZE finder on its context."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE = (400, 225)
YAWS = [-13.0, 0.0, 13.0, 26.0]


def _cams():
    import synth
    return [synth.make_camera(SIZE[0], SIZE[1], 60.0, y, 0.4 * ((i % 3) - 1), 0.3 * ((i % 2) - 0.5), 0.95 + 0.02 * i) for i, y in enumerate(YAWS)]


def _entry_bytes(m):
    return (m.src_img_idx, m.dst_img_idx, m.num_inliers, np.float64(m.confidence).tobytes(), np.asarray(m.matches).tobytes(),
            np.asarray(m.inliers_mask).tobytes(), None if m.H is None else np.asarray(m.H, np.float64).tobytes())


def _feature_bytes(feats):
    return [tuple(a.tobytes() for a in f.download()) for f in feats]


@pytest.fixture(scope="module")
def scene(ctx):
    import synth
    import image_stitching_amd as isa
    cams = _cams()
    frames = [synth.render_frame_gpu(c) for c in cams]
    # the ORB job FIRST: before an AKAZE finder was ever created on this context
    orb = isa.Stitcher(ctx, SIZE, isa.StitchConfig.hot_path())
    pano, mask, feats, pm, idx = orb.stitch(frames, cams)
    before = dict(pano=pano.cpu().numpy(), mask=mask.cpu().numpy(), idx=list(idx), feats=_feature_bytes(feats), entries=[_entry_bytes(m) for m in pm])
    return dict(cams=cams, frames=frames, orb=before)


def test_stitcher_with_akaze_keeps_all_frames_and_composes_the_orb_panorama(ctx, scene):
    import image_stitching_amd as isa
    st = isa.Stitcher(ctx, SIZE, isa.StitchConfig.hot_path(features_type="akaze", match_conf=0.65))
    assert type(st.finder).__name__ == "AkazeFeatureFinder"
    pano, mask, feats, pm, idx = st.stitch(scene["frames"], scene["cams"])
    assert list(idx) == [0, 1, 2, 3] == scene["orb"]["idx"]
    assert all(f.raw.desc_cols == 61 and len(f) > 100 for f in feats)
    assert np.array_equal(pano.cpu().numpy(), scene["orb"]["pano"]) and np.array_equal(mask.cpu().numpy(), scene["orb"]["mask"])
    n = len(feats)
    assert all(pm[i * n + i + 1].num_inliers >= 6 for i in range(n - 1))


def test_single_rank_job_with_akaze_does_the_same(ctx, scene):
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    job = StitchJob(ctx, SIZE, scene["cams"], config=StitchConfig.hot_path(features_type="akaze", match_conf=0.65))
    assert type(job.engine.finder).__name__ == "AkazeFeatureFinder" and job.engine._row_bytes() == 61
    out = job.run({i: f for i, f in enumerate(scene["frames"])})
    assert list(out["indices"]) == [0, 1, 2, 3]
    assert np.array_equal(out["pano"].cpu().numpy(), scene["orb"]["pano"]) and np.array_equal(out["mask"].cpu().numpy(), scene["orb"]["mask"])
    with pytest.raises(NotImplementedError, match="akaze"):
        StitchJob(ctx, SIZE, scene["cams"], rank=0, world_size=2, config=StitchConfig.hot_path(features_type="akaze", match_conf=0.65))


def test_an_orb_job_is_byte_identical_after_the_akaze_finder_ran(ctx, scene):
    """(runs after the AKAZE jobs above used this context's matcher workspace and feature pool)"""
    import image_stitching_amd as isa
    isa.AkazeFeatureFinder(ctx, SIZE).detect(scene["frames"][0])
    orb = isa.Stitcher(ctx, SIZE, isa.StitchConfig.hot_path())
    pano, mask, feats, pm, idx = orb.stitch(scene["frames"], scene["cams"])
    was = scene["orb"]
    assert list(idx) == was["idx"] and _feature_bytes(feats) == was["feats"] and [_entry_bytes(m) for m in pm] == was["entries"]
    assert np.array_equal(pano.cpu().numpy(), was["pano"])
