"""GPU: AkazeFeatureFinder (akaze.hip) against the numpy reference of tests/refimpl_akaze.py, by the scheme of
test_refimpl_sift_gpu.py: every stage is judged against the reference's step applied to the library's own downloaded input of that
stage (tests/akaze_check.py), so rounding never compounds -- the FED schedules to one ulp, every Lt, Lsmooth, flow, Lx, Ly and
Ldet plane inside its band, the k-contrast, every decided keypoint present with its fields inside their bands and nothing beyond
decided + undecided in (level, y, x) order, angles, and every decided descriptor bit.

The bands (4 x the largest float64-against-float32 / other-order difference of the reference's own steps on these shapes, measured
on the CPU by `python tests/akaze_check.py`; the measured values stand beside the constants in tests/akaze_check.py):"""
import numpy as np
import pytest

import akaze_check as ac
import refimpl_akaze as ra
from akaze_check import (BAND_ANGLE, BAND_COORD, BAND_D, BAND_EDGE, BAND_FLOW, BAND_GAP, BAND_LDET, BAND_LSMOOTH, BAND_LT, BAND_LXY, BAND_PT,  # noqa: F401
                         BAND_VALUE, CAP_SKIPPED_ANGLES, CAP_UNDECIDED_BITS, CAP_UNDECIDED_KPS)

pytestmark = pytest.mark.gpu


def _finder(ctx, size, kw):
    import image_stitching_amd as isa
    return isa.AkazeFeatureFinder(ctx, size, kw)


def gpu_run(finder, frame, img=None):
    """One detect and everything the library kept of it, in the form akaze_check.check_run judges."""
    import torch
    img = img if img is not None else torch.from_numpy(frame).cuda()
    feats = finder.detect(img)
    assert feats.img_size == (frame.shape[1], frame.shape[0])
    kps, desc = feats.download()
    counts = finder.debug_counts()
    nlev = len(ra.plan(frame.shape[1], frame.shape[0], finder.params.n_octaves, finder.params.n_octave_layers))
    planes = [{name: finder.debug_level(l, name) for name in finder.PLANES} for l in range(nlev)]
    taus = [finder.debug_fed(l) for l in range(nlev)]
    return dict(planes=planes, taus=taus, counts=counts, kps=kps, class_ids=finder.debug_class_ids(len(kps)), desc=desc), feats


@pytest.fixture(scope="module")
def cases():
    return ac.cases()


@pytest.mark.parametrize("i", range(8))
def test_kernels_match_the_reference(ctx, cases, i):
    c = cases[i]
    frame = c["frame"]
    run, _ = gpu_run(_finder(ctx, (frame.shape[1], frame.shape[0]), c["kw"]), frame)
    rep = ac.check_run(c["tag"], frame, c["kw"], run)
    print(c["tag"], rep)
    if c["kw"].get("max_points"):
        assert len(run["kps"]) == c["kw"]["max_points"]


def test_a_finder_planned_for_a_larger_frame_and_two_runs_give_the_same_bytes(ctx, cases):
    """A finder planned for 640 x 360 detects the 97 x 71 frame and then the 333 x 251 frame (the plan is rebuilt for each size);
    a second detect of the same frame returns identical bytes."""
    finder = _finder(ctx, (640, 360), {})
    for c in (cases[0], cases[3]):
        run, _ = gpu_run(finder, c["frame"])
        ac.check_run(c["tag"] + " (larger plan)", c["frame"], c["kw"], run)
    again, _ = gpu_run(finder, cases[3]["frame"])
    assert again["kps"].tobytes() == run["kps"].tobytes() and again["desc"].tobytes() == run["desc"].tobytes() and len(run["kps"]) > 100


def test_a_batch_of_three_frames_equals_their_single_detects(ctx):
    import torch
    frames = [ac.rendered(333, 251, yaw=y) for y in (20.0, 40.0, 75.0)]
    finder = _finder(ctx, (333, 251), {})
    imgs = [torch.from_numpy(f).cuda() for f in frames]
    batch = finder.detect_batch(imgs)
    assert [f.img_idx for f in batch] == [0, 1, 2]
    for f, img in zip(batch, imgs):
        k, d = f.download()
        k1, d1 = finder.detect(img).download()
        assert len(k) > 50 and k.tobytes() == k1.tobytes() and d.tobytes() == d1.tobytes() and d.shape[1] == 61


def test_refused_parameters_and_capacity(ctx):
    import image_stitching_amd as isa
    for kw in (dict(descriptor_type=4), dict(descriptor_type=3), dict(diffusivity=0), dict(descriptor_size=64), dict(descriptor_channels=1)):
        with pytest.raises(isa.MisError) as e:
            _finder(ctx, (160, 96), kw)
        assert e.value.code == -6, kw
    # a frame of noise has more strict maxima than one in 32 pixels: refused with the count, never truncated
    import torch
    noise = np.random.default_rng(3).integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
    finder = _finder(ctx, (1024, 1024), dict(threshold=0.0))
    try:
        feats = finder.detect(torch.from_numpy(noise).cuda())
        assert finder.debug_counts()["candidates"] <= 1024 * 1024 // 32 and len(feats) <= finder.debug_counts()["candidates"]
    except isa.MisError as e:
        assert e.code == -4 and re_count(str(e)) > 1024 * 1024 // 32


def re_count(text):
    import re
    return int(re.search(r"(\d+) candidates exceed", text).group(1))
