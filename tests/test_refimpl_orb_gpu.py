"""GPU: OrbFeatureFinder.detect / detect_batch (orb.hip) against the numpy reference of tests/refimpl_orb.py -- the gray level,
the NMS map and the blurred level of every pyramid level exactly, then the keypoints as sets per level, their canonical order,
the angles within the reference's band and every determined descriptor bit.

describe_direct_kernel is the only descriptor path: the pattern of every accepted patch size (2 .. 40) reaches at most
round(20 sqrt 2) = 28 = DD_R, which orb.hip asserts at compile time.  It computes the angle and blurs at the sample points of
the patch it stages; no blurred pyramid is built.  blur_kernel exists for the debug view of the blurred level only and runs
here through it."""
import numpy as np
import pytest

import refimpl_orb as ro
from test_refimpl_orb_cpu import (MAX_NFEATURES, REGIMES, REGIME_IDS, TIE_BEYOND_SLACK, TIE_INSIDE_SLACK, binary_noise, report,
                                  synth_frame, tie_motif, uniform_noise)

pytestmark = pytest.mark.gpu

E_OVERFLOW = -4


def _finder(ctx, size, kw):
    import image_stitching_amd as isa
    return isa.OrbFeatureFinder(ctx, size, isa.stitching.orb_params(**kw))


def check_gpu(finder, frame, kw, tag, img=None, stages=True):
    """One detect against the reference (img: the device tensor to detect on, default the frame uploaded)."""
    import torch
    p = ro.params(**kw)
    ref = ro.orb(frame, p, stages=stages)
    feats = finder.detect(img if img is not None else torch.from_numpy(frame).cuda())
    assert feats.img_size == (frame.shape[1], frame.shape[0])
    if stages:
        for l in range(p["nlevels"]):
            assert np.array_equal(finder.debug_level(l, 0), ref["gray"][l]), (tag, "gray", l)
            assert np.array_equal(finder.debug_level(l, 1), ref["nms"][l]), (tag, "nms", l)
            assert np.array_equal(finder.debug_level(l, 2), ref["blur"][l]), (tag, "blur", l)
    kps, desc = feats.download()
    c = ro.compare_features(kps, desc, ref)
    assert not c["errors"], (tag, c["errors"])
    report(tag, c)
    return kps, desc, ref


@pytest.mark.parametrize("tag,make,kw", REGIMES, ids=REGIME_IDS)
def test_kernels_match_reference(ctx, tag, make, kw):
    frame = make()
    finder = _finder(ctx, (frame.shape[1], frame.shape[0]), kw)
    check_gpu(finder, frame, kw, tag)


def test_1080p_and_4k_then_small_frames_after_replan(ctx):
    """A 1080p and a 4K frame (BASELINE configs 2 and 3) with the default parameters; the 4K finder then detects smaller frames
    (the plan is rebuilt for each size) and the 4K frame again."""
    import synth
    f2 = synth.render_frame(synth.workload("config2")[1])
    check_gpu(_finder(ctx, (1920, 1080), {}), f2, {}, "1080p", stages=False)
    f4 = synth.render_frame(synth.workload("config3")[7])
    finder = _finder(ctx, (3840, 2160), {})
    k4, d4, _ = check_gpu(finder, f4, {}, "4k", stages=False)
    assert len(k4) == 4000
    check_gpu(finder, synth_frame(333, 257), {}, "333x257 after 4k")
    check_gpu(finder, synth_frame(97, 71), {}, "97x71 after 4k")
    import torch
    k, d = finder.detect(torch.from_numpy(f4).cuda()).download()
    assert np.array_equal(k, k4) and np.array_equal(d, d4)


def test_detect_batch_of_three_frames(ctx):
    """Three frames of different content in one batch: each equals its single detect and the reference."""
    import torch
    w, h = 333, 257
    frames = [synth_frame(w, h, 10.0), uniform_noise(w, h, 9), binary_noise(w, h, 4)]
    kw = dict(nfeatures=1500, nlevels=6, patch_size=30)
    finder = _finder(ctx, (w, h), kw)
    batch = [f.download() for f in finder.detect_batch([torch.from_numpy(f).cuda() for f in frames])]
    for i, (f, (bk, bd)) in enumerate(zip(frames, batch)):
        k, d, ref = check_gpu(finder, f, kw, "batch frame %d" % i, stages=False)
        assert np.array_equal(bk, k) and np.array_equal(bd, d)
        assert not ro.compare_features(bk, bd, ref)["errors"]


def test_detect_batch_of_more_frames_than_a_group(ctx):
    """17 frames in one batch: a full group of ORB_BATCH = 16 workspaces and a second group of one, the counts and the overflow
    flags of 17 + 16 places gathered at the end.  Each result equals its single detect bit for bit; the first frame and the last
    (the second group's) equal the reference."""
    import torch
    w, h = 97, 71
    makers = [lambda s: synth_frame(w, h, 5.0 + 3.0 * s), lambda s: uniform_noise(w, h, 20 + s), lambda s: binary_noise(w, h, 40 + s)]
    frames = [makers[i % 3](i) for i in range(17)]
    kw = dict(nfeatures=300, nlevels=4)
    finder = _finder(ctx, (w, h), kw)
    imgs = [torch.from_numpy(f).cuda() for f in frames]
    batch = [f.download() for f in finder.detect_batch(imgs)]
    assert len(batch) == 17
    for i, (img, (bk, bd)) in enumerate(zip(imgs, batch)):
        if i in (0, 16):
            k, d, _ = check_gpu(finder, frames[i], kw, "batch of 17, frame %d" % i, img=img)
        else:
            k, d = finder.detect(img).download()
        assert np.array_equal(bk, k) and np.array_equal(bd, d), i


def test_strided_unaligned_bgr_view(ctx):
    """A BGR view with a padded row stride that is not a multiple of 4 and a column offset of one pixel (3 bytes): gray_kernel's
    byte path."""
    import torch
    w, h = 131, 97
    frame = synth_frame(w, h, 35.0)
    big = torch.zeros((h, w + 7, 3), dtype=torch.uint8, device="cuda")
    view = big[:, 1:1 + w]
    view.copy_(torch.from_numpy(frame).cuda())
    assert view.data_ptr() % 4 != 0 and view.stride(0) % 4 != 0
    check_gpu(_finder(ctx, (w, h), {}), frame, {}, "strided view", img=view)


def test_ties_inside_the_slack_exact_beyond_it_overflow(ctx):
    """Ties at both retainBest cuts keep 60 + n_b keypoints for a budget of 100.  Inside the 128 keypoints of slack the result is
    the reference's; beyond it the detect fails with MIS_E_OVERFLOW, and the finder is correct afterwards."""
    import torch
    import image_stitching_amd as isa
    inside, kw = tie_motif(TIE_INSIDE_SLACK)
    beyond, _ = tie_motif(TIE_BEYOND_SLACK)
    finder = _finder(ctx, (200, 200), kw)
    k, _, ref = check_gpu(finder, inside, kw, "ties inside the slack")
    assert len(k) == 60 + TIE_INSIDE_SLACK > kw["nfeatures"]
    assert len(ro.orb(beyond, ro.params(**kw), stages=False)["kps"]) == 60 + TIE_BEYOND_SLACK
    with pytest.raises(isa.MisError) as e:
        finder.detect(torch.from_numpy(beyond).cuda())
    assert e.value.code == E_OVERFLOW
    check_gpu(finder, inside, kw, "ties inside the slack, after the overflow")
    with pytest.raises(isa.MisError) as e:
        finder.detect_batch([torch.from_numpy(inside).cuda(), torch.from_numpy(beyond).cuda()])
    assert e.value.code == E_OVERFLOW
    check_gpu(finder, inside, kw, "ties inside the slack, after the batch overflow")
    assert MAX_NFEATURES == max(n for n in range(8800, 8900) if max(ro.level_budgets(ro.params(nfeatures=n))) <= ro.MAX_LEVEL_FEATURES)
