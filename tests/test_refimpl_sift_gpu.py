"""GPU: SiftFeatureFinder (sift.hip) against the numpy reference of tests/refimpl_sift.py over the regimes of
test_refimpl_sift_cpu.py -- every Gaussian level inside the band of the reference's blur of the library's own previous level, every
DoG level the exact float32 difference, the keypoints of stages 7 - 11 run on the library's downloaded pyramid (every decided one
present with its fields inside their bands, nothing beyond decided + undecided, octave fields equal, KeyPoint_LessThan order, no
duplicates), every descriptor element within 0.5 + band of the reference's value for the library's own keypoint -- and bit for bit
against oracle.Sift with the same parameters, as test_sift_gpu.py does for the defaults.

Kernels the defaults never run and these regimes do: sift_extrema_generic_kernel (n_octave_layers != 3), the N = 0 instances of
sift_blur_rows_kernel / sift_blur_cols_kernel (7, 9, 15, 19, 37 and 91 taps, rows wider than one 2048-output block), the direct
appends of sift_extrema_kernel<3> past its 1024-entry tile list."""
import ctypes as C

import numpy as np
import pytest

import refimpl_sift as rs
from test_refimpl_sift_cpu import REGIMES, REGIME_IDS, blocks, check, oracle_pyramid, rendered, sigma_at_cap

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -6


def _finder(ctx, size, kw):
    import image_stitching_amd as isa
    return isa.SiftFeatureFinder(ctx, size, kw)


def gpu_pyramid(finder, img, w, h, nl):
    """Every Gaussian and DoG level of the library's scale space of `img`, downloaded through mis_sift_debug_level."""
    from image_stitching_amd.stitching import as_image
    im = as_image(img)
    gauss, dog = [], []
    for o, (ow, oh) in enumerate(rs.octave_sizes(w, h)):
        for store, n, flag in ((gauss, nl + 3, 0), (dog, nl + 2, 1)):
            lv = np.zeros((n, oh, ow), np.float32)
            for i in range(n):
                gw, gh = C.c_int(), C.c_int()
                finder.ctx.check(finder.ctx.lib.mis_sift_debug_level(finder.h, C.byref(im), o, i, flag, lv[i].ctypes.data_as(C.c_void_p), C.byref(gw), C.byref(gh)))
                assert (gw.value, gh.value) == (ow, oh), (o, i, gw.value, gh.value)
            store.append(lv)
    return dict(gauss=gauss, dog=dog)


def check_gpu(finder, oracle_mod, tag, frame, kw, img=None):
    """One detect against the reference and, bit for bit, against the oracle (img: the device tensor to detect on)."""
    import torch
    h, w = frame.shape[:2]
    nl = rs.params(**kw)["n_octave_layers"]
    img = img if img is not None else torch.from_numpy(frame).cuda()
    feats = finder.detect(img)
    assert feats.img_size == (w, h)
    kps, desc = feats.download()
    counts = finder.debug_counts()
    assert counts["keypoints"] == len(kps) <= counts["raw"]
    pyr = gpu_pyramid(finder, img, w, h, nl)
    check(tag, frame, kw, pyr, kps, desc, counts)
    o = oracle_mod.Sift(w, h, kw)
    ko, do = o.run(frame)
    opyr = oracle_pyramid(o, nl)
    assert len(pyr["gauss"]) == o.num_octaves()
    for k in range(o.num_octaves()):
        assert np.array_equal(pyr["gauss"][k].view(np.uint32), opyr["gauss"][k].view(np.uint32)), (tag, "gauss", k)
        assert np.array_equal(pyr["dog"][k].view(np.uint32), opyr["dog"][k].view(np.uint32)), (tag, "dog", k)
    assert (counts["candidates"], counts["refined"], counts["raw"]) == (o.num_candidates(), o.num_refined(), o.num_raw_keypoints()), (tag, counts)
    assert len(kps) == len(ko), (tag, len(kps), len(ko))
    assert kps.tobytes() == ko.tobytes(), tag
    assert desc.dtype == np.float32 and np.array_equal(desc, do), tag
    return kps, desc


@pytest.mark.parametrize("tag,make,kw", REGIMES, ids=REGIME_IDS)
def test_kernels_match_reference_and_oracle(ctx, oracle_mod, tag, make, kw):
    frame = make()
    check_gpu(_finder(ctx, (frame.shape[1], frame.shape[0]), kw), oracle_mod, tag, frame, kw)


def test_finder_planned_for_a_larger_frame(ctx, oracle_mod):
    """A finder planned for 640 x 360 detects a 97 x 71 frame and then a 333 x 251 frame: the plan is rebuilt for each size."""
    finder = _finder(ctx, (640, 360), {})
    check_gpu(finder, oracle_mod, "97x71 in 640x360", rendered(97, 71, 10.0), {})
    check_gpu(finder, oracle_mod, "333x251 in 640x360", rendered(333, 251), {})


def test_detect_batch_with_four_octave_layers(ctx, oracle_mod):
    """Three frames in one batch with n_octave_layers = 4: the helper lanes are finders of their own and must take the parent's
    parameters.  Each frame equals its single detect and the reference."""
    import torch
    kw = dict(n_octave_layers=4)
    w, h = 200, 150
    frames = [rendered(w, h, yaw) for yaw in (0.0, 40.0, 80.0)]
    finder = _finder(ctx, (w, h), kw)
    singles = [check_gpu(finder, oracle_mod, "200x150-nl4 frame %d" % i, fr, kw) for i, fr in enumerate(frames)]
    batch = finder.detect_batch([torch.from_numpy(fr).cuda() for fr in frames])
    assert [b.img_idx for b in batch] == [0, 1, 2]
    for (ks, ds), b in zip(singles, batch):
        kb, db = b.download()
        assert len(ks) > 20 and kb.tobytes() == ks.tobytes() and np.array_equal(db, ds)


def test_strided_unaligned_bgr_view(ctx, oracle_mod):
    """A BGR view with an odd row stride and a column offset of one pixel (3 bytes)."""
    import torch
    w, h = 131, 97
    frame = rendered(w, h, 35.0)
    big = torch.zeros((h, w + 6, 3), dtype=torch.uint8, device="cuda")
    view = big[:, 1:1 + w]
    view.copy_(torch.from_numpy(frame).cuda())
    assert view.data_ptr() % 4 != 0 and view.stride(0) % 2 == 1
    check_gpu(_finder(ctx, (w, h), {}), oracle_mod, "strided view", frame, {}, img=view)


@pytest.mark.parametrize("nl", [1, 3])
def test_sigma_at_the_tap_limit_runs_and_beyond_it_is_refused(ctx, oracle_mod, nl):
    """The largest kernel the library holds has 127 taps: a sigma that needs exactly that runs whole (never truncated) and matches the
    reference; the next sigma is refused by mis_sift_create with MIS_E_UNSUPPORTED, and the context serves a valid create after."""
    import image_stitching_amd as isa
    frame = blocks(160, 120)
    kw = dict(n_octave_layers=nl, sigma=sigma_at_cap(nl, False))
    kps, _ = check_gpu(_finder(ctx, (160, 120), kw), oracle_mod, "160x120-blocks-nl%d-sigma-at-cap" % nl, frame, kw)
    assert len(kps) > 10
    with pytest.raises(isa.stitching.MisError) as e:
        _finder(ctx, (160, 120), dict(n_octave_layers=nl, sigma=sigma_at_cap(nl, True)))
    assert e.value.code == E_UNSUPPORTED and "tap" in str(e.value)
    check_gpu(_finder(ctx, (96, 80), {}), oracle_mod, "96x80 after a refused create", rendered(96, 80, 10.0), {})
