"""Self-checks of tests/refimpl_expos_family.py (the numpy reference of the gain, channels and channels-blocks exposure compensators
and of nr_feeds > 1), the configuration checks of the new names, the 128-bit -> double rounding of the exact sum of norms, and the
DECIDEDNESS condition the multi-feed GPU tests rest on: every intermediate gain of every scene they use is further from a float32
rounding boundary than its tolerance, so (float)g -- and with it every later feed's input -- is the same on both sides."""
import ctypes as C
import functools
from fractions import Fraction
import math
import os
import subprocess

import numpy as np
import pytest

import refimpl_expos as rx
import refimpl_expos_family as fx

HERE = os.path.dirname(os.path.abspath(__file__))
SCENES = fx.scenes()
MULTI_FEEDS = {"gain": 3, "channels": 3, "gain_blocks": 2, "channels_blocks": 2}     # the largest nr_feeds the GPU tests run per type


@functools.lru_cache(maxsize=None)
def scene(name):
    c, i, m = SCENES[name]()
    for a in i + m:
        a.setflags(write=False)
    return c, i, m


@functools.lru_cache(maxsize=None)
def fed(kind, name, nr_feeds=1, bw=64, bh=64):
    return fx.feed(kind, scene(name), nr_feeds, bw, bh)


def stats_error_allowance(fd):
    """gain_blocks keeps the ordered kernel: its running float64 sums differ from fsum by at most count * 2^-53 relative per I
    (count <= the block area), which enters A twice and the gains through cond_2(A)."""
    if fd.kind != "gain_blocks":
        return 0.0
    area = int((fd.grid.blocks[:, 2] * fd.grid.blocks[:, 3]).max())
    cond = max([float(np.linalg.cond(fx.normal_matrix(*s[0]), 2)) for s in fd.stats if len(fx.normal_matrix(*s[0]))], default=0.0)
    return 4 * cond * area * fx.U53


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("kind", ["gain", "channels"])
@pytest.mark.parametrize("name", ["three_way", "byte_masks", "masked_out", "tiny", fx.SEAM_SCALE_4K])
def test_frame_gains_minimise_the_error_function(kind, name):
    fd = fed(kind, name)
    for (count, N, I), g in zip(fd.stats[0], fd.gains[0]):
        e0 = rx.error_function(g, count, N, I)
        for k in np.nonzero(rx.active_blocks(count))[0]:
            for d in (1e-3, -1e-3):
                gk = g.copy()
                gk[k] += d
                assert rx.error_function(gk, count, N, I) > e0, (kind, name, k, d)
        assert np.all(g[~rx.active_blocks(count)] == 1.0)


def test_channels_on_a_grey_image_is_the_single_channel_gain():
    """B = G = R = v: the three channels of ChannelsCompensator agree exactly with each other, and they are GainCompensator on
    the one-channel image: the norm of (v, v, v) is v sqrt(3), so the three-channel statistics divided by sqrt(3) give the
    same gains (E is not scale-free: beta weighs (1 - g)^2 against alpha I^2, so the undivided ones do not)."""
    corners, images, masks = scene("three_way")
    grey = [np.repeat(im[:, :, :1], 3, axis=2) for im in images]
    ch = fx.feed("channels", (corners, grey, masks))
    assert np.array_equal(ch.acc[0], ch.acc[1]) and np.array_equal(ch.acc[0], ch.acc[2])
    g = fx.feed("gain", (corners, grey, masks))
    (count, N, I), (count1, N1, I1) = g.stats[0][0], ch.stats[0][0]
    assert np.array_equal(count, count1) and np.array_equal(N, N1)
    assert np.abs(I / math.sqrt(3) - I1).max() <= 1e-13 * I1.max()
    assert np.abs(rx.gains(count, N, I / math.sqrt(3)) - ch.acc[0]).max() <= 1e-12 and np.abs(ch.acc[0] - 1).max() > 0.02
    assert np.abs(g.acc[0] - ch.acc[0]).max() > 0.01
    # the statistics of a channel from a plain loop over the pano pixels of frames 0 and 1
    count, N, I = ch.stats[0][0]
    cnt, s0, s1 = 0, 0, 0
    (x0, y0), (x1, y1) = corners[0], corners[1]
    for y in range(max(y0, y1), min(y0 + masks[0].shape[0], y1 + masks[1].shape[0])):
        for x in range(max(x0, x1), min(x0 + masks[0].shape[1], x1 + masks[1].shape[1])):
            if masks[0][y - y0, x - x0] == 255 and masks[1][y - y1, x - x1] == 255:
                cnt += 1
                s0 += int(grey[0][y - y0, x - x0, 0])
                s1 += int(grey[1][y - y1, x - x1, 0])
    assert cnt == count[0, 1] == N[0, 1] and I[0, 1] == s0 / cnt and I[1, 0] == s1 / cnt


@pytest.mark.parametrize("params", rx.PARAMS, ids=["%dx%d-f%d" % p for p in rx.PARAMS])
def test_blocks_with_one_feed_is_the_existing_reference(params):
    for name in rx.SCENES:
        _, want = rx.reference_maps(scene(name), *params)
        got = fx.gain_maps(fed("gain_blocks", name, 1, params[0], params[1]), params[2])
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), name
        ch = fx.gain_maps(fed("channels_blocks", name, 1, params[0], params[1]), params[2])
        assert all(c.shape == w.shape + (3,) for c, w in zip(ch, want)), name


def test_feeds_converge_and_never_alter_the_scene():
    """The product of the feeds' gains: a second feed on the corrected images finds gains much closer to 1."""
    for kind in fx.TYPES:
        corners, images, masks = scene("three_way")
        before = [im.copy() for im in images]
        fd = fx.feed(kind, (corners, images, masks), 3)
        assert all(np.array_equal(a, b) for a, b in zip(before, images))
        first, later = max(np.abs(g - 1).max() for g in fd.gains[0]), max(np.abs(g - 1).max() for g in fd.gains[2])
        assert first > 0.05 and later < 0.2 * first, (kind, first, later)


def test_apply_scalar_is_the_float32_product():
    v = np.arange(256, dtype=np.uint8)
    for g in (0.72, 1.33, 1.0, 0.5, 1.9999999):
        want = [min(255, max(0, int(np.rint(np.float32(np.float32(x) * np.float32(g)))))) for x in range(256)]
        assert fx.apply_scalar(v, g).tolist() == want
    assert fx.apply_scalar(np.array([[[1, 2, 3]]], np.uint8), [2.0, 0.5, 100.0]).tolist() == [[[2, 1, 255]]]      # rint(1.0) of 2 * 0.5; saturation


# ------------------------------------------------------------------------------------------------ decidedness
@pytest.mark.parametrize("kind", fx.TYPES)
def test_intermediate_gains_are_decided_in_float32(kind):
    worst = (math.inf, None, 0.0)
    for name in SCENES:
        fd = fed(kind, name, MULTI_FEEDS[kind])
        margin, tol = fx.decidedness(fd)
        tol += stats_error_allowance(fd)
        assert margin > tol, "%s %s: an intermediate gain is %.3g (relative) from a float32 boundary, tolerance %.3g" % (kind, name, margin, tol)
        if margin < worst[0]:
            worst = (margin, name, tol)
        for stats in fd.stats:
            for s in stats:
                A = fx.normal_matrix(*s)
                assert not len(A) or np.linalg.cond(A, 2) < 100, (kind, name)
    print("%s, %d feeds: smallest relative float32 margin %.3g (%s), its tolerance %.3g" % (kind, MULTI_FEEDS[kind], worst[0], worst[1], worst[2]))


def test_float32_margin():
    one = np.float64(np.float32(1.33))
    assert abs(fx.float32_margin([one])[0] - 2.0 ** -24 / one) < 1e-15      # a float32 value in [1, 2): half an ulp (2^-24) from both boundaries
    edge = (np.float64(np.float32(1.33)) + np.float64(np.nextafter(np.float32(1.33), np.float32(2)))) / 2
    assert fx.float32_margin([edge])[0] == 0.0


# ------------------------------------------------------------------------------------------------ configuration
def test_config_accepts_the_family_and_refuses_bad_values():
    from image_stitching_amd.stitching import StitchConfig, check_seam_config
    for name in ("no", "gain", "gain_blocks", "channels_blocks"):
        for feeds in (1, 2, 5):
            check_seam_config(StitchConfig(expos_comp_type=name, expos_comp_nr_feeds=feeds))
    assert StitchConfig().expos_comp_nr_feeds == 1 and StitchConfig().expos_comp_type == "gain_blocks"
    # "channels" stays refused as a configuration name (stitching.EXPOS_COMP_TYPES says why); ChannelsCompensator is built all the same
    for name in ("gain_channels", "channels"):
        with pytest.raises(NotImplementedError):
            check_seam_config(StitchConfig(expos_comp_type=name))
    for bad in (0, -1, 1.5, "2", True, None):
        with pytest.raises(ValueError):
            check_seam_config(StitchConfig(expos_comp_type="gain", expos_comp_nr_feeds=bad))


def test_job_checks_the_feeds_at_construction():
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    with pytest.raises(ValueError):
        StitchJob(None, (64, 64), [], engine=object(), config=StitchConfig.hot_path(expos_comp_type="channels_blocks", expos_comp_nr_feeds=0))


# ------------------------------------------------------------------------------------------------ 128 bits -> double
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("exact") / "libexactsum.so")
    r = subprocess.run(["c++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", os.path.join(HERE, "harness", "exact_sum_harness.cpp"), "-o", so],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    lib.harness_limbs_to_double.restype = C.c_double
    lib.harness_limbs_to_double.argtypes = [C.c_uint64, C.c_uint64]
    lib.harness_add_norm.argtypes = [C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return lib


def _want(lo, hi):
    return float(Fraction((hi << 32) + lo, 2 ** 52))


def test_limbs_round_once_to_nearest_even(harness):
    """Limb patterns around rounding ties: T = m * 2^k + r with 53-bit m (even and odd) and r just below, at and just above half of
    2^k, for k up to the 43 bits that 2^32 pixels can add above a double's 53.  Fraction.__float__ rounds correctly (ties to even)."""
    rng = np.random.default_rng(1)
    cases = [0, 1, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, 2 ** 96 - 1]
    for k in (1, 2, 11, 31, 32, 33, 43):
        for m in (2 ** 52, 2 ** 52 + 1, 2 ** 53 - 1, 2 ** 53 - 2, int(rng.integers(2 ** 52, 2 ** 53)), int(rng.integers(2 ** 52, 2 ** 53)) | 1):
            half = 2 ** (k - 1)
            for r in sorted(r for r in {0, 1, half - 1, half, half + 1, 2 ** k - 1} if 0 <= r < 2 ** k):
                cases.append(m * 2 ** k + r)
    assert max(cases) < 2 ** 96
    for t in cases:
        # the same T from different limb splits: the high counter may hold any carry of the low one
        for hi in {t >> 32, max(0, (t >> 32) - 1), max(0, (t >> 32) - 0xffffffff)}:
            lo = t - (hi << 32)
            if lo >= 2 ** 64:
                continue
            got = harness.harness_limbs_to_double(lo, hi)
            assert got == _want(lo, hi), (t, lo, hi, got)


def test_limb_sums_equal_fsum(harness):
    """The kernel's split and the host's rounding over random sums of three squares, in two orders, against math.fsum."""
    rng = np.random.default_rng(2)
    for n in (1, 2, 1000, 20000):
        ss = rng.integers(0, 3 * 255 * 255 + 1, n)
        ss[0] = 3 * 255 * 255
        want = math.fsum(math.sqrt(int(s)) for s in ss)
        for order in (ss, ss[::-1]):
            lo, hi = C.c_uint64(0), C.c_uint64(0)
            for s in order:
                harness.harness_add_norm(int(s), C.byref(lo), C.byref(hi))
            assert harness.harness_limbs_to_double(lo.value, hi.value) == want, n
