"""The numpy reference of the resize and rotate operators (tests/refimpl_imgops.py) anchored on facts that do not depend on its
restatement of INTER_LINEAR_EXACT, then the oracle (oracle/mo_imgops.c, whose coefficient routine and pixel loop are the kernel's)
pinned to it: the sweep of small geometries of test_refimpl_imgops_gpu.py, the by-factor cases and the rotations."""
import numpy as np
import pytest

import refimpl_imgops as rio


# ------------------------------------------------------------------------------------------------ anchors
@pytest.mark.parametrize("c", [1, 3])
def test_factor_one_and_equal_size_are_the_identity(c):
    for h, w in ((1, 1), (5, 7), (33, 65)):
        a = rio.image(h, w, c, "rand", seed=h + w)
        assert np.array_equal(rio.resize_linear_exact(a, fx=1.0, fy=1.0), a)
        assert np.array_equal(rio.resize_linear_exact(a, dsize=(w, h)), a)


@pytest.mark.parametrize("c", [1, 3])
def test_exact_halving_is_the_2x2_mean(c):
    """OpenCV switches INTER_LINEAR_EXACT to INTER_AREA at a scale of exactly 2: (a + b + c + d + 2) >> 2.  The bilinear weights
    there are 128 / 128 both ways, which is the same number."""
    a = rio.image(18, 26, c, "rand", seed=3).astype(np.int64)
    want = (a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2] + 2) >> 2
    assert np.array_equal(rio.resize_linear_exact(a.astype(np.uint8), fx=0.5, fy=0.5), want)
    assert np.array_equal(rio.resize_linear_exact(a.astype(np.uint8), dsize=(13, 9)), want)


def test_constant_images_stay_constant_at_every_geometry():
    """Weights sum to 256 in each pass, so 255 stays 255 (and fits 16 bits after the horizontal pass) wherever it is sampled."""
    for sw, sh, dw, dh in rio.sweep()[::7]:
        for value in (255, 1, 128):
            out = rio.resize_linear_exact(np.full((sh, sw, 3), value, np.uint8), dsize=(dw, dh))
            assert out.shape == (dh, dw, 3) and (out == value).all()


def test_upscaling_by_256_rounds_every_tie_to_even():
    """Source position (i + 0.5) / 256 - 0.5: frac * 256 = k + 0.5 at every interior destination index, so each weight is a tie and
    half to even gives 0, 2, 2, 4, 4, ...; half up would give the odd neighbours."""
    i0, i1, w = rio.axis_table(4, 1024, 256.0)
    inner = slice(128, 1024 - 128)
    frac256 = ((np.arange(1024) + 0.5) / 256.0 - 0.5) % 1.0 * 256.0
    assert np.array_equal(frac256[inner] % 1.0, np.full(768, 0.5))
    assert (w[inner] % 2 == 0).all()
    assert list(w[128:135]) == [0, 2, 2, 4, 4, 6, 6] and w[inner].max() == 256
    half_up = np.floor(frac256[inner] + 0.5)
    assert int((half_up != w[inner]).sum()) == 384
    assert (w[:128] == 0).all() and (i0[:128] == 0).all() and (w[-128:] == 0).all() and (i0[-128:] == 3).all()        # the edge sample
    a = rio.image(3, 4, 1, "rand", seed=5)
    out = rio.resize_linear_exact(a, fx=256.0, fy=256.0)
    assert out.shape == (768, 1024) and np.array_equal(out[:128, :128], np.full((128, 128), a[0, 0]))


def test_by_factor_and_by_size_give_different_tables():
    """133 x 77 at 0.5: cvRound gives 66 x 38; called by factor the scale is 2, called by size 133 / 66 and 77 / 38."""
    assert rio.geometry(133, 77, None, 0.5, 0.5)[:2] == (66, 38)
    tf, ts = rio.axis_table(133, 66, 0.5), rio.axis_table(133, 66, 66 / 133)
    assert not np.array_equal(tf[2], ts[2])
    a = rio.image(77, 133, 1, "rand", seed=7)
    f, s = rio.resize_linear_exact(a, fx=0.5, fy=0.5), rio.resize_linear_exact(a, dsize=(66, 38))
    assert f.shape == s.shape == (38, 66) and (f != s).mean() > 0.5
    # cvRound's ties: 5 -> 2, 7 -> 4, 3 -> 2
    assert [rio.geometry(n, n, None, 0.5, 0.5)[0] for n in (5, 7, 3)] == [2, 4, 2]


def test_rotate_is_rot90():
    a = rio.image(2, 3, 1, "ramp")
    assert rio.rotate(a, 0).tolist() == [[a[1, 0], a[0, 0]], [a[1, 1], a[0, 1]], [a[1, 2], a[0, 2]]]       # clockwise: the left column becomes the top row
    assert rio.rotate(a, 1).tolist() == a[::-1, ::-1].tolist()
    assert np.array_equal(rio.rotate(rio.rotate(a, 0), 2), a) and np.array_equal(rio.rotate(rio.rotate(a, 1), 1), a)


# ------------------------------------------------------------------------------------------------ the oracle against the reference
@pytest.mark.parametrize("c", [1, 3])
def test_oracle_resize_equals_reference_on_the_sweep(oracle_mod, c):
    cases = rio.sweep()
    assert len(cases) == 4032
    for k, (sw, sh, dw, dh) in enumerate(cases):
        a = rio.image(sh, sw, c, ("rand", "ramp", "full")[k % 3], seed=k)
        got, want = oracle_mod.resize_exact(a, dsize=(dw, dh)), rio.resize_linear_exact(a, dsize=(dw, dh))
        assert got.shape == want.shape and np.array_equal(got, want), (sw, sh, dw, dh, c)


@pytest.mark.parametrize("h,w,fx,fy", rio.BY_FACTOR)
def test_oracle_resize_by_factor_equals_reference(oracle_mod, h, w, fx, fy):
    for c in (1, 3):
        a = rio.image(h, w, c, "rand", seed=h * w)
        got, want = oracle_mod.resize_exact(a, fx=fx, fy=fy), rio.resize_linear_exact(a, fx=fx, fy=fy)
        assert got.shape == want.shape and np.array_equal(got, want), c
        dsize = (want.shape[1], want.shape[0])
        assert np.array_equal(oracle_mod.resize_exact(a, dsize=dsize), rio.resize_linear_exact(a, dsize=dsize)), c


@pytest.mark.parametrize("c", [1, 3])
def test_oracle_rotate_equals_reference(oracle_mod, c):
    for h, w in rio.ROTATE_SIZES:
        a = rio.image(h, w, c, "rand", seed=h + 3 * w)
        for code in (0, 1, 2):
            assert np.array_equal(oracle_mod.rotate(a, code), rio.rotate(a, code)), (h, w, code)
