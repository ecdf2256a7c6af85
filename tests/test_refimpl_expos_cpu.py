"""The oracle of the step between warp and blend (oracle/mo_expos.c, mo_imgops.c) against the numpy reference of
tests/refimpl_expos.py, over the scenes and block geometries shared with test_refimpl_expos_gpu.py: gain maps within the derived
float32 bound, Voronoi masks and seam masks exactly, every applied byte inside its candidate range.  The self-checks pin the
reference's building blocks to the written-out error function and to brute force, so that it is not merely a third copy.

NOT PINNED (refimpl_expos.py): whether a pair of blocks whose rectangles intersect but whose masks do not un-skips its blocks.
test_unskip_readings_on_the_scenes prints the largest difference between the two readings over the scenes: 3.6e-5 in the gain
maps of `three_way` at 32 x 48 blocks without filtering (six maps beyond the gain-map tolerance, all of `three_way`), so the reading
IS observable and stays NOT PINNED; the oracle and the product both take the first reading, which is what these tests check."""
import functools

import numpy as np
import pytest

import oracle
import refimpl_expos as rx

PARAM_IDS = ["%dx%d-f%d" % p for p in rx.PARAMS]


@functools.lru_cache(maxsize=None)
def scene(name):
    c, i, m = rx.SCENES[name]()
    for a in i + m:
        a.setflags(write=False)
    return c, i, m


@functools.lru_cache(maxsize=None)
def ref_maps(name, params, strict=False):
    return rx.reference_maps(scene(name), *params, strict=strict)


@functools.lru_cache(maxsize=None)
def oracle_comp(name, params):
    comp = oracle.Compensator(*params)
    comp.feed(*scene(name))
    return comp


def apply_images(map_shape):
    """The image sizes (w, h) an apply test runs at: larger than the map, the map's own size, smaller, one row, one column."""
    rng = np.random.default_rng(11)
    return [rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for w, h in [(517, 389), (map_shape[1], map_shape[0]), (2, 2), (300, 1), (1, 200)]]


def check_candidates(got, gmap, img, what):
    """-> the share of undecided bytes; asserts got inside the candidates and the share at most 1 %."""
    lo, hi = rx.apply_candidates(gmap, img)
    bad = (got < lo) | (got > hi)
    assert not bad.any(), "%s: %d bytes outside their candidates, first at %s" % (what, bad.sum(), np.argwhere(bad)[0])
    share = float((lo != hi).mean())
    assert share <= 0.01, "%s: %.3f %% of the bytes undecided: the check is too weak" % (what, 100 * share)
    return share


def one_sample_apply(gmap, img):
    """apply() of a 1 x 1 map, exactly: every tap of the resize is the one sample and every fraction is clamped to 0, so the gain is
    the sample itself and a byte is cvRound((float)v * g) -- one correctly rounded float32 product, no band."""
    assert gmap.shape == (1, 1)
    return np.clip(np.rint(img.astype(np.float32) * np.float32(gmap[0, 0])), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ oracle vs reference
@pytest.mark.parametrize("params", rx.PARAMS, ids=PARAM_IDS)
def test_oracle_gain_maps_within_tolerance(params):
    worst = 0.0
    for name in rx.SCENES:
        grid, maps = ref_maps(name, params)
        comp = oracle_comp(name, params)
        for k, ref in enumerate(maps):
            got = comp.gain_map(k)
            assert got.dtype == np.float32 and got.shape == ref.shape == grid.shapes[k], (name, k)
            err = float(np.abs(got.astype(np.float64) - ref).max())
            worst = max(worst, err / (rx.U24 * np.abs(ref).max()))
            assert err <= rx.gain_map_tol(ref, params[2]), (name, k, err, rx.gain_map_tol(ref, params[2]))
            if name in rx.ALL_ONES:
                assert np.all(got == np.float32(1)), name
    print("gain maps %s: max |oracle - ref| = %.2f x 2^-24 max|map| (bound %d)" % (params, worst, 1 + 4 * params[2]))


@pytest.mark.parametrize("name", list(rx.SCENES))
def test_oracle_voronoi_equals_reference(name):
    corners, _, masks = scene(name)
    want = rx.voronoi(corners, masks)
    got = oracle.voronoi_seams(corners, masks)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (name, k, int((g != w).sum()))


@pytest.mark.parametrize("params", rx.PARAMS, ids=PARAM_IDS)
def test_oracle_apply_inside_candidates(params):
    """Every scene's maps applied to the fed image and to a random image of another size."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for name in rx.SCENES:
        corners, images, _ = scene(name)
        comp = oracle_comp(name, params)
        for k, img in enumerate(images):
            gmap = comp.gain_map(k)
            other = rng.integers(0, 256, (2 * img.shape[0] - 3, 2 * img.shape[1] - 5, 3)).astype(np.uint8)
            for im in (img, other):
                worst = max(worst, check_candidates(comp.apply(k, im), gmap, im, "%s[%d] %s" % (name, k, im.shape)))
    print("apply %s: at most %.3f %% of the bytes undecided" % (params, 100 * worst))


@pytest.mark.parametrize("name", ["three_way", "tiny"])
def test_oracle_apply_sizes_inside_candidates(name):
    comp = oracle_comp(name, (64, 64, 2))
    gmap = comp.gain_map(0)
    if name == "tiny":
        assert gmap.shape == (1, 1)
    for im in apply_images(gmap.shape):
        share = check_candidates(comp.apply(0, im), gmap, im, "%s %s" % (name, im.shape))
        if name == "tiny":
            assert np.array_equal(comp.apply(0, im), one_sample_apply(gmap, im)), im.shape
        print("apply %s map %s image %s: %.3f %% undecided" % (name, gmap.shape, im.shape[:2], 100 * share))


@pytest.mark.parametrize("geometry", rx.SEAM_GEOMETRIES, ids=lambda g: "%dx%d-to-%dx%d" % (g[0] + g[1]))
def test_oracle_seam_mask_equals_reference(geometry):
    for byte_values in (False, True):
        seam, mask = rx.seam_case(geometry, byte_values)
        want = rx.seam_mask_apply(seam, mask)
        assert np.array_equal(oracle.seam_mask_apply(seam, mask), want), byte_values
        if geometry[0] != (1, 1):
            assert want.any() and (want != mask).any()


# ------------------------------------------------------------------------------------------------ self-checks of the reference
def test_block_grid_tiles_every_image():
    for W, H, bw, bh in [(40, 30, 64, 64), (200, 150, 32, 48), (131, 97, 17, 64), (300, 200, 200, 200), (65, 129, 64, 64)]:
        g = rx.block_grid([(-7, 3)], [(W, H)], bw, bh)
        ny, nx = g.shapes[0]
        assert (nx, ny) == (-(-W // bw), -(-H // bh)) and len(g.blocks) == nx * ny
        cover = np.zeros((H, W), np.int32)
        for x, y, w, h, k in g.blocks:
            assert w > 0 and h > 0 and w <= -(-W // nx) and h <= -(-H // ny) and k == 0
            cover[y - 3:y - 3 + h, x + 7:x + 7 + w] += 1
        assert np.all(cover == 1)
        assert np.array_equal(g.blocks[:, 0], np.sort(g.blocks[:, 0].reshape(ny, nx), axis=1).ravel())      # row-major


def test_overlap_stats_against_a_pixel_loop():
    """byte_masks, two blocks picked by hand: the count and the means from a plain loop over the pano pixels."""
    corners, images, masks = scene("byte_masks")
    grid = rx.block_grid(corners, [(m.shape[1], m.shape[0]) for m in masks], 64, 64)
    count, N, I = rx.overlap_stats(corners, images, masks, grid)
    pairs = [(i, j) for i in range(len(count)) for j in range(i + 1, len(count)) if count[i, j] > 0 and grid.blocks[i, 4] != grid.blocks[j, 4]]
    assert pairs
    for i, j in pairs[:3]:
        (xa, ya, wa, ha, a), (xb, yb, wb, hb, b) = grid.blocks[i], grid.blocks[j]
        cnt, s1, s2 = 0, 0.0, 0.0
        for y in range(max(ya, yb), min(ya + ha, yb + hb)):
            for x in range(max(xa, xb), min(xa + wa, xb + wb)):
                pa, pb = (y - corners[a][1], x - corners[a][0]), (y - corners[b][1], x - corners[b][0])
                if masks[a][pa] == 255 and masks[b][pb] == 255:
                    cnt += 1
                    s1 += float(np.sqrt(float((images[a][pa].astype(np.int64) ** 2).sum())))
                    s2 += float(np.sqrt(float((images[b][pb].astype(np.int64) ** 2).sum())))
        assert cnt == count[i, j] == N[i, j]
        assert abs(s1 / cnt - I[i, j]) <= 1e-12 * I[i, j] and abs(s2 / cnt - I[j, i]) <= 1e-12 * I[j, i]
        assert ((masks[a] != 0) & (masks[a] != 255)).any()      # bytes other than 0 and 255 are there and were not counted


@pytest.mark.parametrize("name", ["three_way", "byte_masks", "masked_out", "tiny"])
def test_gains_minimise_the_error_function(name):
    corners, images, masks = scene(name)
    grid = rx.block_grid(corners, [(m.shape[1], m.shape[0]) for m in masks], 64, 64)
    count, N, I = rx.overlap_stats(corners, images, masks, grid)
    for strict in (False, True):
        g = rx.gains(count, N, I, strict)
        e0 = rx.error_function(g, count, N, I, strict)
        for k in np.nonzero(rx.active_blocks(count, strict))[0]:
            for d in (1e-3, -1e-3):
                gk = g.copy()
                gk[k] += d
                assert rx.error_function(gk, count, N, I, strict) > e0, (name, strict, k, d)
        assert np.all(g[~rx.active_blocks(count, strict)] == 1.0)


def test_l1_distance_is_the_brute_force_minimum():
    rng = np.random.default_rng(3)
    f = rng.random((17, 23)) < 0.04
    assert f.any()
    ys, xs = np.nonzero(f)
    yy, xx = np.mgrid[0:17, 0:23]
    want = (np.abs(yy[..., None] - ys) + np.abs(xx[..., None] - xs)).min(axis=-1)
    assert np.array_equal(rx.l1_distance(f), want)
    assert np.all(rx.l1_distance(np.zeros((17, 23), bool)) == rx.EMPTY_DIST) and rx.EMPTY_DIST > 17 + 23


def test_scenes_move_what_they_are_meant_to_move():
    for name in rx.SCENES:
        corners, images, masks = scene(name)
        _, maps = ref_maps(name, (64, 64, 2))
        moved = max(float(np.abs(m - 1).max()) for m in maps)
        changed = sum(int((a != b).sum()) for a, b in zip(rx.voronoi(corners, masks), masks))
        if name in rx.ALL_ONES:
            assert moved == 0.0, name
        else:
            assert moved > 0.02, (name, moved)
        assert (changed == 0) == (name in rx.NO_SEAM), (name, changed)
    assert ref_maps("tiny", (64, 64, 2))[0].shapes == [(1, 1), (1, 1)]
    # masked_out: rectangles that intersect with no common valid pixel -> count 0, N = 1, I = 0
    corners, images, masks = scene("masked_out")
    grid = rx.block_grid(corners, [(m.shape[1], m.shape[0]) for m in masks], 64, 64)
    count, N, I = rx.overlap_stats(corners, images, masks, grid)
    zero = (count == 0)
    assert zero.any() and np.all(N[zero] == 1) and np.all(I[zero] == 0)
    # contained / identical: an empty unique mask
    for name in ("contained", "identical"):
        corners, _, masks = scene(name)
        out = rx.voronoi(corners, masks)
        assert sum(not o.any() for o in out) == 1, name          # one frame loses its whole (shared) mask
    assert not rx.voronoi(*scene("identical")[::2])[0].any()     # the tie d1 == d2: frame i loses
    # strip4 at 64 x 64: the number of block pairs is no multiple of the four pairs a thread block of the kernel takes
    corners, images, masks = scene("strip4")
    grid = rx.block_grid(corners, [(m.shape[1], m.shape[0]) for m in masks], 64, 64)
    assert int(np.triu(rx.overlap_stats(corners, images, masks, grid)[0] >= 0).sum()) % 4 != 0
    # thin overlaps: one pixel wide / high
    for name, axis in (("thin_col", 0), ("thin_row", 1)):
        corners, _, masks = scene(name)
        lo = max(corners[0][axis], corners[1][axis])
        hi = min(corners[0][axis] + masks[0].shape[1 - axis], corners[1][axis] + masks[1].shape[1 - axis])
        assert hi - lo == 1, name


def test_unskip_readings_on_the_scenes():
    """NOT PINNED reading (module docstring): prints the largest gain-map difference between 'any rectangle overlap un-skips'
    and 'only a non-zero count un-skips', and says whether it exceeds the gain-map tolerance anywhere."""
    worst, where, differs = 0.0, None, []
    for params in rx.PARAMS:
        for name in rx.SCENES:
            loose, strict = ref_maps(name, params)[1], ref_maps(name, params, True)[1]
            for a, b in zip(loose, strict):
                d = float(np.abs(a - b).max())
                if d > worst:
                    worst, where = d, (name, params)
                if d > rx.gain_map_tol(a, params[2]):
                    differs.append((name, params, d))
    print("un-skip readings: largest gain-map difference %.3g at %s; beyond the tolerance in %d cases %s" % (worst, where, len(differs), differs[:4]))
    # which blocks the readings treat differently at all
    corners, images, masks = scene("masked_out")
    grid = rx.block_grid(corners, [(m.shape[1], m.shape[0]) for m in masks], 64, 64)
    count = rx.overlap_stats(corners, images, masks, grid)[0]
    assert (rx.active_blocks(count) != rx.active_blocks(count, True)).any(), "masked_out must reach the case the readings differ on"
