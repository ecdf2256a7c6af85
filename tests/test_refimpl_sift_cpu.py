"""The SIFT oracle (oracle/mo_sift.c) against the numpy reference of tests/refimpl_sift.py, stage by stage, over the regimes that
test_refimpl_sift_gpu.py runs on the kernels.  test_sift_gpu.py compares the kernels with the oracle bit for bit; this pins the
oracle itself to OpenCV's documented semantics, independently of how it was written, at every parameter path (n_octave_layers,
sigma, contrast and edge thresholds) and not only at SIFT::create()'s defaults.  The reference's own conditions (tap counts, the
folded reflection, the caps on undecided branches, the rejection reasons reached) are checked here as well, without a GPU."""
import numpy as np
import pytest

import refimpl_sift as rs

MAX_TAPS = 127            # the largest Gaussian kernel the library and the oracle hold; parameters that need more are refused


# ------------------------------------------------------------------------------------------------ frames (shared with the GPU file)
def rendered(w, h, yaw=40.0, fov=60.0, pitch=3.0):
    import synth
    return synth.render_frame(synth.make_camera(w, h, fov, yaw, pitch))


def uniform_noise(w, h, seed):
    """Independent uniform byte noise in every channel.  After the doubling and the blur to sigma 1.6 it leaves about one extremum per
    1000 pixels of octave 0, with contrasts low enough for every branch of the refinement.  Seed 67 is the first of 0 .. 299 whose 92
    candidates reach the six rejection reasons of rs.REJECT_REASONS."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def blocks(w, h, seed=4, lo=70, hi=180):
    """8 x 8 blocks of two gray levels, drawn at random: runs of equal blocks give exactly flat and exactly repeated DoG values."""
    b = np.random.default_rng(seed).integers(0, 2, ((h + 7) // 8, (w + 7) // 8))
    g = np.where(np.kron(b, np.ones((8, 8), int))[:h, :w] > 0, hi, lo).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


def squares(w=160, h=128, seed=0, pitch=20):
    """Rectangles of 4 .. 6 pixels a side on a dark ground.  The doubled image is mirror symmetric about the half-pixel centre of each,
    so octave 0 holds pairs of adjacent DoG pixels that are equal to the last bit: both are extrema under `>=`, neither under `>`.
    The fit puts such a pair's offset at a half, so none of them survives the refinement (they end at the step limit or leave the
    layers): the scan's `>=` shows in the candidate count, which both tested sides report, and not in the keypoints."""
    rng = np.random.default_rng(seed)
    g = np.full((h, w), 30, np.uint8)
    for y in range(8, h - 12, pitch):
        for x in range(8, w - 12, pitch):
            n, m = int(rng.integers(4, 7)), int(rng.integers(4, 7))
            g[y:y + n, x:x + m] = rng.integers(90, 256)
    return np.repeat(g[:, :, None], 3, axis=2)


def flat(w, h, v=90):
    return np.full((h, w, 3), v, np.uint8)


def stripes_and_blobs(w=256, h=48):
    """Default parameters, more than 1024 candidates in one 256 x 32 tile of octave 0: vertical stripes of period 5 (10 in the doubled
    image) are constant along y, so every pixel of a ridge or valley line of the DoG ties with its vertical neighbours and is an
    extremum (`>=`): 2 columns in 10 on one layer, 256 * 32 / 5 = 1638 in a full tile.  Columns 100 .. 127 of every tile row hold
    noise blobs instead, which give that tile ordinary keypoints next to the ties.  Nearly all the ties end as `det <= 0`; that every
    one of them was appended, past the tile list too, shows in the tested side's candidate count (6122, equal to the reference's)."""
    x = np.arange(w)
    g = np.tile(np.where(x % 5 < 2, 220, 40).astype(np.uint8), (h, 1))
    rng = np.random.default_rng(11)
    for x0 in range(100, w, 128):
        blob = np.kron(rng.integers(0, 256, ((h + 3) // 4, 7)), np.ones((4, 4), int))[:h, :28]
        g[:, x0:x0 + 28] = blob[:, :min(28, w - x0)]
    return np.repeat(g[:, :, None], 3, axis=2)


# (id, frame builder, SIFT parameters) -- the regimes of both files
REGIMES = [
    ("333x251-rendered-defaults", lambda: rendered(333, 251), {}),
    ("129x67-rendered-defaults", lambda: rendered(129, 67, 204.0, 16.0, -15.0), {}),
    ("255x40-rendered-defaults", lambda: rendered(255, 40, 199.0, 32.0, -15.0), {}),
    ("1300x72-nl2", lambda: rendered(1300, 72, 10.0), dict(n_octave_layers=2)),
    ("160x120-nl1", lambda: rendered(160, 120, 10.0), dict(n_octave_layers=1)),
    ("160x120-blocks-nl1", lambda: blocks(160, 120), dict(n_octave_layers=1)),
    ("160x120-nl2", lambda: rendered(160, 120, 10.0), dict(n_octave_layers=2)),
    ("160x120-nl4", lambda: rendered(160, 120, 10.0), dict(n_octave_layers=4)),
    ("160x120-nl5", lambda: rendered(160, 120, 10.0), dict(n_octave_layers=5)),
    ("160x120-nl8", lambda: rendered(160, 120, 10.0), dict(n_octave_layers=8)),
    ("160x120-sigma1.2", lambda: rendered(160, 120, 10.0), dict(sigma=1.2)),
    ("160x120-sigma2.4", lambda: rendered(160, 120, 10.0), dict(sigma=2.4)),
    ("160x120-contrast0.01", lambda: rendered(160, 120, 10.0), dict(contrast_threshold=0.01)),
    ("160x120-contrast0.09", lambda: rendered(160, 120, 10.0), dict(contrast_threshold=0.09)),
    ("160x120-edge5", lambda: rendered(160, 120, 10.0), dict(edge_threshold=5.0)),
    ("160x120-edge20", lambda: rendered(160, 120, 10.0), dict(edge_threshold=20.0)),
    ("16x16-rendered", lambda: rendered(16, 16), {}),
    ("17x23-rendered", lambda: rendered(17, 23), {}),
    ("16x300-rendered", lambda: rendered(16, 300), {}),
    ("200x150-noise-contrast0.01", lambda: uniform_noise(200, 150, 67), dict(contrast_threshold=0.01)),
    ("160x128-blocks", lambda: blocks(160, 128), {}),
    ("160x128-squares", squares, {}),
    ("64x48-flat", lambda: flat(64, 48), {}),
    ("256x48-stripes-and-blobs", stripes_and_blobs, {}),
]
REGIME_IDS = [r[0] for r in REGIMES]
# Keypoints (decided, on the reference) a rendered-frame regime must yield: more than 200 at 333 x 251.  The two small frames do not
# reach 200 with any view tried: a sweep of the renderer's cameras over fov 8 .. 60, yaw 0 .. 355 and pitch -45 .. 45 in steps of 5
# degrees (15 048 views a size), then in steps of 1 degree around the four richest (2 268 more), ends at 134 keypoints for 129 x 67
# (fov 16, yaw 204, pitch -15) and 147 for 255 x 40 (fov 32, yaw 199, pitch -15: 145 decided).  The regimes use those two views and are
# held just under what they reach.
MIN_KEYPOINTS = {"333x251-rendered-defaults": 200, "129x67-rendered-defaults": 130, "255x40-rendered-defaults": 140}
NOISE = "200x150-noise-contrast0.01"


def sigma_at_cap(nl, over):
    """The largest sigma (in steps of 1/64) whose largest kernel still has MAX_TAPS taps, or the next step when `over`."""
    s = 0.75
    while rs.max_ksize(rs.params(n_octave_layers=nl, sigma=s + 1.0 / 64)) <= MAX_TAPS:
        s += 1.0 / 64
    return s + 1.0 / 64 if over else s


def report(tag, rep):
    print("%-30s candidates %5d refined %5d kept %5d keypoints %5d (decided %d, forgiven %d) rejected %s undecided %s orientation %s byte %d tile max %d | ratios %s" % (
        tag, rep["candidates"], rep["refined"], rep["kept"], rep["output"], rep["keypoints"], rep["forgiven"], rep["rejected"], rep["undecided"], rep["undecided_orient"],
        rep["byte_undecided"], rep["per_tile_max"], {k: float("%.3g" % v) for k, v in rep["ratio"].items()}))


def check(tag, frame, kw, pyr, kps, desc, counts):
    """One side (oracle or kernels) against the reference: no error, the caps on undecided branches, the regime's own conditions.
    counts: that side's own dict(candidates, refined) of the run."""
    c = rs.compare_all(frame, rs.params(**kw), pyr, kps, desc, counts)
    rep = c["report"]
    report(tag, rep)
    assert not c["errors"], (tag, c["errors"][:8])
    und, und_o = sum(rep["undecided"].values()), sum(rep["undecided_orient"].values())
    assert und <= max(2, rep["candidates"] // 100), (tag, "undecided refinements", rep["undecided"], rep["candidates"])
    assert und_o <= rep["kept"] // 50, (tag, "undecided orientations", rep["undecided_orient"], rep["kept"])
    if tag in MIN_KEYPOINTS:
        assert rep["keypoints"] > MIN_KEYPOINTS[tag], (tag, rep["keypoints"])
    if tag == NOISE:
        assert set(rs.REJECT_REASONS) <= set(rep["rejected"]), (tag, rep["rejected"])
    return c


def oracle_pyramid(o, nl):
    n = o.num_octaves()
    return dict(gauss=[np.stack([o.gauss(k, i) for i in range(nl + 3)]) for k in range(n)],
                dog=[np.stack([o.dog(k, i) for i in range(nl + 2)]) for k in range(n)])


def check_oracle(oracle_mod, tag, frame, kw):
    h, w = frame.shape[:2]
    o = oracle_mod.Sift(w, h, kw)
    kps, desc = o.run(frame)
    c = check(tag, frame, kw, oracle_pyramid(o, rs.params(**kw)["n_octave_layers"]), kps, desc, dict(candidates=o.num_candidates(), refined=o.num_refined()))
    # before duplicate removal every keypoint is one orientation peak of one surviving candidate; two candidates that walk to the
    # same final position give the same keypoints twice
    c["raw"] = o.num_raw_keypoints()
    assert c["raw"] >= len(kps)
    print("%-30s raw keypoints %d, after duplicate removal %d" % (tag, c["raw"], len(kps)))
    return c


# ------------------------------------------------------------------------------------------------ the reference's own conditions
def test_tap_counts_of_the_parameter_paths():
    """ksize = cvRound(8 s + 1) | 1 without a cap: the defaults' five counts (the fused kernel's instances), the generic counts of
    n_octave_layers 2, 4 and 8, and the 91 taps of n_octave_layers = 1 that a 63-tap clamp used to truncate."""
    counts = lambda **kw: sorted({rs.gaussian_ksize(s) for s in rs.incremental_sigmas(rs.params(**kw))[1:]} | {rs.gaussian_ksize(rs.base_sigma(rs.params(**kw)))})
    assert counts() == [11, 13, 17, 21, 27]
    assert set(counts(n_octave_layers=2)) - {11, 13, 17, 21, 27} == {15, 19, 37}
    assert set(counts(n_octave_layers=4)) - {11, 13, 17, 21, 27} == {9, 15}
    assert set(counts(n_octave_layers=8)) - {11, 13, 17, 21, 27} == {7, 9}
    assert rs.max_ksize(rs.params(n_octave_layers=1)) == 91
    assert rs.max_ksize(rs.params(sigma=4.0)) <= 63 < rs.max_ksize(rs.params(sigma=4.2))
    for nl in (1, 3):
        assert rs.max_ksize(rs.params(n_octave_layers=nl, sigma=sigma_at_cap(nl, False))) == MAX_TAPS
        assert rs.max_ksize(rs.params(n_octave_layers=nl, sigma=sigma_at_cap(nl, True))) == MAX_TAPS + 2
    assert [rs.num_octaves(w, h) for w, h in ((16, 16), (17, 23), (333, 251), (1300, 72))] == [4, 4, 8, 6]


def test_reflection_folds_as_often_as_needed():
    """The closed form (period 2 (len - 1)) against numpy's own reflect padding, for lengths far below the reach."""
    for n in (1, 2, 3, 4, 8, 33):
        a = np.arange(n)
        idx = rs.reflect101(np.arange(-45, n + 45), n)
        assert np.array_equal(a[idx], np.pad(a, 45, mode="reflect") if n > 1 else np.zeros(n + 90, int))


def test_upsample_is_the_stated_coordinate_map():
    g = np.random.default_rng(0).integers(0, 256, (5, 7), dtype=np.uint8)
    up = rs.upsample2x(g)
    for y in range(10):
        for x in range(14):
            fy, fx = (y + 0.5) / 2 - 0.5, (x + 0.5) / 2 - 0.5
            y0, x0 = int(np.floor(fy)), int(np.floor(fx))
            wy, wx = fy - y0, fx - x0
            cl = lambda v, n: min(max(v, 0), n - 1)
            v = sum(float(g[cl(y0 + dy, 5), cl(x0 + dx, 7)]) * (wy if dy else 1 - wy) * (wx if dx else 1 - wx) for dy in (0, 1) for dx in (0, 1))
            assert up[y, x] == v


def test_blur_of_a_constant_and_of_an_impulse():
    c = np.full((9, 40), 77.0, np.float32)
    v, e = rs.blur(c, 11.09)                                 # 91 taps on 9 rows: ten folds
    assert np.all(np.abs(v - 77.0) <= e) and e.max() < 1e-3
    imp = np.zeros((41, 41), np.float32)
    imp[20, 20] = 1.0
    v, _ = rs.blur(imp, 1.6)
    t = rs.gaussian_taps(1.6).astype(np.float64)
    assert len(t) == 15 and np.allclose(v[13:28, 13:28], np.outer(t, t), rtol=0, atol=1e-17)


def test_order_and_duplicate_checks_bite():
    k = np.zeros(3, rs.KP_DTYPE)
    k["x"], k["size"] = [1, 1, 2], [3, 2, 1]
    assert rs.order_errors(k) == []
    k["size"] = [2, 3, 1]
    assert rs.order_errors(k) == ["not in KeyPoint_LessThan order"]
    k["size"] = [3, 3, 1]
    k["response"] = [2, 1, 0]
    assert rs.order_errors(k) == ["1 duplicated keypoints"]


def test_more_than_1024_candidates_in_one_tile():
    """The input of the regime `256x48-stripes-and-blobs` fills the per-tile candidate list (1024 entries of a 256 x 32 tile of
    octave 0) of sift_extrema_kernel<3>, so the kernel's direct appends run; counted on the reference from the reference's own
    float64 pyramid rounded to float32 (no tested side involved)."""
    frame = stripes_and_blobs()
    p = rs.params()
    base = rs.upsample2x(rs.bgr2gray(frame))
    g = [rs.blur(base, rs.base_sigma(p))[0].astype(np.float32)]
    for s in rs.incremental_sigmas(p)[1:]:
        g.append(rs.blur(g[-1], s)[0].astype(np.float32))
    dog = np.stack([g[i + 1] - g[i] for i in range(5)])
    cand = rs.candidates(dog, p)
    tiles = np.bincount(((cand[:, 1] - 5) // 32) * 16 + (cand[:, 2] - 5) // 256)
    assert tiles.max() > 1024, tiles


# ------------------------------------------------------------------------------------------------ the oracle against the reference
@pytest.mark.parametrize("tag,make,kw", REGIMES, ids=REGIME_IDS)
def test_oracle_matches_reference(oracle_mod, tag, make, kw):
    c = check_oracle(oracle_mod, tag, make(), kw)
    if tag == "64x48-flat":
        assert c["report"]["candidates"] == 0 and c["report"]["output"] == 0
    if tag == "160x120-blocks-nl1":
        assert c["report"]["keypoints"] > 200                # the rendered frame of `160x120-nl1` keeps one keypoint under the 91-tap blur
    if tag == "160x128-blocks":
        assert c["raw"] > c["report"]["output"]              # two candidates walked to one final position: a duplicate removed


def test_taps_bit_for_bit(oracle_mod):
    for s in (1.2489996, 1.6, 2.0158737, 3.0, 11.0851, 15.7):
        assert np.array_equal(oracle_mod.gaussian_taps_f32(s).view(np.uint32), rs.gaussian_taps(s).view(np.uint32)), s
    with pytest.raises(ValueError):
        oracle_mod.gaussian_taps_f32(16.0)                   # 129 taps


@pytest.mark.parametrize("nl", [1, 3])
def test_sigma_at_the_tap_limit_is_accepted_and_beyond_it_refused(oracle_mod, nl):
    """Blocks keep keypoints under a 127-tap blur (the rendered frame keeps none), so every stage runs at these parameters."""
    c = check_oracle(oracle_mod, "160x120-blocks-nl%d-sigma-at-cap" % nl, blocks(160, 120), dict(n_octave_layers=nl, sigma=sigma_at_cap(nl, False)))
    assert c["report"]["keypoints"] > 10
    with pytest.raises(ValueError):
        oracle_mod.Sift(160, 120, dict(n_octave_layers=nl, sigma=sigma_at_cap(nl, True)))
