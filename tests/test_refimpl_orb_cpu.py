"""The ORB oracle (oracle/mo_orb.c) against the numpy reference of tests/refimpl_orb.py, stage by stage, over the regimes of
test_refimpl_orb_gpu.py that fit on the CPU.  The GPU tests compare the kernels with the oracle bit for bit; this pins the oracle
itself to OpenCV's documented semantics, independently of how it was written."""
import numpy as np
import pytest

import refimpl_orb as ro

MAX_NFEATURES = 8843      # the largest nfeatures the library accepts at scale 1.2 x 8 levels: level 0 gets 1920 keypoints


# ------------------------------------------------------------------------------------------------ frames (shared with the GPU file)
def synth_frame(w, h, yaw=20.0):
    import synth
    return synth.render_frame(synth.make_camera(w, h, 60.0, yaw, 0.3, -0.2))


def flat(w, h, v):
    return np.full((h, w, 3), v, np.uint8)


def checker(w, h):
    """1-px checkerboard of 0 / 255."""
    yy, xx = np.mgrid[0:h, 0:w]
    return np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def binary_noise(w, h, seed=1):
    """Neighbours 0 or 255: FAST differences of +-255."""
    g = (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


def uniform_noise(w, h, seed=2):
    """Independent colour noise: the densest FAST response there is."""
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def dots(w, h, pts, vals):
    """Single grey dots on black.  A dot of value v is a FAST corner of score v - 1 and nothing around it is one; dots 10 pixels
    apart have identical 9 x 9 Harris windows, so equal dots tie exactly in both scores."""
    img = np.zeros((h, w, 3), np.uint8)
    for (x, y), v in zip(pts, vals):
        img[y, x] = v
    return img


def tie_motif(n_b, seed=3):
    """200 x 200, nlevels 1, nfeatures 100: 60 dots of 255, n_b dots of 200 and 50 of 120 on a 10-pixel grid (shuffled).  The
    2N = 200 cut on the FAST score falls inside the 200-dots (score 199: all n_b kept, the 120-dots dropped); the N = 100 cut on
    the Harris response falls inside them again, so 60 + n_b keypoints are kept for a budget of 100."""
    grid = [(10 + 10 * i, 10 + 10 * j) for j in range(19) for i in range(19)]
    order = np.random.default_rng(seed).permutation(len(grid))
    vals = [255] * 60 + [200] * n_b + [120] * 50
    pts = [grid[k] for k in order[:len(vals)]]
    return dots(200, 200, pts, vals), dict(nfeatures=100, nlevels=1)


TIE_INSIDE_SLACK = 150     # 210 kept for a budget of 100: inside the library's 128 slack for ties
TIE_BEYOND_SLACK = 200     # 260 kept: beyond it


def edge_motif(e, w=128, h=112):
    """Dots on both sides of the edge_threshold boundary: x = e - 1, e and w - e - 1, w - e (y likewise), clamped to FAST's
    3 <= x < w - 3."""
    xs = sorted({min(max(3, v), w - 4) for v in (e - 1, e, w - e - 1, w - e)})
    ys = sorted({min(max(3, v), h - 4) for v in (e - 1, e, h - e - 1, h - e)})
    # the x probes on rows, the y probes on columns near the centre (inside every band tested), no two dots adjacent
    pts = [(x, h // 2 - 4 + 2 * i) for i, x in enumerate(xs)] + [(w // 2 - 4 + 2 * i, y) for i, y in enumerate(ys)]
    return dots(w, h, pts, [255] * len(pts)), dict(edge_threshold=e, nlevels=1, nfeatures=500)


# (id, frame builder, ORB parameters) -- the regimes of both files.  Sizes: 64 x 64 is the smallest frame, odd widths and pyramid
# tails not a multiple of 4; 87 x 99 lands on 72.5 x 82.5 at level 1 (float32 division), which cvRound takes to 72 x 82.
REGIMES = [
    ("64x64-synth-default", lambda: synth_frame(64, 64), {}),
    ("65x67-scale2-tiny-levels", lambda: synth_frame(65, 67), dict(scale_factor=2.0, nlevels=8, patch_size=7, nfeatures=1000)),
    ("97x71-scale105-16lv-patch2-fast1-edge0-score1", lambda: synth_frame(97, 71), dict(scale_factor=1.05, nlevels=16, patch_size=2,
                                                                                    fast_threshold=1, edge_threshold=0, score_type=1)),
    ("127x64-binary-fast254-patch3-edge3", lambda: binary_noise(127, 64), dict(fast_threshold=254, patch_size=3, edge_threshold=3)),
    ("87x99-half-even-level-size", lambda: synth_frame(87, 99), {}),
    ("333x257-16lv", lambda: synth_frame(333, 257), dict(nlevels=16, patch_size=30)),
    ("160x120-uniform-noise", lambda: uniform_noise(160, 120), {}),
    ("160x120-uniform-noise-score1-edge4", lambda: uniform_noise(160, 120, 5), dict(score_type=1, edge_threshold=4, nfeatures=300)),
    ("96x80-checker", lambda: checker(96, 80), dict(patch_size=7)),
    ("96x80-binary-noise", lambda: binary_noise(96, 80), dict(fast_threshold=1)),
    ("64x64-zeros", lambda: flat(64, 64, 0), {}),
    ("64x64-ones", lambda: flat(64, 64, 255), {}),
    ("64x64-flat128", lambda: flat(64, 64, 128), dict(fast_threshold=1)),
    ("200x150-nfeatures1", lambda: synth_frame(200, 150), dict(nfeatures=1)),
    ("200x150-nfeatures7", lambda: synth_frame(200, 150), dict(nfeatures=7)),
    ("200x150-nfeatures7-score1", lambda: synth_frame(200, 150), dict(nfeatures=7, score_type=1)),
    ("tie-motif-inside-slack", lambda: tie_motif(TIE_INSIDE_SLACK)[0], tie_motif(TIE_INSIDE_SLACK)[1]),
    ("edge-motif-0", lambda: edge_motif(0)[0], edge_motif(0)[1]),
    ("edge-motif-4", lambda: edge_motif(4)[0], edge_motif(4)[1]),
    ("edge-motif-31", lambda: edge_motif(31)[0], edge_motif(31)[1]),
    ("edge-motif-50", lambda: edge_motif(50)[0], edge_motif(50)[1]),
    ("640x480-uniform-noise-max-nfeatures", lambda: uniform_noise(640, 480, 7), dict(nfeatures=MAX_NFEATURES)),
]
REGIME_IDS = [r[0] for r in REGIMES]

# (parameters, frame size, why) the library and the oracle refuse, and their accepted neighbours
REFUSED = [(dict(patch_size=31), (640, 480), "patch_size 31"),
           (dict(nfeatures=MAX_NFEATURES + 1), (640, 480), "level budget"),
           (dict(nlevels=1, nfeatures=1921), (640, 480), "level budget"),
           (dict(scale_factor=2.0, nlevels=8, nfeatures=1000), (64, 64), "empty level"),          # 64 / 128 = 0.5 -> 0
           (dict(scale_factor=2.0, nlevels=13, nfeatures=1000), (1920, 1080), "empty level")]     # 1080 / 2048 -> 1, / 4096 -> 0
ACCEPTED = [(dict(patch_size=30), (640, 480)), (dict(patch_size=32), (640, 480)), (dict(nfeatures=MAX_NFEATURES), (640, 480)),
            (dict(nlevels=1, nfeatures=1920), (640, 480)), (dict(scale_factor=2.0, nlevels=7, nfeatures=1000), (64, 64)),
            (dict(scale_factor=2.0, nlevels=12, nfeatures=1000), (1920, 1080))]


def report(tag, cmp_):
    print("%-48s undetermined bits %.2e, max angle band %.2e deg" % (tag, cmp_["undetermined_share"] or 0.0, cmp_["max_angle_band"] or 0.0))


# ------------------------------------------------------------------------------------------------ tables
def test_gaussian_taps_are_derived_bit_exactly():
    assert ro.gaussian_taps_q8() == [18, 34, 48, 56, 48, 34, 18]


def test_reflect101_closed_form_against_border_interpolate():
    def bi(p, n):                       # core/copy.cpp borderInterpolate(BORDER_REFLECT_101), the loop as written there
        if n == 1:
            return 0
        while not 0 <= p < n:
            p = -p if p < 0 else 2 * n - 2 - p
        return p
    for n in (1, 2, 3, 4, 7, 64):
        ps = np.arange(-40, n + 40)
        assert ro.reflect101(ps, n).tolist() == [bi(int(p), n) for p in ps], n
    assert ro.reflect101(np.arange(-5, 7), 2).tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0]
    assert ro.reflect101(np.arange(-6, 9), 3).tolist() == [2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0, 1, 2, 1, 0]


@pytest.mark.parametrize("kw", [{}, dict(scale_factor=1.05, nlevels=16), dict(scale_factor=2.0, nlevels=5, nfeatures=1000), dict(nlevels=1, nfeatures=1920),
                                dict(nfeatures=1), dict(nfeatures=7), dict(nfeatures=MAX_NFEATURES), dict(patch_size=2),
                                dict(patch_size=3), dict(patch_size=7), dict(patch_size=30)])
def test_level_sizes_budgets_umax_pattern(oracle_mod, kw):
    p = ro.params(**kw)
    o = None
    for w, h in ((64, 64), (65, 67), (87, 99), (333, 257), (1920, 1080), (3840, 2160)):
        if ro.refused(p, w, h):
            continue
        o = oracle_mod.Orb(w, h, oracle_mod.orb_default_params(**kw))
        for l, (size, n) in enumerate(zip(ro.level_sizes(p, w, h), ro.level_budgets(p))):
            assert o.level_size(l) == size and o.level_nfeatures(l) == n, (w, h, l)
            assert o.level_scale(l) == ro.level_scales(p)[l]
    assert np.array_equal(o.umax(), ro.umax_table(p["patch_size"]))
    assert np.array_equal(o.pattern().astype(np.int64), ro.pattern(p["patch_size"]))


def test_half_even_level_size():
    """87 x 99 at 1.2: level 1 is 72.5 x 82.5 after the float32 division; cvRound keeps the even neighbours."""
    p = ro.params()
    s = ro.level_scales(p)[1]
    assert np.float32(87) / s == 72.5 and np.float32(99) / s == 82.5
    assert ro.level_sizes(p, 87, 99)[1] == (72, 82)


def test_gray_exact(oracle_mod):
    img = uniform_noise(131, 37, 11)
    assert np.array_equal(oracle_mod.bgr2gray(img), ro.bgr2gray(img))
    ext = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 1, 1]]], np.uint8)
    assert ro.bgr2gray(ext)[0].tolist() == [0, 255, 29, 150, 76, 1]


# ------------------------------------------------------------------------------------------------ the whole path
def check_oracle(oracle_mod, frame, kw, tag):
    h, w = frame.shape[:2]
    p = ro.params(**kw)
    ref = ro.orb(frame, p)
    o = oracle_mod.Orb(w, h, oracle_mod.orb_default_params(**kw))
    kps, desc = o.run(frame)
    for l in range(p["nlevels"]):
        assert o.level_size(l) == ref["levels"][l], (tag, l)
        assert np.array_equal(o.level_gray(l), ref["gray"][l]), (tag, "gray", l)
        assert np.array_equal(o.level_nms(l), ref["nms"][l]), (tag, "nms", l)
        assert np.array_equal(o.level_blur(l), ref["blur"][l]), (tag, "blur", l)
        assert [o.level_count(l, k) for k in range(3)] == list(ref["counts"][l]), (tag, "counts", l)
    c = ro.compare_features(kps, desc, ref)
    assert not c["errors"], (tag, c["errors"])
    assert ro.canonical_order_ok(ref["kps"])
    report(tag, c)
    return ref


@pytest.mark.parametrize("tag,make,kw", REGIMES, ids=REGIME_IDS)
def test_oracle_matches_reference(oracle_mod, tag, make, kw):
    ref = check_oracle(oracle_mod, make(), kw, tag)
    if tag.startswith("64x64-") and tag.split("-")[1] in ("zeros", "ones", "flat128"):
        assert len(ref["kps"]) == 0
    if tag == "65x67-scale2-tiny-levels":
        assert [s for s in ref["levels"][5:]] == [(2, 2), (1, 1), (1, 1)]


def test_oracle_ties_at_both_cuts_kept(oracle_mod):
    for n_b in (TIE_INSIDE_SLACK, TIE_BEYOND_SLACK):
        frame, kw = tie_motif(n_b)
        ref = check_oracle(oracle_mod, frame, kw, "tie-motif-%d" % n_b)
        n0, n1, n2 = ref["counts"][0]
        assert (n0, n1, n2) == (60 + n_b + 50, 60 + n_b, 60 + n_b)      # FAST cut inside the 200-dots, Harris cut likewise
        r = ref["kps"]["response"]
        assert len(np.unique(r)) == 2 and n2 > 100


def test_edge_threshold_boundary(oracle_mod):
    for e in (0, 4, 31, 50):
        frame, kw = edge_motif(e)
        ref = check_oracle(oracle_mod, frame, kw, "edge-%d" % e)
        k = ref["kps"]
        h, w = frame.shape[:2]
        got = sorted(zip(k["x"].astype(int).tolist(), k["y"].astype(int).tolist()))
        ys, xs = np.nonzero(frame[:, :, 0])
        want = sorted((x, y) for x, y in zip(xs.tolist(), ys.tolist()) if e <= x < w - e and e <= y < h - e)
        assert got == want and len(want) >= 2, (e, got, want)


def test_oracle_refuses_what_the_library_refuses(oracle_mod):
    """patch_size 31 (bit_pattern_31_), a level budget above 1920, an empty pyramid level: ValueError from the binding."""
    for kw, size, why in REFUSED:
        assert ro.refused(ro.params(**kw), *size) == why
        with pytest.raises(ValueError):
            oracle_mod.Orb(size[0], size[1], oracle_mod.orb_default_params(**kw))
    for kw, size in ACCEPTED:
        assert not ro.refused(ro.params(**kw), *size)
        oracle_mod.Orb(size[0], size[1], oracle_mod.orb_default_params(**kw)).close()
