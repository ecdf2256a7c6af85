"""The matcher's Hamming 2-NN pass enqueued ahead of the matcher call, behind the ORB batch (mis_orb_arm_knn_ahead): a matcher call
that adopts the pass and one that runs its own give the same MatchesInfo table byte for byte, the pass is adopted exactly when the
call matches the armed batch with the armed selection (mis_debug_knn_ahead_adopted counts the adoptions, so a silent fallback
cannot pass for an adoption, nor an adoption for a fallback), and a pass that nobody adopts is never read.

Small shapes: 5 synthetic frames of 320 x 240, the real ORB finder with nfeatures 500 (only the finder publishes device counts;
its blocks hold 1524 features, so the capacity plan has six query blocks per directed pair where the counts fill at most two).
The reference of every case is the unarmed path on the same frames -- ORB is deterministic --, computed once per frame set
and selection.  (No frame is at its exact capacity: a level keeps at most its budget plus ties, and the budgets sum to nfeatures.)
Both paths run the same kernel, so test_plain_adoption, test_counts_that_differ and the many-frames and overflow cases also hold
every pair's match list to the exact reference of tests/refimpl.py.  The finder cannot place a count on an edge: the count edges,
the rows between count and capacity and the cached plan are pinned through a test aid in test_knn_ahead_edges_gpu.py; the last
section here holds the drop rules that only the finder can reach (another batch size, world_size 2, more than 64 frames, blocks
over 8192 features, an overflowing batch) and the affine model."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, NF = 320, 240, 5


@functools.lru_cache(maxsize=None)
def frame_set(name):
    """textured: a yaw sweep.  four: its first four frames.  gray: the same with frame 2 constant gray (no keypoints).  uneven: frame 1 nearly flat, a few dozen
    keypoints at the corners of three bright squares; frame 3 a crop of texture in a flat frame."""
    import synth
    frames = [synth.render_frame(synth.make_camera(W, H, 60.0, 9.0 * i - 18.0, 0.3 * i, -0.2 * i)) for i in range(NF)]
    if name == "gray":
        frames[2] = np.full((H, W, 3), 128, np.uint8)
    if name == "four":
        frames = frames[:4]
    if name == "uneven":
        flat = np.full((H, W, 3), 110, np.uint8)
        rng = np.random.RandomState(5)
        for _ in range(3):
            x, y, s = rng.randint(50, W - 70), rng.randint(50, H - 70), rng.randint(9, 17)
            flat[y:y + s, x:x + s] = rng.randint(200, 256)
        frames[1] = flat
        part = np.full((H, W, 3), 90, np.uint8)
        part[60:180, 80:240] = frames[3][60:180, 80:240]
        frames[3] = part
    for f in frames:
        f.setflags(write=False)
    return tuple(frames)


@pytest.fixture(scope="module")
def finder(ctx):
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import orb_params
    f = isa.OrbFeatureFinder(ctx, (W, H), orb_params(nfeatures=500))
    yield f
    f.close()


@functools.lru_cache(maxsize=None)
def device_frames(name):
    import torch
    return [torch.from_numpy(np.array(f)).cuda() for f in frame_set(name)]


def adopted(ctx):
    return ctx.lib.mis_debug_knn_ahead_adopted(ctx.h)


def matcher_for(ctx, range_width):
    import image_stitching_amd as isa
    return isa.BestOf2NearestMatcher(ctx, 0.32) if range_width == -1 else isa.BestOf2NearestRangeMatcher(ctx, range_width, 0.32)


def table(pm):
    """every field of every MatchesInfo entry, as bytes where a field is an array or a float"""
    out = []
    for m in pm:
        out.append((m.src_img_idx, m.dst_img_idx, len(m.matches), np.asarray(m.matches).tobytes(), np.asarray(m.inliers_mask).tobytes(), m.num_inliers,
                    m.H is not None, b"" if m.H is None else np.asarray(m.H, np.float64).tobytes(), np.float64(m.confidence).tobytes()))
    return out


def assert_reference_lists(pm, feats, match=(-1, None)):
    """every selected pair's match list against the exact reference (tests/refimpl.py) on the downloaded descriptors, the mirrored
    entry its transpose: what the armed and the unarmed path could both get wrong, they run the same kernel"""
    import refimpl as ri
    n = len(feats)
    desc = [f.download()[1] for f in feats]
    for i in range(n):
        for j in range(i + 1, n):
            if not ((match[1] is None or match[1][i, j]) and (match[0] == -1 or j < i + match[0])):
                continue
            ref = ri.best_of_2_nearest_matches(desc[i], desc[j], 0.32)
            g, tr = pm[i * n + j].matches, pm[j * n + i].matches
            assert np.array_equal(g, ref.astype(g.dtype)), (i, j, len(g), len(ref))
            assert np.array_equal(tr["query_idx"], g["train_idx"]) and np.array_equal(tr["train_idx"], g["query_idx"]), (i, j)
            assert np.array_equal(tr["distance"], g["distance"]), (i, j)


def run(ctx, finder, name, arm=None, match=(-1, None), pick=None, reference_lists=False, frames=None, make_matcher=matcher_for, arm_n=NF, arm_world=1):
    """one batch (armed with the selection `arm` = (range_width, mask), or not) and one matcher call with the selection `match` of
    the features `pick` makes of the batch's (default: as they are) -> (table, adoptions of the call, counts)"""
    if arm is not None:
        finder.arm_knn_ahead(arm_n, arm[1], arm[0], 0, arm_world)
    feats = finder.detect_batch(device_frames(name) if frames is None else frames)
    counts = [len(f) for f in feats]
    lst = feats if pick is None else pick(ctx, feats)
    a0 = adopted(ctx)
    pm = make_matcher(ctx, match[0])(lst, mask=match[1])
    n_adopted = adopted(ctx) - a0
    if reference_lists:
        assert_reference_lists(pm, lst, match)
    return table(pm), n_adopted, counts


_REF = {}


def reference(ctx, finder, name, match=(-1, None), pick=None, key=None):
    """the unarmed path, once per (frame set, selection, list)"""
    k = (name, match[0], None if match[1] is None else match[1].tobytes(), key)
    if k not in _REF:
        t, n_adopted, counts = run(ctx, finder, name, None, match, pick)
        assert n_adopted == 0
        _REF[k] = (t, counts)
    return _REF[k]


def band_mask():
    m = np.zeros((NF, NF), np.uint8)
    for i, j in ((0, 1), (0, 3), (1, 2), (2, 4), (3, 4)):
        m[i, j] = 1
    m[4, 0] = m[2, 2] = 1          # lower triangle and diagonal: not read
    return m


def test_plain_adoption(ctx, finder):
    want, counts = reference(ctx, finder, "textured")
    print("counts", counts)
    assert min(counts) > 256, "the frames should fill more than one query block"
    got, n_adopted, c = run(ctx, finder, "textured", arm=(-1, None), reference_lists=True)
    assert c == counts
    assert n_adopted == 1, "the armed path did not adopt the pass"
    assert got == want
    assert sum(1 for e in want if e[6]) >= 8, "the sweep should connect its neighbours (an H both ways)"


def test_frame_without_keypoints(ctx, finder):
    want, counts = reference(ctx, finder, "gray")
    assert counts[2] == 0 and min(counts[:2] + counts[3:]) > 0
    got, n_adopted, _ = run(ctx, finder, "gray", arm=(-1, None))
    assert n_adopted == 0          # an empty frame: the call plans fewer pairs than the pass ran, it runs its own
    assert got == want


@pytest.mark.parametrize("sel", ["width2", "mask", "width3-and-mask"])
def test_selections(ctx, finder, sel):
    match = {"width2": (2, None), "mask": (-1, band_mask()), "width3-and-mask": (3, band_mask())}[sel]
    want, _ = reference(ctx, finder, "textured", match)
    got, n_adopted, _ = run(ctx, finder, "textured", arm=match, match=match)
    assert n_adopted == 1
    assert got == want
    full, _ = reference(ctx, finder, "textured")
    assert got != full             # (the selection selects)


@pytest.mark.parametrize("armed, matched", [((-1, None), (2, None)), ((2, None), (-1, None)), ((-1, band_mask()), (-1, None)),
                                            ((-1, None), (-1, band_mask())), ((-1, band_mask()), (-1, np.triu(np.ones((NF, NF), np.uint8))))])
def test_mismatched_selection(ctx, finder, armed, matched):
    want, _ = reference(ctx, finder, "textured", matched)
    got, n_adopted, _ = run(ctx, finder, "textured", arm=armed, match=matched)
    assert n_adopted == 0
    assert got == want


def _reordered(ctx, feats):
    return feats[::-1]


def _subset(ctx, feats):
    return feats[1:]


def _uploaded(ctx, feats):
    import image_stitching_amd as isa
    out = []
    for i, f in enumerate(feats):
        k, d = f.download()
        out.append(isa.ImageFeatures.upload(ctx, f.img_size, k, d, i))
    return out


def _one_swapped_for_upload(ctx, feats):
    return feats[:3] + _uploaded(ctx, feats[3:4]) + feats[4:]


@pytest.mark.parametrize("pick", [_reordered, _subset, _uploaded, _one_swapped_for_upload], ids=lambda f: f.__name__.strip("_"))
def test_different_feature_list(ctx, finder, pick):
    want, _ = reference(ctx, finder, "textured", pick=pick, key=pick.__name__)
    got, n_adopted, _ = run(ctx, finder, "textured", arm=(-1, None), pick=pick)
    assert n_adopted == 0
    assert got == want
    if pick in (_uploaded, _one_swapped_for_upload):
        assert got == reference(ctx, finder, "textured")[0]        # the same features from other blocks: the same table


def test_arming_without_a_matcher_call(ctx, finder):
    """two armed batches in a row, of different frames; the second is matched: its own pass is adopted, the first one's is gone"""
    want, _ = reference(ctx, finder, "uneven")
    finder.arm_knn_ahead(NF, None, -1)
    first = finder.detect_batch(device_frames("textured"))
    got, n_adopted, _ = run(ctx, finder, "uneven", arm=(-1, None))
    assert n_adopted == 1
    assert got == want
    # and the first batch's features, matched now, run their own pass
    a0 = adopted(ctx)
    t = table(matcher_for(ctx, -1)(first))
    assert adopted(ctx) == a0 and t == reference(ctx, finder, "textured")[0]


def test_armed_batch_then_unarmed_batch(ctx, finder):
    """an unarmed batch drops the pass of the armed one before it; and an arm is one-shot"""
    want, _ = reference(ctx, finder, "textured")
    finder.arm_knn_ahead(NF, None, -1)
    finder.detect_batch(device_frames("uneven"))
    got, n_adopted, _ = run(ctx, finder, "textured")
    assert n_adopted == 0 and got == want


def test_counts_that_differ(ctx, finder):
    want, counts = reference(ctx, finder, "uneven")
    print("counts", counts)
    assert 0 < min(counts) < 100 and max(counts) >= 400, counts        # a few dozen corners beside full frames
    assert len({(c + 255) // 256 for c in counts}) >= 2                 # and different numbers of query blocks
    got, n_adopted, c = run(ctx, finder, "uneven", arm=(-1, None), reference_lists=True)
    assert c == counts and n_adopted == 1
    assert got == want


def test_three_armed_job_steps(ctx):
    """StitchJob.run arms its finder on a single rank: three steps back to back on one job adopt three passes and give the same
    result each time (arena reuse, the drained flag), which is also what the job gives when it does not arm."""
    import synth
    import torch
    from image_stitching_amd.distributed import StitchJob
    cams = [synth.make_camera(W, H, 60.0, 12.0 * i - 18.0, 0.3 * i, -0.2 * i) for i in range(4)]
    frames = {i: torch.from_numpy(synth.render_frame(c)).cuda() for i, c in enumerate(cams)}

    def digest(out):
        return (out["indices"], np.asarray(out["confidence"]).tobytes(), table(out["matches"]), out["pano"].cpu().numpy().tobytes(), out["mask"].cpu().numpy().tobytes())
    job = StitchJob(ctx, (W, H), cams)
    a0 = adopted(ctx)
    outs = [digest(job.run(frames)) for _ in range(3)]
    assert adopted(ctx) - a0 == 3
    assert outs[0] == outs[1] == outs[2]
    plain = StitchJob(ctx, (W, H), cams)
    plain.engine.finder.arm_knn_ahead = lambda *a, **k: None
    a0 = adopted(ctx)
    assert digest(plain.run(frames)) == outs[0]
    assert adopted(ctx) == a0


# ------------------------------------------------------------------------------------------------ the header's other drop rules
def test_armed_for_another_batch_size(ctx, finder):
    """armed for 5 frames, the batch has 4: nothing is enqueued"""
    want, _, counts = run(ctx, finder, "four")
    assert len(counts) == 4
    got, n_adopted, _ = run(ctx, finder, "four", arm=(-1, None), arm_n=5)
    assert n_adopted == 0 and got == want


def test_armed_with_world_size_2(ctx, finder):
    got, n_adopted, _ = run(ctx, finder, "textured", arm=(-1, None), arm_world=2)
    assert n_adopted == 0 and got == reference(ctx, finder, "textured")[0]


SW, SH = 97, 71


@functools.lru_cache(maxsize=None)
def small_frames(n):
    """n frames of 97 x 71 from a sweep of 17 views (repeated from the 18th on)"""
    import synth
    import torch
    views = [torch.from_numpy(synth.render_frame(synth.make_camera(SW, SH, 60.0, 3.0 * i - 24.0, 0.3 * i, -0.2 * i))).cuda() for i in range(17)]
    return [views[i % 17] for i in range(n)]


@pytest.fixture(scope="module")
def small_finder(ctx):
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import orb_params
    f = isa.OrbFeatureFinder(ctx, (SW, SH), orb_params(nfeatures=300, nlevels=4))
    yield f
    f.close()


@pytest.mark.parametrize("n, range_width, expect", [(17, 3, 1), (65, 2, 0)])
def test_many_armed_frames(ctx, small_finder, n, range_width, expect):
    """17 frames are two groups of the ORB batch and more train frames than the workgroup table has lists: adopted.  65 are more
    than a pass takes: nothing is enqueued."""
    sel = (range_width, None)
    want, n0, counts = run(ctx, small_finder, None, match=sel, frames=small_frames(n))
    print("counts", counts)
    assert n0 == 0 and len(counts) == n and min(counts) > 0
    got, n_adopted, c = run(ctx, small_finder, None, arm=sel, match=sel, frames=small_frames(n), arm_n=n, reference_lists=n == 17)
    assert c == counts and n_adopted == expect
    assert got == want


def test_capacity_above_8192(ctx):
    """nfeatures 7200 on 8 levels: blocks of 7200 + 8 x 128 = 8224 features, more than the Hamming pass on the matrix cores takes"""
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import orb_params
    big = isa.OrbFeatureFinder(ctx, (W, H), orb_params(nfeatures=7200))
    try:
        want, _, counts = run(ctx, big, "textured")
        got, n_adopted, c = run(ctx, big, "textured", arm=(-1, None))
        assert c == counts and n_adopted == 0 and got == want
    finally:
        big.close()


def test_overflowing_armed_batch(ctx):
    """A batch that overflows its candidate buffers (ties beyond the slack) fails with MIS_E_OVERFLOW; its pass is nobody's: the
    next matcher call, on a good unarmed batch, runs its own and is right, and the next armed good batch is adopted."""
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import orb_params
    from test_refimpl_orb_cpu import TIE_BEYOND_SLACK, TIE_INSIDE_SLACK, tie_motif
    beyond, kw = tie_motif(TIE_BEYOND_SLACK)
    good = [torch.from_numpy(tie_motif(TIE_INSIDE_SLACK, seed=s)[0]).cuda() for s in (3, 4)]
    bad = [good[0], torch.from_numpy(beyond).cuda()]
    f = isa.OrbFeatureFinder(ctx, (200, 200), orb_params(**kw))
    try:
        want, n0, counts = run(ctx, f, None, frames=good, reference_lists=True)
        assert n0 == 0 and min(counts) > 0
        f.arm_knn_ahead(2, None, -1)
        with pytest.raises(isa.MisError) as e:
            f.detect_batch(bad)
        assert e.value.code == -4          # MIS_E_OVERFLOW
        got, n_adopted, c = run(ctx, f, None, frames=good, reference_lists=True)
        assert c == counts and n_adopted == 0 and got == want
        got, n_adopted, c = run(ctx, f, None, arm=(-1, None), frames=good, arm_n=2, reference_lists=True)
        assert c == counts and n_adopted == 1 and got == want
    finally:
        f.close()


def test_affine_matcher_adopts(ctx, finder):
    """adoption does not depend on the model: the affine matcher takes the pass and gives its unarmed table"""
    import image_stitching_amd as isa

    def affine(ctx, range_width):
        return isa.AffineBestOf2NearestMatcher(ctx, match_conf=0.32)
    want, n0, counts = run(ctx, finder, "textured", make_matcher=affine)
    assert n0 == 0
    got, n_adopted, c = run(ctx, finder, "textured", arm=(-1, None), make_matcher=affine)
    assert c == counts and n_adopted == 1 and got == want
    assert got != reference(ctx, finder, "textured")[0]        # (another model)
