"""The 2-NN pass enqueued ahead of the matcher call (mis_knn_ahead_enqueue) at the count edges and at every drop rule of
mistitch.h, against the exact references of tests/refimpl.py.

The real ORB finder cannot put a count on an edge, so the pass is driven through the test aid mis_debug_knn_ahead: uploaded blocks
of `cap` rows of which the first `count` are live, the count written into the block's device slot, the pass planned from the
capacities -- what mis_orb_detect_batch does behind its gather.  The rows count .. cap - 1 of a frame are adversarial tails: exact
copies of live descriptors of the OTHER frames of the case (keypoints far off the frame, finite), so whatever reads past a count
as a train finds a distance-0 neighbour with an index >= count.  test_tails_are_adversarial (CPU) proves that of every case.

Every case asserts: the adoptions of the matcher call (1, or 0 where the pass must be dropped), every selected pair's match list
= refimpl.best_of_2_nearest_matches(live_i, live_j, 0.32) element for element, the mirrored entry its transpose, and the whole
MatchesInfo table byte-identical to an unarmed call on fresh uploads of exactly the live rows."""
import ctypes as C
import functools

import numpy as np
import pytest

import refimpl as ri
from test_knn_ahead_gpu import adopted, table
from test_refimpl_match_gpu import _keypoints, hamming_edge_sets, hamming_far_sets, l2_sets

gpu = pytest.mark.gpu
CONF = 0.32
SIZE = (640, 480)
MIS_E_INVALID = -1


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """live: the frames' live descriptor rows; caps: the blocks' capacities; sel = (range_width, mask); far: made by
    hamming_far_sets (an accepted match above distance 128 is required)."""

    def __init__(self, name, live, caps, sel=(-1, None), far=False, kp_n=None):
        assert len(live) == len(caps) and all(len(d) <= c for d, c in zip(live, caps))
        self.name, self.live, self.caps, self.sel, self.far = name, [np.ascontiguousarray(d) for d in live], list(caps), sel, far
        self.kp_n = [len(d) for d in live] if kp_n is None else kp_n       # the keypoint recipe's set sizes (its seeds)
        self._ref = {}

    @property
    def n(self):
        return len(self.live)

    @property
    def counts(self):
        return [len(d) for d in self.live]

    def pairs(self, rank=0, world=1):
        """the selection of FeaturesMatcher::operator() (mask: strict upper triangle; range_width), dealt to `rank` of `world`"""
        rw, mask = self.sel
        out, k = [], 0
        for i in range(self.n):
            for j in range(i + 1, self.n):
                if (mask is None or mask[i, j]) and (rw == -1 or j < i + rw):
                    if k % world == rank:
                        out.append((i, j))
                    k += 1
        return out

    def full(self):
        """the blocks as uploaded: frame i's live rows, then its tail -- copies of the other frames' live rows, in turn"""
        out = []
        for i, d in enumerate(self.live):
            pad = self.caps[i] - len(d)
            others = [self.live[j] for j in range(self.n) if j != i and len(self.live[j])] or [d]      # (a single frame: its own)
            if pad == 0:
                out.append(d)
                continue
            pool = np.concatenate(others[i % len(others):] + others[:i % len(others)])
            out.append(np.concatenate([d, np.resize(pool, (pad,) + d.shape[1:]).astype(d.dtype)]))
        return out

    def ref(self, i, j):
        if (i, j) not in self._ref:
            self._ref[i, j] = ri.best_of_2_nearest_matches(self.live[i], self.live[j], CONF)
        return self._ref[i, j]


def pooled_sets(rng, counts):
    """Frames of one scene: frame i holds counts[i] members of a pool of 400 random descriptors, each with 0 .. 3 bits flipped (its
    counterpart in another frame is at distance <= 6, everything else near 128: accepted), and one exact duplicate (a tie)."""
    pool = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    out = []
    for c in counts:
        d = pool[np.concatenate([rng.permutation(400), rng.integers(0, 400, max(c - 400, 0))])[:c]].copy()     # (past 400: repeats)
        for r in range(c):
            for b in rng.integers(0, 256, int(rng.integers(0, 4))):
                d[r, b >> 3] ^= np.uint8(1 << (b & 7))
        if c >= 3:
            d[c - 1] = d[0]
        out.append(d)
    return out


def band_mask(n, seed):
    """about two thirds of the upper triangle; the lower triangle and the diagonal are set and not read"""
    m = (np.random.default_rng(seed).random((n, n)) < 0.67).astype(np.uint8)
    m[np.tril_indices(n)] = 1
    return m


TRAIN_COUNTS = [1, 2, 3, 31, 32, 33, 255, 256, 257, 511, 512, 513, 767, 768]
GENS = {"far": hamming_far_sets, "edge": hamming_edge_sets}


@functools.lru_cache(maxsize=None)
def count_edge_case(gen, nt):
    """query A (257), train (nt), query B (255), all of capacity 768: 3 query blocks and 24 train tiles planned"""
    rng = np.random.default_rng(2000 + nt + (0 if gen == "far" else 100000))
    q, t = GENS[gen](rng, 257 + 255, nt)
    return Case("count-edge-%s-%d" % (gen, nt), [q[:257], t, q[257:]], [768] * 3, far=gen == "far")


@functools.lru_cache(maxsize=None)
def max_trains_sets():
    return hamming_edge_sets(np.random.default_rng(8192), 8192, 8192)


@functools.lru_cache(maxsize=None)
def max_trains_case(c0):
    """counts (c0, 8192) in blocks of HM_MAX_TRAINS.  A frame at its exact capacity has no tail; with (8192, 8192) neither has,
    and the CPU condition does not apply to that case."""
    q, t = max_trains_sets()
    return Case("max-trains-%d" % c0, [q[:c0], t], [8192, 8192])


@functools.lru_cache(maxsize=None)
def arena_cases():
    """the stale-arena sequence: full blocks, then few live rows under the same (cached) plan, then other capacities, then the
    first capacities again.  In each group the larger capacities come first."""
    rng = np.random.default_rng(77)
    X = pooled_sets(rng, [768, 768, 768])
    Y = pooled_sets(rng, [5, 33, 257])
    Z = pooled_sets(rng, [300, 512, 31])
    W = pooled_sets(rng, [257, 2, 400])
    return [Case("arena-full", X, [768] * 3), Case("arena-small", Y, [768] * 3), Case("arena-replanned", Z, [1024, 512, 768]),
            Case("arena-again", W, [768] * 3)]


MANY_COUNTS = [1, 2, 32, 256, 257, 320, 31, 33, 255, 3, 64, 100, 319, 129, 200, 300, 65]


@functools.lru_cache(maxsize=None)
def many_frames_case(n):
    """more frames than the workgroup table has train lists (8)"""
    if n in (9, 17):
        return Case("frames-%d" % n, pooled_sets(np.random.default_rng(n), MANY_COUNTS[:n]), [320] * n, sel=(3, band_mask(n, n)))
    counts = list(range(1, 65)) + [64] * (n - 64)
    return Case("frames-%d" % n, pooled_sets(np.random.default_rng(n), counts), [64] * n, sel=(2, None))


@functools.lru_cache(maxsize=None)
def base_case(sel="all"):
    """three frames of one scene, counts off every edge: the entries, the models and the drop rules"""
    s = {"all": (-1, None), "width2": (2, None), "mask": (-1, np.array([[1, 1, 0], [1, 1, 1], [1, 0, 0]], np.uint8))}[sel]
    return Case("base-" + sel, pooled_sets(np.random.default_rng(5), [300, 257, 40]), [384, 640, 320], sel=s)


def all_cases():
    """every case that carries tails (the list of test_tails_are_adversarial)"""
    out = [count_edge_case(g, nt) for g in GENS for nt in TRAIN_COUNTS]
    out += [max_trains_case(8191)]              # (8192, 8192): no tail, the condition does not apply
    out += arena_cases()[1:]                    # arena-full: counts = capacities, no tail
    out += [many_frames_case(n) for n in (9, 17, 64, 65)]
    out += [base_case(s) for s in ("all", "width2", "mask")]
    return out


def test_tails_are_adversarial():
    """Of every case: matching the full blocks (tails as if they were live) differs from matching the live rows in at least one
    selected pair, and a far-set case has an accepted match above distance 128 (where a zero padding row, at 128, would win)."""
    for case in all_cases():
        assert any(c < cap for c, cap in zip(case.counts, case.caps)), case.name
        full = case.full()
        differs = False
        for i, j in case.pairs():
            differs = differs or not np.array_equal(ri.best_of_2_nearest_matches(full[i], full[j], CONF), case.ref(i, j))
            if differs:
                break
        assert differs, "%s: the tails would go unnoticed" % case.name
        if case.far and min(case.counts) >= 2:
            assert max(case.ref(i, j)["distance"].max(initial=0) for i, j in case.pairs()) > 128, case.name


# ------------------------------------------------------------------------------------------------ the device side
def _kps(case, i, cap):
    """cap keypoints of frame i: the live rows' as test_refimpl_match_gpu._upload makes them; the tail's far off the frame, finite"""
    from image_stitching_amd.stitching import KP_DTYPE
    n_live = len(case.live[i])
    k = np.zeros(cap, KP_DTYPE)
    k[:n_live] = _keypoints(case.kp_n[i], i, SIZE)[:n_live]
    k["x"][n_live:] = 1.0e6 + 3.0 * np.arange(cap - n_live)
    k["y"][n_live:] = -2.0e6 - 5.0 * np.arange(cap - n_live)
    return k


def upload_live(ctx, case):
    import image_stitching_amd as isa
    return [isa.ImageFeatures.upload(ctx, SIZE, _kps(case, i, len(d)), d, i) for i, d in enumerate(case.live)]


def upload_armed(ctx, case, sel=None, rank=0, world=1, counts=None):
    """the full blocks uploaded and handed to mis_debug_knn_ahead with the case's counts -> the feature list, its structs at the counts"""
    import image_stitching_amd as isa
    from image_stitching_amd import _capi as capi
    rw, mask = case.sel if sel is None else sel
    counts = case.counts if counts is None else counts
    feats = [isa.ImageFeatures.upload(ctx, SIZE, _kps(case, i, case.caps[i]), d, i) for i, d in enumerate(case.full())]
    assert [len(f) for f in feats] == case.caps
    n = case.n
    arr = (capi.MisFeatures * n)()
    for k, f in enumerate(feats):
        C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
    cnt = (C.c_int * n)(*counts)
    m = None if mask is None else np.ascontiguousarray(mask != 0, np.uint8)
    ctx.check(ctx.lib.mis_debug_knn_ahead(ctx.h, arr, n, cnt, None if m is None else m.ctypes.data_as(C.c_void_p), int(rw), rank, world))
    for k, f in enumerate(feats):
        assert arr[k].n == counts[k] and arr[k].owner_ == f.raw.owner_
        f.raw.n = arr[k].n
    return feats


def matcher_for(ctx, case, model="homography"):
    import image_stitching_amd as isa
    rw = case.sel[0]
    if model == "affine":
        m = isa.AffineBestOf2NearestMatcher(ctx, match_conf=CONF)
        m.range_width = rw
        return m
    return isa.BestOf2NearestMatcher(ctx, CONF) if rw == -1 else isa.BestOf2NearestRangeMatcher(ctx, rw, CONF)


def assert_lists(case, pm, rank=0, world=1):
    """every selected pair's list against the exact reference, the mirrored entry its transpose, unselected entries default"""
    n = case.n
    sel = set(case.pairs(rank, world))
    for i in range(n):
        for j in range(i + 1, n):
            g, tr = pm[i * n + j].matches, pm[j * n + i].matches
            if (i, j) not in sel or not len(case.live[i]) or not len(case.live[j]):
                assert len(g) == 0 and len(tr) == 0, (case.name, i, j)
                continue
            ref = case.ref(i, j)
            assert np.array_equal(g, ref.astype(g.dtype)), (case.name, i, j, len(g), len(ref))
            assert np.array_equal(tr["query_idx"], g["train_idx"]) and np.array_equal(tr["train_idx"], g["query_idx"]), (case.name, i, j)
            assert np.array_equal(tr["distance"], g["distance"]), (case.name, i, j)


def unarmed_table(ctx, case, model="homography", rank=0, world=1):
    a0 = adopted(ctx)
    t = table(matcher_for(ctx, case, model)(upload_live(ctx, case), rank=rank, world_size=world, mask=case.sel[1]))
    assert adopted(ctx) == a0
    return t


def check(ctx, case, expect=1, model="homography", lists=True):
    """the aid, one matcher call on its list: `expect` adoptions, the reference's lists, the unarmed table"""
    want = unarmed_table(ctx, case, model)
    feats = upload_armed(ctx, case)
    a0 = adopted(ctx)
    pm = matcher_for(ctx, case, model)(feats, mask=case.sel[1])
    assert adopted(ctx) - a0 == expect, case.name
    if lists:
        assert_lists(case, pm)
    assert table(pm) == want, case.name
    return feats


def assert_usable(ctx):
    """the context adopts the next pass and is right"""
    check(ctx, base_case("all"))


# ------------------------------------------------------------------------------------------------ the tests
@gpu
@pytest.mark.parametrize("nt", TRAIN_COUNTS)
@pytest.mark.parametrize("gen", list(GENS))
def test_count_edges(ctx, gen, nt):
    case = count_edge_case(gen, nt)
    check(ctx, case)
    if case.far and nt >= 2:
        assert sum(len(case.ref(i, j)) for i, j in case.pairs()) > 0


@gpu
@pytest.mark.parametrize("c0", [8191, 8192])
def test_count_at_max_trains(ctx, c0):
    check(ctx, max_trains_case(c0))


@gpu
def test_stale_arena_under_a_cached_plan(ctx):
    """Full blocks fill the expanded arena; the next batch, under the same plan, has few live rows and rewrites the arena only up to
    its padded counts -- what lies behind is the earlier batch's.  Then other capacities (the plan is rebuilt), then the first again."""
    for case in arena_cases():
        check(ctx, case)


@gpu
@pytest.mark.parametrize("n, expect", [(9, 1), (17, 1), (64, 1), (65, 0)])
def test_more_frames_than_train_lists(ctx, n, expect):
    """9 and 17 frames: trains of frame t and t + 8 (and t + 16) share a list.  64 frames is the most a pass takes; for 65 nothing
    is enqueued and the matcher call runs its own."""
    check(ctx, many_frames_case(n), expect=expect)


@gpu
@pytest.mark.parametrize("sel, model", [("all", "homography"), ("width2", "homography"), ("mask", "homography"), ("all", "affine"),
                                        ("width2", "affine")])
def test_entries_and_models(ctx, sel, model):
    """mis_match_all_pairs, mis_match_pairs_select and mis_match_pairs_model (MIS_MATCH_AFFINE_PARTIAL) adopt alike.  The affine
    entry is held to its own unarmed table."""
    check(ctx, base_case(sel), model=model, lists=model == "homography")


@gpu
def test_dropped_world_2_in_the_aid(ctx):
    case = base_case("all")
    want = unarmed_table(ctx, case)
    feats = upload_armed(ctx, case, world=2)
    a0 = adopted(ctx)
    pm = matcher_for(ctx, case)(feats)
    assert adopted(ctx) == a0
    assert_lists(case, pm)
    assert table(pm) == want
    assert_usable(ctx)


@gpu
def test_dropped_capacity_above_max_trains(ctx):
    b = base_case("all")
    check(ctx, Case("cap-8193", b.live, [384, 8193, 320]), expect=0)
    assert_usable(ctx)


@gpu
def test_dropped_float_descriptors(ctx):
    rng = np.random.default_rng(11)
    qa, t = l2_sets(rng, 120, 300, 64)
    qb, _ = l2_sets(rng, 50, 300, 64)
    check(ctx, Case("float", [qa, t, qb], [256, 320, 64]), expect=0)
    assert_usable(ctx)


@gpu
def test_dropped_single_frame(ctx):
    b = base_case("all")
    check(ctx, Case("one-frame", b.live[:1], b.caps[:1]), expect=0)
    assert_usable(ctx)


@gpu
def test_dropped_sharded_matcher_call(ctx):
    """armed for one rank, matched as rank 0 of 2"""
    case = base_case("all")
    want = unarmed_table(ctx, case, rank=0, world=2)
    feats = upload_armed(ctx, case)
    a0 = adopted(ctx)
    pm = matcher_for(ctx, case)(feats, rank=0, world_size=2)
    assert adopted(ctx) == a0
    assert_lists(case, pm, 0, 2)
    assert table(pm) == want
    assert_usable(ctx)


@gpu
def test_dropped_count_changed_after_the_aid(ctx):
    b = base_case("all")
    short = Case("one-fewer", [b.live[0], b.live[1][:-1], b.live[2]], b.caps, kp_n=b.kp_n)
    want = unarmed_table(ctx, short)            # (before the aid: a matcher call in between would consume the pass)
    feats = upload_armed(ctx, b)
    feats[1].raw.n -= 1
    a0 = adopted(ctx)
    pm = matcher_for(ctx, b)(feats)
    assert adopted(ctx) == a0
    assert_lists(short, pm)
    assert table(pm) == want
    assert_usable(ctx)


@gpu
def test_pass_is_one_shot(ctx):
    case = base_case("all")
    want = unarmed_table(ctx, case)
    feats = check(ctx, case)
    a0 = adopted(ctx)
    pm = matcher_for(ctx, case)(feats)          # (nothing between the adopting call and this one)
    assert adopted(ctx) == a0, "a second call on the same list adopted the pass again"
    assert_lists(case, pm)
    assert table(pm) == want
    assert_usable(ctx)


@gpu
def test_failed_matcher_call_consumes_the_pass(ctx):
    import image_stitching_amd as isa
    case = base_case("all")
    want = unarmed_table(ctx, case)
    feats = upload_armed(ctx, case)
    fl = isa.ImageFeatures.upload(ctx, SIZE, _keypoints(50, 2, SIZE), l2_sets(np.random.default_rng(3), 50, 60, 64)[0], 2)
    a0 = adopted(ctx)
    with pytest.raises(isa.MisError) as e:
        matcher_for(ctx, case)(feats[:2] + [fl])
    assert e.value.code == MIS_E_INVALID
    pm = matcher_for(ctx, case)(feats)
    assert adopted(ctx) == a0, "the pass survived a failed matcher call"
    assert_lists(case, pm)
    assert table(pm) == want
    assert_usable(ctx)


def _freed_set(ctx):
    import image_stitching_amd as isa
    b = base_case("all")
    caps = [384, 701, 320]
    case = Case("freed", [b.live[0], Case("", b.live, caps).full()[1], b.live[2]], caps)
    assert case.counts[1] == case.caps[1] == 701
    want = unarmed_table(ctx, case)
    feats = upload_armed(ctx, case)
    owner = feats[1].raw.owner_
    k, d = feats[1].download()
    feats[1].close()
    again = isa.ImageFeatures.upload(ctx, SIZE, k, d, 1)
    a0 = adopted(ctx)
    pm = matcher_for(ctx, case)([feats[0], again, feats[2]])
    print("the freed block came back from the pool:", again.raw.owner_ == owner, "| adoptions:", adopted(ctx) - a0)
    assert adopted(ctx) == a0, "a freed set's pass was adopted"
    assert_lists(case, pm)
    assert table(pm) == want
    assert_usable(ctx)


@gpu
def test_freed_set_whose_block_comes_back():
    """Frame 1 is at its exact capacity: downloaded, freed and uploaded again it takes a block of the same size from the pool -- in
    a context of its own, whose pool holds nothing else of that size, the very block the pass was enqueued on.
    mis_features_free dropped the pass."""
    import image_stitching_amd as isa
    own = isa.Context(0)
    try:
        _freed_set(own)
    finally:
        own.close()


@gpu
def test_aid_argument_errors(ctx):
    from image_stitching_amd import _capi as capi
    case = base_case("all")
    feats = upload_live(ctx, case)
    arr = (capi.MisFeatures * 3)()
    for k, f in enumerate(feats):
        C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
    good = (C.c_int * 3)(*case.counts)
    lib = ctx.lib
    assert lib.mis_debug_knn_ahead(None, arr, 3, good, None, -1, 0, 1) == MIS_E_INVALID
    assert lib.mis_debug_knn_ahead(ctx.h, None, 3, good, None, -1, 0, 1) == MIS_E_INVALID
    assert lib.mis_debug_knn_ahead(ctx.h, arr, 3, None, None, -1, 0, 1) == MIS_E_INVALID
    assert lib.mis_debug_knn_ahead(ctx.h, arr, 3, (C.c_int * 3)(1, -1, 1), None, -1, 0, 1) == MIS_E_INVALID
    assert lib.mis_debug_knn_ahead(ctx.h, arr, 3, (C.c_int * 3)(1, case.counts[1] + 1, 1), None, -1, 0, 1) == MIS_E_INVALID
    assert [a.n for a in arr] == case.counts
    assert_usable(ctx)
