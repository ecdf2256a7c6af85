"""The oracle's DpSeamFinder (oracle/mo_seam.c) against the numpy / scipy reference of tests/refimpl_seam_dp.py on the scenes of
that module -- the smallest inputs at which each branch of the finder can go wrong -- and the reference against itself by other
methods, so that it is not merely a third copy: Dijkstra over the seam's step graph, monotonicity, the tips, masks that only
lose pixels, resolved pairs that share nothing.

NOT PINNED (refimpl_seam_dp.py): the order of pairs at equal centre distance.  test_tie_order_readings prints on which scenes,
and by how many mask pixels, the two readings differ; the oracle and the product take tie_order="reversed", which is what the
comparisons here check.

Mutation record (each applied alone to a scratch copy of oracle/mo_seam.c, rebuilt; test_oracle_equals_reference then fails on
the scenes named):
  `< 100` -> `<= 100` in the cluster test        cluster_at_10
  `>` -> `>=` in the choice of the seam axis     corner_square_2 (corner_square's tie cannot show it: both axes force the same diagonal
                                                 seam there, and the pixel below and the pixel right of it lie on the same side)
  0.05 -> 0.1 in the contour rule                side_by_side, stacked_slant, two_firsts, bytes, tie_three, five
  the step-code tiebreak reversed                flat, flat_stacked, near_edges
  only (c2, c1) of the resolved edge erased      every scene with a conflict: the same conflict is found for ever (the run was
                                                 ended by a time limit; it is a hang, not a failed assertion)
  only (c1, c2) of the resolved edge erased      none, and none can: the direction (c2, c1) is never read (reference docstring)
  the seam on the lower side of pixels           stacked, stacked_slant, corner_wide, gap, two_firsts, six, tie_three, five
  `!= 255` dropped in the contour pass           every scene with a seam (18, seam_scale among them)
  `!= 255` dropped in the seam pass              none, and none can: a seam has one point per line across its axis, so the pixel
                                                 below (right of) a seam point is never a seam point still marked 255, and the
                                                 contour pass before it leaves no 255 behind
"""
import collections
import functools

import numpy as np
import pytest

import oracle
import refimpl_seam_dp as rs

NAMES = list(rs.SCENES)


@functools.lru_cache(maxsize=None)
def scene(name):
    im, c, m = rs.seam_scale_scene() if name == "seam_scale" else rs.scene(name)
    for a in im + m:
        a.setflags(write=False)
    return im, c, m


@functools.lru_cache(maxsize=None)
def reference(name, tie_order="reversed"):
    """-> (masks, trace, seam records); the small scenes run under the exactness condition."""
    im, c, m = scene(name)
    trace, seams = collections.Counter(), []
    out = rs.find(im, c, m, check_exact=name != "seam_scale", tie_order=tie_order, trace=trace, seams=seams)
    return out, trace, seams


def overlap(c, a, b, i, j):
    x0, y0 = max(c[i][0], c[j][0]), max(c[i][1], c[j][1])
    x1, y1 = min(c[i][0] + a.shape[1], c[j][0] + b.shape[1]), min(c[i][1] + a.shape[0], c[j][1] + b.shape[0])
    if x0 >= x1 or y0 >= y1:
        return None
    return a[y0 - c[i][1]:y1 - c[i][1], x0 - c[i][0]:x1 - c[i][0]], b[y0 - c[j][1]:y1 - c[j][1], x0 - c[j][0]:x1 - c[j][0]]


@pytest.mark.parametrize("name", NAMES + ["seam_scale"])
def test_oracle_equals_reference(name):
    im, c, m = scene(name)
    want = reference(name)[0]
    got = oracle.dp_seams(im, c, m)
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), "%s: mask %d differs in %d pixels, first at %s" % (name, k, (g != w).sum(), np.argwhere(g != w)[0])


def test_trace_covers_every_event():
    total = collections.Counter()
    for name in NAMES:
        tr = reference(name)[1]
        print("%-14s %s" % (name, dict(tr)))
        total += tr
    missing = [e for e in rs.EVENTS if not total[e]]
    assert not missing, missing


def test_scene_sizes():
    """Frames of at most about 64 x 48 pixels, some corners negative, masks of bytes 0 / 1 / 128 / 255."""
    neg, values = False, set()
    for name in NAMES:
        im, c, m = scene(name)
        for i, (cx, cy), k in zip(im, c, m):
            assert i.shape == k.shape + (3,) and i.dtype == k.dtype == np.uint8
            assert k.shape[0] * k.shape[1] <= 64 * 48 and max(k.shape) <= 64, (name, k.shape)
            neg |= cx < 0 or cy < 0
            values |= set(np.unique(k).tolist())
    assert neg and values == {0, 1, 128, 255}


def test_exactness_condition():
    """On every small scene every float32 sum stays below 2^23 and the integer and the float32 programme choose the same seam
    (rs.find asserts both under check_exact; restated here on the records)."""
    nseams = 0
    for name in NAMES:
        for rec in reference(name)[2]:
            print("%-14s %s: largest float32 sum %.1f" % (name, rec["tag"], rec["big"]))
            assert rec["big"] < rs.EXACT_BOUND and rec["other_dp_same"] is True
            nseams += 1
    assert nseams >= 30


@pytest.mark.parametrize("name", NAMES)
def test_seams_by_another_method(name):
    """Every seam of the reference: its cost is the shortest path of the step graph (Dijkstra), it is monotone along its axis with
    steps of at most one across, and it runs from tip to tip; an unreachable destination is unreachable for Dijkstra too."""
    for rec in reference(name)[2]:
        sp = rs.seam_shortest_path(rec)
        print("%-14s %s: DP %s, Dijkstra %s" % (name, rec["tag"], rec["total"], sp))
        assert sp == rec["total"]
        if rec["seam"] is None:
            assert sp is None
            continue
        s = np.array(rec["seam"])
        along, across = (0, 1) if rec["horizontal"] else (1, 0)
        d = np.diff(s[:, along])
        assert np.all(d == (-1 if rec["swapped"] else 1)) and np.all(np.abs(np.diff(s[:, across])) <= 1)
        assert tuple(s[0]) == tuple(rec["p1"]) and tuple(s[-1]) == tuple(rec["p2"])
        assert len(s) == abs(rec["p2"][along] - rec["p1"][along]) + 1


@pytest.mark.parametrize("name", NAMES + ["seam_scale"])
def test_masks_only_lose_and_resolved_pairs_share_nothing(name):
    im, c, m = scene(name)
    out, trace, _ = reference(name)
    for a, b in zip(out, m):
        assert not np.any((a != b) & (a != 0))                # a byte keeps its value or becomes 0
    if trace["inters_without_neighbour"]:
        return
    for i in range(len(m)):
        for j in range(i + 1, len(m)):
            ov = overlap(c, out[i], out[j], i, j)
            if ov is not None:
                assert not np.any((ov[0] > 0) & (ov[1] > 0)), (i, j)


def test_partition_is_strict_at_ten():
    """ClosePoints(10): squared distance 100 does not join, 99 does; classes are numbered by first member."""
    assert rs.partition_close([(0, 0), (6, 8), (16, 8)]).tolist() == [0, 1, 2]
    assert rs.partition_close([(0, 0), (30, 0), (7, 7), (30, 9), (14, 14)]).tolist() == [0, 1, 0, 1, 0]


def test_pair_order():
    """The most distant centres first; centres use integer halves; equal distances in reverse generation order by default."""
    pairs, dist = rs.pair_order([(0, 0), (10, 0), (0, 10)], [(5, 5), (5, 5), (5, 5)])
    assert pairs == [(1, 2), (0, 2), (0, 1)] and dist[(0, 1)] == dist[(0, 2)] == 100
    assert rs.pair_order([(0, 0), (10, 0), (0, 10)], [(5, 5)] * 3, "forward")[0] == [(1, 2), (0, 1), (0, 2)]
    assert rs.pair_order([(0, 0), (3, 0)], [(5, 5), (3, 3)])[1] == {(0, 1): 4 + 1}


def test_order_of_pairs_changes_the_six_frame_result():
    im, c, m = scene("six")
    pairs = rs.pair_order(c, [(k.shape[1], k.shape[0]) for k in m])[0]
    other = rs.find(im, c, m, order=pairs[::-1])
    n = sum(int((a != b).sum()) for a, b in zip(other, reference("six")[0]))
    print("six: processing the pairs in the opposite order changes %d mask pixels" % n)
    assert n > 0


def test_tie_order_readings():
    """NOT PINNED: prints where the two readings of the order of equally distant pairs differ.  No assertion on the figures."""
    for name in NAMES:
        if len(scene(name)[2]) < 3:
            continue
        a, b = reference(name)[0], reference(name, "forward")[0]
        print("%-14s equal-distance pairs %s: tie_order reversed / forward differ in %d mask pixels"
              % (name, bool(reference(name)[1]["equal_distance_pairs"]), sum(int((x != y).sum()) for x, y in zip(a, b))))


def test_seam_scale_integer_programme():
    """The seam-scale scene passes 2^23, so float32 alone is the reference; prints what the exact programme would have done."""
    im, c, m = scene("seam_scale")
    out, _, seams = reference("seam_scale")
    assert seams and max(r["big"] for r in seams) > rs.EXACT_BOUND
    exact = rs.find(im, c, m, dp="int")
    for r in seams:
        print("seam_scale %s: largest float32 sum %.1f, the integer programme chooses %s seam" % (r["tag"], r["big"], "the same" if r["other_dp_same"] else "ANOTHER"))
    print("seam_scale: masks of the two programmes differ in %d pixels" % sum(int((a != b).sum()) for a, b in zip(out, exact)))
