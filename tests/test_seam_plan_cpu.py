"""The seam finders' pair plan (csrc/seam_plan.h: which pairs overlap, in what order, at which dependency level) on the host, without
a GPU: tools/micro/seam_plan_dump.cpp is built with the address and undefined-behaviour sanitizers and run as a child process on
every layout below in both orders; its pairs, levels and level count are compared with the two references' own pair lists --
tests/refimpl_seam_dp.pair_order(tie_order="reversed") for DpSeamFinder::find's order, tests/refimpl_seam_graphcut.pair_list for
PairwiseSeamFinder::run's -- and with the level rule restated here."""
import os
import subprocess

import numpy as np
import pytest

import refimpl_seam_dp as dp
import refimpl_seam_graphcut as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layouts():
    """name -> (corners, sizes)"""
    out = {
        "n0": ([], []),
        "n1": ([(3, -4)], [(20, 10)]),
        "n2": ([(0, 0), (12, 5)], [(20, 10), (20, 10)]),
        "n2_disjoint": ([(0, 0), (40, 0)], [(20, 10), (20, 10)]),
        # zero-width and zero-height overlaps are no pairs; (0, 3) share a corner point only
        "touching": ([(0, 0), (20, 0), (0, 10), (20, 10), (19, 9)], [(20, 10)] * 4 + [(2, 2)]),
        "inside": ([(0, 0), (10, 8), (12, 9)], [(64, 48), (20, 16), (4, 4)]),
        "identical": ([(5, 5)] * 5, [(16, 12)] * 5),                     # distance 0 everywhere: all ties
        "grid3x3": ([(30 * (k % 3), 20 * (k // 3)) for k in range(9)], [(40, 28)] * 9),       # many equal centre distances
        # 16 frames in a sweep like config 3's at seam scale: ~105 px a step, frames ~436 wide, small jitter -> 54 overlapping pairs
        "ring16": ([(105 * i + (7 * i) % 5 - 2, (5 * i) % 7 - 3) for i in range(16)], [(436 + i % 3, 246 + i % 4) for i in range(16)]),
        "negative": ([(-100, -50), (-90, -45), (-130, -70), (-5, -5), (-101, -51)], [(30, 20), (30, 20), (45, 30), (10, 10), (1, 1)]),
    }
    rng = np.random.default_rng(20241)
    for k in range(200):
        n = int(rng.integers(2, 13))
        sizes = [(int(rng.integers(1, 65)), int(rng.integers(1, 65))) for _ in range(n)]
        corners = [(int(rng.integers(-60, 61)), int(rng.integers(-60, 61))) for _ in range(n)]
        out["random%03d" % k] = (corners, sizes)
    return out


LAYOUTS = _layouts()


def _levels(pairs, n):
    """The level rule: 1 + the highest level among the earlier pairs that share an image."""
    last, levels = [0] * n, []
    for i, j in pairs:
        levels.append(max(last[i], last[j]) + 1)
        last[i] = last[j] = levels[-1]
    return levels, max(levels, default=0)


def _expected(corners, sizes, order):
    """-> ([(i, j, level, x0, y0, x1, y1)], level count) from the references' pair lists"""
    rois = {(i, j): (x, y, x + w, y + h) for i, j, (x, y, w, h) in gc.pair_list(corners, sizes)}
    if order == "run":
        pairs = list(rois)       # pair_list's own order
    else:
        pairs = [p for p in dp.pair_order(corners, sizes, tie_order="reversed")[0] if p in rois]
    levels, nlevels = _levels(pairs, len(sizes))
    return [(i, j, lv) + rois[(i, j)] for (i, j), lv in zip(pairs, levels)], nlevels


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """(layout name, order) -> (rows, level count) as the program printed them: one build, one run over every layout"""
    exe = str(tmp_path_factory.mktemp("seam_plan") / "seam_plan_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tools", "micro", "seam_plan_dump.cpp"), "-o", exe], check=True)
    keys = [(name, order) for name in LAYOUTS for order in ("run", "distance")]
    text = []
    for name, order in keys:
        corners, sizes = LAYOUTS[name]
        text.append("%s %d" % (order, len(sizes)))
        text += ["%d %d %d %d" % (c[0], c[1], s[0], s[1]) for c, s in zip(corners, sizes)]
    r = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out, lines = {}, iter(r.stdout.splitlines())
    for key in keys:
        head = next(lines).split()
        assert head[0] == "plan"
        out[key] = ([tuple(int(v) for v in next(lines).split()) for _ in range(int(head[1]))], int(head[2]))
    assert next(lines, None) is None
    return out


@pytest.mark.parametrize("order", ["run", "distance"])
def test_plan_equals_the_references(plans, order):
    for name, (corners, sizes) in LAYOUTS.items():
        want_rows, want_levels = _expected(corners, sizes, order)
        rows, nlevels = plans[(name, order)]
        assert rows == want_rows, (name, order)
        assert nlevels == want_levels, (name, order)


def test_layouts_reach_their_regimes(plans):
    """The layouts are what they are meant to be: empty plans, edge contact that is no pair, ties, several levels."""
    for name in ("n0", "n1", "n2_disjoint"):
        assert plans[(name, "run")] == ([], 0) and plans[(name, "distance")] == ([], 0)
    assert plans[("n2", "run")] == ([(0, 1, 1, 12, 5, 20, 10)], 1)
    touching = {(r[0], r[1]) for r in plans[("touching", "run")][0]}
    assert touching == {(0, 4), (1, 4), (2, 4), (3, 4)}       # the four quadrants meet only the small frame over their common corner
    assert len(plans[("inside", "run")][0]) == 3
    for name in ("identical", "grid3x3"):
        corners, sizes = LAYOUTS[name]
        dist = dp.pair_order(corners, sizes)[1]
        assert len(set(dist.values())) < len(dist) / 2, name      # equal centre distances
    assert len(set(dp.pair_order(*LAYOUTS["identical"])[1].values())) == 1
    # the two orders differ where distances do, and the plan has as many pairs either way
    assert [r[:2] for r in plans[("ring16", "run")][0]] != [r[:2] for r in plans[("ring16", "distance")][0]]
    assert len(plans[("ring16", "run")][0]) == len(plans[("ring16", "distance")][0]) == 54
    assert plans[("ring16", "run")][1] > 1 and plans[("ring16", "distance")][1] > 1
    # side by side: some level of the ring holds more than one pair
    levels = [r[2] for r in plans[("ring16", "distance")][0]]
    assert max(levels.count(lv) for lv in set(levels)) > 1
