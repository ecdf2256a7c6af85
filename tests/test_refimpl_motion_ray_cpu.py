"""The ray bundle adjuster against the independent reading of tests/refimpl_motion_ray.py, without a GPU: the host twin of
tests/harness/ba_ray_host_harness.cpp (the library's solver and arithmetic headers, the kernels' work in plain loops).  Run with
-s for the measured ratios (DESIGN.md section 8 quotes them)."""
import numpy as np
import pytest

import ba_ray_twin as twin
import refimpl_motion as rm
import refimpl_motion_ray as rr


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    lib = twin.build(tmp_path_factory.mktemp("baray"))
    if lib is None:
        pytest.skip("hipcc not present")
    return lib


@pytest.mark.parametrize("name,eligible", rr.RAY_CASES, ids=[c[0] for c in rr.RAY_CASES])
def test_ray_adjustment_reaches_the_reference_minimum(harness, name, eligible):
    scene = rr.get_ray_scene(name)
    ref = rr.get_ray_reference(name)
    rc, got = twin.run(harness, scene["n"], scene["xy"], rm.table(scene), scene["start"], rm.THR)
    assert rc == 0
    print("\n    %d observations, S* %.6g" % (ref["n_obs"], ref["S"]))
    twin.report("    twin", name, rr.check_ba_ray(ref, got, eligible))


def test_principal_point_and_aspect_are_not_read(harness):
    """K comes from img_w / 2, img_h / 2: a start with ppx, ppy 40 px off and aspect 1.1 gives the same bits, and gets its own
    three fields back."""
    scene = rr.get_ray_scene("chain5")
    tab = rm.table(scene)
    shifted = rr.shifted_start(scene)
    rc0, a = twin.run(harness, scene["n"], scene["xy"], tab, scene["start"], rm.THR)
    rc1, b = twin.run(harness, scene["n"], scene["xy"], tab, shifted, rm.THR)
    assert rc0 == 0 and rc1 == 0 and twin.same_bits(a, b)
    for g, s in zip(b, shifted):
        assert all(np.array_equal(rm._bits(g[k]), rm._bits(s[k])) for k in rr.FIXED)
    rr.check_ba_ray(rr.reference_ba_ray(scene, tab, rm.THR, start=shifted), b, True)


def test_refused_input(harness):
    scene = rr.get_ray_scene("chain5")
    tab = rm.table(scene)
    n = scene["n"]
    assert rr.reference_ba_ray(scene, tab, 1e9) is None
    assert twin.run(harness, n, scene["xy"], tab, scene["start"], 1e9)[0] != 0                     # no pair above the threshold
    bad = [dict(m) for m in tab]
    mm = bad[1]["matches"].copy()
    mm["train_idx"][3] = len(scene["xy"][1])                                                      # one past the last keypoint of image 1
    bad[1]["matches"] = mm
    assert twin.run(harness, n, scene["xy"], bad, scene["start"], rm.THR)[0] != 0
    mm = bad[1]["matches"].copy()
    mm["train_idx"][3], mm["query_idx"][5] = 0, -1                                                # a negative index
    bad[1]["matches"] = mm
    assert twin.run(harness, n, scene["xy"], bad, scene["start"], rm.THR)[0] != 0
    assert twin.run(harness, n, scene["xy"], tab, scene["start"], rm.THR)[0] == 0


def test_ray_case_list():
    for name, eligible in rr.RAY_CASES:
        assert eligible == (rr.get_ray_reference(name)["cond"] <= rm.COND_CAP), name
    # the scenes are what their names say
    assert 2 not in rr.get_ray_reference("iso3")["in_edge"]
    assert len(set(rr.get_ray_reference("two-comp")["anchor"])) == 2
    assert (1, 3) not in [(o[0], o[1]) for o in rr.get_ray_reference("conf-equal")["obs"]]
    assert (0, 2) not in [(o[0], o[1]) for o in rr.get_ray_reference("zero-edge")["obs"]]
    assert [len(o[2]) for o in rr.get_ray_reference("chain5-one")["obs"] if (o[0], o[1]) == (0, 2)] == [1]
    assert max(len(o[2]) for o in rr.get_ray_reference("big3")["obs"]) > 512
    assert rr.get_ray_reference("chain17")["n_obs"] > 0 and rr.get_ray_scene("chain17")["n"] * 4 > 64
    assert rr.get_ray_reference("star")["centre"] == 3 and rr.get_ray_reference("centre-off")["centre"] == 1
