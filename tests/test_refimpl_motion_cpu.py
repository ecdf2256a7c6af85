"""Camera refinement against the independent reading of tests/refimpl_motion.py, without a GPU: the oracle (oracle/mo_motion.c,
mo_match.c), the library's bundle-adjustment host code through tests/harness/ba_host_harness.cpp, and the library's
mis_wave_correct / mis_leave_biggest_component_conf, which need no device.  Every bundle-adjustment case also requires the harness
and the oracle to agree bit for bit: the twin check of test_motion_host_cpu.py on loop closures, isolated cameras, two components,
n = 17, every mask.  Run with -s for the measured ratios (DESIGN.md section 2 quotes them)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import refimpl_motion as rm

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = "/opt/rocm/bin/hipcc"
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not present")
    so = str(tmp_path_factory.mktemp("ba") / "libbaharness.so")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-x", "hip",
                        os.path.join(HERE, "harness", "ba_host_harness.cpp"), "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return C.CDLL(so)


def run_harness(lib, scene, tab, start, thr, mask):
    """-> (return code, cameras) of the library's host code on host keypoints."""
    from image_stitching_amd import _capi as capi
    n = scene["n"]
    keep = []
    fa = (capi.MisFeatures * n)()
    for i, xy in enumerate(scene["xy"]):
        kp = np.zeros(len(xy), KP)
        kp["x"], kp["y"] = xy[:, 0], xy[:, 1]
        keep.append(kp)
        fa[i].img_idx, fa[i].img_w, fa[i].img_h, fa[i].n = i, rm.W, rm.H, len(kp)
        fa[i].keypoints = kp.ctypes.data
    mis = (capi.MisMatchesInfo * (n * n))()
    for k, m in enumerate(tab):
        mm = np.ascontiguousarray(m["matches"])
        mk = np.ascontiguousarray(m["inliers_mask"], np.uint8)
        keep += [mm, mk]
        mis[k].src_img_idx, mis[k].dst_img_idx, mis[k].n_matches = int(m["src_img_idx"]), int(m["dst_img_idx"]), len(mm)
        mis[k].matches = C.cast(mm.ctypes.data, C.POINTER(capi.MisDMatch)) if len(mm) else None
        mis[k].inliers_mask = C.cast(mk.ctypes.data, C.POINTER(C.c_uint8)) if len(mk) else None
        mis[k].num_inliers, mis[k].has_H, mis[k].confidence = int(m["num_inliers"]), 1 if m["has_H"] else 0, float(m["confidence"])
        if m["has_H"]:
            for q, v in enumerate(np.asarray(m["H"], np.float64).reshape(9)):
                mis[k].H[q] = v
    cams = (capi.MisCameraParams * n)()
    for k, c in enumerate(start):
        cams[k].focal, cams[k].aspect, cams[k].ppx, cams[k].ppy = c["focal"], c["aspect"], c["ppx"], c["ppy"]
        for q, v in enumerate(np.asarray(c["R"], np.float64).reshape(9)):
            cams[k].R[q] = v
    rc = lib.dbg_bundle_adjust(fa, mis, n, C.c_float(thr), mask.encode(), cams)
    return rc, [dict(focal=cams[k].focal, aspect=cams[k].aspect, ppx=cams[k].ppx, ppy=cams[k].ppy, R=np.array(list(cams[k].R)).reshape(3, 3)) for k in range(n)]


def run_oracle(oracle, scene, tab, start, thr, mask):
    feats = [dict(img_w=rm.W, img_h=rm.H, xy=xy, desc=np.zeros((len(xy), 32), np.uint8)) for xy in scene["xy"]]
    return oracle.bundle_adjust_reproj(feats, tab, start, thr, mask)


def same_bits(a, b):
    return all(np.array_equal(rm._bits(x["R"]), rm._bits(y["R"])) and all(np.array_equal(rm._bits(x[k]), rm._bits(y[k])) for k in rm.INTR) for x, y in zip(a, b))


def report(tag, name, mask, res):
    print("%s %-11s %s excess %+.3e  /Y %+8.3f  /E %+.2e  raw excess %+.3e (Y raw %+.3e)  parameters / bound %s  cond %.3g" % (
        tag, name, mask, res["excess"], res["over_Y"], res["over_E"], res["raw_excess"], res["Y_raw"],
        "cost only" if res["par_ratio"] is None else "%.3f" % res["par_ratio"], res["cond"]))


@pytest.mark.parametrize("name,mask,eligible", rm.BA_CASES, ids=["%s-%s%s" % (n, m, "" if e else "-cost-only") for n, m, e in rm.BA_CASES])
def test_bundle_adjustment_reaches_the_reference_minimum(harness, oracle_mod, name, mask, eligible):
    scene = rm.get_scene(name)
    tab = rm.table(scene)
    ref = rm.get_reference(name, mask)
    want, iters = run_oracle(oracle_mod, scene, tab, scene["start"], rm.THR, mask)
    rc, got = run_harness(harness, scene, tab, scene["start"], rm.THR, mask)
    assert rc == 0
    print("\n    LM iterations %d, %d observations" % (iters, ref["n_obs"]))
    report("    oracle ", name, mask, rm.check_ba(ref, want, eligible))
    report("    library", name, mask, rm.check_ba(ref, got, eligible))
    assert same_bits(got, want), "the library's host code and the oracle differ in some bit"


def test_skew_position_of_the_mask_has_no_effect(harness, oracle_mod):
    for name in ("chain5", "loop8"):
        scene = rm.get_scene(name)
        tab = rm.table(scene)
        a, _ = run_oracle(oracle_mod, scene, tab, scene["start"], rm.THR, "xxxxx")
        b, _ = run_oracle(oracle_mod, scene, tab, scene["start"], rm.THR, "x_xxx")
        assert same_bits(a, b)
        assert same_bits(run_harness(harness, scene, tab, scene["start"], rm.THR, "x_xxx")[1], a)


def test_long_run_case_runs_long(oracle_mod):
    """`____x` from the standard start is the long Levenberg-Marquardt run; a solver cut short there fails the cost bound."""
    scene = rm.get_scene("chain5")
    iters = run_oracle(oracle_mod, scene, rm.table(scene), scene["start"], rm.THR, "____x")[1]
    print("iterations", iters)
    assert iters >= 8


def test_refused_input(harness, oracle_mod):
    scene = rm.get_scene("chain5")
    tab = rm.table(scene)
    assert rm.reference_ba(scene, tab, 1e9, "xxxxx") is None
    assert run_harness(harness, scene, tab, scene["start"], 1e9, "xxxxx")[0] != 0                 # no pair above the threshold
    with pytest.raises(RuntimeError):
        run_oracle(oracle_mod, scene, tab, scene["start"], 1e9, "xxxxx")
    bad = [dict(m) for m in tab]
    mm = bad[1]["matches"].copy()
    mm["train_idx"][3] = len(scene["xy"][1])                                                      # one past the last keypoint of image 1
    bad[1]["matches"] = mm
    assert run_harness(harness, scene, bad, scene["start"], rm.THR, "xxxxx")[0] != 0
    mm = bad[1]["matches"].copy()
    mm["train_idx"][3], mm["query_idx"][5] = 0, -1
    bad[1]["matches"] = mm
    assert run_harness(harness, scene, bad, scene["start"], rm.THR, "xxxxx")[0] != 0


def test_case_list_shares():
    cost_only = [c for c in rm.BA_CASES if not c[2]]
    assert 4 * len(cost_only) <= len(rm.BA_CASES)
    for name in {c[0] for c in rm.BA_CASES}:
        assert any(c[2] for c in rm.BA_CASES if c[0] == name), name
    for name, mask, eligible in rm.BA_CASES:
        assert eligible == (rm.get_reference(name, mask)["cond"] <= rm.COND_CAP), (name, mask)
    # the scenes are what their names say
    assert rm.get_reference("star", "_____")["centre"] == 3 and rm.get_reference("centre-off", "xxxxx")["centre"] == 1
    assert rm.get_reference("even-path", "_____")["centre"] == 2 and rm.get_reference("no-H", "_____")["centre"] == 2
    assert 2 not in rm.get_reference("iso3", "_____")["in_edge"]
    assert len(set(rm.get_reference("two-comp", "_____")["anchor"])) == 2
    assert (1, 3) not in [(o[0], o[1]) for o in rm.get_reference("conf-equal", "_____")["obs"]]
    n_und = n_all = 0
    for name, Rs, kinds, undecided in rm.wave_cases():
        for kind in kinds:
            n_all += 1
            n_und += rm.wave_correct(Rs, kind)[2] is not None
    assert 10 * n_und <= n_all


# ------------------------------------------------------------------------------------------------ wave correction
_WAVE = [(name, Rs, kind, und) for name, Rs, kinds, und in rm.wave_cases() for kind in kinds]
_flips = {}


@pytest.mark.parametrize("name,Rs,kind,undecided", _WAVE, ids=["%s-%s" % (w[0], "vert" if w[2] else "horiz") for w in _WAVE])
def test_wave_correct_against_the_reference(oracle_mod, name, Rs, kind, undecided):
    import image_stitching_amd as isa
    want, band, reason, info = rm.wave_correct(Rs, kind)
    assert (reason is not None) == undecided, reason
    sides = dict(oracle=oracle_mod.wave_correct(Rs, kind), library=isa.wave_correct(Rs, kind))
    for a, b in zip(sides["oracle"], sides["library"]):
        assert np.array_equal(rm._bits(a), rm._bits(b))
    _flips[(name, kind)] = info["conf"] < 0
    for side, got in sides.items():
        for g in got:
            assert np.array_equal(g, rm.f32(g))
        if reason is not None:
            print("\n    %s undecided: %s; largest |difference| %.3g" % (side, reason, max(np.abs(g - w).max() for g, w in zip(got, want))))
            continue
        worst = max((np.abs(g - w).max(axis=1) / band).max() for g, w in zip(got, want))
        print("\n    %s largest |difference| %.3g, largest difference / band %.3g (rel. gap %.3g, |rg0| / n %.3g, conf %+.3g)" % (
            side, max(np.abs(g - w).max() for g, w in zip(got, want)), worst, info["rel_gap"], info["rg0_over_n"], info["conf"]))
        assert worst <= 1.0
        # Rg of the tested side: orthonormal within the band, relative rotations preserved
        Rg = got[0] @ np.linalg.inv(rm.f32(Rs[0]))
        assert np.abs(Rg @ Rg.T - np.eye(3)).max() <= 2 * np.sqrt(3) * band.max() + 16 * rm.U24
        for i in range(len(Rs) - 1):
            rel_in = np.linalg.inv(rm.f32(Rs[i])) @ rm.f32(Rs[i + 1])
            assert np.abs(np.linalg.inv(got[i]) @ got[i + 1] - rel_in).max() <= 4 * np.sqrt(3) * band.max() + 32 * rm.U24


def test_wave_cases_reach_the_flip():
    cases = {(n, k): rm.wave_correct(Rs, k)[3]["conf"] < 0 for n, Rs, k, _ in _WAVE}
    for kind in (0, 1):
        assert any(v for (n, k), v in cases.items() if k == kind) and any(not v for (n, k), v in cases.items() if k == kind)


def test_wave_correct_edges(oracle_mod):
    import image_stitching_amd as isa
    one = [rm.rot_yxz(10, 20, 30) + 1e-9]
    two = [np.eye(3) + 1e-12, np.diag([1.0, -1.0, -1.0]) - 1e-12]           # sum z = 0 exactly once rounded to float32: nothing is written
    for kind in (0, 1):
        for Rs in (one, two):
            assert rm.wave_correct(Rs, kind)[3]["untouched"]
            for got in (oracle_mod.wave_correct(Rs, kind), isa.wave_correct(Rs, kind)):
                assert all(np.array_equal(rm._bits(g), rm._bits(r)) for g, r in zip(got, Rs))
    with pytest.raises(ValueError):
        rm.wave_correct(two, 2)
    with pytest.raises(isa.MisError):
        isa.wave_correct(two, 2)
    with pytest.raises(RuntimeError):
        oracle_mod.wave_correct(two, -1)


# ------------------------------------------------------------------------------------------------ leaveBiggestComponent
def test_leave_biggest_component(oracle_mod):
    from image_stitching_amd.stitching import leaveBiggestComponentConf
    ties = 0
    for name, conf in rm.lbc_cases():
        want = rm.leave_biggest_component(conf, rm.THR)
        assert [int(i) for i in oracle_mod.leave_biggest_component(conf, rm.THR)] == want, name
        assert [int(i) for i in leaveBiggestComponentConf(conf, rm.THR)] == want, name
        link = ~(conf < rm.THR_D)
        sizes = np.bincount(rm.connected_components(rm.csr_matrix(link | link.T), directed=False)[1])
        ties += int((sizes == sizes.max()).sum() > 1)
    assert ties >= 8                                    # the tie rule is exercised
    # a value on the threshold links (`<` skips), one float32 ulp below does not
    c = np.zeros((3, 3))
    c[0, 2] = rm.THR_D
    c[2, 1] = float(np.nextafter(np.float32(rm.THR), np.float32(0)))
    for f in (rm.leave_biggest_component, oracle_mod.leave_biggest_component, leaveBiggestComponentConf):
        assert [int(i) for i in f(c, rm.THR)] == [0, 2]
