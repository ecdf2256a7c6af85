"""What an AKAZE run (the library on the GPU, or the host emulation of its kernels) is held to against tests/refimpl_akaze.py.
Every stage is judged against the reference's step applied to the run's OWN input of that stage, so rounding never compounds.

A band is the largest difference, on the shapes of cases(), between the reference step in float64 and the same step in float32 with
another summation order (both on the same float32-valued inputs), measured on the CPU by measure_bands() below and multiplied by 4:
a kernel may legitimately contract to FMA and reorder once more.  The measured values stand beside the constants.

Steps 5 and 6 (threshold, eight neighbours, dominance) compare values of the run's own Ldet plane with each other and with the
float32 threshold: those comparisons involve no arithmetic, so they are exact and carry no band; the radius test compares
integer-valued squared distances with r^2 and gets a relative 1e-5.  The refinement's |d| <= 1 carries BAND_D."""
import math

import numpy as np

import refimpl_akaze as ra

# name = 4 * measured                         measured on the CPU (python tests/akaze_check.py)
BAND_LSMOOTH = 4 * 4.85e-07     # Gaussian of the level start (values in [0, 1])
BAND_LT = 4 * 8.41e-07          # the whole FED cycle of a level from its start and flow
BAND_FLOW = 4 * 1.16e-07        # 1 / (1 + |grad|^2 / k^2)
BAND_LXY = 4 * 1.63e-08         # first derivatives at scale sigma_size
BAND_LDET = 4 * 6.82e-09        # determinant of the Hessian, scaled by sigma_size^4
BAND_D = 4 * 1.31e-07           # the refinement's offsets dx, dy (level pixels)
BAND_PT = 4 * 6.1e-05           # pt is stored as float32: four ulps at 512 .. 1024 (the largest coordinate here), beside BAND_D * 2^octave
BAND_ANGLE = 4 * 2.29e-05       # degrees, stored as float32 (an ulp at 256 .. 360 is 3.1e-5)
BAND_GAP = 4 * 5.13e-07         # relative difference of the best two windows' scores below which the angle is not compared
BAND_EDGE = 4 * 4.8e-07         # a sample's angle this close to a window edge (radians) is not compared: float32's ulp at 2 pi, not a measurement
BAND_COORD = 4 * 3.19e-05       # sample coordinates (level pixels): a rounding tie inside it counts both ways
BAND_VALUE = 4 * 2.75e-07       # cell means
# caps: conditions, not measurements
CAP_UNDECIDED_KPS, CAP_UNDECIDED_BITS, CAP_SKIPPED_ANGLES = 0.05, 0.02, 0.02


def rendered(w, h, yaw=40.0, fov=60.0, pitch=3.0):
    import synth
    return synth.render_frame(synth.make_camera(w, h, fov, yaw, pitch))


def cases():
    """The smallest shapes at which each path can go wrong (the frames are the rendered scene the SIFT tests use)."""
    out = [dict(tag="97x71 one octave, odd", frame=rendered(97, 71), kw={}),
           dict(tag="160x96 second octave exactly 80 wide", frame=rendered(160, 96), kw={}),
           dict(tag="159x96 second octave 79 wide: one octave", frame=rendered(159, 96), kw={}),
           dict(tag="333x251 three octaves, fractional area average", frame=rendered(333, 251), kw={}),
           dict(tag="640x320 four octaves, sixteen levels", frame=rendered(640, 320), kw={}),
           dict(tag="333x251 three layers", frame=rendered(333, 251, yaw=75.0), kw=dict(n_octave_layers=3)),
           dict(tag="333x251 threshold 0.01", frame=rendered(333, 251), kw=dict(threshold=0.01)),
           dict(tag="640x320 max_points 50", frame=rendered(640, 320), kw=dict(max_points=50))]
    return out


def ulp_diff32(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _near(tag, name, got, want, band):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert got.shape == want.shape and np.all(np.isfinite(got)), (tag, name, got.shape, want.shape)
    assert d.max() <= band, (tag, name, float(d.max()), band)
    return float(d.max())


def check_planes(tag, frame, kw, run):
    """FED schedules, every plane of every level, the k-contrast.  -> (levels, the largest deviations)"""
    p = ra.params(**kw)
    h, w = frame.shape[:2]
    levels = ra.plan(w, h, p["n_octaves"], p["n_octave_layers"])
    planes = run["planes"]
    assert len(planes) == len(levels), (tag, len(planes), len(levels))
    worst = {}
    k_run = run["counts"]["kcontrast"]
    k_ref, hmax, nz = ra.kcontrast(planes[0]["Lsmooth"])
    if abs(k_ref - k_run) > 1e-6 * k_ref:
        # off by one histogram bin is allowed when a magnitude sits within the band of a bin edge (the Scharr sums of Lsmooth carry
        # 16 times Lsmooth's rounding)
        assert abs(k_ref - k_run) <= hmax / 300 * (1 + 1e-6) and ra.kcontrast_bin_edge_distance(nz, hmax) <= 32 * BAND_LSMOOTH, (tag, "kcontrast", k_ref, k_run)
    for i, lv in enumerate(levels):
        P = planes[i]
        assert P["Lt"].shape == (lv["h"], lv["w"]), (tag, i, P["Lt"].shape)
        if i == 0:
            assert len(run["taus"][0]) == 0
            worst["Lsmooth"] = max(worst.get("Lsmooth", 0), _near(tag, "Lsmooth[0]", P["Lsmooth"], ra.gauss_blur(ra.gray01(frame), 1.6), BAND_LSMOOTH))
            assert np.array_equal(P["Lt"], P["Lsmooth"]), (tag, "Lt[0] is Lsmooth[0]")
        else:
            n, taus, _ = ra.level_schedule(levels, i)
            assert len(run["taus"][i]) == n, (tag, "FED n", i, len(run["taus"][i]), n)
            assert ulp_diff32(run["taus"][i], taus.astype(np.float32)).max() <= 1, (tag, "FED taus", i)
            start = ra.level_start(planes[i - 1]["Lt"], levels[i - 1], lv)
            worst["Lsmooth"] = max(worst.get("Lsmooth", 0), _near(tag, "Lsmooth[%d]" % i, P["Lsmooth"], ra.gauss_blur(start, 1.0), BAND_LSMOOTH))
            worst["Lt"] = max(worst.get("Lt", 0), _near(tag, "Lt[%d]" % i, P["Lt"], ra.diffuse(start, P["flow"], run["taus"][i].astype(np.float64), lv["octave"]), BAND_LT))
        worst["flow"] = max(worst.get("flow", 0), _near(tag, "flow[%d]" % i, P["flow"], ra.flow(P["Lsmooth"], ra.level_k(np.float32(k_run), lv["octave"], np.float32)), BAND_FLOW))
        lx, ly = ra.first_derivatives(P["Lsmooth"], lv["sigma_size"])
        worst["Lxy"] = max(worst.get("Lxy", 0), _near(tag, "Lx[%d]" % i, P["Lx"], lx, BAND_LXY), _near(tag, "Ly[%d]" % i, P["Ly"], ly, BAND_LXY))
        worst["Ldet"] = max(worst.get("Ldet", 0), _near(tag, "Ldet[%d]" % i, P["Ldet"], ra.ldet(P["Lx"], P["Ly"], lv["sigma_size"]), BAND_LDET))
    return levels, worst


def check_keypoints(tag, levels, kw, run):
    """Steps 5 - 8 on the run's own planes.  -> report"""
    p = ra.params(**kw)
    planes, kps, ids = run["planes"], run["kps"], run["class_ids"]
    stats = {}
    ref = ra.keypoints([P["Ldet"] for P in planes], levels, np.float32(p["threshold"]), p["max_points"], 0.0, BAND_D, stats)
    assert run["counts"]["candidates"] == stats.get("candidates", 0), (tag, "candidates", run["counts"], stats)
    assert run["counts"]["suppressed"] == stats.get("suppressed", 0), (tag, "after suppression", run["counts"], stats)
    decided = [k for k in ref if k["state"] == ra.YES]
    undecided = [k for k in ref if k["state"] != ra.YES]
    assert len(undecided) <= CAP_UNDECIDED_KPS * max(len(decided), 1) or not decided and len(undecided) <= 1, (tag, "undecided keypoints", len(undecided), len(decided))
    assert len(kps) == len(ids)
    # the run's keypoints -> the reference's, by level and position
    by_level = {}
    for k in ref:
        by_level.setdefault(k["level"], []).append(k)
    matched, order_keys = [], []
    pt_band = lambda k: BAND_D * levels[k["level"]]["ratio"] + BAND_PT
    for q, l in zip(kps, ids):
        best = None
        for k in by_level.get(int(l), []):
            d = max(abs(k["pt"][0] - q["x"]), abs(k["pt"][1] - q["y"]))
            if d <= pt_band(k) and (best is None or d < best[0]):
                best = (d, k)
        assert best is not None, (tag, "a keypoint beyond decided + undecided", q, int(l))
        k = best[1]
        matched.append(k)
        order_keys.append((k["level"], k["y"], k["x"]))
        assert q["octave"] == k["octave"] and int(l) == k["class_id"], (tag, "octave / class_id", q, k)
        assert abs(q["size"] - k["size"]) <= 1e-6 * k["size"], (tag, "size", q, k)
        assert q["response"] == np.float32(k["response"]), (tag, "response", q, k)
    assert order_keys == sorted(order_keys) and len(set(order_keys)) == len(order_keys), (tag, "(level, y, x) order, no duplicates")
    present = set(order_keys)
    for k in decided:
        assert (k["level"], k["y"], k["x"]) in present, (tag, "a decided keypoint is missing", k)
    if p["max_points"] > 0:
        assert len(kps) <= p["max_points"]
    # angles, on the run's Lx / Ly at the run's own position
    skipped = 0
    for q, l in zip(kps, ids):
        lv, P = levels[int(l)], planes[int(l)]
        ang, gap, edge, tie = ra.orientation(P["Lx"], P["Ly"], lv, (q["x"], q["y"]), q["size"])
        assert 0 <= q["angle"] < 360, (tag, q)
        if gap <= BAND_GAP or edge <= BAND_EDGE or tie <= BAND_COORD:
            skipped += 1
            continue
        d = abs(float(q["angle"]) - ang)
        assert min(d, 360 - d) <= BAND_ANGLE, (tag, "angle", q, ang, gap, edge)
    assert skipped <= max(CAP_SKIPPED_ANGLES * len(kps), 1 if len(kps) < 50 else 0), (tag, "angles skipped", skipped, len(kps))
    return dict(keypoints=len(kps), decided=len(decided), undecided=len(undecided), angles_skipped=skipped)


def check_descriptors(tag, levels, run):
    planes, kps, ids, desc = run["planes"], run["kps"], run["class_ids"], run["desc"]
    assert desc.shape == (len(kps), 61) and desc.dtype == np.uint8
    if not len(kps):
        return dict(bits=0, undecided_bits=0)
    assert not np.any(desc[:, 60] & 0xC0), (tag, "pad bits")
    undecided = 0
    for q, l, row in zip(kps, ids, desc):
        lv, P = levels[int(l)], planes[int(l)]
        vals, lo, hi = ra.mldb_values(P["Lt"], P["Lx"], P["Ly"], lv, (q["x"], q["y"]), q["size"], q["angle"], tie_band=BAND_COORD)
        dec = ra.mldb_decided(lo, hi, 2 * BAND_VALUE)
        want, got = ra.mldb_bits(vals), ra.unpack_bits(row)
        assert np.array_equal(got[dec], want[dec]), (tag, "decided bits differ", q, int(np.sum(got[dec] != want[dec])))
        undecided += int(np.sum(~dec))
    assert undecided <= CAP_UNDECIDED_BITS * 486 * len(kps), (tag, "undecided bits", undecided, 486 * len(kps))
    return dict(bits=486 * len(kps), undecided_bits=undecided)


def check_run(tag, frame, kw, run):
    levels, worst = check_planes(tag, frame, kw, run)
    rep = dict(levels=len(levels), worst=worst)
    rep.update(check_keypoints(tag, levels, kw, run))
    rep.update(check_descriptors(tag, levels, run))
    return rep


def reference_run(frame, kw, dt=np.float32, alt=True):
    """The reference itself in the form of a run (float32 planes, another summation order): what check_run must accept."""
    p = ra.params(**kw)
    levels, planes, k0, kps = ra.detect(frame, dt, alt, **p)
    stats = {}
    ra.keypoints([P["Ldet"] for P in planes], levels, np.float32(p["threshold"]), p["max_points"], stats=stats)
    out = np.zeros(len(kps), [("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
    for q, k in zip(out, kps):
        q["x"], q["y"], q["size"], q["angle"], q["response"], q["octave"] = k["pt"][0], k["pt"][1], k["size"], k["angle"], k["response"], k["octave"]
    # the descriptors of the keypoints as stored (float32 fields), as a run computes them
    desc = np.zeros((len(kps), 61), np.uint8)
    for i, (q, k) in enumerate(zip(out, kps)):
        P = planes[k["level"]]
        desc[i] = ra.pack_bits(ra.mldb_bits(ra.mldb_values(P["Lt"], P["Lx"], P["Ly"], levels[k["level"]], (q["x"], q["y"]), q["size"], q["angle"], dt, alt)[0]))
    taus = [np.zeros(0, np.float32)] + [ra.level_schedule(levels, i)[1].astype(np.float32) for i in range(1, len(levels))]
    return dict(planes=[{k: v.astype(np.float32) for k, v in P.items()} for P in planes], taus=taus,
                counts=dict(candidates=stats.get("candidates", 0), suppressed=stats.get("suppressed", 0), refined=len(kps), kcontrast=float(np.float32(k0))),
                kps=out, class_ids=np.array([k["class_id"] for k in kps], np.int32), desc=desc)


# ------------------------------------------------------------------------------------------------ the bands
def measure_bands():
    """The float64 reference against its float32 / other-order self, step by step on float32-valued inputs, over cases()."""
    f32, f64 = np.float32, np.float64
    m = {}

    def upd(name, a, b):
        m[name] = max(m.get(name, 0.0), float(np.max(np.abs(np.asarray(a, f64) - np.asarray(b, f64)))) if np.size(a) else 0.0)
    for c in cases():
        frame, p = c["frame"], ra.params(**c["kw"])
        levels, planes, k0, kps = ra.detect(frame, **p)
        P32 = [{k: v.astype(f32) for k, v in P.items()} for P in planes]
        upd("Lsmooth", ra.gauss_blur(ra.gray01(frame), 1.6), ra.gauss_blur(ra.gray01(frame, f32), 1.6, f32, True))
        for i, lv in enumerate(levels):
            P = P32[i]
            if i:
                s64 = ra.level_start(P32[i - 1]["Lt"], levels[i - 1], lv)
                s32 = ra.level_start(P32[i - 1]["Lt"], levels[i - 1], lv, f32, True)
                upd("Lsmooth", ra.gauss_blur(s64, 1.0), ra.gauss_blur(s32, 1.0, f32, True))
                taus = ra.level_schedule(levels, i)[1].astype(f32)
                upd("Lt", ra.diffuse(s64, P["flow"], taus.astype(f64), lv["octave"]), ra.diffuse(s32, P["flow"], taus, lv["octave"], f32, True))
            k = ra.level_k(f32(k0), lv["octave"], f32)
            upd("flow", ra.flow(P["Lsmooth"], k), ra.flow(P["Lsmooth"], k, f32, True))
            a, b = ra.first_derivatives(P["Lsmooth"], lv["sigma_size"]), ra.first_derivatives(P["Lsmooth"], lv["sigma_size"], f32, True)
            upd("Lxy", a[0], b[0]); upd("Lxy", a[1], b[1])
            upd("Ldet", ra.ldet(P["Lx"], P["Ly"], lv["sigma_size"]), ra.ldet(P["Lx"], P["Ly"], lv["sigma_size"], f32, True))
        for k in kps:
            lv, P = levels[k["level"]], P32[k["level"]]
            upd("d", ra.refine(P["Ldet"], k["x"], k["y"]), ra.refine(P["Ldet"], k["x"], k["y"], f32, True))
            pt, size = (f32(k["pt"][0]), f32(k["pt"][1])), f32(k["size"])
            a64 = ra.orientation(P["Lx"], P["Ly"], lv, pt, size)
            a32 = ra.orientation(P["Lx"], P["Ly"], lv, pt, size, f32, True)
            if a64[1] > 1e-3 and a64[2] > 1e-4:      # the same window, the same samples: the arithmetic's difference alone
                d = abs(a64[0] - float(f32(a32[0])))
                upd("angle", min(d, 360 - d), 0.0)
            upd("gap", abs(a64[1] - a32[1]), 0.0)
            # sample coordinates and angles
            r = lv["ratio"]
            s = float(ra.fround(0.5 * float(size) / r))
            ang = math.radians(a64[0])
            co, si = math.cos(ang), math.sin(ang)
            for kk in (-10.0, 10.0):
                for ll in (-10.0, 10.0):
                    x64 = float(pt[0]) / r + (-ll * si + kk * co) * s
                    x32 = f32(pt[0]) / f32(r) + (f32(kk) * f32(co) - f32(ll) * f32(si)) * f32(s)
                    upd("coord", x64, x32)
            v64 = ra.mldb_values(P["Lt"], P["Lx"], P["Ly"], lv, pt, size, f32(a64[0]), tie_band=1e-3)
            v32 = ra.mldb_values(P["Lt"], P["Lx"], P["Ly"], lv, pt, size, f32(a64[0]), f32, True)
            same = np.all(v64[1] == v64[2], axis=1)      # cells with no sample near a rounding tie
            upd("value", v64[0][same], v32[0][same])
    return m


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # the synth package
    for k, v in measure_bands().items():
        print("%-8s %.3g" % (k, v))
