"""The panorama mode without cameras (cv::Stitcher::create(PANORAMA): HomographyBasedEstimator, BundleAdjusterRay, wave correction)
end to end on the two rendered scenes of tests/refimpl_estimator.py: Stitcher.create_panorama(...).stitch(frames); the estimator
on the device's match table against the float64 reference; the ray cost from the estimate to the adjusted cameras and at the
truth; the same composition assembled from the single calls; estimate_transform + compose_panorama; the C++ driver's
--estimator homography.

Recorded on the MI355X (printed by the tests, not asserted), adjusted median focal against truth and the adjacent pairs' rotation
errors before -> after the adjustment: see DESIGN.md section 8, "panorama mode without cameras"."""
import os
import subprocess

import numpy as np
import pytest

import refimpl_estimator as re_
import refimpl_motion as rm
import refimpl_motion_ray as rr
from test_refimpl_estimator_cpu import lib_candidates

pytestmark = pytest.mark.gpu

_runs = {}


def _run(ctx, name, **overrides):
    """-> (stitcher, device frames, pano, mask, features, matches, kept indices) of one stitch without cameras; run once."""
    import torch
    import image_stitching_amd as isa
    key = (name, tuple(sorted(overrides.items())))
    if key not in _runs:
        w, h, cams, host = re_.scene(name)
        frames = [torch.from_numpy(f).cuda() for f in host]
        st = isa.Stitcher.create_panorama(ctx, (w, h), **overrides)
        pano, mask, feats, pm, idx = st.stitch(frames)
        ctx.synchronize()
        _runs[key] = (st, frames, pano, mask, feats, pm, idx)
    return _runs[key]


def _xy(feats):
    return [np.stack([k["x"], k["y"]], 1).astype(np.float32) for k, _ in (f.download() for f in feats)]


def truth_cameras(cams, centre, size):
    """The scene's cameras as the adjuster returns its own: focal, the image centre, rotations relative to the tree's centre."""
    Rc = np.asarray(cams[centre]["R"], np.float64)
    return [dict(focal=float(c["f"]), aspect=1.0, ppx=0.5 * size[0], ppy=0.5 * size[1], R=Rc.T @ np.asarray(c["R"], np.float64)) for c in cams]


def adjacent_errors(got, cams):
    """Rotation error of every adjacent pair (i, i + 1) against the truth, degrees; the rotations projected on SO(3)."""
    return [re_.angle_deg(np.asarray(cams[i]["R"]).T @ np.asarray(cams[i + 1]["R"]),
                          re_.project_so3(np.linalg.inv(np.asarray(got[i]["R"], np.float64)) @ np.asarray(got[i + 1]["R"], np.float64))) for i in range(len(cams) - 1)]


def ray_checks(name, est, adj, xy, tab, cams, size, conf_thresh):
    """The ray-cost assertions on the estimated and the adjusted cameras of one table."""
    n = len(cams)
    ref = rr.reference_ba_ray(dict(name="panorama-" + name, n=n, xy=xy, start=est), tab, conf_thresh, size=size)
    obs = ref["obs"]
    s_est, s_adj = rr.cost(rm.projected(est), obs, size), rr.cost(rm.projected(adj), obs, size)
    s_truth = rr.cost(truth_cameras(cams, ref["centre"], size), obs, size)
    focals = sorted(c["focal"] for c in adj)
    print("\n    scene %s: S estimated %.2f adjusted %.2f reference minimum %.2f truth %.2f over %d observations (slack %.2e)"
          % (name, s_est, s_adj, ref["S"], s_truth, ref["n_obs"], ref["slack"]))
    print("    median focal estimated %.2f adjusted %.2f true %.2f; adjacent pairs off by %s -> %s degrees"
          % (est[0]["focal"], focals[n // 2] if n % 2 else 0.5 * (focals[n // 2 - 1] + focals[n // 2]), cams[0]["f"],
             ", ".join("%.3f" % e for e in adjacent_errors(est, cams)), ", ".join("%.3f" % e for e in adjacent_errors(adj, cams))))
    assert s_adj <= s_est, "the adjuster raised the ray cost"
    res = rr.check_ba_ray(ref, adj, ref["cond"] <= rm.COND_CAP)
    print("    excess %+.3e  /E %+.2e  parameters / bound %s  cond %.3g" % (res["excess"], res["over_E"], res["par_ratio"], ref["cond"]))
    assert s_truth >= s_adj - ref["slack"], ("the truth costs less than the adjusted cameras: the adjuster is in another basin", s_truth, s_adj)
    return ref


@pytest.mark.parametrize("name", ["A", "B"])
def test_panorama_mode_stitches_without_cameras(ctx, name):
    import image_stitching_amd as isa
    w, h, cams, _ = re_.scene(name)
    n = len(cams)
    st, frames, pano, mask, feats, pm, idx = _run(ctx, name)
    assert st.cfg.matcher_type == "homography" and st.cfg.wave_correct == "horiz" and st.kind == isa.WARP_SPHERICAL
    assert [int(i) for i in idx] == list(range(n)) == st.indices
    # the estimator on the device's table against the float64 reference on that table
    tab = re_.table_of(pm)
    for k in range(n * n):
        if tab[k]["has_H"]:
            got, want = isa.focals_from_homography(tab[k]["H"]), re_.focals_from_homography(tab[k]["H"])
            assert got[2:] == want[2:] and np.array_equal(rm._bits(got[:2]), rm._bits(want[:2])), (divmod(k, n), got, want)
    ref = re_.estimate_cameras(n, tab, [(w, h)] * n)
    cand = lib_candidates(n, tab)
    assert len(cand) == len(ref["candidates"]) and np.array_equal(rm._bits(cand), rm._bits(ref["candidates"])), (cand, ref["candidates"])
    assert np.array_equal(rm._bits(isa.estimate_focal(pm, (w, h))), rm._bits([ref["focal"]] * n))
    worst = re_.check_cameras(ref, isa.estimate_homography_cameras(pm, (w, h)), [(w, h)] * n)
    ratio, errs = re_.scene_conditions(ref, cams[0]["f"], [c["R"] for c in cams])
    print("\n    scene %s: %d candidates, median focal %.2f (true %.2f, ratio %.3f), tree edges off by %s degrees, rotations / bound %.3f"
          % (name, len(ref["candidates"]), ref["focal"], cams[0]["f"], ratio, ", ".join("%.2f" % e for e in errs), worst))
    # the panorama shows the sweep: wider than a frame by a good part of the yaw range (12 of the 60 degrees per step), its mask mostly set
    assert pano.shape[1] > w + 0.4 * (n - 1) * 12.0 / 60.0 * w and float((mask > 0).float().mean()) > 0.6


@pytest.mark.parametrize("name", ["A", "B"])
def test_ray_adjuster_from_the_estimated_start(ctx, name):
    import image_stitching_amd as isa
    w, h, cams, _ = re_.scene(name)
    st, frames, pano, mask, feats, pm, idx = _run(ctx, name)
    est = isa.estimate_homography_cameras(pm, (w, h))
    adj = isa.bundle_adjust_ray(ctx, feats, pm, est, st.cfg.conf_thresh)
    ray_checks(name, est, adj, _xy(feats), re_.table_of(pm), cams, (w, h), st.cfg.conf_thresh)


def _assemble(ctx, st, frames, feats, pm):
    """The composition from the single calls at the Stitcher's scales: estimate_homography_cameras, bundle_adjust_ray, wave_correct,
    the seam-scale step where configured, warp_fused of the configured warper and the configured blender
    -> (pano, mask, the cameras composed from)."""
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as s
    cfg, (W, H) = st.cfg, st.frame_size
    est = isa.estimate_homography_cameras(pm, st.work_size)
    adj = isa.bundle_adjust_ray(ctx, feats, pm, est, cfg.conf_thresh)
    Rs = [c["R"] for c in adj]
    if cfg.wave_correct != "no":
        Rs = isa.wave_correct(Rs, s.WAVE_CORRECT_VERT if cfg.wave_correct == "vert" else s.WAVE_CORRECT_HORIZ)
    cams = [dict(K=np.array([[c["focal"], 0, c["ppx"]], [0, c["focal"] * c["aspect"], c["ppy"]], [0, 0, 1]], np.float64), R=np.asarray(R, np.float32))
            for c, R in zip(adj, Rs)]
    work = cams
    scale = isa.Stitcher.warped_image_scale(cams)
    g = s.compose_geometry(cfg, (W, H), scale, st.work_scale)
    seam = None
    if cfg.expos_comp_type != "no" or cfg.seam_find_type != "no":
        items = [s.seam_scale_warp(ctx, cfg, (W, H), f, c, scale, st.work_scale) for f, c in zip(frames, cams)]
        seam = s.seam_solve(ctx, cfg, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items])
    if g.aspect != 1.0:
        cams = [s.scaled_camera(c, g.aspect) for c in cams]
    assert g.size == (W, H)         # compose_megapix -1: frames at full resolution
    warper = s.make_warper(ctx, g.warp_scale, cfg.warp_type)
    rois = [warper.warp_roi((W, H), c["K"], c["R"]) for c in cams]
    corners, sizes = [(r[0], r[1]) for r in rois], [(r[2], r[3]) for r in rois]
    x, y, pw, ph = isa.result_roi(corners, sizes)
    btype, bands, sharp = isa.blend_config(cfg.blend_type, cfg.blend_strength, (pw, ph))
    assert btype == isa.BLEND_MULTI_BAND
    blender = isa.MultiBandBlender(ctx, bands)
    blender.prepare(corners, sizes)
    for k, (f, c, roi) in enumerate(zip(frames, cams, rois)):
        tl, img_s, mask = warper.warp_fused(f, c["K"], c["R"], roi)
        if seam is not None:
            if seam[0] is not None:
                seam[0].apply(k, corners[k], img_s, mask)
            isa.seam_mask_apply(ctx, seam[1][k], mask)
        blender.feed(img_s, mask, tl)
    pano, mask = blender.blend()
    return pano, mask, work


@pytest.mark.parametrize("name,overrides", [("A", {}), ("B", {}), ("A", dict(work_megapix=0.1)),
                                            ("B", dict(warp_type="cylindrical", expos_comp_type="gain_blocks", seam_find_type="dp_color"))],
                         ids=["A", "B", "A-work0.1", "B-cylindrical-gain_blocks-dp_color"])
def test_panorama_equals_the_composition_from_single_calls(ctx, name, overrides):
    import torch
    w, h, cams, _ = re_.scene(name)
    n = len(cams)
    st, frames, pano, mask, feats, pm, idx = _run(ctx, name, **overrides)
    assert [int(i) for i in idx] == list(range(n))
    if "work_megapix" in overrides:
        assert st.work_scale < 1.0 and st.work_size != (w, h) and st.cameras[0]["K"][0, 2] == 0.5 * st.work_size[0]
    for k, v in overrides.items():
        assert getattr(st.cfg, k) == v
    apano, amask, work = _assemble(ctx, st, frames, feats, pm)
    ctx.synchronize()
    assert torch.equal(pano, apano) and torch.equal(mask, amask)
    for i in range(n):
        assert np.array_equal(rm._bits(st.cameras[i]["K"]), rm._bits(work[i]["K"])) and np.array_equal(st.cameras[i]["R"], work[i]["R"])
        assert st.cameras[i]["R"].dtype == np.float32


def test_estimate_transform_then_compose_panorama(ctx):
    import torch
    import image_stitching_amd as isa
    w, h, cams, host = re_.scene("B")
    st, frames, pano, mask, feats, pm, idx = _run(ctx, "B")
    st2 = isa.Stitcher.create_panorama(ctx, (w, h))
    f2, pm2, idx2 = st2.estimate_transform(frames)
    assert st2.indices == [0, 1, 2] and sorted(st2.cameras) == [0, 1, 2]
    p2, m2 = st2.compose_panorama(frames)
    ctx.synchronize()
    assert torch.equal(p2, pano) and torch.equal(m2, mask)
    # a second frame set of the same rig: composed from the kept registration, no finder or matcher call
    seq = ctx.lib.mis_match_sequence(ctx.h)

    def refuse(*a, **k):
        raise AssertionError("compose_panorama ran the finder or the matcher")
    st2.features = st2.match = refuse
    kept = {i: dict(c) for i, c in st2.cameras.items()}
    dimmed = [(f.to(torch.float32) * 0.8).to(torch.uint8) for f in frames]
    p3, m3 = st2.compose_panorama(dimmed)
    ctx.synchronize()
    assert ctx.lib.mis_match_sequence(ctx.h) == seq
    assert p3.shape == pano.shape and torch.equal(m3, mask) and not torch.equal(p3, pano)
    assert all(np.array_equal(kept[i]["R"], st2.cameras[i]["R"]) and np.array_equal(kept[i]["K"], st2.cameras[i]["K"]) for i in kept)
    assert float(p3[m3 > 0].float().mean()) < 0.9 * float(pano[mask > 0].float().mean())


def test_stitch_main_estimator_homography(ctx, tmp_path):
    """stitch_main <dir> --estimator homography --ba ray with no camera files: the Python mode's panorama byte for byte and its
    cameras in cams.data; the refused estimator names; a run without --estimator and without camera files fails as before."""
    from image_stitching_amd import serializer as ser
    from test_host_cpp import HOST, _build
    _build()
    w, h, cams, host = re_.scene("B")
    n = len(cams)
    tmp = str(tmp_path)
    for i, f in enumerate(host):
        with open(os.path.join(tmp, "%d.ppm" % (i + 1)), "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (w, h))
            fh.write(f[:, :, ::-1].tobytes())
    exe = os.path.join(HOST, "stitch_main")
    r = subprocess.run([exe, tmp, "--estimator", "homography", "--ba", "ray"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    st, frames, pano, mask, feats, pm, idx = _run(ctx, "B")
    assert ser.deserializeIndices(os.path.join(tmp, "indices.data")) == list(range(n))
    ser.serializeCameraParams([dict(st.cameras[i]["params"], R=np.asarray(st.cameras[i]["R"], np.float32)) for i in range(n)], os.path.join(tmp, "cams_py.data"))
    assert open(os.path.join(tmp, "cams.data")).read() == open(os.path.join(tmp, "cams_py.data")).read()
    with open(os.path.join(tmp, "result.ppm"), "rb") as fh:
        assert fh.readline() == b"P6\n"
        pw, ph = [int(v) for v in fh.readline().split()]
        assert fh.readline() == b"255\n"
        got = np.frombuffer(fh.read(), np.uint8).reshape(ph, pw, 3)
    want = np.clip(pano.cpu().numpy(), 0, 255).astype(np.uint8)[:, :, ::-1]
    assert got.shape == want.shape and np.array_equal(got, want)
    for bad in ("affine", "nonsense"):
        r = subprocess.run([exe, tmp, "--estimator", bad], capture_output=True, text=True)
        assert r.returncode != 0 and ("'%s'" % bad) in r.stdout, (bad, r.stdout)
    assert "scans" in subprocess.run([exe, tmp, "--estimator", "affine"], capture_output=True, text=True).stdout
    r = subprocess.run([exe, tmp], capture_output=True, text=True)
    assert r.returncode != 0 and "Can't open camera description" in r.stdout


def test_refusals_leave_the_context_usable(ctx):
    import torch
    import synth
    import image_stitching_amd as isa
    w, h, cams, host = re_.scene("B")
    n = len(cams)
    st, frames, pano, mask, feats, pm, idx = _run(ctx, "B")
    with pytest.raises(ValueError, match="estimator is set"):
        st.stitch(frames, [dict(K=c["K"], R=c["R"]) for c in cams])
    # two frames that look at unrelated parts of the scene: the pruning keeps fewer than two
    far = synth.render_frame(synth.make_camera(w, h, 60.0, 150.0, 35.0, 0.0))
    st2 = isa.Stitcher.create_panorama(ctx, (w, h))
    st2.estimate_transform(frames)
    assert st2.indices == list(range(n))
    with pytest.raises(ValueError, match="Need more images"):
        st2.stitch([frames[0], torch.from_numpy(np.ascontiguousarray(far)).cuda()])
    # the failed call leaves no registration: the earlier one is not silently composed from
    assert st2.indices is None and st2.cameras is None
    with pytest.raises(ValueError, match="estimate_transform has not run"):
        st2.compose_panorama(frames)
    # a good call on the same context and the same stitcher gives the bytes it gave
    pano2, mask2, _, _, idx2 = st2.stitch(frames)
    ctx.synchronize()
    assert [int(i) for i in idx2] == list(range(n)) and torch.equal(pano2, pano) and torch.equal(mask2, mask)


def test_cpp_jobs_refuse_estimated_cameras(tmp_path):
    """mis::StitchJob and mis::ShardedJob (one shared JobCore; host/stitch_bench --estimator) run supplied cameras only: "homography"
    is refused by name as mis::Stitcher's, "affine" and a name that is no estimator as mis::Stitcher refuses them."""
    from test_host_cpp import HOST, _build, write_cams_file
    _build()
    cams_path = str(tmp_path / "cams.txt")
    write_cams_file(cams_path, re_.scene("B")[2])
    exe = os.path.join(HOST, "stitch_bench")
    for flow in ([], ["--comm", "host"]):      # mis::StitchJob; mis::ShardedJob on one rank
        for name, text in (("homography", "runs supplied cameras only; estimator_type 'homography' is mis::Stitcher's"),
                           ("affine", "estimator_type 'affine': AffineBasedEstimator runs in mode = \"scans\""),
                           ("nonsense", "estimator_type 'nonsense': 'supplied' or 'homography'")):
            r = subprocess.run([exe, cams_path, "--steps", "1", "--warmup", "0", "--estimator", name] + flow, capture_output=True, text=True, timeout=120)
            assert r.returncode == 1 and text in r.stdout, (flow, name, r.stdout + r.stderr)
