"""ba_cost_func = "ray" through the jobs: the 640 x 360 five-camera job of test_motion_gpu.py from perturbed cameras, its sharded
path, the C++ driver's --ba ray, and the configuration's refusals."""
import os
import subprocess

import numpy as np
import pytest

import refimpl_motion as rm
import refimpl_motion_ray as rr

W, H, N = 640, 360, 5


def test_config_names():
    import image_stitching_amd as isa
    assert isa.StitchConfig.hot_path(ba_cost_func="ray").ba_cost_func == "ray"
    with pytest.raises(NotImplementedError, match="affine"):
        isa.StitchConfig.hot_path(ba_cost_func="affine")
    with pytest.raises(ValueError, match="rays"):
        isa.StitchConfig.hot_path(ba_cost_func="rays")


def _params(c):
    return dict(focal=float(c["K"][0, 0]), aspect=float(c["K"][1, 1] / c["K"][0, 0]), ppx=float(c["K"][0, 2]), ppy=float(c["K"][1, 2]), R=np.asarray(c["R"], np.float64))


@pytest.mark.gpu
def test_job_with_ray_refinement_from_perturbed_cameras(ctx, oracle_mod, tmp_path):
    import torch
    import synth
    import image_stitching_amd as isa
    from image_stitching_amd import serializer as ser
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import leaveBiggestComponent, refine_cameras
    from test_host_cpp import HOST, _build, _desc
    exact = [synth.make_camera(W, H, 60.0, 11.0 * i - 22.0, 2.5 * ((i % 3) - 1), 1.5 * ((i % 2) - 0.5)) for i in range(N)]
    host_frames = [synth.render_frame(c) for c in exact]
    frames = {i: torch.from_numpy(f).cuda() for i, f in enumerate(host_frames)}
    rng = np.random.default_rng(9)
    noisy, sensor = [], []
    for c in exact:
        d = dict(c)
        # (through the C++ driver's re-handing of a sensor rotation, so that stitch_main below starts from the same matrices)
        sensor.append(oracle_mod.camera_rehand(synth.rotation_yxz(*np.radians(rng.normal(0, 0.5, 3))) @ c["R"], False))
        d["R"] = oracle_mod.camera_rehand(sensor[-1], False)
        noisy.append(d)
    cfg = isa.StitchConfig.hot_path(ba_cost_func="ray")
    job = StitchJob(ctx, (W, H), noisy, config=cfg)
    out = job.run(frames)
    assert out["indices"] == list(range(N))
    feats, pm = out["features"], out["matches"]
    # the job's cameras = the adjuster + wave correction called directly on the job's own features and matches
    direct = isa.bundle_adjust_ray(ctx, feats, pm, [_params(c) for c in noisy], conf_thresh=cfg.conf_thresh)
    Rs = isa.wave_correct([c["R"] for c in direct], isa.stitching.WAVE_CORRECT_HORIZ)
    for c, d, R, s in zip(job.cams, direct, Rs, noisy):
        assert np.array_equal(rm._bits(c["R"]), rm._bits(R)) and np.array_equal(rm._bits(c["K"][0, 0]), rm._bits(d["focal"]))
        assert c["K"][0, 2] == s["K"][0, 2] and c["K"][1, 2] == s["K"][1, 2]
    # the sharded job's path (match entries gathered, table rebuilt on the host): same cameras, same panorama
    job2 = StitchJob(ctx, (W, H), noisy, config=cfg, force_collectives=True)
    out2 = job2.run(frames)
    for a, b in zip(job.cams, job2.cams):
        assert np.array_equal(rm._bits(a["R"]), rm._bits(b["R"])) and np.array_equal(rm._bits(a["K"]), rm._bits(b["K"]))
    assert torch.equal(out2["pano"], out["pano"]) and torch.equal(out2["mask"], out["mask"])
    # against the reference on those matches
    xy = [np.stack([k["x"], k["y"]], 1).astype(np.float32) for k, _ in (f.download() for f in feats)]
    tab = [dict(src_img_idx=m.src_img_idx, dst_img_idx=m.dst_img_idx, matches=m.matches, inliers_mask=m.inliers_mask, num_inliers=m.num_inliers,
                has_H=1 if m.H is not None else 0, H=m.H, confidence=m.confidence) for m in pm]
    start = [_params(c) for c in noisy]
    ref = rr.reference_ba_ray(dict(name="job", n=N, xy=xy, start=start), tab, cfg.conf_thresh)
    s_noisy, s_exact = rr.cost(start, ref["obs"]), rr.cost([_params(c) for c in exact], ref["obs"])
    print("\n    ray cost: noisy %.1f exact %.1f refined %.1f (reference minimum %.1f), %d observations" % (s_noisy, s_exact, rr.cost(rm.projected(direct), ref["obs"]), ref["S"], ref["n_obs"]))
    assert s_noisy > 4 * s_exact
    res = rr.check_ba_ray(ref, direct, ref["cond"] <= rm.COND_CAP)
    assert ref["cond"] <= rm.COND_CAP
    print("    excess %+.3e  /E %+.2e  parameters / bound %.3f" % (res["excess"], res["over_E"], res["par_ratio"]))
    # the C++ driver on the same frames and camera descriptions writes the cams.data the Python side produces
    _build()
    tmp = str(tmp_path)
    for i, (f, c, Rs_) in enumerate(zip(host_frames, noisy, sensor)):
        with open(os.path.join(tmp, "%d.ppm" % (i + 1)), "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (W, H))
            fh.write(f[:, :, ::-1].tobytes())
        with open(os.path.join(tmp, "%d.txt" % (i + 1)), "w") as fh:
            fh.write(_desc(c, Rs_))
    r = subprocess.run([os.path.join(HOST, "stitch_main"), tmp, "--ba", "ray", "--wave_correct", "no"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cfg_nw = isa.StitchConfig.hot_path(ba_cost_func="ray", wave_correct="no")
    st = isa.Stitcher(ctx, (W, H), cfg_nw)
    sfeats = st.features([frames[i] for i in range(N)])
    spm = st.match(sfeats)
    idx = [int(i) for i in leaveBiggestComponent(spm, N, cfg_nw.conf_thresh)]
    assert idx == list(range(N)) == ser.deserializeIndices(os.path.join(tmp, "indices.data"))
    refined = refine_cameras(ctx, sfeats, spm, idx, noisy, cfg_nw)
    ser.serializeCameraParams([dict(_params(c), R=np.asarray(c["R"], np.float32)) for c in refined], os.path.join(tmp, "cams_py.data"))
    assert open(os.path.join(tmp, "cams.data")).read() == open(os.path.join(tmp, "cams_py.data")).read()
    for a, d in zip(refined, direct):
        assert np.array_equal(rm._bits(a["K"][0, 0]), rm._bits(d["focal"]))
    r = subprocess.run([os.path.join(HOST, "stitch_main"), tmp, "--ba", "affine"], capture_output=True, text=True)
    assert r.returncode == 1 and "'no', 'reproj' and 'ray'" in r.stdout
