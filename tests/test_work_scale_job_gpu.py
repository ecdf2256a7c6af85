"""GPU: jobs with work_megapix >= 0 (image_stitching.cpp:589-603, :607, :613, :635-637, :1113-1125).  Features, matching, bundle
adjustment and the median focal run at work scale; the yardstick is the sequence restated from those lines over the oracle's
stage functions (tests/refjob_work_scale.py), bit for bit.  The C++ jobs and the sharded job are compared with the Python job."""
import json
import os
import subprocess
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "host")


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


def _compare_features(gfeats, ofeats, size):
    assert len(gfeats) == len(ofeats)
    for i, (g, o) in enumerate(zip(gfeats, ofeats)):
        assert tuple(g.img_size) == tuple(size) == (o["img_w"], o["img_h"]), "img_size of frame %d" % i
        k, d = g.download()
        assert len(k) == len(o["kps"]), "keypoint count of frame %d" % i
        for name in ("x", "y", "size", "angle", "response"):
            assert np.array_equal(k[name].view(np.uint32), o["kps"][name].view(np.uint32)), (i, name)
        assert np.array_equal(k["octave"], o["kps"]["octave"])
        assert d.dtype == o["desc"].dtype and np.array_equal(d, o["desc"]), "descriptors of frame %d" % i


def _compare_matches(pm, ref_pm):
    assert len(pm) == len(ref_pm)
    for g, o in zip(pm, ref_pm):
        assert g.src_img_idx == o["src_img_idx"] and g.dst_img_idx == o["dst_img_idx"]
        assert np.array_equal(g.matches, o["matches"].astype(g.matches.dtype))
        assert np.array_equal(g.inliers_mask, o["inliers_mask"]) and g.num_inliers == o["num_inliers"]
        assert (g.H is not None) == o["has_H"]
        if o["has_H"]:
            assert np.array_equal(_bits(g.H), _bits(o["H"]))
        assert g.confidence == o["confidence"]


def _six_4k():
    import synth
    cams = synth.workload("config3")[:6]
    return cams, (cams[0]["width"], cams[0]["height"])


@pytest.fixture(scope="module")
def job_4k(ctx):
    """Six config-3 4K frames through StitchJob.run at work_megapix = 0.6 (one run shared by the tests below)."""
    import torch
    import synth
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    cams, size = _six_4k()
    dev = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    torch.cuda.synchronize()
    job = StitchJob(ctx, size, cams, config=isa.StitchConfig.hot_path(work_megapix=0.6))
    out = job.run(dev)
    return cams, size, dev, job, out


def test_features_matches_and_panorama_at_work_scale_bit_exact(job_4k, oracle_mod):
    import refjob_work_scale as rj
    cams, size, dev, job, out = job_4k
    host = [dev[i].cpu().numpy() for i in range(len(cams))]
    ref = rj.stitch_job_work_scale(host, cams, 0.6)
    assert ref["work_size"] == (1033, 581) and job.work_size == (1033, 581) and job.work_scale == ref["work_scale"]
    _compare_features(out["features"], ref["features"], (1033, 581))
    assert [len(f) for f in out["features"]] == [4000] * 6
    _compare_matches(out["matches"], ref["matches"])
    assert np.array_equal(np.asarray(out["confidence"]).reshape(6, 6), ref["confidence"])
    assert out["indices"] == ref["indices"] == [0, 1, 2, 3, 4, 5]                     # all frames kept: the restated sequence keeps them too
    for i in range(5):
        assert ref["matches"][i * 6 + i + 1]["num_inliers"] > 500
    # the job's cameras are in work units, the caller's stay as given
    for i, c in enumerate(ref["cameras"]):
        assert float(job.cams[i]["K"][0, 0]) == c["focal"] and float(job.cams[i]["K"][0, 2]) == c["ppx"] and float(job.cams[i]["K"][1, 2]) == c["ppy"]
        assert job.cams0[i] is cams[i]
    assert float(np.float32(job.scale)) == float(np.float32(ref["scale"]))
    assert [tuple(job._compose_rois[i]) for i in ref["indices"]] == [tuple(r) for r in ref["rois"]]
    assert out["num_bands"] == ref["num_bands"] and tuple(out["pano_size"]) == tuple(ref["pano_size"])
    assert np.array_equal(out["mask"].cpu().numpy(), ref["mask"])
    assert np.array_equal(out["pano"].cpu().numpy(), ref["pano"])


def test_features_equal_those_of_a_job_on_frames_resized_beforehand(job_4k, ctx):
    """Oracle-free: the features of the work-scale job are those of a work_megapix = -1 job run on frames resized with the
    single-image entry; and the engine's work frames live in buffers that a second run reuses."""
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    cams, size, dev, job, out = job_4k
    ws = job.work_scale
    small = {i: isa.resize(ctx, dev[i], fx=ws, fy=ws) for i in dev}
    assert tuple(small[0].shape[:2]) == (581, 1033)
    wcams = [isa.stitching.scaled_camera(c, ws) for c in cams]
    plain = StitchJob(ctx, (1033, 581), wcams, config=isa.StitchConfig.hot_path()).run(small)
    for a, b in zip(out["features"], plain["features"]):
        assert a.img_size == b.img_size == (1033, 581)
        ka, da = a.download()
        kb, db = b.download()
        assert np.array_equal(ka, kb) and np.array_equal(da, db)
    assert torch.equal(out["confidence"].cpu(), plain["confidence"].cpu())
    for a, b in zip(out["matches"], plain["matches"]):
        assert np.array_equal(a.matches, b.matches) and np.array_equal(a.inliers_mask, b.inliers_mask) and a.confidence == b.confidence
    ptrs = [t.data_ptr() for t in job.engine._work_frames]
    assert len(ptrs) == 6
    out2 = job.run(dev)
    assert [t.data_ptr() for t in job.engine._work_frames] == ptrs
    assert torch.equal(out2["pano"], out["pano"]) and torch.equal(out2["mask"], out["mask"])
    for a, b in zip(out2["features"], out["features"]):
        assert np.array_equal(a.download()[1], b.download()[1])


def test_work_scale_one_is_the_identity(ctx):
    """work_megapix = 100 (work scale 1) = work_megapix = -1, byte for byte."""
    import torch
    import synth
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    w, h = 640, 360
    cams = [synth.make_camera(w, h, 60.0, 13.0 * i - 26.0, 0.4 * ((i % 3) - 1), 0.3 * ((i % 2) - 0.5), 0.95 + 0.02 * i) for i in range(5)]
    dev = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    a = StitchJob(ctx, (w, h), cams, config=isa.StitchConfig.hot_path(work_megapix=-1)).run(dev)
    jb = StitchJob(ctx, (w, h), cams, config=isa.StitchConfig.hot_path(work_megapix=100))
    b = jb.run(dev)
    assert jb.work_scale == 1.0 and jb.cams is cams and not jb.engine._work_frames
    assert a["indices"] == b["indices"] and torch.equal(a["confidence"].cpu(), b["confidence"].cpu())
    for fa, fb in zip(a["features"], b["features"]):
        ka, da = fa.download()
        kb, db = fb.download()
        assert fa.img_size == fb.img_size == (w, h) and np.array_equal(ka, kb) and np.array_equal(da, db)
    for ma, mb in zip(a["matches"], b["matches"]):
        assert np.array_equal(ma.matches, mb.matches) and np.array_equal(ma.inliers_mask, mb.inliers_mask) and ma.confidence == mb.confidence
    assert torch.equal(a["pano"], b["pano"]) and torch.equal(a["mask"], b["mask"])


def _noisy_sweep(w, h, n):
    import synth
    exact = [synth.make_camera(w, h, 60.0, 12.0 * i - 30.0, 2.0 * ((i % 3) - 1), 1.2 * ((i % 2) - 0.5), 0.96 + 0.015 * i) for i in range(n)]
    rng = np.random.default_rng(5)
    noisy = []
    for c in exact:
        d = dict(c)
        d["R"] = synth.rotation_yxz(*np.radians(rng.normal(0, 0.4, 3))) @ c["R"]
        noisy.append(d)
    return exact, noisy, [synth.render_frame(c) for c in exact]


def test_reference_configuration_at_work_scale_bit_exact(ctx, oracle_mod):
    """StitchConfig.reference(work_megapix=...): bundle adjustment (reproj) + wave correction HORIZ on work-unit cameras, gain blocks +
    dp_color at seam scale (seam_work_aspect = seam_scale / work_scale), composition at compose scale (compose_work_aspect =
    compose_scale / work_scale), on a small sweep from perturbed cameras, with the megapixel options scaled down with the frames
    (work scale 0.72, seam scale 0.29, compose scale 0.59)."""
    import torch
    import image_stitching_amd as isa
    import refjob_work_scale as rj
    from image_stitching_amd.distributed import StitchJob
    w, h, n = 640, 360, 6
    exact, noisy, host = _noisy_sweep(w, h, n)
    cfg = isa.StitchConfig.reference(work_megapix=0.12, compose_megapix=0.08, seam_megapix=0.02)
    job = StitchJob(ctx, (w, h), noisy, config=cfg)
    assert abs(job.work_scale - 0.7217) < 1e-3 and job.work_size == (462, 260)
    dev = {i: torch.from_numpy(f).cuda() for i, f in enumerate(host)}
    out = job.run(dev)
    ref = rj.stitch_job_work_scale(host, noisy, 0.12, refine=True, seams=True, seam_megapix=0.02, compose_megapix=0.08)
    assert out["indices"] == ref["indices"] and len(ref["indices"]) == n
    _compare_features(out["features"], ref["features"], (462, 260))
    assert np.array_equal(np.asarray(out["confidence"].cpu()).reshape(n, n), ref["confidence"])
    for i, c in zip(ref["indices"], ref["cameras"]):
        got = job.cams[i]
        assert np.array_equal(_bits(got["R"]), _bits(c["R"])), "R of frame %d" % i
        assert np.array_equal(_bits([got["K"][0, 0], got["K"][0, 2], got["K"][1, 2]]), _bits([c["focal"], c["ppx"], c["ppy"]])), "intrinsics of frame %d" % i
    assert float(np.float32(job.scale)) == float(np.float32(ref["scale"]))
    compensator, seam_masks = job.engine._seam
    for k in range(n):
        assert np.array_equal(seam_masks[k].cpu().numpy(), ref["seam_masks"][k]), "seam mask %d" % k
        assert np.array_equal(compensator.gain_map(k).view(np.uint32), ref["gain_maps"][k].view(np.uint32)), "gain map %d" % k
    assert [tuple(job._compose_rois[i]) for i in ref["indices"]] == [tuple(r) for r in ref["rois"]]
    assert out["num_bands"] == ref["num_bands"] and tuple(out["pano_size"]) == tuple(ref["pano_size"])
    assert np.array_equal(out["mask"].cpu().numpy(), ref["mask"])
    assert np.array_equal(out["pano"].cpu().numpy(), ref["pano"])
    # the per-call mirror of the compositing loop with the job's refined (work-unit) cameras
    st = isa.Stitcher(ctx, (w, h), cfg)
    pano2, mask2 = st.compose(dev, job.cams, out["indices"])
    assert np.array_equal(mask2.cpu().numpy(), ref["mask"]) and np.array_equal(pano2.cpu().numpy(), ref["pano"])


def test_stitcher_stitch_at_work_scale_equals_the_job(ctx):
    """Stitcher.stitch (per-call mirror) = StitchJob at the same work_megapix."""
    import torch
    import synth
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    w, h = 640, 360
    cams = [synth.make_camera(w, h, 60.0, 13.0 * i - 26.0, 0.4 * ((i % 3) - 1), 0.3 * ((i % 2) - 0.5), 0.95 + 0.02 * i) for i in range(5)]
    dev = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    cfg = isa.StitchConfig.hot_path(work_megapix=0.1)
    out = StitchJob(ctx, (w, h), cams, config=cfg).run(dev)
    st = isa.Stitcher(ctx, (w, h), cfg)
    assert st.work_size == (422, 237)
    pano, mask, feats, pm, idx = st.stitch([dev[i] for i in range(5)], cams)
    assert list(idx) == out["indices"]
    for a, b in zip(feats, out["features"]):
        assert a.img_size == b.img_size == (422, 237) and np.array_equal(a.download()[1], b.download()[1])
    assert torch.equal(pano, out["pano"]) and torch.equal(mask, out["mask"])


def test_sift_at_work_scale_bit_exact(ctx, oracle_mod):
    import torch
    import synth
    import image_stitching_amd as isa
    import refjob_work_scale as rj
    from image_stitching_amd.distributed import StitchJob
    w, h = 640, 360
    cams = [synth.make_camera(w, h, 60.0, 11.0 * i - 16.0, 0.4 * ((i % 3) - 1)) for i in range(4)]
    host = [synth.render_frame(c) for c in cams]
    cfg = isa.StitchConfig.hot_path(features_type="sift", work_megapix=0.1)
    job = StitchJob(ctx, (w, h), cams, config=cfg)
    out = job.run({i: torch.from_numpy(f).cuda() for i, f in enumerate(host)})
    ws = rj.work_scale_of(0.1, w, h)
    ref = rj.features_of(rj.work_images(host, ws), "sift")
    assert job.work_size == (422, 237)
    _compare_features(out["features"], ref, (422, 237))
    assert min(len(f["kps"]) for f in ref) > 200


def _rank(rank, world, port, out_path, work_megapix):
    """One rank of a 2-process job on the same GPU (gloo rendezvous, device tensors staged through the host)."""
    import sys
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import synth
        import image_stitching_amd as isa
        from image_stitching_amd.distributed import StitchJob
        w, h = 640, 360
        cams = _sweep_cams(w, h)
        job = StitchJob(isa.Context(0), (w, h), cams, rank=rank, world_size=world, group=dist.group.WORLD, config=isa.StitchConfig.hot_path(work_megapix=work_megapix))
        frames = {i: synth.render_frame_gpu(cams[i]) for i in job.my_frames}
        out = job.run(frames)
        if rank == 0:
            np.savez(out_path, pano=out["pano"].cpu().numpy(), mask=out["mask"].cpu().numpy(), conf=out["confidence"].cpu().numpy().reshape(-1),
                     indices=np.array(out["indices"]), sizes=np.array([f.img_size for f in out["features"]]), nfeat=np.array([len(f) for f in out["features"]]))
    finally:
        dist.destroy_process_group()


def _sweep_cams(w, h):
    import synth
    yaws = [-30.0, -18.0, -6.0, 6.0, 18.0, 30.0]
    return [synth.make_camera(w, h, 60.0, y, 0.4 * ((i % 3) - 1), 0.3 * ((i % 2) - 0.5), 0.95 + 0.02 * i) for i, y in enumerate(yaws)]


def _run_ranks(fn, args, world, limit_s):
    """The ranks as child processes, the group under one time limit: a rank that fails or a limit that passes ends the others,
    and nothing is started afterwards."""
    import torch.multiprocessing as mp
    pc = mp.start_processes(fn, args=args, nprocs=world, join=False, start_method="spawn")
    deadline = time.monotonic() + limit_s
    try:
        while not pc.join(timeout=2.0):          # raises when a rank failed (the others are ended by torch)
            if time.monotonic() > deadline:
                raise TimeoutError("the ranks did not finish within %d s" % limit_s)
    finally:
        for p in pc.processes:
            if p.is_alive():
                p.kill()
            p.join(10)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_two_ranks_on_one_gpu_match_single_rank_at_work_scale(ctx, tmp_path):
    import synth
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    w, h = 640, 360
    cams = _sweep_cams(w, h)
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    ref = StitchJob(ctx, (w, h), cams, config=isa.StitchConfig.hot_path(work_megapix=0.1)).run(frames)
    out_path = str(tmp_path / "rank0.npz")
    _run_ranks(_rank, (2, _free_port(), out_path, 0.1), 2, 300)
    got = np.load(out_path)
    assert list(got["indices"]) == ref["indices"]
    assert [tuple(s) for s in got["sizes"]] == [(422, 237)] * 6             # the gathered features carry the work size
    assert list(got["nfeat"]) == [len(f) for f in ref["features"]]
    assert np.array_equal(got["conf"], ref["confidence"].cpu().numpy().reshape(-1))
    assert np.array_equal(got["mask"], ref["mask"].cpu().numpy())
    d = np.abs(got["pano"].astype(np.int32) - ref["pano"].cpu().numpy().astype(np.int32))
    assert d.max() <= 1 and (d > 0).mean() < 0.02          # f32 weight sums in a different order where >= 3 frames overlap


# ---- C++ host ---------------------------------------------------------------------------------------------------------------
def _build():
    subprocess.run(["make", "-C", HOST], check=True, capture_output=True)


def test_stitch_main_work_megapix_equals_python_stitcher(tmp_path, ctx, oracle_mod):
    """stitch_main --work_megapix: result.ppm, result_mask.pgm and the kept indices as the Python Stitcher gives them; cams.data
    holds work-unit cameras (focal, ppx, ppy times work_scale), as the reference's checkpoint does."""
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd import serializer as ser
    from test_host_cpp import _read_ppm, _write_job
    _build()
    tmp = str(tmp_path)
    cams, frames = _write_job(tmp, oracle_mod, n=3, w=480, h=270)
    size = (480, 270)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    exe = os.path.join(HOST, "stitch_main")
    r = subprocess.run([exe, tmp, "--work_megapix", "0.09"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    cfg = isa.StitchConfig.hot_path(work_megapix=0.09)
    st = isa.Stitcher(ctx, size, cfg)
    ws = st.work_scale
    assert st.work_size == (400, 225)
    res, mask, feats, pm, idx = st.stitch(dev, cams)
    counts = [int(l.rsplit(":", 1)[1]) for l in r.stdout.splitlines() if l.startswith("Features in image #")]
    assert counts == [len(f) for f in feats]
    assert ser.deserializeIndices(os.path.join(tmp, "indices.data")) == [int(i) for i in idx] == [0, 1, 2]
    assert np.array_equal(_read_ppm(os.path.join(tmp, "result.ppm")), np.clip(res.cpu().numpy(), 0, 255).astype(np.uint8))
    raw = open(os.path.join(tmp, "result_mask.pgm"), "rb").read().split(b"\n255\n", 1)[1]
    assert np.array_equal(np.frombuffer(raw, np.uint8).reshape(mask.shape), mask.cpu().numpy())
    # cams.data: the checkpoint text of the work-unit cameras, byte for byte
    wcams = st.work_cameras(cams)
    ser.serializeCameraParams([dict(aspect=1.0, focal=c["K"][0, 0], ppx=c["K"][0, 2], ppy=c["K"][1, 2], R=c["R"]) for c in wcams], os.path.join(tmp, "py_cams.data"))
    assert open(os.path.join(tmp, "cams.data")).read() == open(os.path.join(tmp, "py_cams.data")).read()
    assert abs(ser.deserializeCameraParams(os.path.join(tmp, "cams.data"))[0]["focal"] - cams[0]["K"][0, 0] * ws) < 1e-3 and ws < 0.84
    # not the full-resolution job's features
    r1 = subprocess.run([exe, tmp], capture_output=True, text=True, timeout=300)
    assert r1.returncode == 0
    assert [int(l.rsplit(":", 1)[1]) for l in r1.stdout.splitlines() if l.startswith("Features in image #")] != counts
    # with the reference's seam step at seam and compose scale: C++ driver = the per-call Python mirror on work-unit cameras
    r = subprocess.run([exe, tmp, "--work_megapix", "0.09", "--expos_comp", "gain_blocks", "--seam", "dp_color", "--compose_megapix", "0.06", "--seam_megapix", "0.02"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    st2 = isa.Stitcher(ctx, size, isa.StitchConfig(work_megapix=0.09, compose_megapix=0.06, seam_megapix=0.02))
    small, _ = st2.compose(dev, st2.work_cameras(cams))
    assert np.array_equal(_read_ppm(os.path.join(tmp, "result.ppm")), np.clip(small.cpu().numpy(), 0, 255).astype(np.uint8))


def test_stitch_bench_work_megapix_equals_python_job(tmp_path, ctx):
    """host/stitch_bench --work_megapix (mis::StitchJob) = the Python job: indices, feature counts, confidences, panorama, mask."""
    import synth
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    from test_host_cpp import _read_dump, write_cams_file
    _build()
    w, h = 640, 360
    cams = _sweep_cams(w, h)
    cams_path, prefix = str(tmp_path / "cams.txt"), str(tmp_path / "out")
    write_cams_file(cams_path, cams)
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "2", "--warmup", "1", "--dump", prefix, "--work_megapix", "0.1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    got = _read_dump(prefix)
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    ref = StitchJob(ctx, (w, h), cams, config=isa.StitchConfig.hot_path(work_megapix=0.1)).run(frames)
    full = StitchJob(ctx, (w, h), cams).run(frames)
    assert got["indices"] == ref["indices"] and line["kept"] == len(ref["indices"])
    assert got["nfeat"] == [len(f) for f in ref["features"]] != [len(f) for f in full["features"]]
    assert np.array_equal(got["conf"], np.asarray(ref["confidence"]).reshape(-1))
    assert got["bands"] == ref["num_bands"]
    assert np.array_equal(got["mask"], ref["mask"].cpu().numpy())
    assert np.array_equal(got["pano"], ref["pano"].cpu().numpy())


def test_stitch_bench_sharded_work_megapix_equals_python_sharded_job(tmp_path, ctx):
    """host/stitch_bench --ranks 2 --comm host --one-gpu --work_megapix (mis::ShardedJob) = the Python sharded job at two ranks,
    byte for byte (same plan, same order of the f32 additions)."""
    from test_host_cpp import _read_dump, write_cams_file
    _build()
    w, h = 640, 360
    cams = _sweep_cams(w, h)
    cams_path, prefix = str(tmp_path / "cams.txt"), str(tmp_path / "out")
    write_cams_file(cams_path, cams)
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "1", "--warmup", "1", "--ranks", "2", "--comm", "host", "--one-gpu", "--dump", prefix,
                        "--work_megapix", "0.1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _read_dump(prefix)
    npz = str(tmp_path / "py.npz")
    _run_ranks(_rank, (2, _free_port(), npz, 0.1), 2, 300)
    py = np.load(npz)
    assert got["indices"] == list(py["indices"])
    assert got["nfeat"] == list(py["nfeat"])
    assert np.array_equal(got["conf"], py["conf"])
    assert np.array_equal(got["mask"], py["mask"]) and np.array_equal(got["pano"], py["pano"])
