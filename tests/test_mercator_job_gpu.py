"""The jobs under warp_type = mercator on the six-frame 640 x 360 sweep of test_range_matcher_job_gpu.py: the Python StitchJob and
Stitcher against the C++ job (host/stitch_bench --warp mercator --dump) byte for byte and against the spherical panorama, every
roi the job used within the reference sets of tests/refimpl_mercator.py; the seam-scale warps of the kind (gain_blocks + dp_color)
within the reference candidates; the two-rank Python sharded job on one GPU against the one-rank job.

mis::Stitcher (the C++ pipeline with the seam-scale step) is reachable from host/stitch_main only, which keeps refusing
`--warp mercator` (tests/test_warpers_job_gpu.py pins that refusal), and host/stitch_bench runs mis::StitchJob / mis::ShardedJob:
no tool exposes mis::Stitcher under this kind, so the seam-scale warps are compared with the reference sets only."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import refimpl as ri
import refimpl_mercator as rm

pytestmark = pytest.mark.gpu

W, H = 640, 360
YAWS = [-26.0, -13.0, 0.0, 13.0, 26.0, 39.0]
CHILD_TIMEOUT = 300     # seconds, each child process


def _cams():
    import synth
    return [synth.make_camera(W, H, 60.0, y, 0.4 * ((i % 3) - 1), 0.3 * ((i % 2) - 0.5), 0.95 + 0.02 * i) for i, y in enumerate(YAWS)]


@pytest.fixture(scope="module")
def single(ctx):
    """The one-rank Mercator job on the sweep, run once for the tests below -> (cams, frames, job, out)."""
    import synth
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    cams = _cams()
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    job = StitchJob(ctx, (W, H), cams, config=StitchConfig.hot_path(warp_type="mercator"))
    assert job.kind == rm.MERCATOR and job.speculation_roi_ok()
    out = job.run(frames)
    assert out["indices"] == [0, 1, 2, 3, 4, 5]
    return cams, frames, job, out


def test_job_and_stitcher_equal_cpp_job_and_differ_from_spherical(tmp_path, ctx, single):
    """StitchJob and Stitcher with hot_path(warp_type="mercator") equal host/stitch_bench --warp mercator --dump byte for byte
    (panorama and mask), and the panorama is not the spherical one; every roi the job used lies in the reference sets."""
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    from test_host_cpp import HOST, _build, _read_dump, write_cams_file
    cams, frames, job, out = single
    _build()
    cams_path, prefix = str(tmp_path / "cams.txt"), str(tmp_path / "out")
    write_cams_file(cams_path, cams)
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "2", "--warmup", "1", "--dump", prefix, "--warp", "mercator"],
                       capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    got = _read_dump(prefix)
    assert got["indices"] == out["indices"] and line["kept"] == 6 and line["speculation_kept"] is True
    assert got["bands"] == out["num_bands"]
    assert np.array_equal(got["mask"], out["mask"].cpu().numpy()) and np.array_equal(got["pano"], out["pano"].cpu().numpy())
    # the Python Stitcher (features, matches, pruning, compose) on the same frames
    res, mask, feats, pm, idx = isa.Stitcher(ctx, (W, H), StitchConfig.hot_path(warp_type="mercator")).stitch([frames[i] for i in range(len(cams))], cams)
    assert list(idx) == out["indices"]
    assert torch.equal(res, out["pano"]) and torch.equal(mask, out["mask"])
    # the rois the job used, at the scale and size it used them
    g = job._geom
    assert job._compose_indices == out["indices"]
    for i in out["indices"]:
        c = job._compose_cams[i]
        ref = rm.warp_roi_f64(g.warp_scale, g.size[0], g.size[1], np.asarray(c["K"], np.float32), np.asarray(c["R"], np.float32))
        assert rm.roi_matches(tuple(job._compose_rois[i]), ref), (i, job._compose_rois[i], ref.get("intervals"))
    sph = StitchJob(ctx, (W, H), cams).run(frames)
    assert sph["pano"].shape != out["pano"].shape or not torch.equal(sph["pano"], out["pano"])


def test_seam_scale_warps_within_reference_and_stitcher_composes(ctx, single):
    """gain_blocks + dp_color under warp_type = mercator: the seam-scale warps of the kind (image LINEAR / REFLECT, mask NEAREST /
    CONSTANT, K scaled by the seam aspect, the warper's own device roi scan) lie within the reference candidates, and the Python
    Stitcher composes with them: another panorama than the hot path's, of the same size."""
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as st
    cams, frames, job, out = single
    cfg = st.StitchConfig.hot_path(warp_type="mercator", expos_comp_type="gain_blocks", seam_find_type="dp_color")
    scale = isa.Stitcher.warped_image_scale(cams)
    seam_scale = min(1.0, float(np.sqrt(cfg.seam_megapix * 1e6 / (W * H))))
    assert seam_scale < 1.0
    swa = np.float32(seam_scale)
    for i in (0, 3, 5):
        tl, iw, mw = st.seam_scale_warp(ctx, cfg, (W, H), frames[i], cams[i], scale)
        small = st.resize(ctx, frames[i], fx=seam_scale, fy=seam_scale).cpu().numpy()
        K = np.array(cams[i]["K"], np.float32).copy()
        K[0, 0] *= swa; K[0, 2] *= swa; K[1, 1] *= swa; K[1, 2] *= swa
        R = np.asarray(cams[i]["R"], np.float32)
        wscale = np.float32(np.float32(scale) * swa)
        sh, sw = small.shape[:2]
        roi = (tl[0], tl[1], iw.shape[1], iw.shape[0])
        assert rm.roi_matches(roi, rm.warp_roi_f64(wscale, sw, sh, K, R)), (i, roi)
        maps = rm.backward_f64(K, R, wscale, roi)
        for name, gotw, cand in (("linear", iw.cpu().numpy(), ri.remap_linear_reflect_candidates(small, maps)),
                                 ("mask", mw.cpu().numpy(), ri.remap_nearest_constant_candidates(np.full((sh, sw), 255, np.uint8), maps))):
            bad, nb, nu = ri.check_candidates(gotw, *cand)
            assert not bad.any(), (i, name, int(bad.sum()))
            assert nb <= 0.40 * bad.size and nu <= 0.10 * bad.size, (i, name, nb, nu, bad.size)      # test_warpers_gpu.py's caps
    res, mask = isa.Stitcher(ctx, (W, H), cfg).compose(frames, cams)
    assert res.shape == out["pano"].shape and mask.shape == out["mask"].shape
    assert not torch.equal(res, out["pano"])


def _rank_main(rank, world, port, out_path):
    """One rank of the Python sharded job with warp_type = mercator, on the one GPU (gloo rendezvous), as _py_rank_warp of
    test_warpers_job_gpu.py."""
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here):
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
        from image_stitching_amd.stitching import StitchConfig
        cams = _cams()
        job = StitchJob(isa.Context(0), (W, H), cams, rank=rank, world_size=world, group=dist.group.WORLD,
                        config=StitchConfig.hot_path(warp_type="mercator"))
        frames = {i: synth.render_frame_gpu(cams[i]) for i in job.my_frames}
        out = job.run(frames)
        if rank == 0:
            np.savez(out_path, pano=out["pano"].cpu().numpy(), mask=out["mask"].cpu().numpy(), conf=out["confidence"].cpu().numpy().reshape(-1),
                     indices=np.array(out["indices"]))
    finally:
        dist.destroy_process_group()


def test_two_rank_sharded_job_equals_one_rank_job(tmp_path, single):
    """The two-rank Python sharded job on one GPU (two fresh child processes, each under its own timeout; three GPU processes
    with this one) against the one-rank job: indices, confidences and mask exact, every pixel within 1 LSB (the ranks' f32 pyramid
    sums are added in rank order, as in test_warpers_job_gpu.py)."""
    cams, frames, job, out = single
    world = 2
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    npz = str(tmp_path / "py.npz")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), str(rank), str(world), str(port), npz], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for rank in range(world)]
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=CHILD_TIMEOUT)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert [p.returncode for p in procs] == [0] * world, "\n".join(logs)
    py = np.load(npz)
    assert list(py["indices"]) == out["indices"]
    assert np.array_equal(py["conf"], np.asarray(out["confidence"]).reshape(-1))
    assert np.array_equal(py["mask"], out["mask"].cpu().numpy())
    d = np.abs(py["pano"].astype(np.int32) - out["pano"].cpu().numpy().astype(np.int32))
    assert d.max() <= 1, d.max()


if __name__ == "__main__":
    _rank_main(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
