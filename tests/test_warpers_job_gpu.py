"""The jobs under warp_type cylindrical and plane: the Python StitchJob's frames against the numpy reference and its panorama
against the oracle blender fed those frames; the C++ job (host/stitch_bench --warp), the C++ pipeline (host/stitch_main --warp,
with the seam-scale step) and the two-rank sharded job against the Python twins, byte for byte.  The plane sweep carries a
stray frame at 150 degrees: its roi is refused, so nothing is speculated, the pruning drops it and the job succeeds."""
import json
import os
import subprocess

import numpy as np
import pytest

import refimpl as ri
import refimpl_warpers as rw
from test_host_cpp import HOST, _build, _read_dump, _read_ppm, _write_job, write_cams_file

pytestmark = pytest.mark.gpu

W, H = 640, 360
SWEEPS = {"cylindrical": [-26.0, -13.0, 0.0, 13.0, 26.0, 39.0], "plane": [-36.0, -24.0, -12.0, 0.0, 12.0, 24.0]}


def _cams(warp, stray=False):
    import synth
    yaws = list(SWEEPS[warp])
    if stray:
        yaws[-1] = 150.0
    return [synth.make_camera(W, H, 60.0, y, 0.4 * ((i % 3) - 1), 0.3 * ((i % 2) - 0.5), 0.95 + 0.02 * i) for i, y in enumerate(yaws)]


CASES = [pytest.param("cylindrical", False, id="cylindrical"), pytest.param("plane", False, id="plane"),
         pytest.param("plane", True, id="plane-stray150")]


@pytest.mark.parametrize("warp,stray", CASES)
def test_python_job_frames_vs_reference_and_oracle_blend(ctx, oracle_mod, warp, stray):
    """Each kept frame, warped by mis_warper_warp_fused_batch at the job's scale and rois, lies within the reference candidates;
    the oracle's blender fed those frames gives the job's panorama and mask byte for byte."""
    import synth
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    cams = _cams(warp, stray)
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    kind = rw.CYLINDRICAL if warp == "cylindrical" else rw.PLANE
    job = StitchJob(ctx, (W, H), cams, config=StitchConfig.hot_path(warp_type=warp))
    assert job.speculation_roi_ok() == (not stray)
    out = job.run(frames)
    idx = out["indices"]
    assert idx == ([0, 1, 2, 3, 4] if stray else [0, 1, 2, 3, 4, 5])
    scale = isa.Stitcher.warped_image_scale([cams[i] for i in idx])
    rois = isa.stitching.warp_rois(ctx, scale, (W, H), [cams[i] for i in idx], kind)
    warped = isa.RotationWarper(ctx, scale, kind).warp_fused_batch([frames[i] for i in idx], [cams[i] for i in idx], rois)
    ctx.synchronize()
    for k, i in enumerate(idx):
        K, R = np.asarray(cams[i]["K"], np.float32), np.asarray(cams[i]["R"], np.float32)
        assert rw.roi_matches(rois[k], rw.warp_roi_f64(kind, scale, W, H, K, R))
        maps = rw.backward_f64(kind, K, R, scale, rois[k])
        img = frames[i].cpu().numpy()
        for name, got, cand in (("linear", warped[k][1].cpu().numpy().astype(np.uint8), ri.remap_linear_reflect_candidates(img, maps)),
                                ("mask", warped[k][2].cpu().numpy(), ri.remap_nearest_constant_candidates(np.full((H, W), 255, np.uint8), maps))):
            bad, nb, nu = ri.check_candidates(got, *cand)
            assert not bad.any(), (warp, i, name, int(bad.sum()))
            assert nu <= 0.10 * bad.size
    # the oracle blender on the same frames
    corners = [r[:2] for r in rois]
    sizes = [r[2:] for r in rois]
    x, y, pw, ph = isa.result_roi(corners, sizes)
    btype, bands, sharp = isa.blend_config(2, 5.0, (pw, ph))
    ob = oracle_mod.Blender(btype, bands, sharp)
    ob.prepare(corners, sizes)
    for (tl, img_s, msk) in warped:
        ob.feed(img_s.cpu().numpy(), msk.cpu().numpy(), tl)
    pano, mask = ob.blend()
    assert np.array_equal(pano, out["pano"].cpu().numpy()) and np.array_equal(mask, out["mask"].cpu().numpy())


@pytest.mark.parametrize("warp,stray", CASES)
def test_cpp_job_equals_python_job(tmp_path, ctx, warp, stray):
    """host/stitch_bench --warp <kind> --dump against the Python StitchJob with that warp_type, byte for byte."""
    import synth
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    _build()
    cams = _cams(warp, stray)
    cams_path, prefix = str(tmp_path / "cams.txt"), str(tmp_path / "out")
    write_cams_file(cams_path, cams)
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "2", "--warmup", "1", "--dump", prefix, "--warp", warp],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    got = _read_dump(prefix)
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    ref = StitchJob(ctx, (W, H), cams, config=StitchConfig.hot_path(warp_type=warp)).run(frames)
    assert got["indices"] == ref["indices"] and line["kept"] == len(ref["indices"])
    assert line["speculation_kept"] == (not stray)
    assert got["bands"] == ref["num_bands"]
    assert np.array_equal(got["mask"], ref["mask"].cpu().numpy())
    assert np.array_equal(got["pano"], ref["pano"].cpu().numpy())


@pytest.mark.parametrize("warp", ["cylindrical", "plane"])
def test_stitch_main_warp_equals_python_stitcher(tmp_path, ctx, oracle_mod, warp):
    """host/stitch_main --warp <kind> with gain_blocks + dp_color (the seam-scale warps of the kind) against the Python Stitcher
    with the same warp_type, byte for byte; and the kind is not a spherical panorama under another name."""
    import torch
    import image_stitching_amd as isa
    _build()
    cams, frames = _write_job(str(tmp_path), oracle_mod, n=3, w=480, h=270)
    size = (frames[0].shape[1], frames[0].shape[0])
    dev = [torch.from_numpy(f).cuda() for f in frames]
    r = subprocess.run([os.path.join(HOST, "stitch_main"), str(tmp_path), "--expos_comp", "gain_blocks", "--seam", "dp_color", "--warp", warp],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _read_ppm(os.path.join(str(tmp_path), "result.ppm"))
    cfg = isa.StitchConfig.hot_path(compose_megapix=-1, warp_type=warp, expos_comp_type="gain_blocks", seam_find_type="dp_color")
    res, _ = isa.Stitcher(ctx, size, cfg).compose(dev, cams)
    assert np.array_equal(np.clip(res.cpu().numpy(), 0, 255).astype(np.uint8), got)
    sph, _ = isa.Stitcher(ctx, size, isa.StitchConfig.hot_path(compose_megapix=-1, expos_comp_type="gain_blocks", seam_find_type="dp_color")).compose(dev, cams)
    assert sph.shape != res.shape or not torch.equal(sph, res)
    r = subprocess.run([os.path.join(HOST, "stitch_main"), str(tmp_path), "--warp", "mercator"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "not implemented" in r.stdout + r.stderr


def _py_rank_warp(rank, world, port, out_path, warp, stray):
    """One rank of the Python sharded job with a warp_type, on the one GPU (gloo rendezvous)."""
    import sys
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
        cams = _cams(warp, stray)
        job = StitchJob(isa.Context(0), (W, H), cams, rank=rank, world_size=world, group=dist.group.WORLD,
                        config=StitchConfig.hot_path(warp_type=warp))
        frames = {i: synth.render_frame_gpu(cams[i]) for i in job.my_frames}
        out = job.run(frames)
        if rank == 0:
            np.savez(out_path, pano=out["pano"].cpu().numpy(), mask=out["mask"].cpu().numpy(), conf=out["confidence"].cpu().numpy().reshape(-1),
                     indices=np.array(out["indices"]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("warp,stray", [pytest.param("cylindrical", False, id="cylindrical"), pytest.param("plane", True, id="plane-stray150")])
def test_cpp_sharded_job_equals_python_sharded_job_and_single_process(tmp_path, ctx, warp, stray):
    """host/stitch_bench --ranks 2 --one-gpu --comm host --warp <kind> (mis::ShardedJob: rank split, column-strip exchange,
    exchange_finalize) against the Python two-rank job with that warp_type, byte for byte; and against the single-process job:
    indices, confidences and mask exact, every pixel within 1 LSB (the ranks' f32 pyramid sums are added in rank order).  The
    plane sweep's stray frame is refused by warpRoi, so neither sharded job speculates: the non-speculative branch runs."""
    import socket
    import torch.multiprocessing as mp
    import synth
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    _build()
    world = 2
    cams = _cams(warp, stray)
    cams_path, prefix = str(tmp_path / "cams.txt"), str(tmp_path / "out")
    write_cams_file(cams_path, cams)
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "1", "--warmup", "1", "--ranks", str(world), "--comm", "host",
                        "--one-gpu", "--dump", prefix, "--warp", warp], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert "ShardedJob, %d ranks" % world in line["host"]
    got = _read_dump(prefix)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    npz = str(tmp_path / "py.npz")
    mp.start_processes(_py_rank_warp, args=(world, port, npz, warp, stray), nprocs=world, join=True, start_method="spawn")
    py = np.load(npz)
    kept = [0, 1, 2, 3, 4] if stray else [0, 1, 2, 3, 4, 5]
    assert got["indices"] == list(py["indices"]) == kept
    assert line["kept"] == len(kept) and line["speculation_kept"] == (not stray)
    assert np.array_equal(got["conf"], py["conf"])
    assert np.array_equal(got["mask"], py["mask"]) and np.array_equal(got["pano"], py["pano"])
    one = StitchJob(ctx, (W, H), cams, config=StitchConfig.hot_path(warp_type=warp)).run({i: synth.render_frame_gpu(c) for i, c in enumerate(cams)})
    assert one["indices"] == kept
    assert np.array_equal(got["conf"], np.asarray(one["confidence"]).reshape(-1))
    assert np.array_equal(got["mask"], one["mask"].cpu().numpy())
    d = np.abs(got["pano"].astype(np.int32) - one["pano"].cpu().numpy().astype(np.int32))
    assert d.max() <= 1, d.max()
    # the kind reached every rank: the spherical panorama of the same cameras is another image
    sph = StitchJob(ctx, (W, H), cams).run({i: synth.render_frame_gpu(c) for i, c in enumerate(cams)})
    assert sph["pano"].shape != one["pano"].shape or not np.array_equal(sph["pano"].cpu().numpy(), got["pano"])
