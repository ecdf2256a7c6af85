"""range_width through the jobs, on the six-frame 640 x 360 sweep of tests/test_warpers_job_gpu.py (13 degree steps): the Python
StitchJob with StitchConfig.hot_path(range_width=3) against the all-pairs job (without bundle adjustment the panorama depends on
the kept set only), the C++ job (host/stitch_bench --rangewidth), the C++ pipeline (host/stitch_main --rangewidth) and the
two-rank sharded jobs against it, byte for byte; range_width=1 selects nothing and ends the job as an empty pruning does."""
import json
import os
import subprocess

import numpy as np
import pytest

from test_host_cpp import HOST, _build, _read_dump, _read_ppm, _write_job, write_cams_file

pytestmark = pytest.mark.gpu

W, H = 640, 360
YAWS = [-26.0, -13.0, 0.0, 13.0, 26.0, 39.0]
N = len(YAWS)
BAND = [(i, j) for i in range(N) for j in range(i + 1, N) if j < i + 3]


def _cams():
    import synth
    return [synth.make_camera(W, H, 60.0, y, 0.4 * ((i % 3) - 1), 0.3 * ((i % 2) - 0.5), 0.95 + 0.02 * i) for i, y in enumerate(YAWS)]


def _entry_bytes(m):
    return (m.src_img_idx, m.dst_img_idx, m.num_inliers, np.float64(m.confidence).tobytes(), np.asarray(m.matches).tobytes(),
            np.asarray(m.inliers_mask).tobytes(), None if m.H is None else np.asarray(m.H, np.float64).tobytes())


def _job_arrays(out):
    return dict(pano=out["pano"].cpu().numpy(), mask=out["mask"].cpu().numpy(), conf=np.asarray(out["confidence"].cpu().numpy(), np.float64).reshape(-1),
                indices=list(out["indices"]), bands=out["num_bands"], nfeat=[len(f) for f in out["features"]],
                entries=[_entry_bytes(m) for m in out["matches"]])


@pytest.fixture(scope="module")
def jobs(ctx):
    """the all-pairs job and the range_width=3 job on the same frames, run once"""
    import synth
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    cams = _cams()
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    full = _job_arrays(StitchJob(ctx, (W, H), cams, config=StitchConfig.hot_path()).run(frames))
    job = StitchJob(ctx, (W, H), cams, config=StitchConfig.hot_path(range_width=3))
    assert job.engine.range_width == 3 and type(job.engine.matcher).__name__ == "BestOf2NearestRangeMatcher"
    band = _job_arrays(job.run(frames))
    return dict(cams=cams, frames=frames, full=full, band=band)


def test_python_job_band_equals_all_pairs_job(jobs):
    import image_stitching_amd as isa
    full, band = jobs["full"], jobs["band"]
    assert isa.selected_pairs(band["nfeat"], 3) == BAND and len(BAND) == 9
    assert band["indices"] == full["indices"] == list(range(N))
    assert band["bands"] == full["bands"] and band["nfeat"] == full["nfeat"]
    assert np.array_equal(band["mask"], full["mask"]) and np.array_equal(band["pano"], full["pano"])
    default = (-1, -1, 0, np.float64(0.0).tobytes(), b"", b"", None)
    sel = set(BAND) | {(j, i) for i, j in BAND}
    for i in range(N):
        for j in range(N):
            k = i * N + j
            if (i, j) in sel:
                assert band["entries"][k] == full["entries"][k] and band["entries"][k][0] == i, (i, j)
                assert band["conf"][k] == full["conf"][k]
            else:
                assert band["entries"][k] == default and band["conf"][k] == 0.0, (i, j)
    # the selection removed something real: the all-pairs job matched the far pairs too
    assert full["entries"][0 * N + 5][0] == 0 and len(full["entries"][0 * N + 3][4]) > 0


def test_cpp_bench_rangewidth_equals_python_job(tmp_path, jobs):
    _build()
    cams_path, prefix = str(tmp_path / "cams.txt"), str(tmp_path / "out")
    write_cams_file(cams_path, jobs["cams"])
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "2", "--warmup", "1", "--dump", prefix, "--rangewidth", "3"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["range_width"] == 3 and line["pairs_matched"] == 9 and line["kept"] == N and line["speculation_kept"] is True
    got, ref = _read_dump(prefix), jobs["band"]
    assert got["indices"] == ref["indices"] and got["nfeat"] == ref["nfeat"] and got["bands"] == ref["bands"]
    assert np.array_equal(got["conf"], ref["conf"])
    assert np.count_nonzero(got["conf"]) <= 2 * len(BAND) and got["conf"][0 * N + 3] == 0.0 and got["conf"][0 * N + 1] > 0.0
    assert np.array_equal(got["mask"], ref["mask"]) and np.array_equal(got["pano"], ref["pano"])


def test_cpp_bench_default_line_reports_all_pairs(tmp_path, jobs):
    _build()
    cams_path = str(tmp_path / "cams.txt")
    write_cams_file(cams_path, jobs["cams"])
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "1", "--warmup", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["range_width"] == -1 and line["pairs_matched"] == 15


def test_width_1_ends_the_jobs_like_an_empty_pruning(tmp_path, ctx, jobs):
    """range_width=1 selects no pair: every confidence is 0, the pruning keeps what it keeps of an unconnected graph (fewer than two
    frames), and the jobs end as they do today in that case -- the C++ job with "Need more images", the Python job with the panorama
    of the kept set, which no longer is the sweep's."""
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig, leaveBiggestComponentConf
    _build()
    cams_path = str(tmp_path / "cams.txt")
    write_cams_file(cams_path, jobs["cams"])
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "1", "--warmup", "0", "--rangewidth", "1"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Need more images" in r.stdout + r.stderr
    kept = [int(i) for i in leaveBiggestComponentConf(np.zeros((N, N)), 0.95)]
    assert len(kept) < 2
    out = StitchJob(ctx, (W, H), jobs["cams"], config=StitchConfig.hot_path(range_width=1)).run(jobs["frames"])
    assert list(out["indices"]) == kept
    assert not np.asarray(out["confidence"].cpu().numpy()).any()
    assert all(m.src_img_idx == -1 and len(m.matches) == 0 and m.H is None for m in out["matches"])
    assert tuple(out["pano"].shape) != jobs["full"]["pano"].shape


def test_stitch_main_rangewidth_equals_python_stitcher(tmp_path, ctx, oracle_mod):
    import torch
    import image_stitching_amd as isa
    _build()
    cams, frames = _write_job(str(tmp_path), oracle_mod, n=5, w=480, h=270)
    size = (frames[0].shape[1], frames[0].shape[0])
    r = subprocess.run([os.path.join(HOST, "stitch_main"), str(tmp_path), "--rangewidth", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _read_ppm(os.path.join(str(tmp_path), "result.ppm"))
    st = isa.Stitcher(ctx, size, isa.StitchConfig.hot_path(compose_megapix=-1, range_width=3))
    assert type(st.matcher).__name__ == "BestOf2NearestRangeMatcher" and st.matcher.range_width == 3
    res, mask, feats, pm, idx = st.stitch([torch.from_numpy(f).cuda() for f in frames], cams)
    assert list(idx) == [0, 1, 2, 3, 4]
    sel = set(isa.selected_pairs([len(f) for f in feats], 3))
    assert len(sel) == 7
    for i in range(5):
        for j in range(5):
            assert (pm[i * 5 + j].src_img_idx >= 0) == ((i, j) in sel or (j, i) in sel), (i, j)
    exp = np.clip(res.cpu().numpy(), 0, 255).astype(np.uint8)
    assert exp.shape == got.shape and np.array_equal(exp, got)
    # the flag reaches the matcher: a width that selects nothing leaves nothing to stitch; a width that is none is refused up front
    r = subprocess.run([os.path.join(HOST, "stitch_main"), str(tmp_path), "--rangewidth", "1"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "Need more images" in r.stdout + r.stderr
    for bad in ("0", "-2"):
        r = subprocess.run([os.path.join(HOST, "stitch_main"), str(tmp_path), "--rangewidth", bad], capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "range_width" in r.stdout + r.stderr and "Features in image" not in r.stdout


def _py_rank_range(rank, world, port, out_path, width):
    """One rank of the Python sharded job with a range_width, on the one GPU (gloo rendezvous)."""
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
        cams = _cams()
        job = StitchJob(isa.Context(0), (W, H), cams, rank=rank, world_size=world, group=dist.group.WORLD, config=StitchConfig.hot_path(range_width=width))
        frames = {i: synth.render_frame_gpu(cams[i]) for i in job.my_frames}
        out = job.run(frames)
        owned = np.array([m.src_img_idx >= 0 for m in out["matches"]])
        np.save(out_path + ".owned%d.npy" % rank, owned)
        if rank == 0:
            np.savez(out_path, pano=out["pano"].cpu().numpy(), mask=out["mask"].cpu().numpy(), conf=out["confidence"].cpu().numpy().reshape(-1),
                     indices=np.array(out["indices"]))
    finally:
        dist.destroy_process_group()


def test_sharded_jobs_rangewidth_equal_single_rank(tmp_path, jobs):
    """The two-rank Python job (gloo, one GPU) and host/stitch_bench --ranks 2 --comm host --one-gpu --rangewidth 3 against the
    single-rank range_width=3 job, byte for byte; the band's pairs are dealt k % 2 over the ranks."""
    import socket
    import torch.multiprocessing as mp
    _build()
    world = 2
    cams_path, prefix = str(tmp_path / "cams.txt"), str(tmp_path / "out")
    write_cams_file(cams_path, jobs["cams"])
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "1", "--warmup", "1", "--ranks", str(world), "--comm", "host",
                        "--one-gpu", "--dump", prefix, "--rangewidth", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert "ShardedJob, %d ranks" % world in line["host"] and line["range_width"] == 3 and line["pairs_matched"] == 9
    got = _read_dump(prefix)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    npz = str(tmp_path / "py.npz")
    mp.start_processes(_py_rank_range, args=(world, port, npz, 3), nprocs=world, join=True, start_method="spawn")
    py = np.load(npz)
    owned = [np.load(npz + ".owned%d.npy" % rk) for rk in range(world)]
    for k, (i, j) in enumerate(BAND):
        assert [bool(o[i * N + j]) for o in owned] == [k % world == rk for rk in range(world)], (i, j)
    assert sum(int(o.sum()) for o in owned) == 2 * len(BAND)
    one = jobs["band"]
    assert got["indices"] == list(py["indices"]) == one["indices"] == list(range(N))
    assert line["kept"] == N and line["speculation_kept"] is True
    assert np.array_equal(got["conf"], py["conf"]) and np.array_equal(got["conf"], one["conf"])
    assert np.array_equal(got["mask"], py["mask"]) and np.array_equal(got["pano"], py["pano"])
    assert np.array_equal(got["mask"], one["mask"])
    d = np.abs(got["pano"].astype(np.int32) - one["pano"].astype(np.int32))
    print("two ranks against one: max |difference| = %d, %d of %d values differ" % (d.max(), int((d > 0).sum()), d.size))
    assert np.array_equal(got["pano"], one["pano"])
