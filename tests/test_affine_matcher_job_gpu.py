"""matcher_type = "affine" through the jobs, on the six-frame 640 x 360 sweep of tests/test_range_matcher_job_gpu.py: the Python
StitchJob with StitchConfig.hot_path(matcher_type="affine"), the C++ job (host/stitch_bench --matcher affine), the C++ pipeline
(host/stitch_main --matcher affine) and the two-rank sharded jobs against it, byte for byte; the options that are refused."""
import json
import os
import subprocess

import numpy as np
import pytest

from test_host_cpp import HOST, _build, _read_dump, _read_ppm, _write_job, write_cams_file
from test_range_matcher_job_gpu import H, N, W, _cams, _entry_bytes, _job_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def jobs(ctx):
    """the affine job on the sweep, run twice"""
    import synth
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    cams = _cams()
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    job = StitchJob(ctx, (W, H), cams, config=StitchConfig.hot_path(matcher_type="affine"))
    assert job.engine.matcher_type == "affine" and type(job.engine.matcher).__name__ == "AffineBestOf2NearestMatcher"
    out = job.run(frames)
    direct = [_entry_bytes(m) for m in job.engine.matcher(out["features"])]
    first = _job_arrays(out)
    second = _job_arrays(job.run(frames))
    return dict(cams=cams, frames=frames, first=first, second=second, direct=direct)


def test_python_job_runs_the_affine_matcher(jobs):
    a, b = jobs["first"], jobs["second"]
    assert a["indices"] == list(range(N))                                       # all six frames are kept
    assert a["entries"] == jobs["direct"]                                       # the job's entries are a direct matcher call's
    assert a["entries"] == b["entries"] and a["indices"] == b["indices"] and np.array_equal(a["conf"], b["conf"])
    assert np.array_equal(a["pano"], b["pano"]) and np.array_equal(a["mask"], b["mask"])
    for k, e in enumerate(a["entries"]):
        if e[6] is not None and k // N < k % N:                                 # the entries (i, j), i < j; a mirror holds the inverse
            Hm = np.frombuffer(e[6], np.float64).reshape(3, 3)
            assert (Hm[2] == (0.0, 0.0, 1.0)).all() and Hm[0, 0] == Hm[1, 1] and Hm[0, 1] == -Hm[1, 0], k
            inv = np.frombuffer(a["entries"][(k % N) * N + k // N][6], np.float64).reshape(3, 3)
            assert np.abs(inv @ Hm - np.eye(3)).max() <= 1e-9, k
    assert a["conf"][0 * N + 1] > 0.95


def test_cpp_bench_matcher_affine_equals_python_job(tmp_path, jobs):
    _build()
    cams_path, prefix = str(tmp_path / "cams.txt"), str(tmp_path / "out")
    write_cams_file(cams_path, jobs["cams"])
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "2", "--warmup", "1", "--dump", prefix, "--matcher", "affine"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["kept"] == N and line["pairs_matched"] == 15
    got, ref = _read_dump(prefix), jobs["first"]
    assert got["indices"] == ref["indices"] and got["nfeat"] == ref["nfeat"] and got["bands"] == ref["bands"]
    assert np.array_equal(got["conf"], ref["conf"])
    assert np.array_equal(got["mask"], ref["mask"]) and np.array_equal(got["pano"], ref["pano"])


def test_refused_options_name_themselves(tmp_path, jobs):
    _build()
    cams_path = str(tmp_path / "cams.txt")
    write_cams_file(cams_path, jobs["cams"])
    for tool, lead in (("stitch_bench", [cams_path]), ("stitch_main", [str(tmp_path)])):
        r = subprocess.run([os.path.join(HOST, tool)] + lead + ["--matcher", "affine", "--rangewidth", "3"], capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "range_width" in r.stdout + r.stderr and "affine" in r.stdout + r.stderr, tool
        r = subprocess.run([os.path.join(HOST, tool)] + lead + ["--matcher", "nonsense"], capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and "matcher_type" in r.stdout + r.stderr and "nonsense" in r.stdout + r.stderr, tool
        assert "Features in image" not in r.stdout


def test_stitch_main_matcher_affine_equals_python_stitcher(tmp_path, ctx, oracle_mod):
    import torch
    import image_stitching_amd as isa
    _build()
    cams, frames = _write_job(str(tmp_path), oracle_mod, n=5, w=480, h=270)
    size = (frames[0].shape[1], frames[0].shape[0])
    r = subprocess.run([os.path.join(HOST, "stitch_main"), str(tmp_path), "--matcher", "affine"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _read_ppm(os.path.join(str(tmp_path), "result.ppm"))
    st = isa.Stitcher(ctx, size, isa.StitchConfig.hot_path(compose_megapix=-1, matcher_type="affine"))
    assert type(st.matcher).__name__ == "AffineBestOf2NearestMatcher"
    res, mask, feats, pm, idx = st.stitch([torch.from_numpy(f).cuda() for f in frames], cams)
    assert list(idx) == [0, 1, 2, 3, 4]
    exp = np.clip(res.cpu().numpy(), 0, 255).astype(np.uint8)
    assert exp.shape == got.shape and np.array_equal(exp, got)


def _py_rank_affine(rank, world, port, out_path):
    """One rank of the Python sharded job with the affine matcher, on the one GPU (gloo rendezvous)."""
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
        job = StitchJob(isa.Context(0), (W, H), cams, rank=rank, world_size=world, group=dist.group.WORLD, config=StitchConfig.hot_path(matcher_type="affine"))
        frames = {i: synth.render_frame_gpu(cams[i]) for i in job.my_frames}
        out = job.run(frames)
        if rank == 0:
            np.savez(out_path, pano=out["pano"].cpu().numpy(), mask=out["mask"].cpu().numpy(), conf=out["confidence"].cpu().numpy().reshape(-1),
                     indices=np.array(out["indices"]))
    finally:
        dist.destroy_process_group()


def test_sharded_jobs_matcher_affine_equal_single_rank(tmp_path, jobs):
    """The two-rank Python job (gloo, one GPU) and host/stitch_bench --ranks 2 --comm host --one-gpu --matcher affine against the
    single-rank affine job, byte for byte."""
    import socket
    import torch.multiprocessing as mp
    _build()
    world = 2
    cams_path, prefix = str(tmp_path / "cams.txt"), str(tmp_path / "out")
    write_cams_file(cams_path, jobs["cams"])
    r = subprocess.run([os.path.join(HOST, "stitch_bench"), cams_path, "--steps", "1", "--warmup", "1", "--ranks", str(world), "--comm", "host",
                        "--one-gpu", "--dump", prefix, "--matcher", "affine"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    line = json.loads([l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1])
    assert "ShardedJob, %d ranks" % world in line["host"] and line["kept"] == N
    got = _read_dump(prefix)
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    npz = str(tmp_path / "py.npz")
    mp.start_processes(_py_rank_affine, args=(world, port, npz), nprocs=world, join=True, start_method="spawn")
    py = np.load(npz)
    one = jobs["first"]
    assert got["indices"] == list(py["indices"]) == one["indices"] == list(range(N))
    assert np.array_equal(got["conf"], py["conf"]) and np.array_equal(got["conf"], one["conf"])
    assert np.array_equal(got["mask"], py["mask"]) and np.array_equal(got["pano"], py["pano"])
    assert np.array_equal(got["mask"], one["mask"]) and np.array_equal(got["pano"], one["pano"])
