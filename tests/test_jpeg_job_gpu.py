"""JPEG ingest through the jobs, on the three 480 x 270 frames of tests/golden/jpeg/job (test_host_cpp._write_job's sweep, encoded
4:2:0 by tools/make_jpeg_fixtures.py; <k>.npz is Pillow's decode, <k>.txt the camera):

  * isa.imread_batch of the .jpg files gives Pillow's pixels, and Stitcher.stitch of those device frames equals the stitch of the
    .npz arrays: panorama, mask, kept indices, feature counts;
  * host/stitch_main on a directory of <k>.jpg alone writes the result.ppm, result_mask.pgm and cams.data of a directory that holds
    the decoded pixels as <k>.ppm;
  * a directory with both <k>.ppm and <k>.jpg reads its pixels from the .ppm as before (the .jpg files there are other frames)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_host_cpp import HOST, _build

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
JOB = os.path.join(HERE, "golden", "jpeg", "job")
W, H, N = 480, 270, 3
OUTPUTS = ("result.ppm", "result_mask.pgm", "cams.data")


@pytest.fixture(scope="module")
def decoded():
    """Pillow's decode of the job's frames, BGR"""
    return [np.ascontiguousarray(np.load(os.path.join(JOB, "%d.npz" % (k + 1)))["rgb"][:, :, ::-1]) for k in range(N)]


def _cams(oracle_mod):
    import synth
    cams = []
    for i in range(N):
        c = dict(synth.make_camera(W, H, 60.0, 14.0 * i - 10.0, 0.5 * (i - 1), -0.3 * i))
        c["R"] = oracle_mod.camera_rehand(oracle_mod.camera_rehand(c["R"], False), False)       # what stitch_main uses (_write_job)
        cams.append(c)
    return cams


def test_manifest_job_set():
    m = json.load(open(os.path.join(HERE, "golden", "jpeg", "MANIFEST.json")))
    assert [e["name"] for e in m["job"]] == ["job/1", "job/2", "job/3"]
    for k in range(N):
        assert os.path.getsize(os.path.join(JOB, "%d.jpg" % (k + 1))) <= 64 * 1024


def test_imread_batch_feeds_the_stitcher(ctx, oracle_mod, decoded):
    import torch
    import image_stitching_amd as isa
    frames = isa.imread_batch(ctx, [os.path.join(JOB, "%d.jpg" % (k + 1)) for k in range(N)])
    for f, d in zip(frames, decoded):
        assert f.is_cuda and np.array_equal(f.cpu().numpy(), d)
    cams = _cams(oracle_mod)
    cfg = isa.StitchConfig.hot_path(compose_megapix=-1)
    res, mask, feats, pm, idx = isa.Stitcher(ctx, (W, H), cfg).stitch(frames, cams)
    eres, emask, efeats, epm, eidx = isa.Stitcher(ctx, (W, H), cfg).stitch([torch.from_numpy(d).cuda() for d in decoded], cams)
    assert list(idx) == list(eidx) == [0, 1, 2]
    assert [len(f) for f in feats] == [len(f) for f in efeats] and min(len(f) for f in feats) > 100
    assert np.array_equal(res.cpu().numpy(), eres.cpu().numpy()) and np.array_equal(mask.cpu().numpy(), emask.cpu().numpy())
    assert mask.cpu().numpy().any()


def _write_ppm(path, bgr):
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (bgr.shape[1], bgr.shape[0]))
        fh.write(bgr[:, :, ::-1].tobytes())


def _run_stitch_main(directory):
    r = subprocess.run([os.path.join(HOST, "stitch_main"), directory], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "kept 3 of 3 images" in r.stdout
    return {name: open(os.path.join(directory, name), "rb").read() for name in OUTPUTS}


@pytest.fixture(scope="module")
def ppm_run(tmp_path_factory, decoded):
    """stitch_main on the decoded pixels as <k>.ppm"""
    _build()
    d = str(tmp_path_factory.mktemp("jpegjob_ppm"))
    for k in range(N):
        _write_ppm(os.path.join(d, "%d.ppm" % (k + 1)), decoded[k])
        shutil.copy(os.path.join(JOB, "%d.txt" % (k + 1)), d)
    return _run_stitch_main(d)


def test_stitch_main_reads_a_directory_of_jpeg_frames(tmp_path, ppm_run):
    for k in range(N):
        shutil.copy(os.path.join(JOB, "%d.jpg" % (k + 1)), str(tmp_path))
        shutil.copy(os.path.join(JOB, "%d.txt" % (k + 1)), str(tmp_path))
    got = _run_stitch_main(str(tmp_path))
    for name in OUTPUTS:
        assert got[name] == ppm_run[name], name
    assert len(got["result.ppm"]) > W * H * 3


def test_ppm_frames_beside_jpeg_files_are_still_the_frames(tmp_path, decoded, ppm_run):
    """<k>.ppm with <k>.jpg beside it: the pixels are the .ppm's (here the .jpg files are the sweep in reverse order, and carry no EXIF,
    so the cameras come from <k>.txt)"""
    for k in range(N):
        _write_ppm(str(tmp_path / ("%d.ppm" % (k + 1))), decoded[k])
        shutil.copy(os.path.join(JOB, "%d.jpg" % (N - k)), str(tmp_path / ("%d.jpg" % (k + 1))))
        shutil.copy(os.path.join(JOB, "%d.txt" % (k + 1)), str(tmp_path))
    got = _run_stitch_main(str(tmp_path))
    for name in OUTPUTS:
        assert got[name] == ppm_run[name], name


def test_stitch_main_names_a_refused_jpeg(tmp_path):
    _build()
    shutil.copy(os.path.join(JOB, "1.jpg"), str(tmp_path / "1.jpg"))
    shutil.copy(os.path.join(HERE, "golden", "jpeg", "refuse_progressive.jpg"), str(tmp_path / "2.jpg"))
    r = subprocess.run([os.path.join(HOST, "stitch_main"), str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "2.jpg" in r.stdout and "SOF2" in r.stdout
