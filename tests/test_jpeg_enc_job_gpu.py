"""JPEG output of the host tool, on the three 480 x 270 frames of tests/golden/jpeg/job: `stitch_main <dir> --jpeg` writes result.jpg,
byte for byte the numpy reference's encode (quality 95, 4:2:0: cv::imwrite's defaults) of the result.ppm the same run wrote, and
leaves result.ppm and result_mask.pgm what a run without the flag writes; the flag works the same in the mode without supplied
cameras (--estimator homography --ba ray), there with a quality given."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import refimpl_jpeg_enc as ref
from test_host_cpp import HOST, _build

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
JOB = os.path.join(HERE, "golden", "jpeg", "job")
N = 3


def _job_dir(path):
    for k in range(N):
        shutil.copy(os.path.join(JOB, "%d.jpg" % (k + 1)), path)
        shutil.copy(os.path.join(JOB, "%d.txt" % (k + 1)), path)
    return path


def _run(directory, *options):
    r = subprocess.run([os.path.join(HOST, "stitch_main"), directory, *options], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "kept 3 of 3 images" in r.stdout
    return r


def _read_ppm(path):
    with open(path, "rb") as fh:
        assert fh.readline() == b"P6\n"
        w, h = [int(v) for v in fh.readline().split()]
        assert fh.readline() == b"255\n"
        return np.frombuffer(fh.read(), np.uint8).reshape(h, w, 3)


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_stitch_main_writes_result_jpg(tmp_path):
    _build()
    plain, flagged = str(tmp_path / "plain"), str(tmp_path / "flagged")
    for d in (plain, flagged):
        os.makedirs(d)
        _job_dir(d)
    _run(plain)
    _run(flagged, "--jpeg")
    assert not os.path.exists(os.path.join(plain, "result.jpg"))
    for name in ("result.ppm", "result_mask.pgm", "cams.data"):
        assert _read(os.path.join(flagged, name)) == _read(os.path.join(plain, name)), name
    rgb = _read_ppm(os.path.join(flagged, "result.ppm"))
    assert rgb.shape[0] * rgb.shape[1] > 480 * 270
    assert _read(os.path.join(flagged, "result.jpg")) == ref.encode(rgb, 95, "420", 0)


def test_the_flag_does_not_depend_on_the_mode(tmp_path):
    _build()
    d = _job_dir(str(tmp_path))
    _run(d, "--estimator", "homography", "--ba", "ray", "--jpeg", "60")
    rgb = _read_ppm(os.path.join(d, "result.ppm"))
    assert _read(os.path.join(d, "result.jpg")) == ref.encode(rgb, 60, "420", 0)


def test_the_flag_closes_the_command_line(tmp_path):
    _build()
    exe = os.path.join(HOST, "stitch_main")
    for bad in (["--jpeg", "--mode", "scans"], ["--jpeg", "0"], ["--jpeg", "101"], ["--jpeg", "high"]):
        r = subprocess.run([exe, str(tmp_path)] + bad, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--jpeg" in r.stdout, (bad, r.stdout)
