"""tests/harness/jpeg_enc_host_harness.cpp, built by the host compiler alone: jpeg_enc_core.h's per-pixel and per-block functions --
the source the kernels of jpeg_enc.hip compile -- and jpeg_enc_host.h's coder give Pillow's stream of every fixture on the CPU, and
the coder's stress cases (all-zero and extreme planes, 1 x 1, more chunks than MCU rows, a restart interval of 1) pass."""
import os
import subprocess

import numpy as np
import pytest

from test_refimpl_jpeg_enc_cpu import NAMES, fixture

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLING = {"420": 0, "422": 1, "444": 2}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpegencharness") / "jpeg_enc_host_harness")
    r = subprocess.run(["c++", "-O2", "-std=c++17", os.path.join(HERE, "harness", "jpeg_enc_host_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("name", NAMES)
def test_host_twin_of_the_kernels_equals_pillow(harness, tmp_path, name):
    f, src, jpg, _ = fixture(name)
    raw, out = str(tmp_path / "in.bgr"), str(tmp_path / "out.jpg")
    np.ascontiguousarray(src[:, :, ::-1]).tofile(raw)
    args = [str(v) for v in (f["width"], f["height"], f["quality"], SAMPLING[f["sampling"]], f["restart_interval"], 3)]
    r = subprocess.run([harness, "encode"] + args + [raw, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert open(out, "rb").read() == jpg


def test_stress_cases(harness):
    r = subprocess.run([harness, "stress"], capture_output=True, text=True)
    assert r.returncode == 0 and "stress OK" in r.stdout, r.stdout + r.stderr
