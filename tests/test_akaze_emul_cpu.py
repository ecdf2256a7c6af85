"""csrc/akaze_core.h on the host: tools/micro/akaze_emul.cpp runs the AKAZE finder's kernels element by element in their launch
order, as a stand-alone program built with the address and undefined-behaviour sanitizers, and tests/akaze_check.py judges its
planes, schedules, counts, keypoints and descriptors against tests/refimpl_akaze.py by the rules the library meets on the GPU
(tests/test_akaze_gpu.py): the same shapes, bands and caps."""
import importlib.util
import os

import pytest

import akaze_check as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("_akaze_emul", os.path.join(ROOT, "tools", "akaze_emul.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every case of akaze_check.cases() through ONE sanitized run of the emulation (a non-zero exit fails here)"""
    tool = _tool()
    tmp = str(tmp_path_factory.mktemp("akaze_emul"))
    cases = ac.cases()
    return cases, tool.run(tool.build(tmp, sanitize=True), tmp, [(c["frame"], c["kw"]) for c in cases])


@pytest.mark.parametrize("i", range(8))
def test_emulation_meets_the_reference(runs, i):
    cases, got = runs
    assert len(cases) == 8
    c = cases[i]
    rep = ac.check_run(c["tag"], c["frame"], c["kw"], got[i])
    print(c["tag"], rep)


def test_the_cases_find_keypoints(runs):
    """the shapes are not vacuous: the large frames have hundreds of keypoints, max_points cuts to exactly 50, a high threshold to none"""
    cases, got = runs
    n = {c["tag"]: len(g["kps"]) for c, g in zip(cases, got)}
    assert n["640x320 four octaves, sixteen levels"] > 500 and n["333x251 three octaves, fractional area average"] > 100
    assert n["640x320 max_points 50"] == 50 and n["333x251 threshold 0.01"] == 0 and n["333x251 three layers"] > 100
