"""The device cropper without a GPU: the per-element steps of csrc/crop.hip (csrc/crop_core.h) run on the host by
tools/micro/crop_emul.cpp -- a stand-alone program built with the address and undefined-behaviour sanitizers -- in the kernels'
launch order, against image_stitching_amd/cropper.py stage by stage: every external contour (first pixel, length), the chosen one
with its points' multiplicity and histograms, the filled mask, the rectangle or the error.  Also the new C ABI entries and their
bindings, and stitch_main's refusal of --crop with --timelapse."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import crop_emul  # noqa: E402

ENTRIES = ("mis_crop_rect", "mis_crop", "mis_crop_debug_contour", "mis_crop_stats")


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("crop_emul"))
    return crop_emul.build(tmp), tmp


def _compare(emul, sources):
    crp = crop_emul.cropper()
    got = crop_emul.run(*emul, sources)
    bad = []
    for s, g in zip(sources, got):
        d = crop_emul.differences(g, crop_emul.reference(crp, s))
        if d:
            bad.append((s.tolist(), d))
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(sources), bad[0])
    return got


def test_every_4x4_mask(emul):
    bits = np.arange(1 << 16, dtype=np.uint32)
    masks = (((bits[:, None] >> np.arange(16, dtype=np.uint32)[None, :]) & 1).astype(np.uint8) * 255).reshape(-1, 4, 4)
    got = _compare(emul, list(masks))
    assert {g["status"] for g in got} == {0, 1, 2}        # a rectangle, the empty image and "no interior rectangle" all occur


def test_500_random_masks_up_to_40(emul):
    got = _compare(emul, crop_emul.random_masks(500, 40, seed=7))
    assert max(len(g["contours"]) for g in got) > 10 and max(g["mult"].max() for g in got) >= 2     # many contours, points passed twice


def test_bgr_grey_formula_decides_the_foreground(emul):
    """BGR (1, 0, 0) and (0, 0, 4) have grey 0 (exterior) though a channel is set; (0, 1, 0) has grey 1."""
    img = np.zeros((12, 17, 3), np.uint8)
    img[2:10, 3:14] = (40, 90, 20)
    img[1, 3:14] = (1, 0, 0); img[10, 3:14] = (0, 0, 4); img[2:10, 2] = (0, 1, 0)
    got = _compare(emul, [img, np.ascontiguousarray(img[:, :, 0])])
    assert got[0]["rect"][:2] == (2, 2)


def test_the_library_exports_and_binds_the_new_entries():
    from image_stitching_amd import _capi
    lib = _capi.load()
    header = _capi.header_functions()
    for name in ENTRIES:
        assert name in header and name in _capi.PROTOTYPES and hasattr(lib, name)
    text = open(_capi.HEADER_PATH).read()
    for name in ENTRIES:        # every entry cites the reference lines it replaces
        doc = text[:text.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert re.search(r"cropper\.cpp:\d+", doc), name
    # a null context is refused before anything else
    assert lib.mis_crop_rect(None, None, 4, 4, 1, 4, (C.c_int * 4)(), C.byref(C.c_int())) == _capi.MIS_E_INVALID


def test_python_names():
    import image_stitching_amd as isa
    from image_stitching_amd import cropper, stitching
    assert isa.crop_device is stitching.crop_device is cropper.crop_device
    assert isa.crop_rect_device is stitching.crop_rect_device is cropper.crop_rect_device
    assert callable(isa.Stitcher.crop_panorama)
    assert "crop" not in {f for f in isa.StitchConfig.__dataclass_fields__}       # a call on the result, not a configuration


def test_stitch_main_refuses_crop_with_timelapse(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "stitch_main"])
    for args in (["--crop", "--timelapse"], ["--timelapse", "as_is", "--crop"]):
        r = subprocess.run([os.path.join(ROOT, "host", "stitch_main"), str(tmp_path), *args], capture_output=True, text=True)
        assert r.returncode != 0 and "--timelapse with --crop" in r.stdout, r.stdout
