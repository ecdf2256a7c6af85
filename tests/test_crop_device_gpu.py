"""GPU: the device cropper (mis_crop_rect / mis_crop / mis_crop_debug_contour, csrc/crop.hip) against the host cropper --
image_stitching_amd/cropper.py, and host/cropper_tool at the larger size.  Every comparison is exact integer equality: the
rectangle or the error, the chosen contour's point count and first pixel, both coordinate histograms, the filled mask, the cropped
bytes (the strided view and the dense device copy)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import crop_emul  # noqa: E402  (reference(): the stages of cropper.py; nothing of the emulator runs here)

E_INVALID = -1


@pytest.fixture(scope="module")
def crp():
    return crop_emul.cropper()


def _device_result(ctx, t):
    """Every stage the library exposes for a device tensor, as the dict crop_emul.reference gives."""
    from image_stitching_amd import cropper
    dbg = cropper.crop_debug_device(ctx, t)
    got = dict(count=dbg["count"], first=dbg["first"], xhist=dbg["xhist"], yhist=dbg["yhist"], cmask=dbg["cmask"], rounds=dbg["rounds"],
               launches=dbg["launches"])
    try:
        view, rect = cropper.crop_device(ctx, t)
        dense, rect2 = cropper.crop_copy_device(ctx, t)
        assert rect == rect2
        got.update(status=0, rect=rect, view=view.cpu().numpy(), dense=dense.cpu().numpy())
    except ValueError as e:
        got.update(status=1 if "the image is empty" in str(e) else 2, text=str(e))
        assert got["status"] == 1 or "no interior rectangle found" in str(e)
        with pytest.raises(ValueError, match=str(e)):
            cropper.crop_copy_device(ctx, t)
    return got


def _check(ctx, crp, src, tensor=None):
    import torch
    ref = crop_emul.reference(crp, src)
    got = _device_result(ctx, torch.from_numpy(np.ascontiguousarray(src)).cuda() if tensor is None else tensor)
    for k in ("status", "count", "first"):
        assert got[k] == ref[k], (k, got[k], ref[k], src.shape)
    if ref["status"] != 1:
        for k in ("xhist", "yhist", "cmask"):
            assert np.array_equal(got[k], ref[k]), (k, src.shape)
    if ref["status"] == 0:
        x, y, w, h = ref["rect"]
        assert got["rect"] == ref["rect"], (got["rect"], ref["rect"], src.shape)
        assert np.array_equal(got["view"], src[y:y + h, x:x + w]) and np.array_equal(got["dense"], src[y:y + h, x:x + w])
    return got, ref


def test_every_3x3_mask(ctx, crp):
    """All 512 masks, none left out (k = 1): the debug entry, mis_crop_rect and mis_crop on each, measured at 0.36 ms a call on an
    MI355X (0.55 s for the 1 536 calls with their references)."""
    seen = set()
    for bits in range(512):
        m = np.array([(bits >> i) & 1 for i in range(9)], np.uint8).reshape(3, 3) * 255
        got, _ = _check(ctx, crp, m)
        seen.add(got["status"])
    assert seen == {0, 1, 2}


def test_200_random_masks(ctx, crp):
    rng = np.random.default_rng(11)
    for i in range(200):
        h, w = rng.integers(1, 49, 2)
        m = (rng.random((h, w)) < (0.3, 0.5, 0.7, 0.9)[i % 4]).astype(np.uint8) * 255
        _check(ctx, crp, m)


def _blob(seed, h=90, w=140):
    """tests/test_host_cpp.py::_blob: a smooth random blob with a hole and a detached speck"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ang = np.arctan2(yy - h / 2, xx - w / 2)
    rad = np.hypot((yy - h / 2) / (0.42 * h), (xx - w / 2) / (0.42 * w))
    wob = 1 + 0.12 * np.sin(3 * ang + rng.uniform(0, 6)) + 0.07 * np.sin(7 * ang + rng.uniform(0, 6))
    m = (rad < wob).astype(np.uint8) * 255
    m[h // 2 - 5:h // 2 + 5, w // 2 + 8:w // 2 + 20] = 0
    m[2:5, 3:7] = 255
    return m


def _pano_outline():
    """the slanted outline of tests/test_host_cpp.py::test_crop_known_answers_and_cross_language as a BGR image"""
    yy, xx = np.mgrid[0:120, 0:300]
    pano = ((xx > 20 + 0.25 * yy) & (xx < 280 - 0.15 * (120 - yy)) & (yy > 8 + 0.03 * xx) & (yy < 112 - 0.02 * xx))
    img = np.zeros((120, 300, 3), np.uint8)
    img[pano] = (90, 120, 200)
    return img


def _two_specks():
    m = np.zeros((20, 30), np.uint8)
    m[3:6, 20:23] = 255         # raster-first
    m[10:13, 4:7] = 255         # same contour length, further down
    return m


def _ring_with_comb():
    m = np.zeros((40, 60), np.uint8)
    m[2, 2:58] = m[37, 2:58] = 255; m[2:38, 2] = m[2:38, 57] = 255      # the ring, one pixel thick
    m[6, 6:54] = 255                                                    # the comb's spine ...
    m[6:34, 6:54:2] = 255                                               # ... and its teeth, every pixel passed twice
    return m


def _staircase(n=100):
    return (np.eye(n, dtype=np.uint8) * 255)


def _spiral(h=161, w=193):
    """a one-pixel line wound inwards with one-pixel gaps: one component through the whole image"""
    m = np.zeros((h, w), np.uint8)
    x, y, d = 0, 0, 0
    step = ((1, 0), (0, 1), (-1, 0), (0, -1))
    m[0, 0] = 255

    def free(d):
        x1, y1, x2, y2 = x + step[d][0], y + step[d][1], x + 2 * step[d][0], y + 2 * step[d][1]
        return 0 <= x1 < w and 0 <= y1 < h and not m[y1, x1] and not (0 <= x2 < w and 0 <= y2 < h and m[y2, x2])

    while True:
        if not free(d):
            d = (d + 1) % 4
            if not free(d):
                return m
        x, y = x + step[d][0], y + step[d][1]
        m[y, x] = 255


def _grey_border():
    img = np.zeros((14, 19, 3), np.uint8)
    img[2:12, 3:16] = (40, 90, 20)
    img[1, 3:16] = (1, 0, 0); img[12, 3:16] = (0, 0, 4); img[2:12, 2] = (0, 1, 0)      # grey 0, grey 0, grey 1
    return img


STRUCTURED = {
    "blob-hole-speck": lambda: _blob(1),
    "pano-outline-bgr": _pano_outline,
    "full-64x64": lambda: np.full((64, 64), 255, np.uint8),
    "full-65x129": lambda: np.full((65, 129), 255, np.uint8),
    "row-1x200": lambda: np.full((1, 200), 255, np.uint8),
    "column-200x1": lambda: np.full((200, 1), 255, np.uint8),
    "two-equal-specks": _two_specks,
    "ring-with-comb": _ring_with_comb,
    "staircase-100": _staircase,
    "grey-border-bgr": _grey_border,
}


@pytest.mark.parametrize("name", sorted(STRUCTURED))
def test_structured_mask(ctx, crp, name):
    src = STRUCTURED[name]()
    got, ref = _check(ctx, crp, src)
    w = src.shape[1]
    if name == "two-equal-specks":
        assert [c[1] for c in ref["contours"]] == [8, 8] and got["first"] == 3 * w + 20
    if name == "ring-with-comb":
        comb = src.copy(); comb[2, :] = comb[37, :] = 0; comb[:, 2] = comb[:, 57] = 0
        assert len(crp.findExternalContours(comb)[0]) > got["count"] and got["first"] == 2 * w + 2      # the longer contour is nested
    if name == "grey-border-bgr":
        assert got["rect"][:2] == (2, 2)


def test_spiral_needs_15_doubling_rounds(ctx, crp):
    from scipy import ndimage as ndi
    src = _spiral()
    assert src.shape == (161, 193) and ndi.label(src > 0, structure=np.ones((3, 3)))[1] == 1
    got, ref = _check(ctx, crp, src)
    assert ref["count"] > 1 << 14 and got["rounds"] >= 15


def test_strided_slice_equals_its_contiguous_copy(ctx, crp):
    import torch
    for src in (_pano_outline(), _blob(2)):
        big = torch.full((src.shape[0] + 7, src.shape[1] + 9) + src.shape[2:], 200, dtype=torch.uint8, device="cuda")
        view = big[3:3 + src.shape[0], 4:4 + src.shape[1]]
        view.copy_(torch.from_numpy(src))
        assert not view.is_contiguous()
        a, _ = _check(ctx, crp, src, tensor=view)
        b, _ = _check(ctx, crp, src)
        assert a["rect"] == b["rect"] and np.array_equal(a["cmask"], b["cmask"])


def test_mid_size_tool_crop_device_equals_crop(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "host"), "cropper_tool"])
    tool = os.path.join(ROOT, "host", "cropper_tool")
    h, w = 777, 2051
    yy, xx = np.mgrid[0:h, 0:w]
    m = ((yy > 30 + 25 * np.sin(xx / 90.0)) & (yy < h - 40 + 30 * np.sin(xx / 130.0 + 1)) & (xx > 25 + 20 * np.sin(yy / 60.0)) & (xx < w - 35 + 25 * np.sin(yy / 75.0 + 2)))
    m[300:380, 900:1100] = False        # a hole
    src = str(tmp_path / "m.pgm")
    with open(src, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (w, h))
        f.write((m.astype(np.uint8) * 255).tobytes())
    host, dev = str(tmp_path / "host.pgm"), str(tmp_path / "dev.pgm")
    want = subprocess.check_output([tool, "crop", src, host])
    got = subprocess.check_output([tool, "crop_device", src, dev])
    assert got == want and len(want.split()) == 4
    assert open(dev, "rb").read() == open(host, "rb").read()


def test_crop_panorama_on_the_smoke_job(ctx, crp):
    import torch
    import image_stitching_amd as isa
    import synth
    from image_stitching_amd.distributed import StitchJob
    w, h = 480, 270
    cams = [synth.make_camera(w, h, 60.0, 14.0 * i - 14.0, 0.4 * (i - 1), 0.3 * i) for i in range(3)]
    frames = [synth.render_frame(c) for c in cams]
    out = StitchJob(ctx, (w, h), cams).run({i: torch.from_numpy(f).cuda() for i, f in enumerate(frames)})
    pano, mask, rect = isa.Stitcher(ctx, (w, h)).crop_panorama(out["pano"], out["mask"])
    _, want = crp.crop(out["mask"].cpu().numpy())
    assert rect == tuple(int(v) for v in want)
    x, y, rw, rh = rect
    assert tuple(pano.shape[:2]) == tuple(mask.shape) == (rh, rw)
    assert torch.equal(pano, out["pano"][y:y + rh, x:x + rw])
    mk = mask.cpu().numpy()
    assert mk[0].all() and mk[-1].all() and mk[:, 0].all() and mk[:, -1].all()


def test_error_contract(ctx, crp):
    import torch
    src = _blob(3)
    t = torch.from_numpy(src).cuda()
    lib, rect, status = ctx.lib, (C.c_int * 4)(), C.c_int()
    p, (h, w) = C.c_void_p(t.data_ptr()), src.shape
    xh, yh, cm = (C.c_int32 * w)(), (C.c_int32 * h)(), (C.c_uint8 * (w * h))()
    cnt, first = C.c_int(), C.c_int()
    bad = [
        lib.mis_crop_rect(ctx.h, None, w, h, 1, w, rect, C.byref(status)),
        lib.mis_crop_rect(ctx.h, p, w, h, 1, w, None, C.byref(status)),
        lib.mis_crop_rect(ctx.h, p, w, h, 1, w, rect, None),
        lib.mis_crop_rect(ctx.h, p, w, h, 2, 2 * w, rect, C.byref(status)),
        lib.mis_crop_rect(ctx.h, p, 0, h, 1, w, rect, C.byref(status)),
        lib.mis_crop_rect(ctx.h, p, w, -1, 1, w, rect, C.byref(status)),
        lib.mis_crop_rect(ctx.h, p, w, h, 1, w - 1, rect, C.byref(status)),
        lib.mis_crop_rect(ctx.h, p, 1 << 14, 1 << 14, 1, 1 << 14, rect, C.byref(status)),      # beyond the 32-bit state indices
        lib.mis_crop(ctx.h, p, w, h, 1, w, None, w, rect, C.byref(status)),
        lib.mis_crop(ctx.h, p, w, h, 1, w, p, w - 1, rect, C.byref(status)),
        lib.mis_crop_debug_contour(ctx.h, p, w, h, 1, w, C.byref(cnt), C.byref(first), xh, yh, None),
        lib.mis_crop_debug_contour(ctx.h, p, w, h, 1, w, None, C.byref(first), xh, yh, cm),
    ]
    assert bad == [E_INVALID] * len(bad)
    assert lib.mis_last_error(ctx.h)
    _check(ctx, crp, src, tensor=t)         # the context is as usable as before


def test_stitch_main_crop_writes_the_rectangle(tmp_path, crp, oracle_mod):
    """stitch_main <dir> --crop --jpeg: result.ppm, result_mask.pgm and result.jpg are the printed rectangle of what the driver
    writes without the flag, and the rectangle is the host cropper's on the result mask."""
    import image_stitching_amd as isa
    import test_host_cpp as thc
    thc._build()
    exe = os.path.join(ROOT, "host", "stitch_main")
    d = str(tmp_path)
    thc._write_job(d, oracle_mod)
    r = subprocess.run([exe, d], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    full, full_mask = thc._read_pnm(os.path.join(d, "result.ppm")), thc._read_pnm(os.path.join(d, "result_mask.pgm"))
    r = subprocess.run([exe, d, "--crop", "--jpeg"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [ln for ln in r.stdout.split("\n") if ln.startswith("crop ")]
    assert len(line) == 1
    x, y, w, h = rect = tuple(int(v) for v in line[0].split()[1:])
    assert rect == tuple(int(v) for v in crp.crop(full_mask)[1])
    assert np.array_equal(thc._read_pnm(os.path.join(d, "result.ppm")), full[y:y + h, x:x + w])
    assert np.array_equal(thc._read_pnm(os.path.join(d, "result_mask.pgm")), full_mask[y:y + h, x:x + w])
    info = isa.jpeg_info(open(os.path.join(d, "result.jpg"), "rb").read())
    assert (info["width"], info["height"]) == (w, h)
