"""The JPEG decode's host layer, pinned without a GPU.

  * tests/refimpl_jpeg.py (an independent numpy decoder written from the arithmetic: parser, Huffman, int64 islow IDCT, triangle
    upsampling, fixed-point colour) equals Pillow's (libjpeg-turbo's) decode of every fixture in tests/golden/jpeg byte for byte --
    against the committed .npy, and against PIL itself where it is installed;
  * mis_jpeg_info and mis_jpeg_debug_coefficients (no context, no device): geometry, quantisation tables and every coefficient
    of every fixture equal the reference's;
  * refusals at the host layer: each refusal fixture returns its code and names its cause; every proper prefix of the 17 x 13
    file is refused, never decoded;
  * tests/harness/jpeg_host_harness.cpp runs jpeg_core.h's per-block and per-pixel functions -- the source the kernels compile --
    over the decoded coefficients on the CPU: the pixels equal the .npy."""
import ctypes as C
import io
import json
import os
import subprocess

import numpy as np
import pytest

import refimpl_jpeg as rj

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
DECODE = [e["name"] for e in MANIFEST["decode"]]
REFUSE = [(e["name"], e["code"], e["cause"]) for e in MANIFEST["refuse"]]
# what the error text must say for each cause of the manifest
CAUSE_TEXT = {"SOF2": "SOF2", "4 components": "4 components", "truncated": "truncated"}


def stream(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as fh:
        return fh.read()


def expected_rgb(name):
    return np.load(os.path.join(GOLDEN, name + ".npy"))


@pytest.fixture(scope="module")
def lib():
    from image_stitching_amd import _capi
    return _capi.load()


def host_coefficients(lib, data, component, nblocks):
    out = np.full(nblocks * 64, 0x5555, np.int16)
    q = np.zeros(64, np.uint16)
    rc = lib.mis_jpeg_debug_coefficients(data, len(data), component, out.ctypes.data, out.size, q.ctypes.data)
    return rc, out, q


def test_manifest_lists_the_issue_s_sets():
    assert len(DECODE) == 17 and len(REFUSE) == 3 and len(MANIFEST["job"]) == 3
    assert MANIFEST["pillow"] and MANIFEST["libjpeg_turbo"]
    for e in MANIFEST["decode"]:
        px = expected_rgb(e["name"])
        assert px.shape[:2] == (e["height"], e["width"]) and px.dtype == np.uint8
        assert os.path.getsize(os.path.join(GOLDEN, e["name"] + ".jpg")) <= 64 * 1024


@pytest.mark.parametrize("name", DECODE)
def test_reference_equals_pillow_decode(name):
    got = rj.decode(stream(name))
    want = expected_rgb(name)
    assert got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("name", DECODE)
def test_reference_equals_pil_where_installed(name):
    Image = pytest.importorskip("PIL.Image")
    data = stream(name)
    want = np.asarray(Image.open(io.BytesIO(data)))
    assert np.array_equal(rj.decode(data), want) and np.array_equal(expected_rgb(name), want)


@pytest.mark.parametrize("name", DECODE)
def test_host_layer_equals_reference(lib, name):
    from image_stitching_amd import _capi
    data = stream(name)
    ref_info, ref_planes, ref_tables = rj.coefficients(data)
    info = _capi.MisJpegInfo()
    assert lib.mis_jpeg_info(data, len(data), C.byref(info)) == _capi.MIS_OK
    nc = info.components
    got_info = dict(width=info.width, height=info.height, components=nc, h=list(info.h)[:nc], v=list(info.v)[:nc], restart_interval=info.restart_interval)
    assert got_info == ref_info
    for c in range(nc):
        want = ref_planes[c].reshape(-1)
        rc, got, q = host_coefficients(lib, data, c, want.size // 64)
        assert rc == _capi.MIS_OK, lib.mis_jpeg_last_error()
        assert np.array_equal(got, want), "component %d" % c
        assert np.array_equal(q, ref_tables[c])
        # a capacity one coefficient short is refused and writes nothing
        short = np.full(want.size - 1, 0x5555, np.int16)
        assert lib.mis_jpeg_debug_coefficients(data, len(data), c, short.ctypes.data, short.size, q.ctypes.data) == _capi.MIS_E_INVALID
        assert (short == 0x5555).all()
    rc, _, _ = host_coefficients(lib, data, nc, 1 << 16)
    assert rc == _capi.MIS_E_INVALID


def test_restart_fixtures_have_restart_markers():
    """the restart cases are what they claim: DRI set, and intervals that cross MCU rows in the 131 x 77 file (9 MCUs per row)"""
    assert rj.info(stream("64x48_420_q60_dri2"))["restart_interval"] == 2
    assert rj.info(stream("131x77_420_q92_dri3"))["restart_interval"] == 3 and -(-131 // 16) == 9
    assert rj.info(stream("47x31_420_q30_rows1"))["restart_interval"] == 3      # one MCU row of a 47-wide 4:2:0 file
    assert rj.info(stream("47x31_420_q5_dri1"))["restart_interval"] == 1


@pytest.mark.parametrize("name,code,cause", REFUSE)
def test_refusals_name_their_cause(lib, name, code, cause):
    from image_stitching_amd import _capi
    data = stream(name)
    want = getattr(_capi, code)
    out = np.full(1 << 16, 0x5555, np.int16)
    q = np.zeros(64, np.uint16)
    rc = lib.mis_jpeg_debug_coefficients(data, len(data), 0, out.ctypes.data, out.size, q.ctypes.data)
    assert rc == want and CAUSE_TEXT[cause] in lib.mis_jpeg_last_error().decode()
    assert (out == 0x5555).all() and not q.any()
    info = _capi.MisJpegInfo()
    assert lib.mis_jpeg_info(data, len(data), C.byref(info)) == want and CAUSE_TEXT[cause] in lib.mis_jpeg_last_error().decode()
    with pytest.raises(rj.Unsupported if code == "MIS_E_UNSUPPORTED" else rj.Invalid):
        rj.decode(data)


def test_every_prefix_is_refused(lib):
    from image_stitching_amd import _capi
    data = stream("17x13_420_q85")
    out = np.zeros(1 << 16, np.int16)
    q = np.zeros(64, np.uint16)
    assert lib.mis_jpeg_debug_coefficients(data, len(data), 0, out.ctypes.data, out.size, q.ctypes.data) == _capi.MIS_OK
    codes = set()
    for n in range(len(data)):
        # (bytes(data[:n]) is a buffer of exactly n bytes)
        prefix = bytes(data[:n])
        rc = lib.mis_jpeg_debug_coefficients(prefix, n, 0, out.ctypes.data, out.size, q.ctypes.data)
        assert rc in (_capi.MIS_E_INVALID, _capi.MIS_E_UNSUPPORTED), n
        codes.add(rc)
    assert _capi.MIS_E_INVALID in codes


def handmade_stream(dc_size, dc_bits, qvalue):
    """An 8 x 8 one-component baseline stream written by hand: one quantisation table of `qvalue`, a DC table whose only code
    ('0') is the size `dc_size`, an AC table whose only code ('0') is the end of block; the block is DC = dc_bits, no AC."""
    def seg(marker, payload):
        return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload
    bits = "0" + format(dc_bits, "0%db" % dc_size) + "0"
    bits += "1" * (-len(bits) % 8)
    scan = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    assert 0xFF not in scan
    return (b"\xff\xd8" + seg(0xDB, bytes([0]) + bytes([qvalue] * 64)) + seg(0xC0, bytes([8, 0, 8, 0, 8, 1, 1, 0x11, 0]))
            + seg(0xC4, bytes([0x00, 1] + [0] * 15 + [dc_size])) + seg(0xC4, bytes([0x10, 1] + [0] * 15 + [0x00]))
            + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + scan + b"\xff\xd9")


def test_idct_bound_refuses_a_block_no_encoder_makes(lib):
    """jpeg_core.h: the 32-bit IDCT is exact for blocks with S <= 65000 and the host refuses the rest by name.  A hand-made block of
    DC = 255 * 254 = 64770 is inside and decodes, DC = 255 * 255 = 65025 is outside; every fixture's blocks are below the bound the
    header derives for encoder-made blocks (31500)."""
    from image_stitching_amd import _capi
    inside, outside = handmade_stream(8, 254, 255), handmade_stream(8, 255, 255)
    assert rj.coefficients(inside)[1][0][0, 0, 0] == 254 and rj.coefficients(outside)[1][0][0, 0, 0] == 255
    rc, got, q = host_coefficients(lib, inside, 0, 1)
    assert rc == _capi.MIS_OK and got[0] == 254 and not got[1:].any() and (q == 255).all()
    rc, got, _ = host_coefficients(lib, outside, 0, 1)
    assert rc == _capi.MIS_E_UNSUPPORTED and "32-bit IDCT" in lib.mis_jpeg_last_error().decode() and (got == 0x5555).all()
    w = {0: 1024, 1: 1421, 2: 1971}
    for name in DECODE:
        _, planes, tables = rj.coefficients(stream(name))
        for blocks, t in zip(planes, tables):
            wt = np.array([w[(k >> 3 > 0) + (k & 7 > 0)] for k in range(64)], np.int64) * t.astype(np.int64)
            S = (np.abs(blocks.astype(np.int64)) * wt).sum(axis=-1).max() / 1024.0
            assert S < 31500, (name, S)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jpegharness") / "jpeg_host_harness")
    r = subprocess.run(["c++", "-O2", "-std=c++17", os.path.join(HERE, "harness", "jpeg_host_harness.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("name", DECODE)
def test_host_twin_of_the_kernels_equals_pillow(harness, tmp_path, name):
    out = str(tmp_path / "out.bgr")
    r = subprocess.run([harness, "decode", os.path.join(GOLDEN, name + ".jpg"), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    w, h = [int(v) for v in r.stdout.split()]
    got = np.fromfile(out, np.uint8).reshape(h, w, 3)
    want = expected_rgb(name)
    want = np.repeat(want[:, :, None], 3, axis=2) if want.ndim == 2 else want[:, :, ::-1]
    assert np.array_equal(got, want)


def test_harness_refuses_and_never_decodes_a_prefix(harness):
    """the harness's fuzz mode on the smallest file (all prefixes, a few seeded corruptions): exit 0 means no prefix decoded"""
    r = subprocess.run([harness, "fuzz", "1", "50", os.path.join(GOLDEN, "1x1_420_q90.jpg"), os.path.join(GOLDEN, "refuse_progressive.jpg")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 2 and " whole 0 prefixes ok 0 " in lines[0] and " whole -6 prefixes ok 0 " in lines[1]


@pytest.mark.parametrize("dc_bits,dc", [(254, 254), (1, -254), (200, 200), (127, -128)])
def test_32_bit_idct_equals_int64_at_the_bound(harness, tmp_path, dc_bits, dc):
    """the host twin's 32-bit IDCT on hand-made blocks at the edge of its bound (|DC * q| = 64770: the row pass descales a value of
    2.12e9, just below 2^31) and inside it, against the reference's int64 IDCT"""
    data = handmade_stream(8, dc_bits, 255)
    assert rj.coefficients(data)[1][0][0, 0, 0] == dc
    path, out = str(tmp_path / "hand.jpg"), str(tmp_path / "hand.bgr")
    with open(path, "wb") as fh:
        fh.write(data)
    r = subprocess.run([harness, "decode", path, out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["8", "8"], r.stdout + r.stderr
    want = rj.decode(data)
    assert np.array_equal(np.fromfile(out, np.uint8).reshape(8, 8, 3), np.repeat(want[:, :, None], 3, axis=2))
    assert (want == (255 if dc > 0 else 0)).all()


def test_32_bit_idct_equals_int64_on_random_blocks_up_to_the_bound(harness, tmp_path):
    """jpeg_idct_block (uint32 arithmetic) against the reference's int64 IDCT on 4096 seeded blocks of dequantised coefficients:
    dense and sparse ones, scaled so that the bound's sum S runs from an encoder's range up to the limit of 65000, where the
    partial sums of the 32-bit passes wrap and the descaled values must still be exact"""
    rng = np.random.default_rng(7)
    w1 = np.array([1.0] + [1.3871] * 7)
    wt = np.outer(w1, w1).reshape(64)
    blocks = []
    for i in range(4096):
        x = rng.normal(size=64) * (rng.random(64) < (1.0, 0.3, 0.05)[i % 3])
        if not x.any():
            x[rng.integers(64)] = 1.0
        target = (65000.0, 64000.0, 30000.0, 4000.0)[(i // 3) % 4]
        x = np.trunc(x * (target - 200.0) / (np.abs(x) * wt).sum())       # truncation only lowers S
        assert (np.abs(x) * wt).sum() <= target
        blocks.append(x.astype(np.int32))
    blocks = np.stack(blocks)
    src, out = str(tmp_path / "blocks.i32"), str(tmp_path / "samples.u8")
    blocks.tofile(src)
    r = subprocess.run([harness, "idct", src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, np.uint8).reshape(4096, 8, 8)
    want = rj.idct_plane(blocks.reshape(1, 4096, 64), np.ones(64, np.uint16)).reshape(8, 4096, 8).transpose(1, 0, 2)
    assert np.array_equal(got, want)
    assert 0 < (want == 0).mean() < 1 and 0 < (want == 255).mean() < 1       # both clamps and the range between are exercised
