"""mis_jpeg_encode / mis_jpeg_encode_batch on the device against Pillow's (libjpeg-turbo's) streams of the fixtures in
tests/golden/jpeg_enc (tools/make_jpeg_enc_fixtures.py), byte for byte: every fixture alone, the device's coefficient planes against
the numpy reference's (dummy blocks included), all fixtures in one batch, host / device / odd-stride sources, the round trip through
mis_jpeg_decode, a refused frame in a batch, and the Python entries."""
import ctypes as C
import os

import numpy as np
import pytest

import refimpl_jpeg
from test_refimpl_jpeg_enc_cpu import FIXTURES, GOLDEN, NAMES, fixture, params_of

pytestmark = pytest.mark.gpu


def bgr(src):
    return np.ascontiguousarray(src[:, :, ::-1])


def kwargs(f):
    return dict(quality=f["quality"], sampling=f["sampling"], restart_interval=f["restart_interval"])


def encode_raw(ctx, image, params):
    """mis_jpeg_encode over one MisImage -> bytes"""
    from image_stitching_amd import _capi
    out = _capi.MisJpegStream()
    ctx.check(ctx.lib.mis_jpeg_encode(ctx.h, C.byref(image), C.byref(params), C.byref(out)))
    data = C.string_at(out.data, out.bytes)
    ctx.lib.mis_jpeg_stream_free(C.byref(out))
    return data


@pytest.mark.parametrize("name", NAMES)
def test_encode_equals_pillow(ctx, name):
    import torch
    from image_stitching_amd.stitching import as_image
    f, src, jpg, _ = fixture(name)
    dev = torch.from_numpy(bgr(src)).cuda()
    assert encode_raw(ctx, as_image(dev), params_of(f)) == jpg


@pytest.mark.parametrize("name", NAMES)
def test_device_coefficients_equal_the_reference(ctx, name):
    import torch
    import refimpl_jpeg_enc as ref
    from image_stitching_amd.stitching import as_image
    f, src, jpg, planes = fixture(name)
    dev = torch.from_numpy(bgr(src)).cuda()
    img, p = as_image(dev), params_of(f)
    for c in range(3):
        got = np.full(planes[c].shape, 0x5555, np.int16)
        table = np.zeros(64, np.uint16)
        ctx.check(ctx.lib.mis_jpeg_debug_encode_coefficients(ctx.h, C.byref(img), C.byref(p), c, got.ctypes.data, got.size, table.ctypes.data))
        bad = np.argwhere((got != planes[c]).any(axis=2))
        assert bad.size == 0, "component %d: first differing block (row, column) %s" % (c, bad[0])
        assert np.array_equal(table, ref.tables(f["quality"])[0 if c == 0 else 1])
    # a capacity one short of the plane is refused before anything runs
    got = np.zeros(planes[0].size - 1, np.int16)
    rc = ctx.lib.mis_jpeg_debug_encode_coefficients(ctx.h, C.byref(img), C.byref(p), 0, got.ctypes.data, got.size, table.ctypes.data)
    assert rc == -1 and "capacity" in ctx.lib.mis_last_error(ctx.h).decode()


def test_one_batch_of_every_shape_equals_the_single_calls(ctx):
    """mixed sizes in one call, for each (quality, sampling, restart interval) the fixtures use: the parameters are the call's"""
    import torch
    import image_stitching_amd as isa
    sources = [torch.from_numpy(bgr(fixture(n)[1])).cuda() for n in NAMES]
    seen = set()
    for f in FIXTURES:
        key = (f["quality"], f["sampling"], f["restart_interval"])
        if key in seen:
            continue
        seen.add(key)
        batch = isa.imencode_batch(ctx, sources, **kwargs(f))
        assert len(batch) == len(sources)
        for name, s, b in zip(NAMES, sources, batch):
            assert b == isa.imencode(ctx, s, **kwargs(f)), (name, key)
            if fixture(name)[0]["name"] == f["name"]:
                assert b == fixture(name)[2]
    assert len(seen) >= 6


@pytest.mark.parametrize("name", ["131x77_420_q95", "33x19_422_q75", "8x8_444_q90", "1x1_420_q90"])
def test_host_device_and_strided_sources_give_the_same_bytes(ctx, name):
    import torch
    from image_stitching_amd.stitching import as_image
    f, src, jpg, _ = fixture(name)
    h, w = src.shape[:2]
    host = bgr(src)
    p = params_of(f)
    assert encode_raw(ctx, as_image(host), p) == jpg
    assert encode_raw(ctx, as_image(torch.from_numpy(host).cuda()), p) == jpg
    stride = 3 * w + 5
    wide = torch.full((h, stride), 0xA5, dtype=torch.uint8, device=ctx.device)
    wide[:, :3 * w] = torch.from_numpy(host.reshape(h, 3 * w)).cuda()
    img = as_image(wide[:, :3 * w].as_strided((h, w, 3), (stride, 3, 1)))
    assert img.stride == stride
    assert encode_raw(ctx, img, p) == jpg
    wide_host = np.full((h, stride), 0x5A, np.uint8)
    wide_host[:, :3 * w] = host.reshape(h, 3 * w)
    img = as_image(host)
    img.data, img.stride = wide_host.ctypes.data, stride
    assert encode_raw(ctx, img, p) == jpg


@pytest.mark.parametrize("name", ["131x77_420_q95", "33x19_422_q75", "64x48_420_q60_dri2", "47x31_420_q100_checker"])
def test_decode_of_encode_equals_the_reference_decoder(ctx, name):
    import torch
    import image_stitching_amd as isa
    f, src, jpg, _ = fixture(name)
    data = isa.imencode(ctx, torch.from_numpy(bgr(src)).cuda(), **kwargs(f))
    got = isa.imread(ctx, data).cpu().numpy()
    assert np.array_equal(got[:, :, ::-1], refimpl_jpeg.decode(jpg))


def test_a_refused_frame_refuses_the_batch_and_allocates_nothing(ctx):
    import torch
    from image_stitching_amd import _capi
    from image_stitching_amd.stitching import as_image
    good = torch.from_numpy(bgr(fixture("17x13_420_q85")[1])).cuda()
    grey = torch.zeros((13, 17), dtype=torch.uint8, device=ctx.device)
    four = torch.zeros((13, 17, 4), dtype=torch.uint8, device=ctx.device)
    p = _capi.MisJpegEncodeParams(85, _capi.JPEG_420, 0)
    ctx.synchronize()
    for images, frame, cause in (([good, good, grey, good], 2, "1-channel"), ([good, four], 1, "4-channel")):
        arr = (_capi.MisImage * len(images))(*[as_image(i) for i in images])
        outs = (_capi.MisJpegStream * len(images))()
        for o in outs:
            o.data, o.bytes = 0x1234, 77
        free_before = torch.cuda.mem_get_info(ctx.device)[0]
        rc = ctx.lib.mis_jpeg_encode_batch(ctx.h, arr, len(images), C.byref(p), outs)
        assert rc == _capi.MIS_E_UNSUPPORTED
        text = ctx.lib.mis_last_error(ctx.h).decode()
        assert "frame %d" % frame in text and cause in text, text
        assert torch.cuda.mem_get_info(ctx.device)[0] == free_before
        assert all(o.data == 0x1234 and o.bytes == 77 for o in outs)
    bad = _capi.MisJpegEncodeParams(101, _capi.JPEG_420, 0)
    out = _capi.MisJpegStream()
    img = as_image(good)
    assert ctx.lib.mis_jpeg_encode(ctx.h, C.byref(img), C.byref(bad), C.byref(out)) == _capi.MIS_E_INVALID
    assert "quality" in ctx.lib.mis_last_error(ctx.h).decode() and not out.data
    # the context is as usable as before
    assert encode_raw(ctx, img, p) == fixture("17x13_420_q85")[2]


def test_imencode_and_imwrite(ctx, tmp_path):
    import torch
    import image_stitching_amd as isa
    f, src, jpg, _ = fixture("50x40_420_q95")
    dev = torch.from_numpy(bgr(src)).cuda()
    assert isa.imencode(ctx, dev) == jpg                   # the defaults are cv::imwrite's: quality 95, 4:2:0
    assert isa.imencode(ctx, bgr(src), quality=95, sampling="4:2:0") == jpg
    path = str(tmp_path / "out.jpg")
    assert isa.imwrite(ctx, path, dev) == len(jpg)
    assert open(path, "rb").read() == jpg
    f, src, jpg, _ = fixture("64x48_420_q60_dri2")
    assert isa.imencode(ctx, torch.from_numpy(bgr(src)).cuda(), **kwargs(f)) == jpg
    with pytest.raises(isa.MisError) as err:
        isa.imencode(ctx, dev, sampling="411")
    assert err.value.code == -6 and "4:1:1" in str(err.value)
