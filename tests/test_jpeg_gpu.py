"""mis_jpeg_decode / mis_jpeg_decode_batch on the device against Pillow's (libjpeg-turbo's) decode of the fixtures in
tests/golden/jpeg (tools/make_jpeg_fixtures.py), byte for byte in BGR order: every fixture alone, all of them -- mixed sizes, sampling
layouts, restart intervals, a grey file -- in one batch, caller-provided destinations (device with a wide stride, host), and the
refusals: wrong-size destinations and refused streams leave every output untouched and the context usable."""
import ctypes as C
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "jpeg")
MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
DECODE = [e["name"] for e in MANIFEST["decode"]]
REFUSE = [(e["name"], e["code"], e["cause"]) for e in MANIFEST["refuse"]]
CAUSE_TEXT = {"SOF2": "SOF2", "4 components": "4 components", "truncated": "truncated"}
GOOD = "17x13_420_q85"


def stream(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as fh:
        return fh.read()


@pytest.fixture(scope="module")
def expected():
    """Pillow's decode of every decode fixture as imread returns it: H x W x 3 BGR (a grey file: B = G = R)"""
    out = {}
    for name in DECODE:
        px = np.load(os.path.join(GOLDEN, name + ".npy"))
        out[name] = np.ascontiguousarray(np.repeat(px[:, :, None], 3, axis=2) if px.ndim == 2 else px[:, :, ::-1])
    return out


def decode_batch_raw(ctx, datas, images):
    """mis_jpeg_decode_batch over MisImage structs -> return code"""
    from image_stitching_amd import _capi
    n = len(datas)
    ptrs = (C.c_void_p * n)(*[C.cast(C.c_char_p(d), C.c_void_p) for d in datas])
    sizes = (C.c_size_t * n)(*[len(d) for d in datas])
    arr = (_capi.MisImage * n)(*images)
    return ctx.lib.mis_jpeg_decode_batch(ctx.h, ptrs, sizes, n, arr)


def check_good(ctx, expected):
    import image_stitching_amd as isa
    assert np.array_equal(isa.imread(ctx, stream(GOOD)).cpu().numpy(), expected[GOOD])


@pytest.mark.parametrize("name", DECODE)
def test_decode_equals_pillow(ctx, expected, name):
    import image_stitching_amd as isa
    got = isa.imread(ctx, os.path.join(GOLDEN, name + ".jpg"))
    assert got.is_cuda and tuple(got.shape) == expected[name].shape
    assert np.array_equal(got.cpu().numpy(), expected[name])


def test_batch_of_mixed_frames_equals_pillow(ctx, expected):
    import image_stitching_amd as isa
    got = isa.imread_batch(ctx, [stream(n) for n in DECODE])
    assert len(got) == len(DECODE)
    for name, g in zip(DECODE, got):
        assert np.array_equal(g.cpu().numpy(), expected[name]), name


def test_library_allocated_output(ctx, expected):
    """data == NULL: the library allocates the image in HBM (mis_image_free releases it)"""
    import torch
    from image_stitching_amd import _capi
    data = stream("33x19_422_q75")
    img = _capi.MisImage()
    ctx.check(ctx.lib.mis_jpeg_decode(ctx.h, data, len(data), C.byref(img)))
    want = expected["33x19_422_q75"]
    assert (img.width, img.height, img.channels, img.dtype, img.mem) == (33, 19, 3, _capi.U8, _capi.MEM_DEVICE) and img.data and img.stride >= 99
    dev = torch.empty((19, img.stride), dtype=torch.uint8, device=ctx.device)
    ctx.check(ctx.lib.mis_copy_2d(ctx.h, dev.data_ptr(), img.stride, img.data, img.stride, 99, 19))
    ctx.synchronize()
    assert np.array_equal(dev.cpu().numpy()[:, :99].reshape(19, 33, 3), want)
    ctx.check(ctx.lib.mis_image_free(ctx.h, C.byref(img)))


@pytest.mark.parametrize("name,pad", [("131x77_420_q92_dri3", 7), ("64x48_420_q60_dri2", 64), ("40x24_grey_q80", 1)])
def test_wide_destination_stride_keeps_its_padding(ctx, expected, name, pad):
    """rows at the caller's stride (dword-aligned and not), a sentinel in the padding untouched"""
    import torch
    from image_stitching_amd.stitching import as_image
    want = expected[name]
    h, w = want.shape[:2]
    buf = torch.full((h, 3 * w + pad), 0xA5, dtype=torch.uint8, device=ctx.device)
    view = buf.as_strided((h, w, 3), (3 * w + pad, 3, 1))
    assert decode_batch_raw(ctx, [stream(name)], [as_image(view)]) == 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :3 * w].reshape(h, w, 3), want) and (got[:, 3 * w:] == 0xA5).all()


def test_host_destination_is_staged(ctx, expected):
    from image_stitching_amd.stitching import as_image
    want = expected["47x31_420_q85_opt"]
    host = np.full((31, 47 * 3 + 11), 0xA5, np.uint8)
    view = np.lib.stride_tricks.as_strided(host, (31, 47, 3), (host.strides[0], 3, 1))
    assert decode_batch_raw(ctx, [stream("47x31_420_q85_opt")], [as_image(view)]) == 0
    assert np.array_equal(view, want) and (host[:, 47 * 3:] == 0xA5).all()


@pytest.mark.parametrize("shape", [(13, 16, 3), (12, 17, 3), (13, 17, 1)])
def test_wrong_size_destination_is_invalid(ctx, expected, shape):
    import torch
    from image_stitching_amd import _capi
    from image_stitching_amd.stitching import as_image
    dst = torch.full(shape, 0xA5, dtype=torch.uint8, device=ctx.device)
    img = as_image(dst if shape[2] == 3 else dst[:, :, 0])
    assert decode_batch_raw(ctx, [stream(GOOD)], [img]) == _capi.MIS_E_INVALID
    assert "output 0" in ctx.lib.mis_last_error(ctx.h).decode()
    assert (dst.cpu().numpy() == 0xA5).all()
    check_good(ctx, expected)


@pytest.mark.parametrize("name,code,cause", REFUSE)
def test_refused_stream_in_the_middle_refuses_the_batch(ctx, expected, name, code, cause):
    """[good, refused, good]: the call's code is the refusal's, the text names frame 1 and the cause, nothing is written to the
    outputs on either side, and the context decodes again afterwards"""
    import torch
    from image_stitching_amd import _capi
    from image_stitching_amd.stitching import as_image
    a, b = "131x77_420_q92_dri3", "16x16_444_q90"
    outs = [torch.full(expected[a].shape, 0xA5, dtype=torch.uint8, device=ctx.device),
            torch.full((31, 47, 3), 0xA5, dtype=torch.uint8, device=ctx.device),
            torch.full(expected[b].shape, 0xA5, dtype=torch.uint8, device=ctx.device)]
    rc = decode_batch_raw(ctx, [stream(a), stream(name), stream(b)], [as_image(o) for o in outs])
    text = ctx.lib.mis_last_error(ctx.h).decode()
    assert rc == getattr(_capi, code) and "frame 1" in text and CAUSE_TEXT[cause] in text
    ctx.synchronize()
    for o in outs:
        assert (o.cpu().numpy() == 0xA5).all()
    check_good(ctx, expected)


def test_refused_single_stream_raises_and_context_survives(ctx, expected):
    import image_stitching_amd as isa
    from image_stitching_amd import _capi
    with pytest.raises(isa.MisError) as ei:
        isa.imread(ctx, stream("refuse_progressive"))
    assert ei.value.code == _capi.MIS_E_UNSUPPORTED and "SOF2" in str(ei.value)
    with pytest.raises(isa.MisError) as ei:
        isa.imread_batch(ctx, [stream(GOOD), stream("refuse_truncated")])
    assert ei.value.code == _capi.MIS_E_INVALID and "frame 1" in str(ei.value)
    # a stream whose headers pass and whose scan is cut: refused by the entropy decoder, after the outputs were checked
    data = stream("47x31_420_q100")
    cut = data[:len(data) - 40] + b"\xff\xd9"
    with pytest.raises(isa.MisError) as ei:
        isa.imread_batch(ctx, [stream(GOOD), cut])
    assert ei.value.code == _capi.MIS_E_INVALID and "frame 1" in str(ei.value) and "entropy-coded data ends" in str(ei.value)
    check_good(ctx, expected)
