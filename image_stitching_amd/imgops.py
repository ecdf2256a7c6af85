"""Image operators either side of the path (image_stitching.cpp:571-580, :619, :1144, :1169-1171) and JPEG in and out (:569, :1228)."""
import ctypes as C

import numpy as np

from . import _capi as capi
from .core import MisError, _c_array, _empty_image, _images, as_image, torch

ROTATE_90_CLOCKWISE, ROTATE_180, ROTATE_90_COUNTERCLOCKWISE = 0, 1, 2


def resize(ctx, src, dsize=None, fx=0.0, fy=0.0):
    """cv::resize(src, dst, dsize, fx, fy, INTER_LINEAR_EXACT) on the device (8UC1 / 8UC3)."""
    simg = as_image(src)
    if dsize:
        dw, dh = int(dsize[0]), int(dsize[1])
    else:
        dw, dh = int(np.rint(simg.width * fx)), int(np.rint(simg.height * fy))   # cvRound: half to even
    dst = _empty_image(ctx, dh, dw, simg.channels, torch.uint8)
    dimg = as_image(dst)
    ctx.check(ctx.lib.mis_resize_linear_exact(ctx.h, C.byref(simg), dw if dsize else 0, dh if dsize else 0, float(fx), float(fy), C.byref(dimg)))
    return dst


def resize_batch(ctx, frames, fx, fy, out=None):
    """cv::resize(frame, dst, Size(), fx, fy, INTER_LINEAR_EXACT) for n device frames of one size and type in one launch
    (mis_resize_linear_exact_batch; the work-scale resize of image_stitching.cpp:602) -> list of device images.  `out`: images
    of the destination size to write into (a job allocates them once); allocated here when None."""
    frames = list(frames)
    n = len(frames)
    if n == 0:
        return []
    simgs = [as_image(f) for f in frames]
    if out is None:
        dw, dh = int(np.rint(simgs[0].width * fx)), int(np.rint(simgs[0].height * fy))   # cvRound: half to even
        out = [_empty_image(ctx, dh, dw, simgs[0].channels, torch.uint8) for _ in range(n)]
    out = list(out)[:n]
    sa = _c_array(capi.MisImage, simgs)
    da = _images(out)
    ctx.check(ctx.lib.mis_resize_linear_exact_batch(ctx.h, sa, n, 0, 0, float(fx), float(fy), da))
    return out


def _jpeg_bytes(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    with open(path_or_bytes, "rb") as fh:
        return fh.read()


def jpeg_info(data):
    """The frame header of a JPEG stream (mis_jpeg_info; host logic, no device): dict(width, height, components, h, v,
    restart_interval).  A stream the decoder refuses raises MisError with the cause."""
    data = _jpeg_bytes(data)
    lib = capi.load()
    info = capi.MisJpegInfo()
    rc = lib.mis_jpeg_info(data, len(data), C.byref(info))
    if rc != capi.MIS_OK:
        raise MisError(rc, lib.mis_jpeg_last_error().decode())
    nc = info.components
    return dict(width=info.width, height=info.height, components=nc, h=list(info.h)[:nc], v=list(info.v)[:nc], restart_interval=info.restart_interval)


def imread_batch(ctx, sources):
    """cv::imread (IMREAD_COLOR) of n baseline JPEG files or byte strings of any sizes in one pass (mis_jpeg_decode_batch; the
    imread of image_stitching.cpp:569) -> list of H x W x 3 uint8 BGR device images.  One refused stream refuses the call; the
    error names the frame."""
    datas = [_jpeg_bytes(s) for s in sources]
    n = len(datas)
    if n == 0:
        return []
    out = []
    for i, d in enumerate(datas):
        try:
            info = jpeg_info(d)
        except MisError as e:
            raise MisError(e.code, "frame %d: %s" % (i, str(e).split(": ", 1)[1])) from None
        out.append(_empty_image(ctx, info["height"], info["width"], 3, torch.uint8))
    ptrs = _c_array(C.c_void_p, (C.cast(C.c_char_p(d), C.c_void_p) for d in datas))
    sizes = _c_array(C.c_size_t, (len(d) for d in datas))
    ctx.check(ctx.lib.mis_jpeg_decode_batch(ctx.h, ptrs, sizes, n, _images(out)))
    return out


def imread(ctx, path_or_bytes):
    """cv::imread(path) of one baseline JPEG (file name or bytes) -> H x W x 3 uint8 BGR device image."""
    return imread_batch(ctx, [path_or_bytes])[0]


JPEG_SAMPLING = {"420": capi.JPEG_420, "422": capi.JPEG_422, "444": capi.JPEG_444, "440": capi.JPEG_440, "411": capi.JPEG_411}


def jpeg_encode_params(quality=95, sampling="420", restart_interval=0, optimize=False, progressive=False):
    """MisJpegEncodeParams of the keyword arguments imencode / imwrite take.  The library writes standard Huffman tables in one
    sequential scan: optimize and progressive are refused by name."""
    if optimize:
        raise MisError(capi.MIS_E_UNSUPPORTED, "jpeg: optimised Huffman tables")
    if progressive:
        raise MisError(capi.MIS_E_UNSUPPORTED, "jpeg: progressive output")
    key = str(sampling).replace(":", "")
    if key not in JPEG_SAMPLING:
        raise MisError(capi.MIS_E_UNSUPPORTED, "jpeg: sampling %r (4:2:0, 4:2:2 and 4:4:4 only)" % (sampling,))
    return capi.MisJpegEncodeParams(int(quality), JPEG_SAMPLING[key], int(restart_interval))


def _take_stream(lib, stream):
    try:
        return C.string_at(stream.data, stream.bytes) if stream.data else b""
    finally:
        lib.mis_jpeg_stream_free(C.byref(stream))


def imencode_batch(ctx, images, **params):
    """cv::imwrite's JPEG bytes (image_stitching.cpp:1228) of n 8UC3 BGR images of any sizes -- device tensors or host arrays -- in
    one pass (mis_jpeg_encode_batch) -> list of bytes.  Keywords: quality=95, sampling="420" | "422" | "444", restart_interval=0.
    One refused image refuses the call; the error names the frame."""
    images = list(images)
    n = len(images)
    if n == 0:
        return []
    p = jpeg_encode_params(**params)
    outs = (capi.MisJpegStream * n)()
    ctx.check(ctx.lib.mis_jpeg_encode_batch(ctx.h, _images(images), n, C.byref(p), outs))
    return [_take_stream(ctx.lib, s) for s in outs]


def imencode(ctx, image, quality=95, sampling="420", restart_interval=0, **more):
    """cv::imencode(".jpg", image) with cv::imwrite's defaults: one 8UC3 BGR image -> the file's bytes."""
    return imencode_batch(ctx, [image], quality=quality, sampling=sampling, restart_interval=restart_interval, **more)[0]


def imwrite(ctx, path, image, **params):
    """cv::imwrite(path, image) of image_stitching.cpp:1228 for a .jpg path; returns the number of bytes written."""
    data = imencode(ctx, image, **params)
    with open(path, "wb") as fh:
        fh.write(data)
    return len(data)


def rotate(ctx, src, code):
    """cv::rotate(src, dst, code) on the device (8UC1 / 8UC3)."""
    simg = as_image(src)
    dw, dh = (simg.width, simg.height) if code == ROTATE_180 else (simg.height, simg.width)
    dst = _empty_image(ctx, dh, dw, simg.channels, torch.uint8)
    dimg = as_image(dst)
    ctx.check(ctx.lib.mis_rotate(ctx.h, C.byref(simg), int(code), C.byref(dimg)))
    return dst


def seam_mask_apply(ctx, seam_mask_warped, mask_warped):
    """mask_warped &= resize(dilate(seam_mask_warped), mask_warped.size(), INTER_LINEAR_EXACT), in place
    (image_stitching.cpp:1169-1171)."""
    simg, mimg = as_image(seam_mask_warped), as_image(mask_warped)
    ctx.check(ctx.lib.mis_seam_mask_apply(ctx.h, C.byref(simg), C.byref(mimg)))
    return mask_warped
