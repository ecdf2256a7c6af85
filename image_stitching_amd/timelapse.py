"""timelapse: cv::detail::Timelapser / TimelapserCrop, the compositing loop's other sink (image_stitching.cpp:79, :82, :1083,
:1194-1215): every frame warped into one common canvas and returned as a registered frame of its own, nothing blended."""
import ctypes as C

import numpy as np

from . import _capi as capi
from .core import Handle, _empty_image, _images, _points, as_image, torch

# timelapse_type (image_stitching.cpp:79; Timelapser::AS_IS / CROP) as a configuration name
TIMELAPSE_TYPES = {"as_is": capi.TIMELAPSE_AS_IS, "crop": capi.TIMELAPSE_CROP}


def timelapse_kind(timelapse_type):
    """timelapse_type -> MIS_TIMELAPSE_*; any other name raises by name."""
    if not isinstance(timelapse_type, str) or timelapse_type not in TIMELAPSE_TYPES:
        raise ValueError("timelapse_type %r: 'as_is' or 'crop' (image_stitching.cpp:79)" % (timelapse_type,))
    return TIMELAPSE_TYPES[timelapse_type]


def check_timelapse_config(cfg):
    return timelapse_kind(cfg.timelapse_type)


def _sizes(sizes):
    return (capi.MisSize * max(len(sizes), 1))(*[capi.MisSize(int(s[0]), int(s[1])) for s in sizes])


def result_roi_intersection(corners, sizes):
    """cv::detail::resultRoiIntersection -> (x, y, width, height); an empty intersection is a ValueError that names the rectangle
    (OpenCV fails in Mat::create there)."""
    lib = capi.load()
    n = len(corners)
    if n < 1 or len(sizes) != n:
        raise ValueError("result_roi_intersection: %d corners and %d sizes (as many, at least one)" % (n, len(sizes)))
    r = capi.MisRect()
    if lib.mis_result_roi_intersection(_points(corners), _sizes(sizes), n, C.byref(r)) != capi.MIS_OK:
        tl = (max(int(c[0]) for c in corners), max(int(c[1]) for c in corners))
        br = (min(int(c[0]) + int(s[0]) for c, s in zip(corners, sizes)), min(int(c[1]) + int(s[1]) for c, s in zip(corners, sizes)))
        raise ValueError("result_roi_intersection: the frames' intersection Rect(tl = %r, br = %r) is empty" % (tl, br))
    return r.x, r.y, r.width, r.height


class Timelapser(Handle):
    """Timelapser::createDefault(type) (image_stitching.cpp:1083, :1196): "as_is" sizes the canvas with resultRoi, "crop" with
    resultRoiIntersection.  process() places an already warped 16SC3 image; the fused route is timelapse_warp_batch."""
    DESTROY = "mis_timelapser_destroy"

    def __init__(self, ctx, timelapse_type="crop"):
        self.ctx = ctx
        self.type = timelapse_kind(timelapse_type)
        h = C.c_void_p()
        ctx.check(ctx.lib.mis_timelapser_create(ctx.h, self.type, C.byref(h)))
        self.h = h
        self.dst = None

    def initialize(self, corners, sizes):
        """:1197 -- fixes dst_roi; an empty intersection raises ValueError with the rectangle."""
        n = len(corners)
        if self.type == capi.TIMELAPSE_CROP:
            result_roi_intersection(corners, sizes)
        self.ctx.check(self.ctx.lib.mis_timelapser_initialize(self.h, _points(corners), _sizes(sizes), n))

    def dst_roi(self):
        r = capi.MisRect()
        self.ctx.check(self.ctx.lib.mis_timelapser_dst_roi(self.h, C.byref(r)))
        return r.x, r.y, r.width, r.height

    def process(self, img, mask, tl, dst=None):
        """:1203 -- the canvas set to 0, then the part of img (16SC3, top-left at tl) that lies in dst_roi copied in; mask is
        accepted for signature parity and ignored (the reference passes all ones).  dst: a 16SC3 canvas to fill, else a fresh one.
        -> the canvas, also kept as self.dst."""
        x, y, w, h = self.dst_roi()
        if dst is None:
            dst = _empty_image(self.ctx, h, w, 3, torch.int16)
        i, d = as_image(img), as_image(dst)
        self.ctx.check(self.ctx.lib.mis_timelapser_process(self.h, C.byref(i), capi.MisPoint(int(tl[0]), int(tl[1])), C.byref(d)))
        self.dst = dst
        return dst

    def getDst(self):
        """:1204"""
        return self.dst


def _batch_args(ctx, frames, cameras, rois, dst_roi, gains, dsts, as_u8):
    n = len(frames)
    x, y, w, h = (int(v) for v in dst_roi)
    if dsts is None:
        if w <= 0 or h <= 0:
            raise ValueError("timelapse_warp_batch: empty dst_roi %r" % (tuple(dst_roi),))
        dsts = [_empty_image(ctx, h, w, 3, torch.uint8 if as_u8 else torch.int16) for _ in range(n)]
    Ks = np.ascontiguousarray(np.stack([np.asarray(c["K"], np.float32).reshape(9) for c in cameras]))
    Rs = np.ascontiguousarray(np.stack([np.asarray(c["R"], np.float32).reshape(9) for c in cameras]))
    rs = (capi.MisRect * n)(*[capi.MisRect(int(r[0]), int(r[1]), int(r[2]), int(r[3])) for r in rois])
    g = None if gains is None else np.ascontiguousarray(np.asarray(gains, np.float64).reshape(n, 3))
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    return (dsts, _images(frames), n, Ks, Ks.ctypes.data_as(fp), Rs, Rs.ctypes.data_as(fp), rs, capi.MisRect(x, y, w, h), g,
            None if g is None else g.ctypes.data_as(dp), _images(dsts), capi.U8 if as_u8 else capi.S16)


def timelapse_warp_batch(ctx, kind, frames, cameras, rois, scale, dst_roi, gains=None, as_u8=True, dsts=None):
    """mis_timelapse_warp_batch: warp -> gains -> canvas of all frames in one launch per 16 frames (image_stitching.cpp:1154-1164,
    :1203-1204, :1214) -> the list of canvases of dst_roi's size, packed 8UC3 BGR (as_u8) or 16SC3.  rois: warp_rois of the
    cameras; gains: None or n x 3 float64 as GainCompensator.gains / ChannelsCompensator.gains give them; dsts: canvases to fill."""
    if len(frames) == 0:
        return []
    dsts, im, n, Ks, kp, Rs, rp, rs, dr, g, gp, ds, fmt = _batch_args(ctx, frames, cameras, rois, dst_roi, gains, dsts, as_u8)
    ctx.check(ctx.lib.mis_timelapse_warp_batch(ctx.h, int(kind), im, n, float(scale), kp, rp, rs, C.byref(dr), gp, ds, fmt))
    return dsts


def timelapse_warp_batch_timed(ctx, kind, frames, cameras, rois, scale, dst_roi, gains, dsts, as_u8, repeats):
    """mis_timelapse_warp_batch_timed -> average microseconds of one pass over all frames (a measurement aid)."""
    dsts, im, n, Ks, kp, Rs, rp, rs, dr, g, gp, ds, fmt = _batch_args(ctx, frames, cameras, rois, dst_roi, gains, dsts, as_u8)
    us = C.c_float()
    ctx.check(ctx.lib.mis_timelapse_warp_batch_timed(ctx.h, int(kind), im, n, float(scale), kp, rp, rs, C.byref(dr), gp, ds, fmt, int(repeats), C.byref(us)))
    return float(us.value)
