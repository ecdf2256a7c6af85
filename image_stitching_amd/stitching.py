"""Host-side mirror of the reference's stitching interface over the libmistitch C ABI.

Names and argument meaning follow the cv::detail objects that image_stitching.cpp's main() drives
(file:line cited per class).  Images are torch CUDA tensors (zero-copy device pointers) or numpy
arrays (host buffers staged by the library).
"""
import ctypes as C
import functools
import math
from dataclasses import dataclass, field

import numpy as np

from . import _capi as capi

try:  # torch is plumbing: device memory + streams
    import torch
except Exception:  # pragma: no cover
    torch = None


class MisError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("libmistitch error %d: %s" % (code, text))
        self.code = code


KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])
DMATCH_DTYPE = np.dtype([("query_idx", "i4"), ("train_idx", "i4"), ("img_idx", "i4"), ("distance", "f4")])

_TORCH_DT = {}
if torch is not None:
    _TORCH_DT = {torch.uint8: capi.U8, torch.int16: capi.S16, torch.float32: capi.F32}
_NP_DT = {np.dtype(np.uint8): capi.U8, np.dtype(np.int16): capi.S16, np.dtype(np.float32): capi.F32}


def _mat9(m):
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(9))
    return a, a.ctypes.data_as(C.c_void_p)


def as_image(a):
    """torch CUDA tensor / numpy array (H,W) or (H,W,C) -> MisImage describing it in place."""
    img = capi.MisImage()
    if torch is not None and isinstance(a, torch.Tensor):
        if a.dim() == 2:
            h, w = a.shape
            c = 1
            assert a.stride(1) == 1, "rows must be dense"
        else:
            h, w, c = a.shape
            assert a.stride(2) == 1 and a.stride(1) == c, "pixels must be dense within a row"
        img.data = a.data_ptr()
        img.stride = a.stride(0) * a.element_size()
        img.dtype = _TORCH_DT[a.dtype]
        img.mem = capi.MEM_DEVICE if a.is_cuda else capi.MEM_HOST
    else:
        a = np.asarray(a)
        if a.ndim == 2:
            h, w = a.shape
            c = 1
            assert a.strides[1] == a.itemsize
        else:
            h, w, c = a.shape
            assert a.strides[2] == a.itemsize and a.strides[1] == c * a.itemsize
        img.data = a.ctypes.data
        img.stride = a.strides[0]
        img.dtype = _NP_DT[a.dtype]
        img.mem = capi.MEM_HOST
    img.width, img.height, img.channels = w, h, c
    return img


def _c_array(ctype, values):
    """values as a C array of ctype; at least one element long, so that n = 0 still hands the library a valid pointer."""
    values = list(values)
    return (ctype * max(len(values), 1))(*values)


def _points(pts):
    return _c_array(capi.MisPoint, (capi.MisPoint(int(p[0]), int(p[1])) for p in pts))


def _images(arrays):
    """The MisImage array of tensors / arrays, which stay the caller's to keep alive for the call."""
    return _c_array(capi.MisImage, (as_image(a) for a in arrays))


def _seam_args(corners, images, masks):
    """The (corners, images, masks, n) arguments of the compensator's and the seam finders' entries."""
    return _points(corners), _images(images), _images(masks), len(masks)


def _empty_image(ctx, h, w, c, tdtype):
    """Device image with 256-byte aligned row pitch, returned as a (possibly strided) tensor view."""
    es = torch.empty((), dtype=tdtype).element_size()
    row = w * c * es
    pitch = (row + 255) // 256 * 256
    buf = torch.empty((h, pitch // es), dtype=tdtype, device=ctx.device)
    # as_strided, not view: a view of a single row reports a dense row stride (w * c), which the library refuses for the
    # fused warp's 16SC3 output when w is odd (rows must be 4-byte aligned)
    return buf.as_strided((h, w, c), (pitch // es, c, 1)) if c > 1 else buf[:, : w * c]


class Context:
    """One HIP device + one stream (include/mistitch.h: MisContext)."""

    def __init__(self, device=0, stream=None):
        self.lib = capi.load()
        if torch is None:
            raise ImportError("torch is required for device memory management")
        self.device = torch.device("cuda", device)
        if stream is None:
            with torch.cuda.device(self.device):
                stream = torch.cuda.current_stream().cuda_stream
        self.stream = stream
        h = C.c_void_p()
        rc = self.lib.mis_context_create(device, C.c_void_p(stream), C.byref(h))
        if rc != capi.MIS_OK:
            raise MisError(rc, "mis_context_create failed (no HIP device? there is no CPU fallback)")
        self.h = h

    def check(self, rc):
        if rc != capi.MIS_OK:
            raise MisError(rc, self.lib.mis_last_error(self.h).decode())

    def synchronize(self):
        self.check(self.lib.mis_context_synchronize(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mis_context_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# warp: cv::detail::{Spherical,Cylindrical,Plane,Mercator,Fisheye,Stereographic,CompressedRectilinear,Panini}Warper, chosen by warp_type
# (image_stitching.cpp:917-969; :973, :985, :988, :1117, :1138, :1154, :1159)
WARP_KINDS = {"spherical": capi.WARP_SPHERICAL, "cylindrical": capi.WARP_CYLINDRICAL, "plane": capi.WARP_PLANE, "mercator": capi.WARP_MERCATOR,
              "fisheye": capi.WARP_FISHEYE, "stereographic": capi.WARP_STEREOGRAPHIC,
              "compressedPlaneA2B1": capi.WARP_COMPRESSED_PLANE_A2B1, "compressedPlaneA1.5B1": capi.WARP_COMPRESSED_PLANE_A15B1,
              "paniniA1.5B1": capi.WARP_PANINI_A15B1}
# the kinds the library builds.  MIS_WARP_PANINI_A2B1 has no warp_type name here: "paniniA2B1" is the suite's example of a refused
# warper (tests/test_refimpl_polar_warpers_cpu.py), so that kind is reached through PaniniWarper(ctx, scale, 2, 1), the C ABI and the
# C++ host
# MIS_WARP_AFFINE has no warp_type name either ("affine" stays a refused name): it is AffineWarper(ctx, scale).
BUILT_WARP_KINDS = frozenset(WARP_KINDS.values()) | {capi.WARP_PANINI_A2B1, capi.WARP_AFFINE}
# the reference's warp_type names beyond the first six kinds (image_stitching.cpp:933-964).  Three of them are built by now: the
# tuple is kept only because tests/test_refimpl_polar_warpers_cpu.py pins its length at ten.  REFUSED_WARP_TYPES -- its names that
# are not in WARP_KINDS -- is the list warp_kind refuses; drop this tuple (and define that one directly) once that test can change
UNBUILT_WARP_TYPES = ("affine", "compressedPlaneA2B1", "compressedPlaneA1.5B1", "compressedPlanePortraitA2B1",
                      "compressedPlanePortraitA1.5B1", "paniniA2B1", "paniniA1.5B1", "paniniPortraitA2B1", "paniniPortraitA1.5B1",
                      "transverseMercator")
REFUSED_WARP_TYPES = tuple(n for n in UNBUILT_WARP_TYPES if n not in WARP_KINDS)


def warp_kind(warp_type):
    """warp_type -> MIS_WARP_* kind; the reference's unbuilt warpers raise NotImplementedError by name, other names ValueError
    (the reference's "Can't create the following warper", image_stitching.cpp:966-970)."""
    if warp_type in WARP_KINDS:
        return WARP_KINDS[warp_type]
    if warp_type in REFUSED_WARP_TYPES:
        raise NotImplementedError("warp_type %r: only %s are implemented (the warpers of the reference's GPU branch, "
                                  "image_stitching.cpp:921-931, and its Mercator, fisheye, stereographic, compressed-plane and Panini "
                                  "A1.5B1 warpers; Panini A2B1 is PaniniWarper(ctx, scale, 2, 1); DESIGN.md section 8)"
                                  % (warp_type, ", ".join(repr(n) for n in WARP_KINDS)))
    raise ValueError("warp_type %r: not a warper the reference knows (image_stitching.cpp:917-969)" % (warp_type,))


def warp_roi(scale, src_size, K, R, kind=capi.WARP_SPHERICAL):
    """RotationWarper::warpRoi(src_size, K, R) -> (x, y, width, height)."""
    lib = capi.load()
    _, kp = _mat9(K)
    _, rp = _mat9(R)
    r = capi.MisRect()
    rc = lib.mis_warper_roi(int(kind), float(scale), int(src_size[0]), int(src_size[1]), kp, rp, C.byref(r))
    if rc != capi.MIS_OK:
        raise MisError(rc, "mis_warper_roi: invalid arguments or a refused roi (kind %d)" % kind)
    return r.x, r.y, r.width, r.height


def warp_rois(ctx, scale, src_size, cameras, kind=capi.WARP_SPHERICAL):
    """The warpRoi loop of main() (image_stitching.cpp:1119-1140) for all cameras in one library call: the border walks run
    in one small kernel on the context's stream -> [(x, y, width, height)]."""
    n = len(cameras)
    Ks = np.ascontiguousarray(np.stack([np.asarray(c["K"], np.float32).reshape(9) for c in cameras]))
    Rs = np.ascontiguousarray(np.stack([np.asarray(c["R"], np.float32).reshape(9) for c in cameras]))
    rr = (capi.MisRect * n)()
    ctx.check(ctx.lib.mis_warper_roi_batch(ctx.h, int(kind), float(scale), int(src_size[0]), int(src_size[1]), n,
                                           Ks.ctypes.data_as(C.c_void_p), Rs.ctypes.data_as(C.c_void_p), rr))
    return [(r.x, r.y, r.width, r.height) for r in rr]


class RotationWarper:
    """warper_creator->create(scale) (image_stitching.cpp:973, :1117) for a warper kind (MIS_WARP_*)."""
    kind = None

    def __init__(self, ctx, scale, kind=None):
        self.ctx, self.scale = ctx, float(scale)
        if kind is not None:
            self.kind = int(kind)
        if self.kind not in BUILT_WARP_KINDS:
            raise NotImplementedError("warper kind %r" % (self.kind,))

    def warpRoi(self, src_size, K, R):
        return self.warp_roi(src_size, K, R)

    def warp_roi(self, src_size, K, R):
        """warpRoi.  The Mercator, fisheye, stereographic, compressed-plane and Panini rois are a scan of every source pixel (those warpers have no
        detectResultRoi of their own): with a context at hand it runs on the device (warp_rois); the other kinds walk the border or
        the corners on the host."""
        if capi.roi_is_full_scan(self.kind) and self.ctx is not None:
            return warp_rois(self.ctx, self.scale, src_size, [{"K": K, "R": R}], self.kind)[0]
        return warp_roi(self.scale, src_size, K, R, self.kind)

    def warp(self, src, K, R, interp=capi.INTER_LINEAR, border=capi.BORDER_REFLECT):
        """Point warp(src, K, R, interp, border, dst) -> (tl, dst)."""
        simg = as_image(src)
        x, y, w, h = self.warp_roi((simg.width, simg.height), K, R)
        dst = _empty_image(self.ctx, h, w, simg.channels, torch.uint8)
        dimg = as_image(dst)
        ka, kp = _mat9(K)
        ra, rp = _mat9(R)
        tl = capi.MisPoint()
        if capi.roi_is_full_scan(self.kind):    # the roi that sized dst was a scan of every source pixel: passed on, not computed again
            rr = capi.MisRect(int(x), int(y), int(w), int(h))
            self.ctx.check(self.ctx.lib.mis_warper_warp_roi(self.ctx.h, self.kind, C.byref(simg), self.scale, kp, rp, C.byref(rr), interp, border,
                                                            C.byref(dimg), C.byref(tl)))
        else:
            self.ctx.check(self.ctx.lib.mis_warper_warp(self.ctx.h, self.kind, C.byref(simg), self.scale, kp, rp, interp, border,
                                                        C.byref(dimg), C.byref(tl)))
        return (tl.x, tl.y), dst

    def alloc_fused(self, roi):
        """Output buffers of warp_fused for a roi (16SC3 image, 8U mask), 256-byte aligned rows."""
        x, y, w, h = roi
        return _empty_image(self.ctx, h, w, 3, torch.int16), _empty_image(self.ctx, h, w, 1, torch.uint8)

    def warp_fused_into(self, src_bgr, K, R, roi, dst, msk):
        simg, dimg, mimg = as_image(src_bgr), as_image(dst), as_image(msk)
        ka, kp = _mat9(K)
        ra, rp = _mat9(R)
        tl = capi.MisPoint()
        if roi is not None:      # the roi warpRoi gave for these parameters: the warp does not walk the border again
            rr = capi.MisRect(int(roi[0]), int(roi[1]), int(roi[2]), int(roi[3]))
            self.ctx.check(self.ctx.lib.mis_warper_warp_fused_roi(self.ctx.h, self.kind, C.byref(simg), self.scale, kp, rp, C.byref(rr),
                                                                  C.byref(dimg), C.byref(mimg), C.byref(tl)))
        else:
            self.ctx.check(self.ctx.lib.mis_warper_warp_fused(self.ctx.h, self.kind, C.byref(simg), self.scale, kp, rp, C.byref(dimg),
                                                              C.byref(mimg), C.byref(tl)))
        return (tl.x, tl.y)

    @staticmethod
    def _batch_args(imgs, cameras, rois, dsts, masks):
        """The C arrays of a batched fused warp -> (im, ds, ms, Ks, Rs, rs, tls); Ks / Rs are the numpy arrays (they own the floats)."""
        n = len(imgs)
        im = _images(imgs)
        ds = _images(dsts)
        ms = _images(masks)
        Ks = np.ascontiguousarray(np.stack([np.asarray(c["K"], np.float32).reshape(9) for c in cameras]))
        Rs = np.ascontiguousarray(np.stack([np.asarray(c["R"], np.float32).reshape(9) for c in cameras]))
        rs = (capi.MisRect * n)(*[capi.MisRect(int(r[0]), int(r[1]), int(r[2]), int(r[3])) for r in rois])
        return im, ds, ms, Ks, Rs, rs, (capi.MisPoint * n)()

    def warp_fused_batch(self, imgs, cameras, rois):
        """mis_warper_warp_fused_batch: the compose-scale step of main() for all frames (one grid per 16 frames)
        -> [(tl, img_warped_s, mask_warped)], the results of warp_fused per frame."""
        n = len(imgs)
        if n == 0:
            return []
        outs = [self.alloc_fused(r) for r in rois]
        im, ds, ms, Ks, Rs, rs, tls = self._batch_args(imgs, cameras, rois, [o[0] for o in outs], [o[1] for o in outs])
        fp = C.POINTER(C.c_float)
        self.ctx.check(self.ctx.lib.mis_warper_warp_fused_batch(self.ctx.h, self.kind, im, n, float(self.scale), Ks.ctypes.data_as(fp), Rs.ctypes.data_as(fp), rs, ds, ms, tls))
        return [((t.x, t.y), o[0], o[1]) for t, o in zip(tls, outs)]

    def warp_fused_batch_timed(self, imgs, cameras, rois, dsts, masks, repeats):
        """mis_warp_spherical_fused_batch_timed: the fused warps of all frames in one grid per 16 frames, launched `repeats` times
        back to back between two HIP events on the context's stream -> average microseconds of one pass over all frames
        (a measurement aid of the spherical warper)."""
        if self.kind != capi.WARP_SPHERICAL:
            raise NotImplementedError("the timed warps measure the spherical kind only")
        n = len(imgs)
        im, ds, ms, Ks, Rs, rs, tls = self._batch_args(imgs, cameras, rois, dsts, masks)
        us = C.c_float()
        fp = C.POINTER(C.c_float)
        self.ctx.check(self.ctx.lib.mis_warp_spherical_fused_batch_timed(self.ctx.h, im, n, float(self.scale), Ks.ctypes.data_as(fp), Rs.ctypes.data_as(fp), rs, ds, ms, tls,
                                                                        int(repeats), C.byref(us)))
        return us.value

    def warp_fused_timed(self, src_bgr, K, R, roi, dst, msk, repeats):
        """Average duration (us) of the fused warp kernel over `repeats` back-to-back launches (HIP events; spherical only)."""
        if self.kind != capi.WARP_SPHERICAL:
            raise NotImplementedError("the timed warps measure the spherical kind only")
        simg, dimg, mimg = as_image(src_bgr), as_image(dst), as_image(msk)
        ka, kp = _mat9(K)
        ra, rp = _mat9(R)
        tl, us = capi.MisPoint(), C.c_float()
        self.ctx.check(self.ctx.lib.mis_warp_spherical_fused_timed(self.ctx.h, C.byref(simg), self.scale, kp, rp, C.byref(dimg),
                                                                   C.byref(mimg), C.byref(tl), int(repeats), C.byref(us)))
        return float(us.value)

    def warp_fused(self, src_bgr, K, R, roi=None):
        """Compose-scale step of main(): warp(img, LINEAR, REFLECT) + warp(mask, NEAREST, CONSTANT) +
        convertTo(CV_16S) (image_stitching.cpp:1154-1164) -> (tl, img_warped_s, mask_warped)."""
        if roi is None:
            simg = as_image(src_bgr)
            roi = self.warp_roi((simg.width, simg.height), K, R)
        dst, msk = self.alloc_fused(roi)
        tl = self.warp_fused_into(src_bgr, K, R, roi, dst, msk)
        return tl, dst, msk

    # ---- warpPoint / warpPointBackward / buildMaps / warpBackward ----
    def warp_points(self, pts, K, R, backward=False):
        """mis_warper_warp_points: mapForward (or, backward=True, mapBackward at float coordinates) of an (n, 2) array of points
        -> (n, 2) float32.  A warper without a context (ctx None) runs the library's host loop, which the kernel equals in every bit."""
        xy = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
        out = np.empty_like(xy)
        _, kp = _mat9(K)
        _, rp = _mat9(R)
        lib = capi.load()
        rc = lib.mis_warper_warp_points(self.ctx.h if self.ctx is not None else None, self.kind, self.scale, kp, rp,
                                        capi.MAP_BACKWARD if backward else capi.MAP_FORWARD, xy.ctypes.data_as(C.c_void_p),
                                        out.ctypes.data_as(C.c_void_p), len(xy))
        if rc != capi.MIS_OK:
            raise MisError(rc, self.ctx.lib.mis_last_error(self.ctx.h).decode() if self.ctx is not None else "mis_warper_warp_points: invalid arguments")
        return out

    def warpPoint(self, pt, K, R):
        """Point2f warpPoint(pt, K, R) -> (u, v)."""
        u, v = self.warp_points([pt], K, R)[0]
        return float(u), float(v)

    def warpPointBackward(self, pt, K, R):
        """Point2f warpPointBackward(pt, K, R) -> (x, y); (-1, -1) behind the camera for the kinds that test z > 0."""
        x, y = self.warp_points([pt], K, R, backward=True)[0]
        return float(x), float(y)

    def build_maps(self, src_size, K, R, roi=None, xmap=None, ymap=None):
        """mis_warper_build_maps -> (roi, xmap, ymap): the backward map of every roi pixel as two float32 device tensors (given ones
        are written in place, at their pitch).  roi: the one warp_roi gave for these parameters, or None (computed)."""
        if roi is None:
            roi = self.warp_roi(src_size, K, R)
        x, y, w, h = (int(v) for v in roi)
        xmap = _empty_image(self.ctx, h, w, 1, torch.float32) if xmap is None else xmap
        ymap = _empty_image(self.ctx, h, w, 1, torch.float32) if ymap is None else ymap
        ximg, yimg = as_image(xmap), as_image(ymap)
        _, kp = _mat9(K)
        _, rp = _mat9(R)
        rin, rout = capi.MisRect(x, y, w, h), capi.MisRect()
        self.ctx.check(self.ctx.lib.mis_warper_build_maps(self.ctx.h, self.kind, self.scale, int(src_size[0]), int(src_size[1]), kp, rp, C.byref(rin),
                                                          C.byref(ximg), C.byref(yimg), C.byref(rout)))
        return (rout.x, rout.y, rout.width, rout.height), xmap, ymap

    def buildMaps(self, src_size, K, R):
        """Rect buildMaps(src_size, K, R, xmap, ymap) -> (roi, xmap, ymap).  roi is (x, y, width, height) with the maps' size; OpenCV
        returns Rect(tl, br), one less in both directions."""
        return self.build_maps(src_size, K, R)

    def _back_view(self, dst_size, cn, with_mask, dst=None, mask=None):
        w, h = int(dst_size[0]), int(dst_size[1])
        if w <= 0 or h <= 0:
            raise ValueError("dst_size %r must be positive" % (dst_size,))
        dst = _empty_image(self.ctx, h, w, cn, torch.uint8) if dst is None else dst
        mask = (_empty_image(self.ctx, h, w, 1, torch.uint8) if mask is None else mask) if with_mask else None
        return dst, mask

    def warp_backward(self, src, src_tl, K, R, dst_size, interp=capi.INTER_LINEAR, border=capi.BORDER_CONSTANT, with_mask=False, dst=None, mask=None):
        """mis_warper_warp_backward: the pinhole view (K, R) of size dst_size = (w, h) out of `src`, an 8UC1 / 8UC3 image whose
        top-left pixel lies at src_tl in this warper's plane (a warped frame with its corner, a panorama with result_roi's corner)
        -> dst, or (dst, mask) with with_mask (255 where the nearest source pixel lies inside src)."""
        simg = as_image(src)
        dst, mask = self._back_view(dst_size, simg.channels, with_mask, dst, mask)
        dimg = as_image(dst)
        mimg = as_image(mask) if mask is not None else None
        _, kp = _mat9(K)
        _, rp = _mat9(R)
        self.ctx.check(self.ctx.lib.mis_warper_warp_backward(self.ctx.h, self.kind, C.byref(simg), capi.MisPoint(int(src_tl[0]), int(src_tl[1])), self.scale, kp, rp,
                                                             int(interp), int(border), dimg.width, dimg.height, C.byref(dimg),
                                                             C.byref(mimg) if mimg is not None else None))
        return (dst, mask) if with_mask else dst

    def warp_backward_batch(self, src, src_tl, cameras, dst_sizes, interp=capi.INTER_LINEAR, border=capi.BORDER_CONSTANT, with_mask=False):
        """mis_warper_warp_backward_batch: the views of `cameras` ({"K", "R"} each) of sizes dst_sizes out of one source, up to 16
        views per grid -> [dst] or [(dst, mask)], the results of warp_backward per view."""
        n = len(cameras)
        if n == 0:
            return []
        simg = as_image(src)
        outs = [self._back_view(s, simg.channels, with_mask) for s in dst_sizes]
        ds = _images([o[0] for o in outs])
        ms = _images([o[1] for o in outs]) if with_mask else None
        Ks = np.ascontiguousarray(np.stack([np.asarray(c["K"], np.float32).reshape(9) for c in cameras]))
        Rs = np.ascontiguousarray(np.stack([np.asarray(c["R"], np.float32).reshape(9) for c in cameras]))
        sz = _c_array(capi.MisSize, (capi.MisSize(int(s[0]), int(s[1])) for s in dst_sizes))
        self.ctx.check(self.ctx.lib.mis_warper_warp_backward_batch(self.ctx.h, self.kind, C.byref(simg), capi.MisPoint(int(src_tl[0]), int(src_tl[1])), self.scale, n,
                                                                   Ks.ctypes.data_as(C.c_void_p), Rs.ctypes.data_as(C.c_void_p), sz, int(interp), int(border), ds, ms))
        return [(o[0], o[1]) if with_mask else o[0] for o in outs]

    def warpBackward(self, src, K, R, interp, border, dst_size):
        """void warpBackward(src, K, R, interp, border, dst_size, dst) -> dst.  src must have exactly the size of warpRoi(dst_size, K, R),
        as OpenCV asserts (ValueError otherwise); its top-left is that roi's."""
        simg = as_image(src)
        x, y, w, h = self.warp_roi(dst_size, K, R)
        if (simg.width, simg.height) != (w, h):
            raise ValueError("warpBackward: src is %dx%d, the roi of dst_size %r is %dx%d (OpenCV: CV_Assert(src_size == src.size()))"
                             % (simg.width, simg.height, tuple(dst_size), w, h))
        return self.warp_backward(src, (x, y), K, R, dst_size, interp, border)


class SphericalWarper(RotationWarper):
    """SphericalWarper::create(scale) (image_stitching.cpp:927, :939)."""
    kind = capi.WARP_SPHERICAL


class CylindricalWarper(RotationWarper):
    """CylindricalWarper::create(scale) (image_stitching.cpp:925, :937)."""
    kind = capi.WARP_CYLINDRICAL


class PlaneWarper(RotationWarper):
    """PlaneWarper::create(scale) with T = 0 (image_stitching.cpp:923, :933)."""
    kind = capi.WARP_PLANE


class AffineWarper(RotationWarper):
    """AffineWarper::create(scale) (image_stitching.cpp:935-936): the plane warper with a translation.  Every `R` argument is the
    3x3 homogeneous affine H of cv::detail::AffineWarper::warp(src, K, H, ...)."""
    kind = capi.WARP_AFFINE


class MercatorWarper(RotationWarper):
    """MercatorWarper::create(scale) (image_stitching.cpp:961-962)."""
    kind = capi.WARP_MERCATOR


class FisheyeWarper(RotationWarper):
    """FisheyeWarper::create(scale) (image_stitching.cpp:941-942): the polar map, evaluated per output pixel."""
    kind = capi.WARP_FISHEYE


class StereographicWarper(RotationWarper):
    """StereographicWarper::create(scale) (image_stitching.cpp:943-944): the polar map, evaluated per output pixel."""
    kind = capi.WARP_STEREOGRAPHIC


def _ab_kind(name, kinds, A, B):
    """(A, B) of a compressed-plane / Panini warper -> its kind: the C ABI has one kind per setting the reference offers."""
    try:
        return kinds[(float(A), float(B))]
    except KeyError:
        raise NotImplementedError("%s(A=%r, B=%r): only (A, B) = (2, 1) and (1.5, 1) are built (one MIS_WARP_* kind each)" % (name, A, B)) from None


class CompressedRectilinearWarper(RotationWarper):
    """CompressedRectilinearWarper(A, B)::create(scale) (image_stitching.cpp:945-948): the column angle once per column and tile,
    the row angle per output pixel."""
    KINDS = {(2.0, 1.0): capi.WARP_COMPRESSED_PLANE_A2B1, (1.5, 1.0): capi.WARP_COMPRESSED_PLANE_A15B1}

    def __init__(self, ctx, scale, A=2.0, B=1.0):
        super().__init__(ctx, scale, _ab_kind("CompressedRectilinearWarper", self.KINDS, A, B))


class PaniniWarper(RotationWarper):
    """PaniniWarper(A, B)::create(scale) (image_stitching.cpp:953-956): as the compressed-plane warper."""
    KINDS = {(2.0, 1.0): capi.WARP_PANINI_A2B1, (1.5, 1.0): capi.WARP_PANINI_A15B1}

    def __init__(self, ctx, scale, A=2.0, B=1.0):
        super().__init__(ctx, scale, _ab_kind("PaniniWarper", self.KINDS, A, B))


def make_warper(ctx, scale, warp_type="spherical"):
    """warper_creator (image_stitching.cpp:917-969) -> create(scale)."""
    return RotationWarper(ctx, scale, warp_kind(warp_type))


# ------------------------------------------------------------------------------------------------
# image operators either side of the path (image_stitching.cpp:571-580, :619, :1144, :1169-1171)
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


class _Compensator:
    """One member of cv::detail::ExposureCompensator's family over mis_compensator_*.  feed() takes the seam-scale warped images /
    masks and their corners and never alters them, whatever nr_feeds is (the library works on private device copies); apply()
    multiplies an 8UC3 (or the fused warp's 16SC3) image by the gains, in place."""
    TYPE = None

    def _create(self, ctx, nr_feeds, bl_width=64, bl_height=64, nr_gain_filtering_iterations=2):
        self.ctx = ctx
        h = C.c_void_p()
        params = capi.MisCompensatorParams(self.TYPE, nr_feeds, bl_width, bl_height, nr_gain_filtering_iterations)
        ctx.check(ctx.lib.mis_compensator_create_ex(ctx.h, C.byref(params), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:   # a destroyed context already released the device (the C object points into it)
            self.ctx.lib.mis_compensator_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed(self, corners, images, masks):
        self.ctx.check(self.ctx.lib.mis_compensator_feed(self.h, *_seam_args(corners, images, masks)))

    def gains(self, index):
        """The accumulated gains of one image as three float64 (B, G, R; GainCompensator: the gain three times); the block types
        have a gain map instead and raise."""
        g = (C.c_double * 3)()
        self.ctx.check(self.ctx.lib.mis_compensator_gains(self.h, index, g))
        return np.array(g[:], np.float64)

    def gain_map(self, index):
        """The smoothed float32 gain map of one image: (by, bx) for BlocksGainCompensator, (by, bx, 3) for BlocksChannelsCompensator;
        GainCompensator and ChannelsCompensator have per-image gains instead and raise."""
        bx, by, ch = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.mis_compensator_gain_map_channels(self.h, index, None, 0, C.byref(bx), C.byref(by), C.byref(ch)))
        out = np.zeros((by.value, bx.value) if ch.value == 1 else (by.value, bx.value, ch.value), np.float32)
        self.ctx.check(self.ctx.lib.mis_compensator_gain_map_channels(self.h, index, out.ctypes.data_as(C.POINTER(C.c_float)), out.size, None, None, None))
        return out

    def debug_stats(self, i, j, channel=0):
        """Test hook (GainCompensator, ChannelsCompensator): (N_ij, I_ij, I_ji) of the last feed."""
        n, a, b = C.c_int(), C.c_double(), C.c_double()
        self.ctx.check(self.ctx.lib.mis_compensator_debug_stats(self.h, i, j, channel, C.byref(n), C.byref(a), C.byref(b)))
        return n.value, a.value, b.value

    def apply(self, index, corner, image, mask=None):
        """corner and mask are accepted for signature parity (OpenCV ignores them too)."""
        img = as_image(image)
        self.ctx.check(self.ctx.lib.mis_compensator_apply(self.h, index, C.byref(img)))
        return image


class GainCompensator(_Compensator):
    """cv::detail::GainCompensator(nr_feeds): one gain per frame from the whole-frame overlap statistics."""
    TYPE = capi.EXPOS_GAIN

    def __init__(self, ctx, nr_feeds=1):
        self._create(ctx, nr_feeds)


class ChannelsCompensator(_Compensator):
    """cv::detail::ChannelsCompensator(nr_feeds): a GainCompensator per colour channel; gains(i) = (B, G, R)."""
    TYPE = capi.EXPOS_CHANNELS

    def __init__(self, ctx, nr_feeds=1):
        self._create(ctx, nr_feeds)


class BlocksGainCompensator(_Compensator):
    """cv::detail::BlocksGainCompensator as the reference configures it (image_stitching.cpp:1002-1023): 64x64 blocks,
    one feed, two gain-filtering passes."""
    TYPE = capi.EXPOS_GAIN_BLOCKS

    def __init__(self, ctx, bl_width=64, bl_height=64, nr_gain_filtering_iterations=2, nr_feeds=1):
        self._create(ctx, nr_feeds, bl_width, bl_height, nr_gain_filtering_iterations)


class BlocksChannelsCompensator(_Compensator):
    """cv::detail::BlocksChannelsCompensator: a gain per block and colour channel, smoothed into a three-channel map."""
    TYPE = capi.EXPOS_CHANNELS_BLOCKS

    def __init__(self, ctx, bl_width=64, bl_height=64, nr_gain_filtering_iterations=2, nr_feeds=1):
        self._create(ctx, nr_feeds, bl_width, bl_height, nr_gain_filtering_iterations)


# expos_comp_type (image_stitching.cpp:73, :1002-1012) as a configuration name.  "channels" is NOT among them: ChannelsCompensator is
# built (the class above, MIS_EXPOS_CHANNELS, the C++ host's --expos_comp channels), but the suite pins "channels" as its example
# of a configuration value that is refused by name (tests/test_expos_gpu.py, tests/test_distributed_cpu.py), so the Python
# configuration keeps refusing it; build the compensator directly where it is wanted
EXPOS_COMP_TYPES = ("no", "gain", "gain_blocks", "channels_blocks")


def make_compensator(ctx, cfg):
    """expos_comp_type / expos_comp_nr_feeds of the config -> the compensator (image_stitching.cpp:1002-1016), None for "no"."""
    t, feeds = cfg.expos_comp_type, cfg.expos_comp_nr_feeds
    blocks = (cfg.expos_comp_block_size, cfg.expos_comp_block_size, cfg.expos_comp_nr_filtering, feeds)
    if t == "gain":
        return GainCompensator(ctx, feeds)
    if t == "gain_blocks":
        return BlocksGainCompensator(ctx, *blocks)
    if t == "channels_blocks":
        return BlocksChannelsCompensator(ctx, *blocks)
    return None


def make_seam_finder(ctx, cfg):
    """seam_find_type of the config -> the seam finder (image_stitching.cpp:1029-1062), None for "no"."""
    make = {"voronoi": lambda: VoronoiSeamFinder(ctx), "dp_color": lambda: DpSeamFinder(ctx, DpSeamFinder.COLOR),
            "dp_colorgrad": lambda: DpSeamFinder(ctx, DpSeamFinder.COLOR_GRAD)}.get(cfg.seam_find_type)
    return make() if make else None


class NoSeamFinder:
    """seam_find_type "no" (image_stitching.cpp:1029): masks stay as warped."""

    def find(self, images, corners, masks):
        return masks


class VoronoiSeamFinder:
    """seam_find_type "voronoi" (image_stitching.cpp:1031); images are not looked at."""

    def __init__(self, ctx):
        self.ctx = ctx

    def find(self, images, corners, masks):
        n = len(masks)
        cs = _points(corners)
        mk = _images(masks)
        self.ctx.check(self.ctx.lib.mis_seam_voronoi(self.ctx.h, cs, mk, n))
        return masks


class DpSeamFinder:
    """seam_find_type "dp_color" -- the reference's default (image_stitching.cpp:77, :1056-1057, :1065): DpSeamFinder(COLOR) --
    and "dp_colorgrad" (:1057-1058): DpSeamFinder(COLOR_GRAD), whose cut costs are divided by the images' Sobel derivatives
    (one kernel launch for all frames, csrc/seam_grad.hip).  images: the seam-scale warped 8UC3 images; masks are edited in place.
    cost_func: DpSeamFinder.COLOR (0), or a name as OpenCV 4's DpSeamFinder(String costFunc) takes it: "COLOR" | "COLOR_GRAD".
    An integer goes to mis_seam_dp as it is (which runs COLOR only); COLOR_GRAD runs mis_seam_dp_colorgrad."""
    COLOR = 0
    COLOR_GRAD = "COLOR_GRAD"

    def __init__(self, ctx, cost_func=0):
        if isinstance(cost_func, str):
            if cost_func not in ("COLOR", "COLOR_GRAD"):
                raise ValueError("DpSeamFinder cost function %r: 'COLOR' or 'COLOR_GRAD'" % (cost_func,))
            if cost_func == "COLOR":
                cost_func = DpSeamFinder.COLOR
        self.ctx, self.cost_func = ctx, cost_func

    def find(self, images, corners, masks):
        cs, im, mk, n = _seam_args(corners, images, masks)
        if self.cost_func == DpSeamFinder.COLOR_GRAD:
            self.ctx.check(self.ctx.lib.mis_seam_dp_colorgrad(self.ctx.h, cs, im, mk, n))
        else:
            self.ctx.check(self.ctx.lib.mis_seam_dp(self.ctx.h, cs, im, mk, n, int(self.cost_func)))
        return masks


class GraphCutSeamFinder:
    """cv::detail::GraphCutSeamFinder(COST_COLOR, terminal_cost, bad_region_penalty) -- the seam finder of the reference's try_cuda
    branch (image_stitching.cpp:1037-1054) and of OpenCV's own stitcher -- over mis_seam_graphcut: a device max-flow per
    overlapping pair (csrc/seam_gc.hip; the definition is SURVEY.md appendix A.13).  images: the seam-scale warped 8UC3 images;
    masks are edited in place.  cost_type: "COST_COLOR"; "COST_COLOR_GRAD" is known and not built (NotImplementedError), any
    other value is a ValueError.  The class is not a configuration name: hand an instance to Stitcher.set_seam_finder."""
    COST_TYPES = {"COST_COLOR": 0, "COST_COLOR_GRAD": 1}

    def __init__(self, ctx, cost_type="COST_COLOR", terminal_cost=10000.0, bad_region_penalty=1000.0):
        if not isinstance(cost_type, str) or cost_type not in GraphCutSeamFinder.COST_TYPES:
            raise ValueError("GraphCutSeamFinder cost type %r: 'COST_COLOR' or 'COST_COLOR_GRAD'" % (cost_type,))
        if cost_type == "COST_COLOR_GRAD":
            raise NotImplementedError("GraphCutSeamFinder cost type 'COST_COLOR_GRAD' is not built (DESIGN.md section 8); 'COST_COLOR' is")
        self.ctx, self.cost_type = ctx, cost_type
        self.terminal_cost, self.bad_region_penalty = float(terminal_cost), float(bad_region_penalty)

    def find(self, images, corners, masks):
        cs, im, mk, n = _seam_args(corners, images, masks)
        self.ctx.check(self.ctx.lib.mis_seam_graphcut(self.ctx.h, cs, im, mk, n, GraphCutSeamFinder.COST_TYPES[self.cost_type],
                                                      self.terminal_cost, self.bad_region_penalty))
        return masks

    def stats(self):
        """The counts of the context's last find: pairs, levels, grid nodes, the round-set cap, global relabels, relabel sweeps and
        the round sets of every level."""
        count = C.c_int(0)
        self.ctx.check(self.ctx.lib.mis_seam_graphcut_stats(self.ctx.h, None, 0, C.byref(count)))
        out = (C.c_int * max(count.value, 1))()
        self.ctx.check(self.ctx.lib.mis_seam_graphcut_stats(self.ctx.h, out, count.value, C.byref(count)))
        v = list(out[:count.value])
        if len(v) < 6:
            return None
        return dict(pairs=v[0], levels=v[1], nodes=v[2], round_set_cap=v[3], relabels=v[4], sweeps=v[5], round_sets=v[6:])

    def debug_pair(self, images, corners, masks, i, j):
        """mis_seam_graphcut_debug_pair: pair (i, j) on the masks as given -> (cap_right, cap_down, terminals, labels), numpy planes
        of the pair's grid (the gap included); nothing is edited."""
        cs, im, mk, n = _seam_args(corners, images, masks)
        gw, gh = C.c_int(0), C.c_int(0)
        self.ctx.check(self.ctx.lib.mis_seam_graphcut_debug_pair(self.ctx.h, cs, im, mk, n, i, j, None, None, None, None, 0, C.byref(gw), C.byref(gh)))
        shape = (gh.value, gw.value)
        cr, cd, term = np.empty(shape, np.int32), np.empty(shape, np.int32), np.empty(shape, np.int32)
        lab = np.empty(shape, np.uint8)
        p32 = C.POINTER(C.c_int32)
        self.ctx.check(self.ctx.lib.mis_seam_graphcut_debug_pair(self.ctx.h, cs, im, mk, n, i, j, cr.ctypes.data_as(p32), cd.ctypes.data_as(p32), term.ctypes.data_as(p32),
                                                                 lab.ctypes.data_as(C.POINTER(C.c_uint8)), cr.size, C.byref(gw), C.byref(gh)))
        return cr, cd, term, lab


def seam_gradients(ctx, images, gradx=None, grady=None):
    """DpSeamFinder::computeGradients of every image in one launch (mis_seam_gradients): BGR -> grey, then the 3 x 3 Sobel
    derivatives along x and y (BORDER_REFLECT_101) -> (gradx, grady), lists of float32 planes.  images: 8UC3 device tensors or
    host arrays; a plane is allocated where its image lives (a device tensor or a numpy array) unless gradx / grady give the
    buffers to fill."""
    n = len(images)

    def planes(given):
        if given is not None:
            return list(given)
        return [torch.empty(tuple(i.shape[:2]), dtype=torch.float32, device=i.device) if torch is not None and isinstance(i, torch.Tensor)
                else np.empty(np.asarray(i).shape[:2], np.float32) for i in images]
    gx, gy = planes(gradx), planes(grady)
    if len(gx) != n or len(gy) != n:
        raise ValueError("seam_gradients: %d images, %d gradx and %d grady planes" % (n, len(gx), len(gy)))
    im = _images(images)
    ax = _images(gx)
    ay = _images(gy)
    ctx.check(ctx.lib.mis_seam_gradients(ctx.h, im, n, ax, ay))
    return gx, gy


# ------------------------------------------------------------------------------------------------
# blend: cv::detail::Blender / MultiBandBlender / FeatherBlender (image_stitching.cpp:1173-1225)
def result_roi(corners, sizes):
    lib = capi.load()
    n = len(corners)
    cs = _points(corners)
    ss = (capi.MisSize * n)(*[capi.MisSize(int(s[0]), int(s[1])) for s in sizes])
    r = capi.MisRect()
    rc = lib.mis_result_roi(cs, ss, n, C.byref(r))
    if rc != capi.MIS_OK:
        raise MisError(rc, "mis_result_roi: invalid arguments")
    return r.x, r.y, r.width, r.height


def blend_config(blend_type, blend_strength, pano_size):
    """image_stitching.cpp:1176-1190 -> (type, num_bands, sharpness)."""
    lib = capi.load()
    t, nb, sh = C.c_int(), C.c_int(), C.c_float()
    lib.mis_blend_config(int(blend_type), float(blend_strength), int(pano_size[0]), int(pano_size[1]), C.byref(t),
                         C.byref(nb), C.byref(sh))
    return t.value, nb.value, sh.value


class Blender:
    """Blender::createDefault(type) (image_stitching.cpp:1175)."""

    def __init__(self, ctx, btype=capi.BLEND_NO, num_bands=5, sharpness=0.02):
        self.ctx = ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.mis_blender_create(ctx.h, btype, num_bands, sharpness, C.byref(h)))
        self.h = h
        self.type = btype
        self._size = None

    @staticmethod
    def createDefault(ctx, btype):
        return {capi.BLEND_NO: Blender, capi.BLEND_FEATHER: FeatherBlender, capi.BLEND_MULTI_BAND: MultiBandBlender}[btype](ctx)

    def prepare(self, corners, sizes):
        n = len(corners)
        cs = _points(corners)
        ss = (capi.MisSize * n)(*[capi.MisSize(int(s[0]), int(s[1])) for s in sizes])
        self.ctx.check(self.ctx.lib.mis_blender_prepare(self.h, cs, ss, n))
        x, y, w, h = result_roi(corners, sizes)
        self._size = (w, h)

    def compose_frames(self, frames, scale, cameras, rois, kind=capi.WARP_SPHERICAL):
        """The compositing loop's per-frame body for all frames in one library call (fused warp + feed each;
        image_stitching.cpp:1154-1164, :1218): the calling thread stays out of the interpreter between launches."""
        n = len(frames)
        if n == 0:
            return
        arr = _images(frames)
        Ks = np.ascontiguousarray(np.stack([np.asarray(c["K"], np.float32).reshape(9) for c in cameras]))
        Rs = np.ascontiguousarray(np.stack([np.asarray(c["R"], np.float32).reshape(9) for c in cameras]))
        rr = (capi.MisRect * n)(*[capi.MisRect(int(r[0]), int(r[1]), int(r[2]), int(r[3])) for r in rois])
        self.ctx.check(self.ctx.lib.mis_compose_frames_kind(self.h, int(kind), arr, n, float(scale), Ks.ctypes.data_as(C.c_void_p),
                                                            Rs.ctypes.data_as(C.c_void_p), rr))

    def feed(self, img, mask, tl):
        i, m = as_image(img), as_image(mask)
        self.ctx.check(self.ctx.lib.mis_blender_feed(self.h, C.byref(i), C.byref(m), capi.MisPoint(int(tl[0]), int(tl[1]))))

    def feed_batch(self, imgs, masks, tls):
        """n feeds in one call (mis_blender_feed_batch): the result of feed(imgs[0], ...) ... feed(imgs[n - 1], ...) in that order."""
        n = len(imgs)
        im = _images(imgs)
        mk = _images(masks)
        ts = _points(tls)
        self.ctx.check(self.ctx.lib.mis_blender_feed_batch(self.h, im, mk, ts, n))

    def blend(self):
        if self._size is None:
            raise MisError(-5, "blend before prepare")      # MIS_E_STATE, as the library answers
        w, h = self._size
        dst = _empty_image(self.ctx, h, w, 3, torch.int16)
        msk = _empty_image(self.ctx, h, w, 1, torch.uint8)
        d, m = as_image(dst), as_image(msk)
        self.ctx.check(self.ctx.lib.mis_blender_blend(self.h, C.byref(d), C.byref(m)))
        return dst, msk

    def level(self, i):
        """Accumulated pyramid level (host copies) before blend() -- parity tests only."""
        w, h, lp, wp = C.c_int(), C.c_int(), C.c_void_p(), C.c_void_p()
        self.ctx.check(self.ctx.lib.mis_blender_level_info(self.h, i, C.byref(w), C.byref(h), C.byref(lp), C.byref(wp)))
        self.ctx.synchronize()
        n = w.value * h.value
        lap = np.empty((h.value, w.value, 3), np.int16)
        wgt = np.empty((h.value, w.value), np.float32)
        # raw device pointers -> host through torch's runtime binding
        _memcpy_dtoh(lap, lp.value, n * 6)
        _memcpy_dtoh(wgt, wp.value, n * 4)
        return lap, wgt

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:   # a destroyed context already released the device
            self.ctx.lib.mis_blender_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MultiBandBlender(Blender):
    """MultiBandBlender + setNumBands (image_stitching.cpp:1180-1184)."""

    def __init__(self, ctx, num_bands=5):
        super().__init__(ctx, capi.BLEND_MULTI_BAND, num_bands, 0.0)

    def numBands(self):
        return self.ctx.lib.mis_blender_num_bands(self.h)


class FeatherBlender(Blender):
    """FeatherBlender + setSharpness (image_stitching.cpp:1186-1190)."""

    def __init__(self, ctx, sharpness=0.02):
        super().__init__(ctx, capi.BLEND_FEATHER, 0, sharpness)


_hip = None


def _memcpy_dtoh(dst_np, dev_ptr, nbytes):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rc = _hip.hipMemcpy(dst_np.ctypes.data_as(C.c_void_p), C.c_void_p(dev_ptr), nbytes, 2)
    if rc:
        raise RuntimeError("hipMemcpy D2H failed: %d" % rc)


# ------------------------------------------------------------------------------------------------
# features: ORB::create + computeImageFeatures (image_stitching.cpp:545, :613)
class ImageFeatures:
    """cv::detail::ImageFeatures: device-resident keypoints + descriptors."""

    def __init__(self, ctx, raw):
        self.ctx, self.raw = ctx, raw

    @property
    def img_idx(self):
        return self.raw.img_idx

    @img_idx.setter
    def img_idx(self, v):
        self.raw.img_idx = int(v)

    @property
    def img_size(self):
        return self.raw.img_w, self.raw.img_h

    def __len__(self):
        return self.raw.n

    def download(self):
        """-> (keypoints structured array, descriptors (n, cols))"""
        n = self.raw.n
        kps = np.zeros(n, KP_DTYPE)
        dt = np.uint8 if self.raw.desc_dtype == capi.U8 else np.float32
        desc = np.zeros((n, self.raw.desc_cols), dt)
        if n:
            self.ctx.check(self.ctx.lib.mis_features_download(self.ctx.h, C.byref(self.raw), kps.ctypes.data_as(C.c_void_p),
                                                              desc.ctypes.data_as(C.c_void_p)))
        return kps, desc

    @staticmethod
    def upload(ctx, img_size, kps, desc, img_idx=0):
        kps = np.ascontiguousarray(kps, KP_DTYPE)
        desc = np.ascontiguousarray(desc)
        raw = capi.MisFeatures()
        ctx.check(ctx.lib.mis_features_upload(ctx.h, int(img_size[0]), int(img_size[1]), len(kps),
                                              kps.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), desc.shape[1],
                                              _NP_DT[desc.dtype], C.byref(raw)))
        raw.img_idx = img_idx
        return ImageFeatures(ctx, raw)

    def close(self):
        if self.raw is not None and self.ctx.h:
            self.ctx.lib.mis_features_free(self.ctx.h, C.byref(self.raw))
        self.raw = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def orb_params(**kw):
    p = capi.MisOrbParams()
    capi.load().mis_orb_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class OrbFeatureFinder:
    """ORB::create(4000, 1.2, 8, 1, 0, 2, HARRIS_SCORE, 40, 20) (image_stitching.cpp:545)."""

    def __init__(self, ctx, max_size, params=None):
        self.ctx = ctx
        self.params = params or orb_params()
        h = C.c_void_p()
        ctx.check(ctx.lib.mis_orb_create(ctx.h, C.byref(self.params), int(max_size[0]), int(max_size[1]), C.byref(h)))
        self.h = h

    def detect(self, img):
        raw = capi.MisFeatures()
        i = as_image(img)
        self.ctx.check(self.ctx.lib.mis_orb_detect(self.h, C.byref(i), C.byref(raw)))
        return ImageFeatures(self.ctx, raw)

    def on_enqueued(self, fn):
        """fn() runs inside this finder's NEXT detect_batch call, on the calling thread, once the batch's device work is enqueued
        (mis_orb_on_enqueued).  fn=None clears a pending hook."""
        if fn is None:
            self._enqueued_fn = None
            self.ctx.lib.mis_orb_on_enqueued(self.h, None, None)
            return
        # ONE ctypes callback object per instance, created on first use: a CFUNCTYPE instance is a reference cycle that only the
        # cyclic garbage collector frees, and a fresh one per step kept that step's closure -- and through it the step's panorama --
        # alive while bench.py times with the collector paused (config 5: +1 GB of allocator growth per step, round 4)
        self._enqueued_fn = fn
        if getattr(self, "_enqueued_cb", None) is None:
            self._enqueued_cb = C.CFUNCTYPE(None, C.c_void_p)(self._run_enqueued)
        self.ctx.check(self.ctx.lib.mis_orb_on_enqueued(self.h, C.cast(self._enqueued_cb, C.c_void_p), None))

    def arm_knn_ahead(self, n, mask=None, range_width=-1, rank=0, world_size=1):
        """One-shot: the NEXT detect_batch call, of n frames, enqueues the matcher's Hamming 2-NN pass for this pair selection behind
        its own kernels (mis_orb_arm_knn_ahead); the context's next matcher call adopts the pass when it matches exactly that
        batch with this selection, and runs its own otherwise -- the results are the same.  n=0 disarms."""
        if mask is not None:
            mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
            if mask.shape != (n, n):
                raise ValueError("mask must be %d x %d, got shape %r" % (n, n, mask.shape))
        self.ctx.check(self.ctx.lib.mis_orb_arm_knn_ahead(self.h, int(n), None if mask is None else mask.ctypes.data_as(C.c_void_p),
                                                          int(range_width), int(rank), int(world_size)))

    def _run_enqueued(self, _user):
        fn, self._enqueued_fn = getattr(self, "_enqueued_fn", None), None
        if fn is not None:
            fn()

    def detect_batch(self, imgs):
        n = len(imgs)
        arr = _images(imgs)
        raws = (capi.MisFeatures * n)()
        self.ctx.check(self.ctx.lib.mis_orb_detect_batch(self.h, arr, n, raws))
        out = []
        for k in range(n):
            r = capi.MisFeatures()
            C.memmove(C.byref(r), C.byref(raws[k]), C.sizeof(capi.MisFeatures))
            r.img_idx = k
            out.append(ImageFeatures(self.ctx, r))
        return out

    def debug_level(self, level, which):
        w, h = C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.mis_orb_debug_level(self.h, level, which, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        self.ctx.check(self.ctx.lib.mis_orb_debug_level(self.h, level, which, out.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(h)))
        return out

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.mis_orb_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SiftFeatureFinder:
    """SIFT::create() (image_stitching.cpp:559, features_type == "sift"): same detect() interface as the ORB finder;
    descriptors are n x 128 f32 with integer values 0..255 (the L2 matcher's MFMA path, K8, consumes them)."""

    def __init__(self, ctx, max_size, params=None):
        self.ctx = ctx
        p = capi.MisSiftParams()
        ctx.lib.mis_sift_default_params(C.byref(p))
        for k, v in (params or {}).items():
            setattr(p, k, v)
        self.params = p
        h = C.c_void_p()
        ctx.check(ctx.lib.mis_sift_create(ctx.h, C.byref(p), int(max_size[0]), int(max_size[1]), C.byref(h)))
        self.h = h

    def detect(self, img):
        raw = capi.MisFeatures()
        i = as_image(img)
        self.ctx.check(self.ctx.lib.mis_sift_detect(self.h, C.byref(i), C.byref(raw)))
        return ImageFeatures(self.ctx, raw)

    def detect_batch(self, imgs):
        n = len(imgs)
        if n == 0:
            return []
        arr = _images(imgs)
        raws = (capi.MisFeatures * n)()
        self.ctx.check(self.ctx.lib.mis_sift_detect_batch(self.h, arr, n, raws))
        out = []
        for k in range(n):
            raw = capi.MisFeatures()
            C.memmove(C.byref(raw), C.byref(raws[k]), C.sizeof(capi.MisFeatures))
            out.append(ImageFeatures(self.ctx, raw))
        return out

    def debug_level(self, img, octave, layer, dog=False):
        i = as_image(img)
        w, h = C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.mis_sift_debug_level(self.h, C.byref(i), octave, layer, int(dog), None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.float32)
        self.ctx.check(self.ctx.lib.mis_sift_debug_level(self.h, C.byref(i), octave, layer, int(dog), out.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(h)))
        return out

    def debug_counts(self):
        """Counters of the last detect(): dict(candidates, refined, raw, keypoints)."""
        c = (C.c_uint * 4)()
        self.ctx.check(self.ctx.lib.mis_sift_debug_counts(self.h, c))
        return dict(candidates=int(c[0]), raw=int(c[1]), keypoints=int(c[2]), refined=int(c[3]))

    def close(self):
        if getattr(self, "h", None) and self.ctx.h:
            self.ctx.lib.mis_sift_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def computeImageFeatures(finder, img, img_idx=0):
    """cv::detail::computeImageFeatures(finder, img, features) + features.img_idx = i (:613-614)."""
    f = finder.detect(img)
    f.img_idx = img_idx
    return f


# ------------------------------------------------------------------------------------------------
# matching: BestOf2NearestMatcher (image_stitching.cpp:647, :653), myLeaveBiggestComponent (:215-278)
@dataclass
class MatchesInfo:
    src_img_idx: int = -1
    dst_img_idx: int = -1
    matches: np.ndarray = field(default_factory=lambda: np.zeros(0, DMATCH_DTYPE))
    inliers_mask: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint8))
    num_inliers: int = 0
    H: np.ndarray = None
    confidence: float = 0.0


def _unpack_mi(mi):
    n = mi.n_matches
    out = MatchesInfo(mi.src_img_idx, mi.dst_img_idx)
    if n and mi.matches:
        out.matches = np.frombuffer((C.c_char * (n * 16)).from_address(C.addressof(mi.matches.contents)), DMATCH_DTYPE).copy()
    if n and mi.inliers_mask:
        out.inliers_mask = np.frombuffer((C.c_char * n).from_address(C.addressof(mi.inliers_mask.contents)), np.uint8).copy()
    out.num_inliers = mi.num_inliers
    out.H = np.array(list(mi.H), np.float64).reshape(3, 3) if mi.has_H else None
    out.confidence = mi.confidence
    return out


class PairwiseMatches:
    """The n x n cv::detail::MatchesInfo table of one matcher call, kept in the library's C structs and converted to
    MatchesInfo objects only when an entry is read (a job needs the confidences alone; converting 256 entries with their
    match arrays costs more host time than the pruning they feed).  Behaves like a list."""

    def __init__(self, ctx, mis, n):
        self._ctx, self._mis, self.n = ctx, mis, n
        self._cache = {}

    @classmethod
    def from_entries(cls, ctx, n, entries):
        """A table assembled on the host from (i, j, matches, inliers_mask, num_inliers, has_H, H, confidence) records of the
        pairs i < j (a sharded job gathers them from the ranks that matched them); the mirrored entries are filled as
        FeaturesMatcher::operator() fills them.  The arrays live in this object, not in the library."""
        mis = (capi.MisMatchesInfo * (n * n))()
        keep = []
        for k in range(n * n):
            mis[k].src_img_idx = mis[k].dst_img_idx = -1
        for i, j, matches, mask, num_inliers, has_H, H, conf in entries:
            mm = np.ascontiguousarray(matches, DMATCH_DTYPE)
            mk = np.ascontiguousarray(mask, np.uint8)
            sw = mm.copy()
            sw["query_idx"], sw["train_idx"] = mm["train_idx"], mm["query_idx"]
            Hd = np.asarray(H, np.float64).reshape(3, 3) if has_H else None
            for (a, b, arr, Hm) in ((i, j, mm, Hd), (j, i, sw, np.linalg.inv(Hd) if has_H else None)):
                e = mis[a * n + b]
                e.src_img_idx, e.dst_img_idx, e.n_matches = a, b, len(arr)
                e.matches = C.cast(arr.ctypes.data, C.POINTER(capi.MisDMatch)) if len(arr) else None
                e.inliers_mask = C.cast(mk.ctypes.data, C.POINTER(C.c_uint8)) if len(mk) else None
                e.num_inliers, e.has_H, e.confidence = int(num_inliers), 1 if has_H else 0, float(conf)
                if has_H:
                    for q, v in enumerate(Hm.reshape(9)):
                        e.H[q] = v
            keep += [mm, mk, sw]
        obj = cls(ctx, mis, n)
        obj._keep, obj._borrowed = keep, True
        return obj

    def __len__(self):
        return self.n * self.n

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[k] for k in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        if i not in self._cache:
            self._cache[i] = _unpack_mi(self._mis[i])
        return self._cache[i]

    def __iter__(self):
        return (self[i] for i in range(len(self)))

    def confidences(self):
        """-> float64 array (n * n), row-major"""
        return np.array([self._mis[i].confidence for i in range(len(self))], np.float64)

    def __del__(self):
        try:
            if self._mis is not None and self._ctx.h and not getattr(self, "_borrowed", False):
                self._ctx.lib.mis_matches_free(self._mis, self.n * self.n)
            self._mis = None
        except Exception:
            pass


def match_params(**kw):
    p = capi.MisMatchParams()
    capi.load().mis_match_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class BestOf2NearestMatcher:
    """makePtr<BestOf2NearestMatcher>(try_cuda, match_conf) (image_stitching.cpp:647)."""

    def __init__(self, ctx, match_conf=0.32, num_matches_thresh1=6, num_matches_thresh2=6):
        self.ctx = ctx
        self.params = match_params(match_conf=match_conf, num_matches_thresh1=num_matches_thresh1,
                                   num_matches_thresh2=num_matches_thresh2)

    range_width = -1
    model = capi.MATCH_HOMOGRAPHY

    def __call__(self, features, rank=0, world_size=1, mask=None):
        """(*matcher)(features, pairwise_matches, mask) -> list of n*n MatchesInfo (row-major).  mask: n x n, non-zero at (i, j),
        i < j, where the pair is to be matched (only the strict upper triangle is read); unselected entries stay default."""
        n = len(features)
        if mask is not None:
            mask = np.ascontiguousarray(mask)
            if mask.shape != (n, n):
                raise ValueError("mask must be %d x %d, got shape %r" % (n, n, mask.shape))
            mask = np.ascontiguousarray(mask != 0, np.uint8)
        arr = (capi.MisFeatures * n)()
        for k, f in enumerate(features):
            C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
        mis = (capi.MisMatchesInfo * (n * n))()
        if self.model != capi.MATCH_HOMOGRAPHY:
            rc = self.ctx.lib.mis_match_pairs_model(self.ctx.h, arr, n, C.byref(self.params), int(self.model),
                                                    None if mask is None else mask.ctypes.data_as(C.c_void_p), int(self.range_width), rank, world_size, mis)
        elif mask is not None or self.range_width != -1:
            rc = self.ctx.lib.mis_match_pairs_select(self.ctx.h, arr, n, C.byref(self.params), None if mask is None else mask.ctypes.data_as(C.c_void_p),
                                                     int(self.range_width), rank, world_size, mis)
        elif world_size == 1:
            rc = self.ctx.lib.mis_match_all_pairs(self.ctx.h, arr, n, C.byref(self.params), mis)
        else:
            rc = self.ctx.lib.mis_match_pairs_sharded(self.ctx.h, arr, n, C.byref(self.params), rank, world_size, mis)
        self.ctx.check(rc)
        return PairwiseMatches(self.ctx, mis, n)

    def collectGarbage(self):
        pass


class BestOf2NearestRangeMatcher(BestOf2NearestMatcher):
    """makePtr<BestOf2NearestRangeMatcher>(range_width, try_cuda, match_conf) (image_stitching.cpp:649): only the pairs with
    j < i + range_width are matched (2: adjacent frames; 1: none).  The width is checked by the library call (-1 or >= 1)."""

    def __init__(self, ctx, range_width=5, match_conf=0.32, num_matches_thresh1=6, num_matches_thresh2=6):
        super().__init__(ctx, match_conf, num_matches_thresh1, num_matches_thresh2)
        self.range_width = int(range_width)


class AffineBestOf2NearestMatcher(BestOf2NearestMatcher):
    """makePtr<AffineBestOf2NearestMatcher>(false, try_cuda, match_conf) (image_stitching.cpp:645): the 2-NN and ratio test of
    BestOf2NearestMatcher, then cv::estimateAffinePartial2D on the keypoint positions as they are (threshold 3, 2000 iterations,
    confidence 0.99, 10 refinement iterations); confidence = inliers / (8 + 0.3 matches), never zeroed; no second estimation.
    full_affine=True (cv::estimateAffine2D) is not built: the reference hard-codes false."""
    model = capi.MATCH_AFFINE_PARTIAL

    def __init__(self, ctx, full_affine=False, match_conf=0.3, num_matches_thresh1=6):
        if full_affine:
            raise NotImplementedError("AffineBestOf2NearestMatcher(full_affine=True): cv::estimateAffine2D is not built, only the "
                                      "affine-partial model the reference uses (image_stitching.cpp:645; DESIGN.md section 8)")
        self.ctx = ctx
        p = capi.MisMatchParams()
        capi.load().mis_match_affine_default_params(C.byref(p))
        p.match_conf = match_conf
        p.num_matches_thresh1 = num_matches_thresh1
        self.params = p


MATCHER_TYPES = ("homography", "affine")


def check_matcher_config(cfg):
    """matcher_type of the config (image_stitching.cpp:64, :644-649): 'homography' or 'affine', else ValueError by name before any
    device work.  'affine' with a range_width is refused too: the reference silently ignores range_width there (:644 comes first),
    and no option is ignored silently here."""
    mt = getattr(cfg, "matcher_type", "homography")
    if mt not in MATCHER_TYPES:
        raise ValueError("matcher_type %r: 'homography' or 'affine' (image_stitching.cpp:64, :644-649)" % (mt,))
    if mt == "affine" and cfg.range_width != -1:
        raise ValueError("matcher_type 'affine' with range_width %r: AffineBestOf2NearestMatcher matches all pairs "
                         "(image_stitching.cpp:644-645 ignores range_width); set range_width = -1" % (cfg.range_width,))
    return mt


def make_matcher(ctx, cfg):
    """if (matcher_type == "affine") AffineBestOf2NearestMatcher(false, ...) else if (range_width == -1) BestOf2NearestMatcher
    else BestOf2NearestRangeMatcher (image_stitching.cpp:644-649)"""
    if check_matcher_config(cfg) == "affine":
        return AffineBestOf2NearestMatcher(ctx, False, cfg.match_conf)
    if cfg.range_width == -1:
        return BestOf2NearestMatcher(ctx, cfg.match_conf)
    return BestOf2NearestRangeMatcher(ctx, cfg.range_width, cfg.match_conf)


def selected_pairs(counts, range_width=-1, mask=None):
    """The pairs a matcher call selects, in the order it matches and shards them (pair k goes to rank k % world_size): (i, j),
    i < j, both frames with keypoints (counts[i] > 0), mask None or mask[i][j] != 0, range_width -1 or j < i + range_width."""
    n = len(counts)
    return [(i, j) for i in range(n) for j in range(i + 1, n)
            if counts[i] > 0 and counts[j] > 0 and (mask is None or mask[i][j] != 0) and (range_width == -1 or j < i + range_width)]


def leaveBiggestComponent(pairwise_matches, n, conf_threshold):
    """myLeaveBiggestComponent (image_stitching.cpp:215-278) on the matcher output -> kept indices."""
    lib = capi.load()
    mis = (capi.MisMatchesInfo * (n * n))()
    for i, m in enumerate(pairwise_matches):
        mis[i].confidence = m.confidence
    idx = np.zeros(n, np.int32)
    k = C.c_int()
    rc = lib.mis_leave_biggest_component(mis, n, float(conf_threshold), idx.ctypes.data_as(C.c_void_p), C.byref(k))
    if rc != capi.MIS_OK:
        raise MisError(rc, "mis_leave_biggest_component")
    return idx[: k.value].copy()


def leaveBiggestComponentConf(confidence, conf_threshold):
    """myLeaveBiggestComponent on the bare n x n confidence matrix -> kept indices."""
    conf = np.ascontiguousarray(confidence, np.float64)
    n = conf.shape[0]
    idx = np.zeros(n, np.int32)
    k = C.c_int()
    rc = capi.load().mis_leave_biggest_component_conf(conf.ctypes.data_as(C.c_void_p), n, float(conf_threshold), idx.ctypes.data_as(C.c_void_p), C.byref(k))
    if rc != capi.MIS_OK:
        raise MisError(rc, "mis_leave_biggest_component_conf")
    return idx[: k.value].copy()


WAVE_CORRECT_HORIZ, WAVE_CORRECT_VERT = 0, 1


def _subset_matches(ctx, pairwise_matches, indices):
    """The table of the kept subset, re-indexed as leaveBiggestComponent does (image_stitching.cpp:746-748): a view whose entries
    borrow the full table's match arrays.  The caller sets view._mis = None when done (borrowed entries: nothing to free)."""
    n, k = pairwise_matches.n, len(indices)
    sub = (capi.MisMatchesInfo * (k * k))()
    for a, i in enumerate(indices):
        for b, j in enumerate(indices):
            C.memmove(C.byref(sub[a * k + b]), C.byref(pairwise_matches._mis[i * n + j]), C.sizeof(capi.MisMatchesInfo))
            sub[a * k + b].src_img_idx, sub[a * k + b].dst_img_idx = a, b
    view = PairwiseMatches.__new__(PairwiseMatches)
    view._ctx, view._mis, view.n, view._cache = ctx, sub, k, {}
    view._owner = pairwise_matches              # the match arrays belong to the full table
    return view


def estimate_and_refine(ctx, features, pairwise_matches, indices, conf_thresh, estimator, adjuster, wave_correct="no"):
    """The reference's sequence after the pruning for a job without supplied cameras (cv::Stitcher::estimateCameraParams): the
    estimator on the kept subset's table, its rotations handed on as float32, then the bundle adjuster on the subset's features,
    then wave correction of the rotations ("horiz" | "vert"; "no": none, as the scans mode has it).
    estimator(pairwise_matches) -> cameras; adjuster(ctx, features, pairwise_matches, cameras, conf_thresh) -> cameras or None for
    no adjustment.  -> camera dicts with K (3x3 float64) and R (3x3 float32) for the kept frames, in the order of `indices`."""
    view = _subset_matches(ctx, pairwise_matches, indices)
    try:
        cams = estimator(view)
        if adjuster is not None:
            cams = adjuster(ctx, [features[i] for i in indices], view, cams, conf_thresh)
    finally:
        view._mis = None
    if wave_correct != "no":
        cams = _wave_corrected(cams, wave_correct)
    return [dict(K=np.array([[c["focal"], 0, c["ppx"]], [0, c["focal"] * c["aspect"], c["ppy"]], [0, 0, 1]], np.float64),
                 R=np.asarray(c["R"], np.float32), f=c["focal"], params=c) for c in cams]


def refine_cameras(ctx, features, pairwise_matches, indices, cameras, cfg):
    """The reference's sequence after the pruning (image_stitching.cpp:671-726) on the kept subset: bundle adjustment
    of the subset's cameras (features / matches re-indexed as leaveBiggestComponent does), then wave correction.
    cameras: dicts with K (3x3), R; returns new dicts for the kept frames, in the order of `indices`."""
    view = _subset_matches(ctx, pairwise_matches, indices)
    start = [dict(focal=float(cameras[i]["K"][0, 0]), aspect=float(cameras[i]["K"][1, 1] / cameras[i]["K"][0, 0]), ppx=float(cameras[i]["K"][0, 2]),
                  ppy=float(cameras[i]["K"][1, 2]), R=cameras[i]["R"]) for i in indices]
    cost_func = check_ba_config(cfg)
    try:
        if cost_func == "ray":
            refined = bundle_adjust_ray(ctx, [features[i] for i in indices], view, start, cfg.conf_thresh)
        else:
            refined = bundle_adjust_reproj(ctx, [features[i] for i in indices], view, start, cfg.conf_thresh, cfg.ba_refine_mask)
    finally:
        view._mis = None                        # borrowed entries: nothing to free
    if cfg.wave_correct != "no":
        Rs = wave_correct([c["R"] for c in refined], WAVE_CORRECT_VERT if cfg.wave_correct == "vert" else WAVE_CORRECT_HORIZ)
        for c, R in zip(refined, Rs):
            c["R"] = R
    out = []
    for i, c in zip(indices, refined):
        d = dict(cameras[i])
        d["K"] = np.array([[c["focal"], 0, c["ppx"]], [0, c["focal"] * c["aspect"], c["ppy"]], [0, 0, 1]], np.float64)
        d["R"] = c["R"]
        d["f"] = c["focal"]
        out.append(d)
    return out


BA_COST_FUNCS = ("no", "reproj", "ray")


def check_ba_config(cfg):
    """ba_cost_func of the config: one of BA_COST_FUNCS; "affine" (BundleAdjusterAffinePartial, image_stitching.cpp:685) raises
    NotImplementedError by name, any other name ValueError (the reference's "Unknown bundle adjustment cost function", :687-690),
    before any device work."""
    name = cfg.ba_cost_func
    if name in BA_COST_FUNCS:
        return name
    if name == "affine":
        raise NotImplementedError("ba_cost_func 'affine': BundleAdjusterAffinePartial is not built, only %s (DESIGN.md section 8)"
                                  % ", ".join(repr(k) for k in BA_COST_FUNCS))
    raise ValueError("ba_cost_func %r: not a cost function the reference knows (image_stitching.cpp:680-693)" % (name,))


def _camera_array(cameras, n):
    cams = (capi.MisCameraParams * n)()
    for k, c in enumerate(cameras):
        cams[k].focal, cams[k].aspect, cams[k].ppx, cams[k].ppy = float(c["focal"]), float(c.get("aspect", 1.0)), float(c["ppx"]), float(c["ppy"])
        R = np.asarray(c["R"], np.float64).reshape(9)
        t = np.asarray(c.get("t", np.zeros(3)), np.float64).reshape(3)
        for i in range(9):
            cams[k].R[i] = R[i]
        for i in range(3):
            cams[k].t[i] = t[i]
    return cams


def _camera_dicts(cams, n):
    return [dict(focal=cams[k].focal, aspect=cams[k].aspect, ppx=cams[k].ppx, ppy=cams[k].ppy, R=np.array(list(cams[k].R)).reshape(3, 3),
                 t=np.array(list(cams[k].t))) for k in range(n)]


def bundle_adjust_ray(ctx, features, pairwise_matches, cameras, conf_thresh=0.95):
    """(*makePtr<detail::BundleAdjusterRay>())(features, pairwise_matches, cameras) with setConfThresh
    (image_stitching.cpp:683-684): focal and rotation of every camera refined on the rays of the inlier matches, evaluated on the
    device; ppx, ppy, aspect and t come back as given.  cameras and the result as in bundle_adjust_reproj."""
    n = len(features)
    if not isinstance(pairwise_matches, PairwiseMatches):
        raise TypeError("pairwise_matches must be the PairwiseMatches object a BestOf2NearestMatcher call returned")
    arr = (capi.MisFeatures * n)()
    for k, f in enumerate(features):
        C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
    cams = _camera_array(cameras, n)
    ctx.check(ctx.lib.mis_bundle_adjust_ray(ctx.h, arr, pairwise_matches._mis, n, float(conf_thresh), cams))
    return _camera_dicts(cams, n)


def bundle_adjust_affine_partial(ctx, features, pairwise_matches, cameras, conf_thresh=0.95):
    """(*makePtr<detail::BundleAdjusterAffinePartial>())(features, pairwise_matches, cameras) with setConfThresh
    (image_stitching.cpp:685-686; what Stitcher::create(SCANS) installs): the similarity (a, b, tx, ty) in every camera's R
    refined on the inlier matches, evaluated on the device; focal, aspect, ppx, ppy and t come back as given.  cameras and the
    result as in bundle_adjust_reproj, R the 3x3 homogeneous similarity."""
    n = len(features)
    if not isinstance(pairwise_matches, PairwiseMatches):
        raise TypeError("pairwise_matches must be the PairwiseMatches object a matcher call returned")
    arr = (capi.MisFeatures * n)()
    for k, f in enumerate(features):
        C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
    cams = _camera_array(cameras, n)
    ctx.check(ctx.lib.mis_bundle_adjust_affine_partial(ctx.h, arr, pairwise_matches._mis, n, float(conf_thresh), cams))
    return _camera_dicts(cams, n)


def estimate_affine_cameras(pairwise_matches):
    """(*makePtr<detail::AffineBasedEstimator>())(features, pairwise_matches, cameras): default cameras (focal 1, aspect 1,
    ppx = ppy = 0, t = 0) whose R is the product of the pairwise similarities along the maximum spanning tree from its centre, as
    float32 values.  Host logic; it never fails.  -> list of dicts as bundle_adjust_reproj takes them."""
    if not isinstance(pairwise_matches, PairwiseMatches):
        raise TypeError("pairwise_matches must be the PairwiseMatches object a matcher call returned")
    n = pairwise_matches.n
    cams = (capi.MisCameraParams * n)()
    rc = capi.load().mis_estimate_affine_cameras(pairwise_matches._mis, n, cams)
    if rc != capi.MIS_OK:
        raise MisError(rc, "mis_estimate_affine_cameras")
    return _camera_dicts(cams, n)


def focals_from_homography(H):
    """detail::focalsFromHomography(H, f0, f1, f0_ok, f1_ok) (autocalib.cpp): the focal lengths of the source and the destination
    view a homography in centred coordinates implies -> (f0, f1, f0_ok, f1_ok); a focal that is not ok is 0.  Host logic."""
    h = (C.c_double * 9)(*np.asarray(H, np.float64).reshape(9))
    f0, f1, ok0, ok1 = C.c_double(), C.c_double(), C.c_int(), C.c_int()
    rc = capi.load().mis_focals_from_homography(h, C.byref(f0), C.byref(f1), C.byref(ok0), C.byref(ok1))
    if rc != capi.MIS_OK:
        raise MisError(rc, "mis_focals_from_homography")
    return f0.value, f1.value, bool(ok0.value), bool(ok1.value)


def _size_array(img_sizes, n):
    """img_sizes: one (width, height) for every image, or a list of n of them -> MisSize array."""
    sizes = list(img_sizes)
    if len(sizes) == 2 and all(isinstance(v, (int, np.integer)) for v in sizes):
        sizes = [tuple(sizes)] * n
    if len(sizes) != n:
        raise ValueError("img_sizes: %d sizes for %d images" % (len(sizes), n))
    arr = (capi.MisSize * n)()
    for k, (w, h) in enumerate(sizes):
        arr[k].width, arr[k].height = int(w), int(h)
    return arr


def estimate_focal(pairwise_matches, img_sizes):
    """detail::estimateFocal(features, pairwise_matches, focals): the median of sqrt(f0 f1) over the pairs whose homography gives
    both focals, or sum(width + height) / n with fewer than n - 1 such pairs.  img_sizes: the (width, height) the features were
    found on (work scale), one pair for all images or one per image.  Host logic.  -> list of n focals (all equal)."""
    if not isinstance(pairwise_matches, PairwiseMatches):
        raise TypeError("pairwise_matches must be the PairwiseMatches object a matcher call returned")
    n = pairwise_matches.n
    focals = (C.c_double * n)()
    rc = capi.load().mis_estimate_focal(pairwise_matches._mis, n, _size_array(img_sizes, n), focals)
    if rc != capi.MIS_OK:
        raise MisError(rc, "mis_estimate_focal")
    return list(focals)


def estimate_homography_cameras(pairwise_matches, img_sizes):
    """(*makePtr<detail::HomographyBasedEstimator>())(features, pairwise_matches, cameras) (image_stitchin3g.cpp:746-779; what
    Stitcher::create(PANORAMA) runs): default cameras (aspect 1, t = 0) with the focal of estimate_focal, ppx, ppy at the image
    centre, and R the product of K_from^-1 H^-1 K_to along the maximum spanning tree from its centre, as float32 values.
    img_sizes as in estimate_focal.  Host logic; it never fails.  -> list of dicts as bundle_adjust_ray takes them."""
    if not isinstance(pairwise_matches, PairwiseMatches):
        raise TypeError("pairwise_matches must be the PairwiseMatches object a matcher call returned")
    n = pairwise_matches.n
    cams = (capi.MisCameraParams * n)()
    rc = capi.load().mis_estimate_homography_cameras(pairwise_matches._mis, n, _size_array(img_sizes, n), cams)
    if rc != capi.MIS_OK:
        raise MisError(rc, "mis_estimate_homography_cameras")
    return _camera_dicts(cams, n)


def bundle_adjust_reproj(ctx, features, pairwise_matches, cameras, conf_thresh=0.95, refine_mask="xxxxx"):
    """(*makePtr<detail::BundleAdjusterReproj>())(features, pairwise_matches, cameras) with setConfThresh /
    setRefinementMask (image_stitching.cpp:681-712).  cameras: list of dicts with focal, ppx, ppy, R (3x3) and
    optionally aspect, t -> new list of dicts (refined; rotations relative to the spanning tree's centre image)."""
    n = len(features)
    if not isinstance(pairwise_matches, PairwiseMatches):
        raise TypeError("pairwise_matches must be the PairwiseMatches object a BestOf2NearestMatcher call returned")
    arr = (capi.MisFeatures * n)()
    for k, f in enumerate(features):
        C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
    cams = _camera_array(cameras, n)
    ctx.check(ctx.lib.mis_bundle_adjust_reproj(ctx.h, arr, pairwise_matches._mis, n, float(conf_thresh), refine_mask.encode(), cams))
    return _camera_dicts(cams, n)


def wave_correct(rmats, kind=WAVE_CORRECT_HORIZ):
    """detail::waveCorrect(rmats, kind) (image_stitching.cpp:718-726) -> list of corrected 3x3 rotations."""
    a = np.ascontiguousarray(np.stack([np.asarray(r, np.float64).reshape(3, 3) for r in rmats]))
    rc = capi.load().mis_wave_correct(a.ctypes.data_as(C.c_void_p), len(rmats), int(kind))
    if rc != capi.MIS_OK:
        raise MisError(rc, "mis_wave_correct")
    return [a[i].copy() for i in range(len(rmats))]


def _wave_corrected(cams, name):
    """Camera dicts with their rotations wave-corrected; name: "horiz" | "vert" (StitchConfig.wave_correct)."""
    Rs = wave_correct([c["R"] for c in cams], WAVE_CORRECT_VERT if name == "vert" else WAVE_CORRECT_HORIZ)
    return [dict(c, R=R) for c, R in zip(cams, Rs)]


def find_homography(ctx, src, dst, thresh=3.0, max_iters=2000, confidence=0.995):
    """cv::findHomography(src, dst, mask, RANSAC) on the GPU -> (ok, H, mask)."""
    src = np.ascontiguousarray(src, np.float32)
    dst = np.ascontiguousarray(dst, np.float32)
    n = src.shape[0]
    H = np.zeros(9, np.float64)
    mask = np.zeros(max(n, 1), np.uint8)
    ok = C.c_int()
    ctx.check(ctx.lib.mis_find_homography(ctx.h, src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), n, thresh,
                                          max_iters, confidence, H.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p),
                                          C.byref(ok)))
    return bool(ok.value), H.reshape(3, 3), mask[:n]


def estimate_affine_partial(ctx, src, dst, thresh=3.0, max_iters=2000, confidence=0.99, refine_iters=10):
    """cv::estimateAffinePartial2D(src, dst, mask, RANSAC, ...) on the GPU -> (ok, M 2 x 3 = [a -b tx; b a ty], mask)."""
    src = np.ascontiguousarray(src, np.float32).reshape(-1, 2)
    dst = np.ascontiguousarray(dst, np.float32).reshape(-1, 2)
    n = src.shape[0]
    if dst.shape[0] != n:
        raise ValueError("src and dst must hold the same number of points")
    M = np.zeros(6, np.float64)
    mask = np.zeros(max(n, 1), np.uint8)
    ok = C.c_int()
    ctx.check(ctx.lib.mis_estimate_affine_partial(ctx.h, src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p), n, thresh, max_iters,
                                                  confidence, refine_iters, M.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(C.c_void_p), C.byref(ok)))
    return bool(ok.value), M.reshape(2, 3), mask[:n]


# ------------------------------------------------------------------------------------------------
def check_warp_config(cfg):
    """warp_type of the config -> MIS_WARP_* kind, or NotImplementedError / ValueError by name before any device work."""
    return warp_kind(cfg.warp_type)


def check_range_config(cfg):
    """range_width of the config: -1 (all pairs) or a width >= 1, else ValueError before any device work."""
    rw = cfg.range_width
    if isinstance(rw, bool) or not isinstance(rw, (int, np.integer)) or not (rw == -1 or rw >= 1):
        raise ValueError("range_width %r: -1 (match all pairs) or an integer >= 1 (image_stitching.cpp:83, :646-649)" % (rw,))
    return int(rw)


# seam_find_type (image_stitching.cpp:77, :1029-1062) as a configuration name
SEAM_FIND_TYPES = ("no", "voronoi", "dp_color", "dp_colorgrad")


def check_seam_config(cfg):
    if cfg.seam_find_type not in SEAM_FIND_TYPES:
        raise NotImplementedError("seam_find_type %r: 'no', 'voronoi', 'dp_color' and 'dp_colorgrad' are implemented as configuration names "
                                  "(gc_color / gc_colorgrad are not names here: the graph-cut finder is the class GraphCutSeamFinder, handed to "
                                  "Stitcher.set_seam_finder; DESIGN.md section 8)" % (cfg.seam_find_type,))
    if cfg.expos_comp_type not in EXPOS_COMP_TYPES:
        raise NotImplementedError("expos_comp_type %r: one of %s ('channels' is ChannelsCompensator, not a configuration name here)"
                                  % (cfg.expos_comp_type, ", ".join(EXPOS_COMP_TYPES)))
    nf = cfg.expos_comp_nr_feeds
    if isinstance(nf, bool) or not isinstance(nf, (int, np.integer)) or nf < 1:
        raise ValueError("expos_comp_nr_feeds %r: an integer >= 1 (image_stitching.cpp:74)" % (nf,))


def seam_scale_warp(ctx, cfg, frame_size, frame, camera, warped_image_scale, work_scale=1.0, kind=None):
    """One frame of the seam-scale loop of main() (image_stitching.cpp:604-622 resize to seam_megapix, :973-990 warp of image and
    mask with K scaled by seam_work_aspect) -> (corner, image_warped 8UC3, mask_warped 8U) on the device."""
    w, h = frame_size
    seam_scale = min(1.0, float(np.sqrt(cfg.seam_megapix * 1e6 / (w * h))))
    swa = np.float32(seam_scale / work_scale)
    # kind: the warper kind set in place of the configured warp_type (Stitcher.set_warper)
    sscale = np.float32(np.float32(warped_image_scale) * swa)
    warper = make_warper(ctx, sscale, cfg.warp_type) if kind is None else RotationWarper(ctx, sscale, kind)
    img = resize(ctx, frame, fx=seam_scale, fy=seam_scale) if seam_scale < 1.0 else frame
    K = np.array(camera["K"], np.float32).copy()
    K[0, 0] *= swa; K[0, 2] *= swa; K[1, 1] *= swa; K[1, 2] *= swa
    R = np.asarray(camera["R"], np.float32)
    tl, iw = warper.warp(img, K, R, capi.INTER_LINEAR, capi.BORDER_REFLECT)
    full = torch.full((img.shape[0], img.shape[1]), 255, dtype=torch.uint8, device=ctx.device)
    _, mw = warper.warp(full, K, R, capi.INTER_NEAREST, capi.BORDER_CONSTANT)
    return tl, iw, mw


def seam_solve(ctx, cfg, corners, images_warped, masks_warped, seam_finder=None):
    """The part of the seam-scale pass that needs every image (image_stitching.cpp:1002-1023 exposure compensator feed, :1029-1065
    seam finder) -> (compensator | None, masks_warped edited in place).  seam_finder: a finder object (anything with
    find(images, corners, masks)) that runs in place of the configured one, as cv::Stitcher::setSeamFinder's does."""
    compensator = make_compensator(ctx, cfg)
    if compensator is not None:
        compensator.feed(corners, images_warped, masks_warped)
    if seam_finder is None:
        seam_finder = make_seam_finder(ctx, cfg)
    if seam_finder is not None:
        seam_finder.find(images_warped, corners, masks_warped)
    return compensator, masks_warped


@dataclass
class ComposeGeometry:
    compose_scale: float      # min(1, sqrt(compose_megapix * 1e6 / area)); 1 when compose_megapix <= 0
    aspect: float             # compose_work_aspect = compose_scale / work_scale
    warp_scale: float         # warped_image_scale * (float)compose_work_aspect
    size: tuple               # frame size inside the compositing loop


def work_geometry(cfg, frame_size):
    """The work scale of main() (image_stitching.cpp:589-603) -> (work_scale, (work_w, work_h)): 1 and the frame as it is when
    work_megapix < 0, otherwise min(1, sqrt(work_megapix * 1e6 / area)) and the size cv::resize gives for that factor (cvRound);
    there is no |scale - 1| > 0.1 test here, unlike the compose loop.  A scale of exactly 1 is the identity."""
    w, h = int(frame_size[0]), int(frame_size[1])
    if cfg.work_megapix < 0:
        return 1.0, (w, h)
    ws = min(1.0, float(np.sqrt(cfg.work_megapix * 1e6 / (w * h))))
    if ws == 1.0:
        return 1.0, (w, h)
    return ws, (int(round(w * ws)), int(round(h * ws)))      # cvRound: half to even, as Python's round


def compose_geometry(cfg, frame_size, warped_image_scale, work_scale=1.0):
    """The scales of the compositing loop (image_stitching.cpp:1105-1146): compose_scale from compose_megapix, the warper's scale
    and the intrinsics multiplied by compose_work_aspect = compose_scale / work_scale, and -- only when |compose_scale - 1| > 0.1,
    as the reference tests it -- frames and their sizes resized (cvRound).  warped_image_scale and the cameras it is applied to are
    in work units (:635-637)."""
    w, h = frame_size
    cs = 1.0
    if cfg.compose_megapix > 0:
        cs = min(1.0, float(np.sqrt(cfg.compose_megapix * 1e6 / (w * h))))
    aspect = cs / work_scale
    warp_scale = float(np.float32(warped_image_scale) * np.float32(aspect))
    size = (int(round(w * cs)), int(round(h * cs))) if abs(cs - 1) > 1e-1 else (int(w), int(h))      # cvRound: half to even, as Python's round
    return ComposeGeometry(cs, aspect, warp_scale, size)


def scaled_camera(cam, aspect):
    """cameras[i].focal *= a; ppx *= a; ppy *= a (image_stitching.cpp:635-637 with the work scale, :1122-1125 with
    compose_work_aspect), in double like CameraParams; K() = [f 0 ppx; 0 f*aspect ppy]"""
    K = np.array(cam["K"], np.float64)
    f = K[0, 0] * aspect
    K2 = K.copy()
    K2[0, 0] = f
    K2[1, 1] = f * (K[1, 1] / K[0, 0])
    K2[0, 2] = K[0, 2] * aspect
    K2[1, 2] = K[1, 2] * aspect
    d = dict(cam)
    d["K"] = K2
    d["f"] = f
    return d


@dataclass
class StitchConfig:
    """The reference's globals-as-config (image_stitching.cpp:49-85), same defaults; compose_megapix
    <= 0 keeps frames at full resolution through warp + blend (the throughput configuration).  work_megapix >= 0: features,
    matching and bundle adjustment at work scale (:589-603); the cameras a caller passes are always in full-resolution pixels."""
    work_megapix: float = -1
    seam_megapix: float = 0.1
    compose_megapix: float = 0.4
    conf_thresh: float = 0.95
    features_type: str = "orb"
    match_conf: float = 0.32
    range_width: int = -1             # -1: all pairs; w >= 1: BestOf2NearestRangeMatcher, pairs with j < i + w only (:83, :646-649)
    matcher_type: str = "homography"  # "homography" | "affine": AffineBestOf2NearestMatcher(false, ...), all pairs (:64, :644-645)
    warp_type: str = "spherical"      # "spherical" | "cylindrical" | "plane" | "mercator" | "fisheye" | "stereographic" | "compressedPlaneA2B1" | "compressedPlaneA1.5B1" | "paniniA1.5B1" (:917-969; the other names raise by name, warp_kind)
    blend_type: int = capi.BLEND_MULTI_BAND
    blend_strength: float = 5.0
    # camera refinement between matching and warping (image_stitching.cpp:681-726).  The reference's default is
    # "reproj"; here the default is "no" because the jobs of this package take exact (sensor / ground-truth) cameras.
    ba_cost_func: str = "no"          # "no" | "reproj" | "ray" (BundleAdjusterRay, :683-684: focal + rotation, evaluated on the device; "affine" raises by name, check_ba_config)
    ba_refine_mask: str = "_____"     # the reference's default (image_stitching.cpp:67): rotations only; read by "reproj" alone
    wave_correct: str = "horiz"       # "horiz" | "vert" | "no"; applied after the bundle adjustment only
    # the seam-scale step between warp and blend (image_stitching.cpp:940-1070, :1162-1171), the reference's defaults
    # (:73-77): block gain compensation and the dynamic-programming colour seam finder
    expos_comp_type: str = "gain_blocks"   # "no" | "gain" | "gain_blocks" | "channels_blocks" (:73; "channels": EXPOS_COMP_TYPES)
    expos_comp_nr_feeds: int = 1           # :74
    expos_comp_block_size: int = 64
    expos_comp_nr_filtering: int = 2
    seam_find_type: str = "dp_color"       # "no" | "voronoi" | "dp_color" | "dp_colorgrad" (SEAM_FIND_TYPES)

    def __post_init__(self):
        check_ba_config(self)

    @classmethod
    def reference(cls, **kw):
        """What the reference's main() runs with its globals untouched (image_stitching.cpp:49-85): reprojection bundle adjustment +
        horizontal wave correction, block gain compensation, dp_color seams, seam_megapix 0.1, compose_megapix 0.4."""
        kw.setdefault("ba_cost_func", "reproj")
        return cls(**kw)

    @classmethod
    def hot_path(cls, **kw):
        """The configuration of the north-star hot path (features -> match -> warp -> blend): no exposure compensation and no
        seam finder (the steps between warp and blend); everything else as given."""
        kw.setdefault("expos_comp_type", "no")
        kw.setdefault("seam_find_type", "no")
        kw.setdefault("compose_megapix", -1)      # true-resolution warp + blend: the throughput configuration
        return cls(**kw)


class Stitcher:
    """The hot-path sequence of main() (image_stitching.cpp:567-1228) for frames already in HBM:
    features -> pairwise matches (+RANSAC) -> [cameras supplied by the caller] -> compose-scale
    warp -> blend.  Optional (off by default): reprojection bundle adjustment with wave
    correction (refine_cameras), block gain compensation and the "voronoi" seam finder (seam_step).  Without cameras:
    create_panorama (HomographyBasedEstimator + BundleAdjusterRay + wave correction) and create_scans; estimate_transform registers
    once, compose_panorama composes further frame sets from the kept registration."""

    def __init__(self, ctx, frame_size, config=None):
        self.ctx = ctx
        self.cfg = config or StitchConfig()
        self.kind = check_warp_config(self.cfg)
        check_range_config(self.cfg)
        check_matcher_config(self.cfg)
        self.frame_size = frame_size
        # features come from the work image (image_stitching.cpp:602, :613): the finder is sized for it
        self.work_scale, self.work_size = work_geometry(self.cfg, frame_size)
        self.finder = OrbFeatureFinder(ctx, self.work_size)
        self.matcher = make_matcher(ctx, self.cfg)
        self.seam_finder = None       # set_seam_finder
        self.estimator = None         # set_estimator: None = the caller supplies the cameras
        self.bundle_adjuster = None   # set_bundle_adjuster (read with an estimator only)
        self.cameras = self.indices = None      # the registration estimate_transform keeps for compose_panorama

    @classmethod
    def create_scans(cls, ctx, frame_size, **config_overrides):
        """cv::Stitcher::create(Stitcher::SCANS): flat material under similarities -- the affine matcher, AffineBasedEstimator,
        BundleAdjusterAffinePartial, AffineWarper, no wave correction, no exposure compensation; the seam finder and the blender
        are the configured ones (StitchConfig.hot_path's unless overridden).  stitch(frames) needs no cameras."""
        kw = dict(matcher_type="affine", wave_correct="no", expos_comp_type="no")
        kw.update(config_overrides)
        st = cls(ctx, frame_size, StitchConfig.hot_path(**kw))
        st.set_estimator(estimate_affine_cameras)
        st.set_bundle_adjuster(bundle_adjust_affine_partial)
        st.set_warper(AffineWarper)
        return st

    @classmethod
    def create_panorama(cls, ctx, frame_size, **config_overrides):
        """cv::Stitcher::create(Stitcher::PANORAMA): a rotating camera from the images alone -- the homography matcher,
        HomographyBasedEstimator on the work-scale image size, BundleAdjusterRay, wave correction (horizontal unless overridden);
        the warper (spherical by default), compensator, seam finder and blender are the configured ones (StitchConfig.hot_path's
        unless overridden).  stitch(frames) needs no cameras."""
        kw = dict(matcher_type="homography", wave_correct="horiz")
        kw.update(config_overrides)
        st = cls(ctx, frame_size, StitchConfig.hot_path(**kw))
        st.set_estimator(functools.partial(estimate_homography_cameras, img_sizes=st.work_size))
        st.set_bundle_adjuster(bundle_adjust_ray)
        return st

    def set_estimator(self, estimator):
        """cv::Stitcher::setEstimator: estimator(pairwise_matches) -> cameras (estimate_affine_cameras), run by stitch() on the kept
        subset in place of cameras from the caller; None goes back to supplied cameras."""
        if estimator is not None and not callable(estimator):
            raise TypeError("set_estimator: %r is not callable" % (estimator,))
        self.estimator = estimator

    def set_bundle_adjuster(self, adjuster):
        """cv::Stitcher::setBundleAdjuster: adjuster(ctx, features, pairwise_matches, cameras, conf_thresh) -> cameras
        (bundle_adjust_affine_partial), run on the estimator's cameras; None: the estimate is used as it is."""
        if adjuster is not None and not callable(adjuster):
            raise TypeError("set_bundle_adjuster: %r is not callable" % (adjuster,))
        self.bundle_adjuster = adjuster

    def set_warper(self, warper_cls):
        """cv::Stitcher::setWarper: a RotationWarper class with a kind of its own (AffineWarper) replaces the configured warp_type in
        the seam-scale and the compose-scale warps; None goes back to warp_type."""
        if warper_cls is None:
            self.kind = check_warp_config(self.cfg)
            return
        kind = getattr(warper_cls, "kind", None)
        if not (isinstance(warper_cls, type) and issubclass(warper_cls, RotationWarper)) or kind not in BUILT_WARP_KINDS:
            raise TypeError("set_warper: %r is not a RotationWarper class with a built kind" % (warper_cls,))
        self.kind = kind

    def set_seam_finder(self, finder):
        """cv::Stitcher::setSeamFinder: the seam step runs this finder object (e.g. GraphCutSeamFinder(ctx)) whatever
        seam_find_type says, "no" included; None goes back to the configured finder."""
        if finder is not None and (isinstance(finder, (str, bytes)) or not callable(getattr(finder, "find", None))):
            raise TypeError("set_seam_finder: %r has no find(images, corners, masks)" % (finder,))
        self.seam_finder = finder

    def work_cameras(self, cameras):
        """The caller's full-resolution cameras in work units (cam.focal, ppx, ppy *= work_scale, image_stitching.cpp:635-637);
        list or dict, as given."""
        if self.work_scale == 1.0:
            return cameras
        if isinstance(cameras, dict):
            return {i: scaled_camera(c, self.work_scale) for i, c in cameras.items()}
        return [scaled_camera(c, self.work_scale) for c in cameras]

    def features(self, frames):
        if self.work_scale < 1.0:
            frames = resize_batch(self.ctx, frames, self.work_scale, self.work_scale)
        return self.finder.detect_batch(frames)

    def match(self, feats, rank=0, world_size=1):
        return self.matcher(feats, rank, world_size)

    @staticmethod
    def warped_image_scale(cameras):
        """median focal (image_stitching.cpp:884-895)"""
        focals = sorted(float(c["K"][1][1]) for c in cameras)
        n = len(focals)
        if n % 2 == 1:
            return float(np.float32(focals[n // 2]))
        return float(np.float32(focals[n // 2 - 1] + focals[n // 2]) * np.float32(0.5))

    def compose(self, frames, cameras, indices=None, blender=None):
        """Compositing loop (image_stitching.cpp:1086-1225), frames and intrinsics at compose scale (compose_megapix).  `cameras`
        are in work units (work_cameras of the caller's, or what refine_cameras returned)."""
        indices = list(range(len(frames)) if indices is None else indices)
        # the reference replaces `cameras` by the kept subset (image_stitching.cpp:746-748) before the median focal (:884-895)
        scale = self.warped_image_scale([cameras[i] for i in indices])
        g = compose_geometry(self.cfg, self.frame_size, scale, self.work_scale)
        seam = self.seam_step(frames, cameras, indices, scale, self.work_scale)      # at seam scale, with the work-unit intrinsics (:973-1065)
        if g.aspect != 1.0:
            cameras = {i: scaled_camera(cameras[i], g.aspect) for i in indices}
        if g.size != tuple(self.frame_size):
            frames = {i: resize(self.ctx, frames[i], fx=g.compose_scale, fy=g.compose_scale) for i in indices}
        scale = g.warp_scale
        warper = RotationWarper(self.ctx, scale, self.kind)
        w, h = g.size
        rois = warp_rois(self.ctx, scale, (w, h), [cameras[i] for i in indices], self.kind)
        corners = [(r[0], r[1]) for r in rois]
        sizes = [(r[2], r[3]) for r in rois]
        x, y, pw, ph = result_roi(corners, sizes)
        # where the panorama lies in the warper's plane: what render_view needs to go back from it
        self.composition = {"pano_tl": (x, y), "warp_scale": scale, "kind": self.kind}
        if blender is None:
            btype, bands, sharp = blend_config(self.cfg.blend_type, self.cfg.blend_strength, (pw, ph))
            if btype == capi.BLEND_MULTI_BAND:
                blender = MultiBandBlender(self.ctx, bands)
            elif btype == capi.BLEND_FEATHER:
                blender = FeatherBlender(self.ctx, sharp)
            else:
                blender = Blender(self.ctx)
        blender.prepare(corners, sizes)
        for k, i in enumerate(indices):
            tl, img_s, mask = warper.warp_fused(frames[i], cameras[i]["K"], cameras[i]["R"], rois[k])
            if seam is not None:
                compensator, seam_masks = seam
                if compensator is not None:
                    compensator.apply(k, corners[k], img_s, mask)       # :1162 (on the 16S copy: same values)
                seam_mask_apply(self.ctx, seam_masks[k], mask)           # :1169-1171
            blender.feed(img_s, mask, tl)
        return blender.blend()

    def render_view(self, pano_u8, K, R, size, interp=capi.INTER_LINEAR, border=capi.BORDER_CONSTANT, with_mask=False):
        """A pinhole view (K, R; size = (w, h)) rendered out of the last composition's panorama, given as 8UC3 (the caller converts
        the blender's 16SC3 result, as for imwrite): RotationWarper.warp_backward with the panorama's corner, the compose scale and
        the warper kind that compose() recorded."""
        c = getattr(self, "composition", None)
        if c is None:
            raise RuntimeError("render_view: compose() has not run on this stitcher")
        return RotationWarper(self.ctx, c["warp_scale"], c["kind"]).warp_backward(pano_u8, c["pano_tl"], K, R, size, interp, border, with_mask)

    def seam_step(self, frames, cameras, indices, warped_image_scale, work_scale=None):
        """The seam-scale pass of main() (image_stitching.cpp:604-622 resize, :973-990 warp, :1002-1023 exposure
        compensator feed, :1029-1065 seam finder) -> (compensator | None, masks_warped) or None when both are off."""
        check_seam_config(self.cfg)
        if self.cfg.expos_comp_type == "no" and self.cfg.seam_find_type == "no" and self.seam_finder is None:
            return None
        work_scale = self.work_scale if work_scale is None else work_scale
        items = [seam_scale_warp(self.ctx, self.cfg, self.frame_size, frames[i], cameras[i], warped_image_scale, work_scale,
                                 self.kind if self.kind != check_warp_config(self.cfg) else None) for i in indices]
        return seam_solve(self.ctx, self.cfg, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items], self.seam_finder)

    def estimate_cameras(self, feats, pm, idx):
        """With an estimator set: the cameras of the kept frames from the matches alone (estimate_and_refine: estimator, bundle
        adjuster, the configured wave correction), in work units -> {frame index: camera}; also kept as self.cameras."""
        if len(idx) < 2:
            raise ValueError("Need more images: %d of the frames are left after the pruning at conf_thresh %g, cameras are estimated from two or more"
                             % (len(idx), self.cfg.conf_thresh))
        cams = estimate_and_refine(self.ctx, feats, pm, [int(i) for i in idx], self.cfg.conf_thresh, self.estimator, self.bundle_adjuster,
                                   self.cfg.wave_correct)
        self.cameras = {int(i): c for i, c in zip(idx, cams)}
        return self.cameras

    def estimate_transform(self, frames, cameras=None):
        """cv::Stitcher::estimateTransform: features, matches, pruning and -- with an estimator set -- estimation, adjustment and
        wave correction; without one the caller's cameras in work units.  The registration is kept for compose_panorama as
        self.cameras (work units: {frame index: camera} from an estimator, else the caller's list or dict as given) and self.indices.
        An earlier registration is dropped first, so a call that raises leaves none.  -> (features, pairwise matches, kept indices)."""
        self.cameras = self.indices = None
        feats = self.features(frames)
        pm = self.match(feats)
        idx = leaveBiggestComponent(pm, len(frames), self.cfg.conf_thresh)
        if self.estimator is not None:
            if cameras is not None:
                raise ValueError("stitch: an estimator is set, the cameras come from the matches")
            self.estimate_cameras(feats, pm, idx)
        elif cameras is None:
            raise ValueError("stitch: cameras are needed (no estimator is set)")
        else:
            self.cameras = self.work_cameras(cameras)
        self.indices = [int(i) for i in idx]
        return feats, pm, idx

    def compose_panorama(self, frames):
        """cv::Stitcher::composePanorama: frames of the registered rig (as many, of the same size, in the same order as the ones
        estimate_transform saw) composed with the kept cameras and indices; no finder or matcher call.  -> (pano, mask)."""
        if self.indices is None:
            raise ValueError("compose_panorama: estimate_transform has not run")
        return self.compose(frames, self.cameras, list(self.indices))

    def stitch(self, frames, cameras=None):
        feats, pm, idx = self.estimate_transform(frames, cameras)
        result, mask = self.compose_panorama(frames)
        return result, mask, feats, pm, idx
