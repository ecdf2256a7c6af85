"""warp: cv::detail::{Spherical,Cylindrical,Plane,Mercator,Fisheye,Stereographic,CompressedRectilinear,Panini}Warper, chosen by
warp_type (image_stitching.cpp:917-969; :973, :985, :988, :1117, :1138, :1154, :1159)."""
import ctypes as C

import numpy as np

from . import _capi as capi
from .core import MisError, _c_array, _empty_image, _images, _mat9, as_image, check_rc, torch

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
    check_rc(lib.mis_warper_roi(int(kind), float(scale), int(src_size[0]), int(src_size[1]), kp, rp, C.byref(r)),
             "mis_warper_roi: invalid arguments or a refused roi (kind %d)" % kind)
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


def check_warp_config(cfg):
    """warp_type of the config -> MIS_WARP_* kind, or NotImplementedError / ValueError by name before any device work."""
    return warp_kind(cfg.warp_type)
