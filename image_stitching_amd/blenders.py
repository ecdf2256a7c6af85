"""blend: cv::detail::Blender / MultiBandBlender / FeatherBlender (image_stitching.cpp:1173-1225)."""
import ctypes as C

import numpy as np

from . import _capi as capi
from .core import Handle, MisError, _empty_image, _images, _memcpy_dtoh, _points, as_image, check_rc, torch


def result_roi(corners, sizes):
    lib = capi.load()
    n = len(corners)
    cs = _points(corners)
    ss = (capi.MisSize * n)(*[capi.MisSize(int(s[0]), int(s[1])) for s in sizes])
    r = capi.MisRect()
    check_rc(lib.mis_result_roi(cs, ss, n, C.byref(r)), "mis_result_roi: invalid arguments")
    return r.x, r.y, r.width, r.height


def blend_config(blend_type, blend_strength, pano_size):
    """image_stitching.cpp:1176-1190 -> (type, num_bands, sharpness)."""
    lib = capi.load()
    t, nb, sh = C.c_int(), C.c_int(), C.c_float()
    lib.mis_blend_config(int(blend_type), float(blend_strength), int(pano_size[0]), int(pano_size[1]), C.byref(t),
                         C.byref(nb), C.byref(sh))
    return t.value, nb.value, sh.value


class Blender(Handle):
    """Blender::createDefault(type) (image_stitching.cpp:1175)."""
    DESTROY = "mis_blender_destroy"

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


def make_blender(ctx, blend_type, blend_strength, pano_size, reuse=None):
    """The blender main() builds for a panorama size (image_stitching.cpp:1175-1190) -> (blender, type, num_bands, sharpness).
    reuse: what an earlier call returned; it is returned again when type, band count and sharpness -- the creation parameters --
    come out the same."""
    btype, bands, sharp = key = blend_config(blend_type, blend_strength, pano_size)
    if reuse is not None and reuse[1:] == key:
        return reuse
    if btype == capi.BLEND_MULTI_BAND:
        blender = MultiBandBlender(ctx, bands)
    elif btype == capi.BLEND_FEATHER:
        blender = FeatherBlender(ctx, sharp)
    else:
        blender = Blender(ctx)
    return (blender,) + key
