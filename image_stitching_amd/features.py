"""features: ORB::create / AKAZE::create / SIFT::create + computeImageFeatures (image_stitching.cpp:545, :547-550, :559, :613)."""
import ctypes as C

import numpy as np

from . import _capi as capi
from .core import _NP_DT, Handle, _images, as_image

KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"), ("octave", "i4")])


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


def features_array(feats):
    """The MisFeatures array of ImageFeatures objects (struct copies: the device arrays stay the objects')."""
    arr = (capi.MisFeatures * len(feats))()
    for k, f in enumerate(feats):
        C.memmove(C.byref(arr[k]), C.byref(f.raw), C.sizeof(capi.MisFeatures))
    return arr


def orb_params(**kw):
    p = capi.MisOrbParams()
    capi.load().mis_orb_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


class OrbFeatureFinder(Handle):
    """ORB::create(4000, 1.2, 8, 1, 0, 2, HARRIS_SCORE, 40, 20) (image_stitching.cpp:545)."""
    DESTROY = "mis_orb_destroy"

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


class SiftFeatureFinder(Handle):
    """SIFT::create() (image_stitching.cpp:559, features_type == "sift"): same detect() interface as the ORB finder;
    descriptors are n x 128 f32 with integer values 0..255 (the L2 matcher's MFMA path, K8, consumes them)."""
    DESTROY = "mis_sift_destroy"

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


class AkazeFeatureFinder(Handle):
    """AKAZE::create() (image_stitching.cpp:547-550, features_type == "akaze"): same detect() interface as the other finders;
    descriptors are n x 61 u8 (MLDB, 486 bits; the wide Hamming 2-NN consumes them), keypoints in (level, y, x) order.  params: a
    dict of MisAkazeParams fields (threshold, n_octaves, n_octave_layers, max_points, ...)."""
    DESTROY = "mis_akaze_destroy"
    PLANES = dict(Lt=0, Lsmooth=1, flow=2, Lx=3, Ly=4, Ldet=5)

    def __init__(self, ctx, max_size, params=None):
        self.ctx = ctx
        p = capi.MisAkazeParams()
        ctx.lib.mis_akaze_default_params(C.byref(p))
        for k, v in (params or {}).items():
            setattr(p, k, v)
        self.params = p
        h = C.c_void_p()
        ctx.check(ctx.lib.mis_akaze_create(ctx.h, C.byref(p), int(max_size[0]), int(max_size[1]), C.byref(h)))
        self.h = h

    def detect(self, img):
        raw = capi.MisFeatures()
        i = as_image(img)
        self.ctx.check(self.ctx.lib.mis_akaze_detect(self.h, C.byref(i), C.byref(raw)))
        return ImageFeatures(self.ctx, raw)

    def detect_batch(self, imgs):
        n = len(imgs)
        if n == 0:
            return []
        arr = _images(imgs)
        raws = (capi.MisFeatures * n)()
        self.ctx.check(self.ctx.lib.mis_akaze_detect_batch(self.h, arr, n, raws))
        out = []
        for k in range(n):
            raw = capi.MisFeatures()
            C.memmove(C.byref(raw), C.byref(raws[k]), C.sizeof(capi.MisFeatures))
            out.append(ImageFeatures(self.ctx, raw))
        return out

    def debug_level(self, level, which):
        """Plane `which` ("Lt", "Lsmooth", "flow", "Lx", "Ly", "Ldet") of a level of the last detect, (h, w) f32."""
        k = self.PLANES[which] if isinstance(which, str) else int(which)
        w, h = C.c_int(), C.c_int()
        self.ctx.check(self.ctx.lib.mis_akaze_debug_level(self.h, int(level), k, None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.float32)
        self.ctx.check(self.ctx.lib.mis_akaze_debug_level(self.h, int(level), k, out.ctypes.data_as(C.c_void_p), C.byref(w), C.byref(h)))
        return out

    def debug_counts(self):
        """Counters of the last detect(): dict(candidates, suppressed, refined, kcontrast)."""
        c = (C.c_uint * 4)()
        self.ctx.check(self.ctx.lib.mis_akaze_debug_counts(self.h, c))
        return dict(candidates=int(c[0]), suppressed=int(c[1]), refined=int(c[2]), kcontrast=float(np.array([c[3]], np.uint32).view(np.float32)[0]))

    def debug_class_ids(self, n):
        """The levels (cv::KeyPoint::class_id) of the last detect's n keypoints."""
        out = np.zeros(max(int(n), 1), np.int32)
        self.ctx.check(self.ctx.lib.mis_akaze_debug_class_ids(self.h, out.ctypes.data_as(C.POINTER(C.c_int)), len(out)))
        return out[:n]

    def debug_fed(self, level):
        """The reordered FED steps into a level (empty for level 0), f32."""
        n = C.c_int()
        self.ctx.check(self.ctx.lib.mis_akaze_debug_fed(self.h, int(level), None, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.float32)
        self.ctx.check(self.ctx.lib.mis_akaze_debug_fed(self.h, int(level), out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)))
        return out[:n.value]


def computeImageFeatures(finder, img, img_idx=0):
    """cv::detail::computeImageFeatures(finder, img, features) + features.img_idx = i (:613-614)."""
    f = finder.detect(img)
    f.img_idx = img_idx
    return f
