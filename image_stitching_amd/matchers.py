"""matching: BestOf2NearestMatcher and its kin (image_stitching.cpp:644-653), myLeaveBiggestComponent (:215-278), the RANSAC models."""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _capi as capi
from .core import check_rc
from .features import features_array

DMATCH_DTYPE = np.dtype([("query_idx", "i4"), ("train_idx", "i4"), ("img_idx", "i4"), ("distance", "f4")])


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

    def __init__(self, ctx, mis, n, keep=None):
        self._ctx, self._mis, self.n = ctx, mis, n
        self._cache = {}
        # keep: what the entries' match arrays live in where that is not the library -- from_entries' host arrays, subset's parent
        # table -- held as long as this table; such a table is borrowed and frees nothing
        self._keep, self._borrowed = keep, keep is not None

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
        return cls(ctx, mis, n, keep)

    def subset(self, indices):
        """The table of the frames `indices`, re-indexed as leaveBiggestComponent does (image_stitching.cpp:746-748).  Its entries
        borrow this table's match arrays: the view keeps this table alive and frees nothing."""
        n, k = self.n, len(indices)
        sub = (capi.MisMatchesInfo * (k * k))()
        for a, i in enumerate(indices):
            for b, j in enumerate(indices):
                C.memmove(C.byref(sub[a * k + b]), C.byref(self._mis[i * n + j]), C.sizeof(capi.MisMatchesInfo))
                sub[a * k + b].src_img_idx, sub[a * k + b].dst_img_idx = a, b
        return PairwiseMatches(self._ctx, sub, k, keep=self)

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
            if self._mis is not None and not self._borrowed and self._ctx.h:
                self._ctx.lib.mis_matches_free(self._mis, self.n * self.n)
            self._mis = None
        except Exception:
            pass


def _require_matches(pairwise_matches):
    if not isinstance(pairwise_matches, PairwiseMatches):
        raise TypeError("pairwise_matches must be the PairwiseMatches object a matcher call returned")


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
        arr = features_array(features)
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


def check_range_config(cfg):
    """range_width of the config: -1 (all pairs) or a width >= 1, else ValueError before any device work."""
    rw = cfg.range_width
    if isinstance(rw, bool) or not isinstance(rw, (int, np.integer)) or not (rw == -1 or rw >= 1):
        raise ValueError("range_width %r: -1 (match all pairs) or an integer >= 1 (image_stitching.cpp:83, :646-649)" % (rw,))
    return int(rw)


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
    check_rc(lib.mis_leave_biggest_component(mis, n, float(conf_threshold), idx.ctypes.data_as(C.c_void_p), C.byref(k)), "mis_leave_biggest_component")
    return idx[: k.value].copy()


def leaveBiggestComponentConf(confidence, conf_threshold):
    """myLeaveBiggestComponent on the bare n x n confidence matrix -> kept indices."""
    conf = np.ascontiguousarray(confidence, np.float64)
    n = conf.shape[0]
    idx = np.zeros(n, np.int32)
    k = C.c_int()
    check_rc(capi.load().mis_leave_biggest_component_conf(conf.ctypes.data_as(C.c_void_p), n, float(conf_threshold), idx.ctypes.data_as(C.c_void_p), C.byref(k)),
             "mis_leave_biggest_component_conf")
    return idx[: k.value].copy()


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
