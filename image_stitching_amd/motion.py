"""Camera estimation, bundle adjustment and wave correction (image_stitching.cpp:671-726; cv::Stitcher::estimateCameraParams)."""
import ctypes as C
import functools

import numpy as np

from . import _capi as capi
from .core import check_rc
from .features import features_array
from .matchers import _require_matches

WAVE_CORRECT_HORIZ, WAVE_CORRECT_VERT = 0, 1
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


def _camera_K(c):
    """CameraParams::K() of a camera dict: [f 0 ppx; 0 f*aspect ppy; 0 0 1] in double."""
    return np.array([[c["focal"], 0, c["ppx"]], [0, c["focal"] * c["aspect"], c["ppy"]], [0, 0, 1]], np.float64)


def _bundle_adjust(entry, ctx, features, pairwise_matches, cameras, conf_thresh, *extra):
    """The three adjusters: the library's `entry` (features, matches, n, conf_thresh, *extra, cameras) on the marshalled arguments."""
    n = len(features)
    _require_matches(pairwise_matches)
    cams = _camera_array(cameras, n)
    ctx.check(getattr(ctx.lib, entry)(ctx.h, features_array(features), pairwise_matches._mis, n, float(conf_thresh), *extra, cams))
    return _camera_dicts(cams, n)


def bundle_adjust_ray(ctx, features, pairwise_matches, cameras, conf_thresh=0.95):
    """(*makePtr<detail::BundleAdjusterRay>())(features, pairwise_matches, cameras) with setConfThresh
    (image_stitching.cpp:683-684): focal and rotation of every camera refined on the rays of the inlier matches, evaluated on the
    device; ppx, ppy, aspect and t come back as given.  cameras and the result as in bundle_adjust_reproj."""
    return _bundle_adjust("mis_bundle_adjust_ray", ctx, features, pairwise_matches, cameras, conf_thresh)


def bundle_adjust_affine_partial(ctx, features, pairwise_matches, cameras, conf_thresh=0.95):
    """(*makePtr<detail::BundleAdjusterAffinePartial>())(features, pairwise_matches, cameras) with setConfThresh
    (image_stitching.cpp:685-686; what Stitcher::create(SCANS) installs): the similarity (a, b, tx, ty) in every camera's R
    refined on the inlier matches, evaluated on the device; focal, aspect, ppx, ppy and t come back as given.  cameras and the
    result as in bundle_adjust_reproj, R the 3x3 homogeneous similarity."""
    return _bundle_adjust("mis_bundle_adjust_affine_partial", ctx, features, pairwise_matches, cameras, conf_thresh)


def bundle_adjust_reproj(ctx, features, pairwise_matches, cameras, conf_thresh=0.95, refine_mask="xxxxx"):
    """(*makePtr<detail::BundleAdjusterReproj>())(features, pairwise_matches, cameras) with setConfThresh /
    setRefinementMask (image_stitching.cpp:681-712).  cameras: list of dicts with focal, ppx, ppy, R (3x3) and
    optionally aspect, t -> new list of dicts (refined; rotations relative to the spanning tree's centre image)."""
    return _bundle_adjust("mis_bundle_adjust_reproj", ctx, features, pairwise_matches, cameras, conf_thresh, refine_mask.encode())


def estimate_affine_cameras(pairwise_matches):
    """(*makePtr<detail::AffineBasedEstimator>())(features, pairwise_matches, cameras): default cameras (focal 1, aspect 1,
    ppx = ppy = 0, t = 0) whose R is the product of the pairwise similarities along the maximum spanning tree from its centre, as
    float32 values.  Host logic; it never fails.  -> list of dicts as bundle_adjust_reproj takes them."""
    _require_matches(pairwise_matches)
    n = pairwise_matches.n
    cams = (capi.MisCameraParams * n)()
    check_rc(capi.load().mis_estimate_affine_cameras(pairwise_matches._mis, n, cams), "mis_estimate_affine_cameras")
    return _camera_dicts(cams, n)


def focals_from_homography(H):
    """detail::focalsFromHomography(H, f0, f1, f0_ok, f1_ok) (autocalib.cpp): the focal lengths of the source and the destination
    view a homography in centred coordinates implies -> (f0, f1, f0_ok, f1_ok); a focal that is not ok is 0.  Host logic."""
    h = (C.c_double * 9)(*np.asarray(H, np.float64).reshape(9))
    f0, f1, ok0, ok1 = C.c_double(), C.c_double(), C.c_int(), C.c_int()
    check_rc(capi.load().mis_focals_from_homography(h, C.byref(f0), C.byref(f1), C.byref(ok0), C.byref(ok1)), "mis_focals_from_homography")
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
    _require_matches(pairwise_matches)
    n = pairwise_matches.n
    focals = (C.c_double * n)()
    check_rc(capi.load().mis_estimate_focal(pairwise_matches._mis, n, _size_array(img_sizes, n), focals), "mis_estimate_focal")
    return list(focals)


def estimate_homography_cameras(pairwise_matches, img_sizes):
    """(*makePtr<detail::HomographyBasedEstimator>())(features, pairwise_matches, cameras) (image_stitchin3g.cpp:746-779; what
    Stitcher::create(PANORAMA) runs): default cameras (aspect 1, t = 0) with the focal of estimate_focal, ppx, ppy at the image
    centre, and R the product of K_from^-1 H^-1 K_to along the maximum spanning tree from its centre, as float32 values.
    img_sizes as in estimate_focal.  Host logic; it never fails.  -> list of dicts as bundle_adjust_ray takes them."""
    _require_matches(pairwise_matches)
    n = pairwise_matches.n
    cams = (capi.MisCameraParams * n)()
    check_rc(capi.load().mis_estimate_homography_cameras(pairwise_matches._mis, n, _size_array(img_sizes, n), cams), "mis_estimate_homography_cameras")
    return _camera_dicts(cams, n)


def wave_correct(rmats, kind=WAVE_CORRECT_HORIZ):
    """detail::waveCorrect(rmats, kind) (image_stitching.cpp:718-726) -> list of corrected 3x3 rotations."""
    a = np.ascontiguousarray(np.stack([np.asarray(r, np.float64).reshape(3, 3) for r in rmats]))
    check_rc(capi.load().mis_wave_correct(a.ctypes.data_as(C.c_void_p), len(rmats), int(kind)), "mis_wave_correct")
    return [a[i].copy() for i in range(len(rmats))]


def _wave_corrected(cams, name):
    """Camera dicts with their rotations wave-corrected; name: "horiz" | "vert" (StitchConfig.wave_correct)."""
    Rs = wave_correct([c["R"] for c in cams], WAVE_CORRECT_VERT if name == "vert" else WAVE_CORRECT_HORIZ)
    return [dict(c, R=R) for c, R in zip(cams, Rs)]


def _refined_subset(ctx, features, pairwise_matches, indices, estimator, adjuster, conf_thresh, wave):
    """The sequence both entries below share, on the kept subset (features / matches re-indexed as leaveBiggestComponent does,
    image_stitching.cpp:746-748): estimator(table) -> cameras, the adjuster on them unless None, wave correction unless "no"."""
    view = pairwise_matches.subset(indices)
    cams = estimator(view)
    if adjuster is not None:
        cams = adjuster(ctx, [features[i] for i in indices], view, cams, conf_thresh)
    return cams if wave == "no" else _wave_corrected(cams, wave)


def estimate_and_refine(ctx, features, pairwise_matches, indices, conf_thresh, estimator, adjuster, wave_correct="no"):
    """The reference's sequence after the pruning for a job without supplied cameras (cv::Stitcher::estimateCameraParams): the
    estimator on the kept subset's table, its rotations handed on as float32, then the bundle adjuster on the subset's features,
    then wave correction of the rotations ("horiz" | "vert"; "no": none, as the scans mode has it).
    estimator(pairwise_matches) -> cameras; adjuster(ctx, features, pairwise_matches, cameras, conf_thresh) -> cameras or None for
    no adjustment.  -> camera dicts with K (3x3 float64) and R (3x3 float32) for the kept frames, in the order of `indices`."""
    cams = _refined_subset(ctx, features, pairwise_matches, indices, estimator, adjuster, conf_thresh, wave_correct)
    return [dict(K=_camera_K(c), R=np.asarray(c["R"], np.float32), f=c["focal"], params=c) for c in cams]


def refine_cameras(ctx, features, pairwise_matches, indices, cameras, cfg):
    """The reference's sequence after the pruning (image_stitching.cpp:671-726) on the kept subset: bundle adjustment
    of the subset's cameras (features / matches re-indexed as leaveBiggestComponent does), then wave correction.
    cameras: dicts with K (3x3), R; returns new dicts for the kept frames, in the order of `indices`."""
    start = [dict(focal=float(cameras[i]["K"][0, 0]), aspect=float(cameras[i]["K"][1, 1] / cameras[i]["K"][0, 0]), ppx=float(cameras[i]["K"][0, 2]),
                  ppy=float(cameras[i]["K"][1, 2]), R=cameras[i]["R"]) for i in indices]
    adjuster = bundle_adjust_ray if check_ba_config(cfg) == "ray" else functools.partial(bundle_adjust_reproj, refine_mask=cfg.ba_refine_mask)
    refined = _refined_subset(ctx, features, pairwise_matches, indices, lambda view: start, adjuster, cfg.conf_thresh, cfg.wave_correct)
    return [dict(cameras[i], K=_camera_K(c), R=c["R"], f=c["focal"]) for i, c in zip(indices, refined)]
