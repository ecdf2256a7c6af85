"""Host-side mirror of the reference's stitching interface over the libmistitch C ABI.

Names and argument meaning follow the cv::detail objects that image_stitching.cpp's main() drives
(file:line cited per class).  Images are torch CUDA tensors (zero-copy device pointers) or numpy
arrays (host buffers staged by the library).

This module is the pipeline: the configuration, the geometry of the scales, the seam-scale step and Stitcher.  The stages live in
core, warpers, imgops, seams, blenders, features, matchers and motion; every name of theirs is also a name of this module.
"""
import functools
from dataclasses import dataclass

import numpy as np

from . import _capi as capi
from .core import (Context, Handle, MisError, _NP_DT, _TORCH_DT, _c_array, _empty_image, _images, _mat9, _memcpy_dtoh, _points, as_image,
                   check_rc, torch)
from .warpers import (BUILT_WARP_KINDS, REFUSED_WARP_TYPES, UNBUILT_WARP_TYPES, WARP_KINDS, AffineWarper, CompressedRectilinearWarper,
                      CylindricalWarper, FisheyeWarper, MercatorWarper, PaniniWarper, PlaneWarper, RotationWarper, SphericalWarper,
                      StereographicWarper, _ab_kind, check_warp_config, make_warper, warp_kind, warp_roi, warp_rois)
from .imgops import (JPEG_SAMPLING, ROTATE_90_CLOCKWISE, ROTATE_90_COUNTERCLOCKWISE, ROTATE_180, _jpeg_bytes, _take_stream, imencode,
                     imencode_batch, imread, imread_batch, imwrite, jpeg_encode_params, jpeg_info, resize, resize_batch, rotate,
                     seam_mask_apply)
from .seams import (EXPOS_COMP_TYPES, SEAM_FIND_TYPES, BlocksChannelsCompensator, BlocksGainCompensator, ChannelsCompensator, DpSeamFinder,
                    GainCompensator, GraphCutSeamFinder, NoSeamFinder, VoronoiSeamFinder, _Compensator, _seam_args, apply_seam,
                    check_seam_config, make_compensator, make_seam_finder, seam_gradients)
from .blenders import Blender, FeatherBlender, MultiBandBlender, blend_config, make_blender, result_roi
from .timelapse import (TIMELAPSE_TYPES, Timelapser, check_timelapse_config, result_roi_intersection, timelapse_kind, timelapse_warp_batch,
                        timelapse_warp_batch_timed)
from .cropper import crop_device, crop_rect_device
from .features import KP_DTYPE, AkazeFeatureFinder, ImageFeatures, OrbFeatureFinder, SiftFeatureFinder, computeImageFeatures, features_array, orb_params
from .matchers import (DMATCH_DTYPE, MATCHER_TYPES, AffineBestOf2NearestMatcher, BestOf2NearestMatcher, BestOf2NearestRangeMatcher,
                       MatchesInfo, PairwiseMatches, _require_matches, _unpack_mi, check_matcher_config, check_range_config,
                       estimate_affine_partial, find_homography, leaveBiggestComponent, leaveBiggestComponentConf, match_params,
                       selected_pairs)
from .motion import (BA_COST_FUNCS, WAVE_CORRECT_HORIZ, WAVE_CORRECT_VERT, _camera_array, _camera_dicts, _size_array, _wave_corrected,
                     bundle_adjust_affine_partial, bundle_adjust_ray, bundle_adjust_reproj, check_ba_config, estimate_affine_cameras,
                     estimate_and_refine, estimate_focal, estimate_homography_cameras, focals_from_homography, refine_cameras, wave_correct)


def make_matcher(ctx, cfg):
    """if (matcher_type == "affine") AffineBestOf2NearestMatcher(false, ...) else if (range_width == -1) BestOf2NearestMatcher
    else BestOf2NearestRangeMatcher (image_stitching.cpp:644-649)"""
    if check_matcher_config(cfg) == "affine":
        return AffineBestOf2NearestMatcher(ctx, False, cfg.match_conf)
    if cfg.range_width == -1:
        return BestOf2NearestMatcher(ctx, cfg.match_conf)
    return BestOf2NearestRangeMatcher(ctx, cfg.range_width, cfg.match_conf)


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


def seam_solve(ctx, cfg, corners, images_warped, masks_warped, seam_finder=None, find_seams=True):
    """The part of the seam-scale pass that needs every image (image_stitching.cpp:1002-1023 exposure compensator feed, :1029-1065
    seam finder) -> (compensator | None, masks_warped edited in place).  seam_finder: a finder object (anything with
    find(images, corners, masks)) that runs in place of the configured one, as cv::Stitcher::setSeamFinder's does.
    find_seams False: no finder runs, the configured one included (the timelapse mode: its masks reach no result)."""
    compensator = make_compensator(ctx, cfg)
    if compensator is not None:
        compensator.feed(corners, images_warped, masks_warped)
    if not find_seams:
        return compensator, masks_warped
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
    matching and bundle adjustment at work scale (:589-603); the cameras a caller passes are always in full-resolution pixels.
    match_conf is the caller's: 0.32 is this package's default (ORB), and 0.65 is the reference's value for every non-ORB
    features_type (:59) -- pass it with features_type "akaze"."""
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
    timelapse_type: str = "crop"           # "as_is" | "crop" (:79; read by Stitcher.compose_timelapse / timelapse only)

    def __post_init__(self):
        check_ba_config(self)
        check_timelapse_config(self)

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
        # (:547-550: AKAZE, 61-byte descriptors -> the wide Hamming 2-NN; every other value: the ORB finder)
        self.finder = AkazeFeatureFinder(ctx, self.work_size) if self.cfg.features_type == "akaze" else OrbFeatureFinder(ctx, self.work_size)
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
            blender = make_blender(self.ctx, self.cfg.blend_type, self.cfg.blend_strength, (pw, ph))[0]
        blender.prepare(corners, sizes)
        for k, i in enumerate(indices):
            tl, img_s, mask = warper.warp_fused(frames[i], cameras[i]["K"], cameras[i]["R"], rois[k])
            if seam is not None:
                apply_seam(self.ctx, seam, k, corners[k], img_s, mask)
            blender.feed(img_s, mask, tl)
        return blender.blend()

    def crop_panorama(self, pano, mask):
        """The reference's cropper (cropper.cpp:124-209) on the blender's result: the rectangle crop() finds on the result mask,
        computed on the device -> (pano[y:y + h, x:x + w], mask[y:y + h, x:x + w], (x, y, w, h)), views without a copy."""
        x, y, w, h = crop_rect_device(self.ctx, mask)
        return pano[y:y + h, x:x + w], mask[y:y + h, x:x + w], (x, y, w, h)

    def render_view(self, pano_u8, K, R, size, interp=capi.INTER_LINEAR, border=capi.BORDER_CONSTANT, with_mask=False):
        """A pinhole view (K, R; size = (w, h)) rendered out of the last composition's panorama, given as 8UC3 (the caller converts
        the blender's 16SC3 result, as for imwrite): RotationWarper.warp_backward with the panorama's corner, the compose scale and
        the warper kind that compose() recorded."""
        c = getattr(self, "composition", None)
        if c is None:
            raise RuntimeError("render_view: compose() has not run on this stitcher")
        return RotationWarper(self.ctx, c["warp_scale"], c["kind"]).warp_backward(pano_u8, c["pano_tl"], K, R, size, interp, border, with_mask)

    def seam_step(self, frames, cameras, indices, warped_image_scale, work_scale=None, find_seams=True):
        """The seam-scale pass of main() (image_stitching.cpp:604-622 resize, :973-990 warp, :1002-1023 exposure
        compensator feed, :1029-1065 seam finder) -> (compensator | None, masks_warped) or None when both are off.
        find_seams False: the exposure compensator alone (compose_timelapse); None when it is off."""
        check_seam_config(self.cfg)
        if self.cfg.expos_comp_type == "no" and (not find_seams or (self.cfg.seam_find_type == "no" and self.seam_finder is None)):
            return None
        work_scale = self.work_scale if work_scale is None else work_scale
        items = [seam_scale_warp(self.ctx, self.cfg, self.frame_size, frames[i], cameras[i], warped_image_scale, work_scale,
                                 self.kind if self.kind != check_warp_config(self.cfg) else None) for i in indices]
        return seam_solve(self.ctx, self.cfg, [it[0] for it in items], [it[1] for it in items], [it[2] for it in items], self.seam_finder, find_seams)

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

    def compose_timelapse(self, frames, as_u8=True):
        """The compositing loop with the timelapser as its sink (image_stitching.cpp:1086-1215 with `timelapse` set): frames of the
        registered rig (as compose_panorama takes them) each warped into the common canvas of cfg.timelapse_type -- resultRoi of all
        warp rois ("as_is") or their intersection ("crop") -- after the exposure compensator's apply (:1162); nothing is blended and
        the seam finder does not run (its masks reach no result).  Geometry, cameras, rois and the compose-scale resize are compose()'s.
        No compensator, GainCompensator: one fused launch per 16 frames (timelapse_warp_batch); the block compensators: warp_fused ->
        apply -> Timelapser.process -> saturate_cast<uchar>, frame by frame.
        -> (canvases in kept-index order: packed 8UC3 BGR (as_u8, what imencode_batch reads) or 16SC3, dst_roi)."""
        if self.indices is None:
            raise ValueError("compose_timelapse: estimate_transform has not run")
        indices, cameras = list(self.indices), self.cameras
        scale = self.warped_image_scale([cameras[i] for i in indices])
        g = compose_geometry(self.cfg, self.frame_size, scale, self.work_scale)
        seam = self.seam_step(frames, cameras, indices, scale, self.work_scale, find_seams=False)
        compensator = None if seam is None else seam[0]
        if g.aspect != 1.0:
            cameras = {i: scaled_camera(cameras[i], g.aspect) for i in indices}
        if g.size != tuple(self.frame_size):
            frames = {i: resize(self.ctx, frames[i], fx=g.compose_scale, fy=g.compose_scale) for i in indices}
        scale = g.warp_scale
        cams = [cameras[i] for i in indices]
        rois = warp_rois(self.ctx, scale, g.size, cams, self.kind)
        corners = [(r[0], r[1]) for r in rois]
        sizes = [(r[2], r[3]) for r in rois]
        if check_timelapse_config(self.cfg) == capi.TIMELAPSE_CROP:
            dst_roi = result_roi_intersection(corners, sizes)
        else:
            dst_roi = result_roi(corners, sizes)
        if compensator is None or isinstance(compensator, (GainCompensator, ChannelsCompensator)):
            gains = None if compensator is None else np.stack([compensator.gains(k) for k in range(len(indices))])
            return timelapse_warp_batch(self.ctx, self.kind, [frames[i] for i in indices], cams, rois, scale, dst_roi, gains, as_u8), dst_roi
        warper = RotationWarper(self.ctx, scale, self.kind)
        timelapser = Timelapser(self.ctx, self.cfg.timelapse_type)
        timelapser.initialize(corners, sizes)
        canvases = []
        for k, i in enumerate(indices):
            tl, img_s, mask = warper.warp_fused(frames[i], cameras[i]["K"], cameras[i]["R"], rois[k])
            compensator.apply(k, corners[k], img_s, mask)
            canvas = timelapser.process(img_s, None, tl)
            canvases.append(canvas.clamp(0, 255).to(torch.uint8) if as_u8 else canvas)       # imwrite's saturate_cast<uchar> (:1214)
        return canvases, dst_roi

    def timelapse(self, frames, cameras=None):
        """estimate_transform + compose_timelapse: N frames in, N registered frames out -> (canvases, dst_roi); the kept frame
        indices are self.indices."""
        self.estimate_transform(frames, cameras)
        return self.compose_timelapse(frames)

    def stitch(self, frames, cameras=None):
        feats, pm, idx = self.estimate_transform(frames, cameras)
        result, mask = self.compose_panorama(frames)
        return result, mask, feats, pm, idx
