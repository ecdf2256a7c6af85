"""image_stitching_amd -- MI355X-native hot path of a1q123456/image_stitching.

Host-side mirror (Python) of the interface the reference drives in ``main()``
(image_stitching/image_stitching.cpp:545-1228): ``computeImageFeatures`` / ``BestOf2NearestMatcher`` /
``SphericalWarper`` (``CylindricalWarper``, ``PlaneWarper``, ``MercatorWarper``, ``FisheyeWarper``, ``StereographicWarper``, ``CompressedRectilinearWarper``, ``PaniniWarper``, ``AffineWarper``) / ``MultiBandBlender`` / ``FeatherBlender``, each a thin veneer over the C ABI of
``libmistitch.so`` (include/mistitch.h).  torch is used only to own device memory and streams.

There is no CPU fallback: everything here needs the HIP library and a GPU.
"""
from . import _capi
from ._capi import (BLEND_FEATHER, BLEND_MULTI_BAND, BLEND_NO, BORDER_CONSTANT, BORDER_REFLECT, INTER_LINEAR,
                    INTER_NEAREST, WARP_CYLINDRICAL, WARP_FISHEYE, WARP_MERCATOR, WARP_PLANE, WARP_SPHERICAL, WARP_STEREOGRAPHIC,
                    WARP_COMPRESSED_PLANE_A2B1, WARP_COMPRESSED_PLANE_A15B1, WARP_PANINI_A2B1, WARP_PANINI_A15B1, WARP_AFFINE)
from .stitching import (AffineBestOf2NearestMatcher, BestOf2NearestMatcher, BestOf2NearestRangeMatcher, estimate_affine_partial, Blender, BlocksGainCompensator, GainCompensator, ChannelsCompensator, BlocksChannelsCompensator, NoSeamFinder, VoronoiSeamFinder, DpSeamFinder, GraphCutSeamFinder, Context, FeatherBlender, ImageFeatures, MatchesInfo,
                        MisError, MultiBandBlender, OrbFeatureFinder, SiftFeatureFinder, AkazeFeatureFinder, SphericalWarper, CylindricalWarper, PlaneWarper, MercatorWarper, FisheyeWarper, StereographicWarper, CompressedRectilinearWarper, PaniniWarper, AffineWarper,
                        RotationWarper, StitchConfig, Stitcher,
                        blend_config, bundle_adjust_affine_partial, bundle_adjust_ray, bundle_adjust_reproj, estimate_affine_cameras, estimate_focal, estimate_homography_cameras, focals_from_homography, computeImageFeatures, find_homography, leaveBiggestComponent, resize, resize_batch, result_roi,
                        rotate, seam_gradients, seam_mask_apply, selected_pairs, warp_roi, wave_correct, work_geometry, imread, imread_batch, jpeg_info, imencode, imencode_batch, imwrite, jpeg_encode_params,
                        Timelapser, result_roi_intersection, timelapse_warp_batch, crop_device, crop_rect_device)

__all__ = [
    "Context", "MisError", "SphericalWarper", "Blender", "MultiBandBlender", "FeatherBlender", "OrbFeatureFinder", "SiftFeatureFinder",
    "computeImageFeatures", "ImageFeatures", "BestOf2NearestMatcher", "MatchesInfo", "leaveBiggestComponent",
    "find_homography", "warp_roi", "result_roi", "blend_config", "StitchConfig", "Stitcher", "resize", "rotate",
    "seam_mask_apply", "bundle_adjust_reproj", "bundle_adjust_ray", "wave_correct", "BlocksGainCompensator", "GainCompensator", "ChannelsCompensator", "BlocksChannelsCompensator", "NoSeamFinder", "VoronoiSeamFinder", "DpSeamFinder", "GraphCutSeamFinder",
    "INTER_NEAREST", "INTER_LINEAR", "BORDER_CONSTANT", "BORDER_REFLECT", "BLEND_NO", "BLEND_FEATHER",
    "BLEND_MULTI_BAND", "resize_batch", "work_geometry", "CylindricalWarper", "PlaneWarper", "RotationWarper", "WARP_SPHERICAL", "WARP_CYLINDRICAL", "WARP_PLANE", "WARP_MERCATOR", "MercatorWarper", "WARP_FISHEYE", "WARP_STEREOGRAPHIC", "FisheyeWarper", "StereographicWarper",
    "WARP_COMPRESSED_PLANE_A2B1", "WARP_COMPRESSED_PLANE_A15B1", "WARP_PANINI_A2B1", "WARP_PANINI_A15B1", "CompressedRectilinearWarper", "PaniniWarper",
    "BestOf2NearestRangeMatcher", "selected_pairs", "AffineBestOf2NearestMatcher", "estimate_affine_partial", "seam_gradients",
    "WARP_AFFINE", "AffineWarper", "bundle_adjust_affine_partial", "estimate_affine_cameras",
    "focals_from_homography", "estimate_focal", "estimate_homography_cameras",
    "imread", "imread_batch", "jpeg_info", "imencode", "imencode_batch", "imwrite", "jpeg_encode_params",
]
# AkazeFeatureFinder, Timelapser, result_roi_intersection, timelapse_warp_batch, crop_device and crop_rect_device are names of the package too; __all__ stays the list that
# tests/golden/package_all.txt records
