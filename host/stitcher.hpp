// stitcher.hpp -- C++17 host side of the MI355X stitching hot path: the sequence of the reference's
// main() (image_stitching/image_stitching.cpp:281-1232) re-authored over the C ABI of libmistitch
// (include/mistitch.h).  No OpenCV: plain PODs, std::vector, and the library's opaque handles.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>
#include "../include/mistitch.h"
#include "rotation.hpp"

namespace mis {

// The reference's globals-as-config (image_stitching.cpp:49-85), same defaults.
struct StitchConfig {
    // work_megapix >= 0: features, matching and bundle adjustment on frames resized by work_scale (:589-603, work_geometry below)
    double work_megapix = -1, seam_megapix = 0.1, compose_megapix = -1;  // compose -1: full-resolution warp + blend
    float conf_thresh = 0.95f;
    float match_conf = 0.32f;
    int blend_type = MIS_BLEND_MULTI_BAND;
    float blend_strength = 5;
    std::string features_type = "orb";     // "orb" | "akaze" | "sift" (:543-563)
    // camera refinement (:681-726).  The reference's default is "reproj"; "no" keeps the supplied (sensor) cameras.
    std::string ba_cost_func = "no";       // "no" | "reproj" | "ray"
    std::string ba_refine_mask = "_____";  // the reference's default: rotations only
    std::string wave_correct = "horiz";    // "horiz" | "vert" | "no"; applied after the bundle adjustment only
    // seam-scale step (:940-1070, :1162-1171).  The reference's defaults are "gain_blocks" and "dp_color" (both implemented:
    // mis_compensator_*, mis_seam_dp; "dp_colorgrad" is mis_seam_dp_colorgrad); this struct defaults to the HOT PATH of the north star (no seam-scale step), like
    // image_stitching_amd.StitchConfig.hot_path() -- pass "gain_blocks" / "dp_color" for the reference's configuration.
    std::string expos_comp_type = "no";    // "no" | "gain" | "gain_blocks" | "channels" | "channels_blocks" (:73; 64 x 64 blocks, 2 filtering passes)
    int expos_comp_nr_feeds = 1;           // :74
    std::string seam_find_type = "no";     // "no" | "voronoi" | "dp_color" | "dp_colorgrad" (dp_color: the reference's default; this driver's default is the hot path)
    // warper (:917-969): the three of the reference's GPU branch and its Mercator, fisheye, stereographic, compressed-plane and Panini
    // warpers are built; its other names (the portrait variants, transverseMercator, affine) throw by name (warp_kind)
    std::string warp_type = "spherical";   // "spherical" | "cylindrical" | "plane" | "mercator" | "fisheye" | "stereographic" | "compressedPlaneA2B1" | "compressedPlaneA1.5B1" | "paniniA2B1" | "paniniA1.5B1"
    // matcher (:83, :646-649): -1 BestOf2NearestMatcher (all pairs), w >= 1 BestOf2NearestRangeMatcher (pairs with j < i + w only)
    int range_width = -1;
    // matcher_type (:64, :644-645): "homography" (the two above) | "affine": AffineBestOf2NearestMatcher(false, ...), all pairs
    std::string matcher_type = "homography";
    // cv::Stitcher::Mode: "panorama" (everything above, cameras supplied by the caller) | "scans" (Stitcher::create(SCANS): flat material
    // under similarities -- no cameras are supplied; the affine matcher, AffineBasedEstimator, BundleAdjusterAffinePartial and the
    // AffineWarper run whatever matcher_type, ba_cost_func and warp_type say; no wave correction, no exposure compensation)
    std::string mode = "panorama";
    // where the panorama mode's cameras come from: "supplied" (the caller's, one per frame) | "homography" (HomographyBasedEstimator,
    // image_stitchin3g.cpp:746-779 / Stitcher::create(PANORAMA): no cameras are supplied; focals from the pairwise homographies,
    // rotations chained along the spanning tree, then ba_cost_func and wave_correct as configured).  Not read in the scans mode.
    std::string estimator_type = "supplied";
    // the reference's `timelapse` switch (:82) and timelapse_type = Timelapser::CROP (:79): the compositing loop's other sink.  The flag is
    // what a driver reads to call Stitcher::timelapse in place of stitch (stitch_main --timelapse); stitch() and the jobs refuse it by name
    bool timelapse = false;
    std::string timelapse_type = "crop";   // "as_is" | "crop"
};

// timelapse_type of the config -> MIS_TIMELAPSE_*; any other name is refused by name
inline int timelapse_kind(const std::string& t) {
    if (t == "as_is") return MIS_TIMELAPSE_AS_IS;
    if (t == "crop") return MIS_TIMELAPSE_CROP;
    throw std::runtime_error("timelapse_type '" + t + "': 'as_is' or 'crop' (--timelapse)");
}

// mode of the config -> scans?; an unknown name is refused by name
inline bool mode_is_scans(const std::string& m) {
    if (m == "panorama") return false;
    if (m != "scans") throw std::runtime_error("mode '" + m + "': 'panorama' or 'scans' (--mode)");
    return true;
}

// estimator_type of the config -> does the homography estimator run?; "affine" (AffineBasedEstimator) is the scans mode's and is
// refused by name with that pointer, an unknown name is refused by name
inline bool estimator_is_homography(const std::string& t) {
    if (t == "supplied") return false;
    if (t == "homography") return true;
    if (t == "affine") throw std::runtime_error("estimator_type 'affine': AffineBasedEstimator runs in mode = \"scans\" (--mode scans), not under this name");
    throw std::runtime_error("estimator_type '" + t + "': 'supplied' or 'homography' (--estimator)");
}

// matcher_type of the config -> MIS_MATCH_*, the check before any device work.  An unknown name is refused by name; so is "affine"
// together with a range_width: the reference silently ignores range_width there (:644 comes first), no option is ignored here
inline int matcher_model(const std::string& t, int range_width) {
    if (t == "homography") return MIS_MATCH_HOMOGRAPHY;
    if (t != "affine") throw std::runtime_error("matcher_type '" + t + "': 'homography' or 'affine' (--matcher)");
    if (range_width != -1)
        throw std::runtime_error("matcher_type 'affine' with range_width " + std::to_string(range_width) + " (--matcher affine --rangewidth): AffineBestOf2NearestMatcher matches all pairs");
    return MIS_MATCH_AFFINE_PARTIAL;
}
// expos_comp_type / expos_comp_nr_feeds of the config -> MIS_EXPOS_*, the check before any device work
inline int expos_comp_kind(const std::string& t, int nr_feeds) {
    if (nr_feeds < 1) throw std::runtime_error("expos_comp_nr_feeds " + std::to_string(nr_feeds) + ": an integer >= 1 (--expos_comp_nr_feeds)");
    if (t == "no") return MIS_EXPOS_NO;
    if (t == "gain") return MIS_EXPOS_GAIN;
    if (t == "gain_blocks") return MIS_EXPOS_GAIN_BLOCKS;
    if (t == "channels") return MIS_EXPOS_CHANNELS;
    if (t == "channels_blocks") return MIS_EXPOS_CHANNELS_BLOCKS;
    throw std::runtime_error("exposure compensation '" + t + "': 'no', 'gain', 'gain_blocks', 'channels' or 'channels_blocks' (--expos_comp)");
}
// the matcher's parameters for a model: mis_match_default_params / mis_match_affine_default_params with the config's match_conf
inline MisMatchParams match_params(int model, float match_conf) {
    MisMatchParams mp;
    if (model == MIS_MATCH_AFFINE_PARTIAL) mis_match_affine_default_params(&mp); else mis_match_default_params(&mp);
    mp.match_conf = match_conf;
    return mp;
}

// features_type of the config (image_stitching.cpp:543-565): the finders this library builds, refused in the reference's words otherwise
inline const std::string& check_features_type(const std::string& t) {
    if (t != "orb" && t != "sift" && t != "akaze") throw std::runtime_error("Unknown 2D features type: '" + t + "'.");
    return t;
}
// range_width of the config: -1 or >= 1 (mis_match_pairs_select refuses the rest too; this is the check before any device work)
inline int check_range_width(int w) {
    if (w != -1 && w < 1) throw std::runtime_error("range_width " + std::to_string(w) + ": -1 (match all pairs) or a width >= 1");
    return w;
}
// how many pairs a matcher call selects for these keypoint counts (the rule of mis_match_pairs_select without a mask)
inline int selected_pair_count(const std::vector<int>& counts, int range_width) {
    int np = 0;
    for (size_t i = 0; i < counts.size(); i++)
        for (size_t j = i + 1; j < counts.size(); j++)
            np += counts[i] > 0 && counts[j] > 0 && (range_width == -1 || (int)j < (int)i + range_width);
    return np;
}

// warp_type -> MIS_WARP_*; the reference's other warpers (:933-964) are not implemented, anything else is not a warper at all
inline int warp_kind(const std::string& t) {
    if (t == "spherical") return MIS_WARP_SPHERICAL;
    if (t == "cylindrical") return MIS_WARP_CYLINDRICAL;
    if (t == "plane") return MIS_WARP_PLANE;
    if (t == "mercator") return MIS_WARP_MERCATOR;
    if (t == "fisheye") return MIS_WARP_FISHEYE;
    if (t == "stereographic") return MIS_WARP_STEREOGRAPHIC;
    if (t == "compressedPlaneA2B1") return MIS_WARP_COMPRESSED_PLANE_A2B1;
    if (t == "compressedPlaneA1.5B1") return MIS_WARP_COMPRESSED_PLANE_A15B1;
    if (t == "paniniA2B1") return MIS_WARP_PANINI_A2B1;
    if (t == "paniniA1.5B1") return MIS_WARP_PANINI_A15B1;
    static const char* unbuilt[] = {"affine", "compressedPlanePortraitA2B1", "compressedPlanePortraitA1.5B1", "paniniPortraitA2B1", "paniniPortraitA1.5B1",
                                    "transverseMercator"};
    for (const char* u : unbuilt)
        if (t == u) throw std::runtime_error("warper '" + t + "' is not implemented ('spherical', 'cylindrical', 'plane', 'mercator', 'fisheye', 'stereographic', "
                                             "'compressedPlaneA2B1', 'compressedPlaneA1.5B1', 'paniniA2B1' and 'paniniA1.5B1' are)");
    throw std::runtime_error("Can't create the following warper '" + t + "'");
}

// work scale of main() (:589-603): 1 when work_megapix < 0, else min(1, sqrt(work_megapix * 1e6 / area)) from the first frame; the
// work image has the size cv::resize gives for that factor (cvRound).  No |scale - 1| > 0.1 test here, unlike the compose loop.
struct WorkGeometry { double scale = 1; int width = 0, height = 0; };
inline WorkGeometry work_geometry(const StitchConfig& cfg, int width, int height) {
    WorkGeometry g{1.0, width, height};
    if (cfg.work_megapix < 0) return g;
    g.scale = std::min(1.0, std::sqrt(cfg.work_megapix * 1e6 / ((double)width * height)));
    if (g.scale < 1.0) { g.width = (int)std::nearbyint(width * g.scale); g.height = (int)std::nearbyint(height * g.scale); }
    return g;
}

// cv::detail::CameraParams as main() fills it (focal, aspect, ppx, ppy, R, t)
struct CameraParams {
    double focal = 1, aspect = 1, ppx = 0, ppy = 0;
    Mat3<double> R;
    std::array<double, 3> t{};
    Mat3<double> K() const {
        Mat3<double> k;
        k(0, 0) = focal; k(0, 2) = ppx; k(1, 1) = focal * aspect; k(1, 2) = ppy; k(2, 2) = 1;
        return k;
    }
};

struct HostImage {
    int width = 0, height = 0, channels = 0;
    std::vector<uint8_t> data;
};

// "[a,b,...]" -> n x n row-major doubles, n = floor(sqrt(count))  (serializer.cpp:7-36 parseMatrixStr)
std::vector<double> parseMatrixStr(std::string_view sv, int* side);
// "isPortrait;compass;[proj4x4];[view4x4];[camTransform4x4];[K3x3]" -> CameraParams (image_stitching.cpp:413-517)
CameraParams cameraFromImageDescription(const std::string& desc, bool* isPortrait);
HostImage readPPM(const std::string& path);
void writePPM(const std::string& path, const HostImage& img);
// imread of baseline JPEG files (jpeg.cpp: mis_jpeg_decode_batch, one call for all frames) -> 8UC3 BGR; a refused file throws its cause
std::vector<HostImage> decodeJPEGBatch(MisContext* ctx, const std::vector<std::string>& paths);
HostImage decodeJPEG(MisContext* ctx, const std::string& path);
// imwrite of a JPEG file (jpeg.cpp: mis_jpeg_encode; image_stitching.cpp:1228) from an 8UC3 BGR image in host memory or, as a MisImage,
// wherever it lies: the file's bytes, cv::imwrite's with the defaults (quality 95, 4:2:0); a refused image throws its cause
std::vector<uint8_t> encodeJPEG(MisContext* ctx, const MisImage& bgr, const MisJpegEncodeParams& params = MisJpegEncodeParams{0, MIS_JPEG_420, 0});
std::vector<uint8_t> encodeJPEG(MisContext* ctx, const HostImage& bgr, const MisJpegEncodeParams& params = MisJpegEncodeParams{0, MIS_JPEG_420, 0});
// n files in one mis_jpeg_encode_batch call (the timelapse output's fixed_<k>.jpg, image_stitching.cpp:1214)
std::vector<std::vector<uint8_t>> encodeJPEGBatch(MisContext* ctx, const std::vector<HostImage>& bgrs, const MisJpegEncodeParams& params = MisJpegEncodeParams{0, MIS_JPEG_420, 0});
void writeJPEG(const std::string& path, MisContext* ctx, const MisImage& bgr, const MisJpegEncodeParams& params = MisJpegEncodeParams{0, MIS_JPEG_420, 0});
void writeJPEG(const std::string& path, MisContext* ctx, const HostImage& bgr, const MisJpegEncodeParams& params = MisJpegEncodeParams{0, MIS_JPEG_420, 0});

struct StitchResult {
    HostImage pano;      // 8UC3 (saturate_cast<uchar> of the 16SC3 result, as imwrite does)
    HostImage mask;      // 8UC1
    std::vector<int> indices;          // images kept by the biggest-component pruning
    std::vector<CameraParams> cameras; // of the kept images, after the optional refinement; in work units (focal, ppx, ppy times work_scale, :635-637)
    std::vector<int> num_features;
    std::vector<double> confidence;    // n x n
    double t_features = 0, t_matching = 0, t_compositing = 0;
    // where the panorama lies in the warper's plane: what renderView needs to go back from it
    MisPoint pano_tl{0, 0};            // result_roi's corner
    float warp_scale = 0.f;            // the compositing loop's warper scale
    int warp_kind = MIS_WARP_SPHERICAL;
};

// A pinhole view (K, R: 3x3 row-major float32; width x height) rendered out of a finished panorama: mis_warper_warp_backward of
// result.pano with its corner, scale and kind, (LINEAR, CONSTANT 0) -- a viewer's frame, a cube face, a re-projection into a source
// camera -> 8UC3.  A refused view (a panorama wider than 32767, a scans-mode result: AffineWarper has no warpBackward) throws its cause.
HostImage renderView(MisContext* ctx, const StitchResult& result, const float K[9], const float R[9], int width, int height);

// cv::detail::resultRoiIntersection (mis_result_roi_intersection); an empty intersection throws with the rectangle named
MisRect resultRoiIntersection(const std::vector<MisPoint>& corners, const std::vector<MisSize>& sizes);

// cv::detail::Timelapser over mis_timelapser_* (image_stitching.cpp:1083, :1196-1197, :1203-1204): initialize fixes dst_roi (resultRoi for
// "as_is", resultRoiIntersection for "crop"), process places a warped 16SC3 image (host or device) into a canvas of dst_roi's size
class Timelapser {
public:
    Timelapser(MisContext* ctx, const std::string& type);
    ~Timelapser();
    Timelapser(const Timelapser&) = delete;
    Timelapser& operator=(const Timelapser&) = delete;
    void initialize(const std::vector<MisPoint>& corners, const std::vector<MisSize>& sizes);
    MisRect dstRoi() const;
    // -> the 16SC3 canvas, dst_roi.width * dst_roi.height * 3 values (getDst)
    const std::vector<int16_t>& process(const MisImage& img_s16x3, MisPoint tl);
    const std::vector<int16_t>& getDst() const { return dst_; }

private:
    MisContext* ctx_;
    MisTimelapser* t_ = nullptr;
    std::vector<int16_t> dst_;
};

// what Stitcher::timelapse returns: one registered frame per kept image, all of dst_roi's size
struct TimelapseResult {
    std::vector<HostImage> frames;     // 8UC3 BGR (saturate_cast<uchar> of the 16SC3 canvases, as imwrite does at :1214), kept-index order
    MisRect dst_roi{0, 0, 0, 0};       // where the canvas lies in the warper's plane
    std::vector<int> indices;
    std::vector<CameraParams> cameras;
    std::vector<int> num_features;
    std::vector<double> confidence;
};

class Stitcher {
public:
    explicit Stitcher(int device = 0, const StitchConfig& cfg = StitchConfig());
    ~Stitcher();
    // frames: 8UC3 BGR of one size; cameras: one per frame (sensor / ground-truth K, R); none in the scans mode or with
    // estimator_type = "homography"
    StitchResult stitch(const std::vector<HostImage>& frames, const std::vector<CameraParams>& cameras);
    // the same registration, then the timelapser in place of the blender (:1194-1215): every kept frame warped into the common
    // canvas of cfg.timelapse_type after the exposure compensator's apply; the seam finder does not run (its masks reach no result).
    // expos_comp_type "no", "gain", "channels": one mis_timelapse_warp_batch call; the block types: warp_fused -> apply -> process
    TimelapseResult timelapse(const std::vector<HostImage>& frames, const std::vector<CameraParams>& cameras);

private:
    StitchResult run(const std::vector<HostImage>& frames, const std::vector<CameraParams>& cameras, TimelapseResult* timelapse);
    void check(int rc, const char* what) const;
    StitchConfig cfg_;
    MisContext* ctx_ = nullptr;
};

}  // namespace mis
