// stitcher.cpp -- see stitcher.hpp.  Stage order and log lines follow the reference's main().
#include "stitcher.hpp"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

namespace mis {

static double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

std::vector<double> parseMatrixStr(std::string_view sv, int* side) {
    sv = sv.substr(1, sv.size() - 2);
    std::vector<std::string> items;
    for (auto pos = sv.find(','); pos != sv.npos; pos = sv.find(',')) { items.emplace_back(sv.substr(0, pos)); sv = sv.substr(pos + 1); }
    items.emplace_back(sv);
    int len = (int)std::sqrt((double)items.size());
    std::vector<double> m((size_t)len * len);
    for (int i = 0; i < len * len; i++) m[i] = std::strtod(items[i].c_str(), nullptr);
    if (side) *side = len;
    return m;
}

CameraParams cameraFromImageDescription(const std::string& desc, bool* isPortrait) {
    std::vector<std::string> parts;
    std::string_view sv(desc);
    for (int i = 0; i < 5; i++) {
        auto pos = sv.find(';');
        if (pos == sv.npos) throw std::runtime_error("ImageDescription needs 6 ';'-separated fields");
        parts.emplace_back(sv.substr(0, pos));
        sv = sv.substr(pos + 1);
    }
    while (!sv.empty() && (sv.back() == '\n' || sv.back() == '\r' || sv.back() == ' ')) sv.remove_suffix(1);
    parts.emplace_back(sv);
    const bool portrait = std::strtol(parts[0].c_str(), nullptr, 10) != 0;
    int n4 = 0, n3 = 0;
    std::vector<double> cam = parseMatrixStr(parts[4], &n4), K = parseMatrixStr(parts[5], &n3);
    if (n4 != 4 || n3 != 3) throw std::runtime_error("ImageDescription: camera transform must be 4x4 and K 3x3");
    CameraParams p;
    p.aspect = 1.0;
    p.focal = K[1 * 3 + 1];
    if (portrait) { p.ppx = K[1 * 3 + 2]; p.ppy = K[0 * 3 + 2]; } else { p.ppx = K[0 * 3 + 2]; p.ppy = K[1 * 3 + 2]; }
    Mat3<double> R;
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R(r, c) = cam[r * 4 + c];
    p.t = {cam[3], cam[7], cam[11]};
    p.R = rehandCameraRotation(R, portrait);
    if (isPortrait) *isPortrait = portrait;
    return p;
}

// the scans mode as Stitcher::create(SCANS) sets it up: what the mode replaces is not read from the configuration
static StitchConfig effective_config(StitchConfig cfg) {
    if (mode_is_scans(cfg.mode)) { cfg.matcher_type = "affine"; cfg.wave_correct = "no"; cfg.expos_comp_type = "no"; }
    return cfg;
}

Stitcher::Stitcher(int device, const StitchConfig& cfg) : cfg_(effective_config(cfg)) {
    int rc = mis_context_create(device, nullptr, &ctx_);
    if (rc != MIS_OK) throw std::runtime_error("mis_context_create failed: no HIP device (there is no CPU fallback)");
}
Stitcher::~Stitcher() { mis_context_destroy(ctx_); }

void Stitcher::check(int rc, const char* what) const {
    if (rc != MIS_OK) throw std::runtime_error(std::string(what) + ": " + mis_last_error(ctx_));
}

static MisImage view(const HostImage& im) {
    MisImage v{};
    v.data = (void*)im.data.data(); v.width = im.width; v.height = im.height; v.channels = im.channels;
    v.stride = (size_t)im.width * im.channels; v.dtype = MIS_U8; v.mem = MIS_MEM_HOST;
    return v;
}

// seam_find_type -> the library call of the seam step (find == nullptr: "no"); an unknown name throws
struct SeamFinderEntry { const char *name, *what; int (*find)(MisContext*, const MisPoint*, const MisImage*, MisImage*, int); };
static const SeamFinderEntry& seam_finder(const std::string& type) {
    static const SeamFinderEntry table[] = {
        {"no", "", nullptr},
        {"voronoi", "mis_seam_voronoi", [](MisContext* c, const MisPoint* p, const MisImage*, MisImage* m, int n) { return mis_seam_voronoi(c, p, m, n); }},
        // the reference's default (image_stitching.cpp:77, :1056-1065)
        {"dp_color", "mis_seam_dp", [](MisContext* c, const MisPoint* p, const MisImage* i, MisImage* m, int n) { return mis_seam_dp(c, p, i, m, n, MIS_SEAM_DP_COLOR); }},
        {"dp_colorgrad", "mis_seam_dp_colorgrad", mis_seam_dp_colorgrad},      // DpSeamFinder(COLOR_GRAD) (:1057-1058)
    };
    std::string names;      // 'a', 'b', 'c' and 'd'
    for (const SeamFinderEntry& e : table) {
        if (type == e.name) return e;
        names += std::string(&e == table ? "'" : (&e + 1 == std::end(table) ? " and '" : ", '")) + e.name + "'";
    }
    throw std::runtime_error("seam finder '" + type + "' is not implemented (" + names + " are)");
}

MisRect resultRoiIntersection(const std::vector<MisPoint>& corners, const std::vector<MisSize>& sizes) {
    if (corners.empty() || corners.size() != sizes.size()) throw std::runtime_error("resultRoiIntersection: as many corners as sizes, at least one");
    MisRect r;
    if (mis_result_roi_intersection(corners.data(), sizes.data(), (int)corners.size(), &r) != MIS_OK) {
        long long x0 = corners[0].x, y0 = corners[0].y, x1 = x0 + sizes[0].width, y1 = y0 + sizes[0].height;
        for (size_t i = 1; i < corners.size(); i++) {
            x0 = std::max<long long>(x0, corners[i].x); y0 = std::max<long long>(y0, corners[i].y);
            x1 = std::min<long long>(x1, (long long)corners[i].x + sizes[i].width); y1 = std::min<long long>(y1, (long long)corners[i].y + sizes[i].height);
        }
        throw std::runtime_error("resultRoiIntersection: the frames' intersection Rect(tl = (" + std::to_string(x0) + ", " + std::to_string(y0) + "), br = (" +
                                 std::to_string(x1) + ", " + std::to_string(y1) + ")) is empty");
    }
    return r;
}

Timelapser::Timelapser(MisContext* ctx, const std::string& type) : ctx_(ctx) {
    if (mis_timelapser_create(ctx_, timelapse_kind(type), &t_) != MIS_OK) throw std::runtime_error(std::string("mis_timelapser_create: ") + mis_last_error(ctx_));
}
Timelapser::~Timelapser() { mis_timelapser_destroy(t_); }
void Timelapser::initialize(const std::vector<MisPoint>& corners, const std::vector<MisSize>& sizes) {
    if (corners.size() != sizes.size()) throw std::runtime_error("Timelapser::initialize: as many corners as sizes");
    if (mis_timelapser_initialize(t_, corners.data(), sizes.data(), (int)corners.size()) != MIS_OK)
        throw std::runtime_error(std::string("mis_timelapser_initialize: ") + mis_last_error(ctx_));
}
MisRect Timelapser::dstRoi() const {
    MisRect r;
    if (mis_timelapser_dst_roi(t_, &r) != MIS_OK) throw std::runtime_error(std::string("mis_timelapser_dst_roi: ") + mis_last_error(ctx_));
    return r;
}
const std::vector<int16_t>& Timelapser::process(const MisImage& img, MisPoint tl) {
    const MisRect r = dstRoi();
    dst_.resize((size_t)r.width * r.height * 3);
    MisImage d{dst_.data(), r.width, r.height, 3, (size_t)r.width * 6, MIS_S16, MIS_MEM_HOST};
    if (mis_timelapser_process(t_, &img, tl, &d) != MIS_OK) throw std::runtime_error(std::string("mis_timelapser_process: ") + mis_last_error(ctx_));
    return dst_;
}

StitchResult Stitcher::stitch(const std::vector<HostImage>& frames, const std::vector<CameraParams>& cams_in) {
    if (cfg_.timelapse) throw std::runtime_error("timelapse = true: the timelapse output is Stitcher::timelapse, stitch() blends a panorama");
    return run(frames, cams_in, nullptr);
}

TimelapseResult Stitcher::timelapse(const std::vector<HostImage>& frames, const std::vector<CameraParams>& cams_in) {
    TimelapseResult tl;
    StitchResult r = run(frames, cams_in, &tl);
    tl.indices = std::move(r.indices); tl.cameras = std::move(r.cameras); tl.num_features = std::move(r.num_features); tl.confidence = std::move(r.confidence);
    return tl;
}

// timelapse == nullptr: the panorama (stitch); otherwise the compositing loop ends in the timelapser and the result's pano stays empty
StitchResult Stitcher::run(const std::vector<HostImage>& frames, const std::vector<CameraParams>& cams_in, TimelapseResult* timelapse) {
    const int n = (int)frames.size();
    const bool scans = mode_is_scans(cfg_.mode);
    const bool estimated = scans || estimator_is_homography(cfg_.estimator_type);      // (estimator_type is not read in the scans mode)
    if (n < 2 || (estimated ? !cams_in.empty() : (int)cams_in.size() != n)) throw std::runtime_error("Need more images");
    StitchResult out;
    std::vector<CameraParams> cameras = cams_in;
    if (estimated) {    // default CameraParams until the estimator runs (focal 1, ppx = ppy = 0, R = I)
        cameras.assign(n, CameraParams());
        for (auto& c : cameras) c.R(0, 0) = c.R(1, 1) = c.R(2, 2) = 1;
    }
    const int W = frames[0].width, H = frames[0].height;

    // ---- features (image_stitching.cpp:545, :567-622) on the work images (:589-603: every frame resized by work_scale, one launch) ----
    const WorkGeometry wg = work_geometry(cfg_, W, H);
    const double work_scale = wg.scale;
    double t = now();
    check_features_type(cfg_.features_type);
    if (cfg_.ba_cost_func != "no" && cfg_.ba_cost_func != "reproj" && cfg_.ba_cost_func != "ray")
        throw std::runtime_error("bundle adjustment cost function '" + cfg_.ba_cost_func + "' is not implemented ('no', 'reproj' and 'ray' are)");
    const int expos_kind = expos_comp_kind(cfg_.expos_comp_type, cfg_.expos_comp_nr_feeds);
    const SeamFinderEntry& seam = seam_finder(timelapse ? std::string("no") : cfg_.seam_find_type);     // (the timelapser never sees the seam masks)
    if (timelapse) seam_finder(cfg_.seam_find_type);     // an unknown name is still refused
    const int tl_type = timelapse_kind(cfg_.timelapse_type);
    const int kind = scans ? MIS_WARP_AFFINE : warp_kind(cfg_.warp_type);
    check_range_width(cfg_.range_width);
    const int model = matcher_model(cfg_.matcher_type, cfg_.range_width);
    MisOrb* orb = nullptr;
    MisSift* sift = nullptr;
    MisAkaze* akaze = nullptr;
    std::vector<MisFeatures> features(n);
    std::vector<MisImage> views(n);
    for (int i = 0; i < n; i++) views[i] = view(frames[i]);
    std::vector<MisImage> work(work_scale < 1.0 ? n : 0, MisImage{});       // allocated by the library, in HBM
    if (work_scale < 1.0) check(mis_resize_linear_exact_batch(ctx_, views.data(), n, 0, 0, work_scale, work_scale, work.data()), "mis_resize_linear_exact_batch");
    const MisImage* imgs = work_scale < 1.0 ? work.data() : views.data();
    if (cfg_.features_type == "sift") {
        check(mis_sift_create(ctx_, nullptr, wg.width, wg.height, &sift), "mis_sift_create");
        check(mis_sift_detect_batch(sift, imgs, n, features.data()), "mis_sift_detect_batch");
    } else if (cfg_.features_type == "akaze") {      // AKAZE::create() (:547-550): 61-byte descriptors, the wide Hamming 2-NN
        check(mis_akaze_create(ctx_, nullptr, wg.width, wg.height, &akaze), "mis_akaze_create");
        check(mis_akaze_detect_batch(akaze, imgs, n, features.data()), "mis_akaze_detect_batch");
    } else {
        MisOrbParams op;
        mis_orb_default_params(&op);
        check(mis_orb_create(ctx_, &op, wg.width, wg.height, &orb), "mis_orb_create");
        check(mis_orb_detect_batch(orb, imgs, n, features.data()), "mis_orb_detect_batch");
    }
    for (auto& im : work) mis_image_free(ctx_, &im);
    // cam.focal, ppx, ppy *= work_scale (:635-637): matching, bundle adjustment and the median focal are in work units
    if (work_scale != 1.0)
        for (auto& c : cameras) { c.focal *= work_scale; c.ppx *= work_scale; c.ppy *= work_scale; }
    for (int i = 0; i < n; i++) {
        features[i].img_idx = i;
        std::cout << "Features in image #" << i + 1 << ": " << features[i].n << std::endl;
        out.num_features.push_back(features[i].n);
    }
    out.t_features = now() - t;

    // ---- pairwise matching (:647-655) and pruning (:661) ----
    t = now();
    const MisMatchParams mp = match_params(model, cfg_.match_conf);
    std::vector<MisMatchesInfo> pairwise((size_t)n * n);
    check(mis_match_pairs_model(ctx_, features.data(), n, &mp, model, nullptr, cfg_.range_width, 0, 1, pairwise.data()), "mis_match_pairs_model");
    for (auto& m : pairwise) out.confidence.push_back(m.confidence);
    out.indices.resize(n);
    int kept = 0;
    mis_leave_biggest_component(pairwise.data(), n, cfg_.conf_thresh, out.indices.data(), &kept);
    out.indices.resize(kept);
    // ---- camera refinement on the kept subset (:671-726): bundle adjustment (reprojection or ray cost), wave correction ----
    //      in the scans mode: AffineBasedEstimator on the kept subset's table, then BundleAdjusterAffinePartial
    //      with estimator_type "homography": HomographyBasedEstimator on that table, then the configured adjuster
    if (kept >= 2 && (estimated || cfg_.ba_cost_func != "no")) {
        std::vector<MisFeatures> fsub(kept);
        std::vector<MisMatchesInfo> psub((size_t)kept * kept);
        std::vector<MisCameraParams> cp(kept);
        for (int a = 0; a < kept; a++) {
            fsub[a] = features[out.indices[a]];
            fsub[a].img_idx = a;
            for (int b = 0; b < kept; b++) {
                psub[(size_t)a * kept + b] = pairwise[(size_t)out.indices[a] * n + out.indices[b]];   // borrowed arrays
                psub[(size_t)a * kept + b].src_img_idx = a; psub[(size_t)a * kept + b].dst_img_idx = b;
            }
            const CameraParams& c = cameras[out.indices[a]];
            cp[a].focal = c.focal; cp[a].aspect = c.aspect; cp[a].ppx = c.ppx; cp[a].ppy = c.ppy;
            std::copy(c.R.m.begin(), c.R.m.end(), cp[a].R);
            std::copy(c.t.begin(), c.t.end(), cp[a].t);
        }
        if (scans) check(mis_estimate_affine_cameras(psub.data(), kept, cp.data()), "mis_estimate_affine_cameras");
        else if (estimated) {       // on the sizes of the images the features were found on (work scale)
            std::vector<MisSize> fsizes(kept);
            for (int a = 0; a < kept; a++) fsizes[a] = {fsub[a].img_w, fsub[a].img_h};
            check(mis_estimate_homography_cameras(psub.data(), kept, fsizes.data(), cp.data()), "mis_estimate_homography_cameras");
        }
        const int ba_rc = scans ? mis_bundle_adjust_affine_partial(ctx_, fsub.data(), psub.data(), kept, cfg_.conf_thresh, cp.data())
                        : cfg_.ba_cost_func == "no" ? MIS_OK          // (reached with an estimator only: its cameras are kept)
                        : cfg_.ba_cost_func == "ray" ? mis_bundle_adjust_ray(ctx_, fsub.data(), psub.data(), kept, cfg_.conf_thresh, cp.data())
                                                     : mis_bundle_adjust_reproj(ctx_, fsub.data(), psub.data(), kept, cfg_.conf_thresh, cfg_.ba_refine_mask.c_str(), cp.data());
        if (ba_rc != MIS_OK)
            throw std::runtime_error(std::string("Camera parameters adjusting failed: ") + mis_last_error(ctx_));
        if (cfg_.wave_correct != "no") {
            std::vector<double> rm((size_t)kept * 9);
            for (int a = 0; a < kept; a++) std::copy(cp[a].R, cp[a].R + 9, rm.begin() + 9 * a);
            check(mis_wave_correct(rm.data(), kept, cfg_.wave_correct == "vert" ? 1 : 0), "mis_wave_correct");
            for (int a = 0; a < kept; a++) std::copy(rm.begin() + 9 * a, rm.begin() + 9 * a + 9, cp[a].R);
        }
        for (int a = 0; a < kept; a++) {
            CameraParams& c = cameras[out.indices[a]];
            c.focal = cp[a].focal; c.aspect = cp[a].aspect; c.ppx = cp[a].ppx; c.ppy = cp[a].ppy;
            std::copy(cp[a].R, cp[a].R + 9, c.R.m.begin());
            std::copy(cp[a].t, cp[a].t + 3, c.t.begin());
        }
    }
    mis_matches_free(pairwise.data(), n * n);
    for (auto& f : features) mis_features_free(ctx_, &f);
    if (orb) mis_orb_destroy(orb);
    if (sift) mis_sift_destroy(sift);
    if (akaze) mis_akaze_destroy(akaze);
    out.t_matching = now() - t;
    if (kept < 2) throw std::runtime_error("Need more images");
    out.cameras.clear();
    for (int i : out.indices) out.cameras.push_back(cameras[i]);

    // ---- warped image scale = median focal (:884-895) ----
    std::vector<double> focals;
    for (int i : out.indices) focals.push_back(cameras[i].focal);
    std::sort(focals.begin(), focals.end());
    float warped_image_scale = focals.size() % 2 == 1 ? static_cast<float>(focals[focals.size() / 2])
                                                      : static_cast<float>(focals[focals.size() / 2 - 1] + focals[focals.size() / 2]) * 0.5f;

    // ---- compositing (:1086-1228) at compose scale (:1105-1146): the warper's scale and the intrinsics times compose_work_aspect,
    //      frames (and their sizes, cvRound) resized only when |compose_scale - 1| > 0.1, as the reference tests it ----
    std::cout << "Compositing..." << std::endl;
    t = now();
    double compose_scale = 1.0;
    if (cfg_.compose_megapix > 0) compose_scale = std::min(1.0, std::sqrt(cfg_.compose_megapix * 1e6 / ((double)W * H)));
    const double compose_work_aspect = compose_scale / work_scale;     // :1113
    const bool compose_resized = std::abs(compose_scale - 1) > 1e-1;
    const int cW = compose_resized ? (int)std::nearbyint(W * compose_scale) : W, cH = compose_resized ? (int)std::nearbyint(H * compose_scale) : H;
    const float compose_warp_scale = warped_image_scale * static_cast<float>(compose_work_aspect);
    std::vector<MisPoint> corners(kept);
    std::vector<MisSize> sizes(kept);
    std::vector<std::array<float, 9>> Ks(kept), Rs(kept), cKs(kept);     // Ks: work-scale intrinsics (the seam step), cKs: the compositing loop's
    for (int k = 0; k < kept; k++) {
        const CameraParams& c = cameras[out.indices[k]];
        CameraParams cc = c;
        cc.focal *= compose_work_aspect; cc.ppx *= compose_work_aspect; cc.ppy *= compose_work_aspect;
        Mat3<float> K = c.K().cast<float>(), R = c.R.cast<float>(), cK = cc.K().cast<float>();
        std::copy(K.m.begin(), K.m.end(), Ks[k].begin());
        std::copy(R.m.begin(), R.m.end(), Rs[k].begin());
        std::copy(cK.m.begin(), cK.m.end(), cKs[k].begin());
        MisRect roi;
        // (a roi that scans every source pixel: the batch entry runs that on the device)
        if ((MIS_WARP_ROI_IS_FULL_SCAN(kind) ? mis_warper_roi_batch(ctx_, kind, compose_warp_scale, cW, cH, 1, cKs[k].data(), Rs[k].data(), &roi)
                                       : mis_warper_roi(kind, compose_warp_scale, cW, cH, cKs[k].data(), Rs[k].data(), &roi)) != MIS_OK)
            throw std::runtime_error("mis_warper_roi failed: frame " + std::to_string(out.indices[k]) + " has no " + (scans ? std::string("affine") : cfg_.warp_type) + " warp roi");
        corners[k] = {roi.x, roi.y};
        sizes[k] = {roi.width, roi.height};
    }
    MisRect pano;
    mis_result_roi(corners.data(), sizes.data(), kept, &pano);
    out.pano_tl = {pano.x, pano.y}; out.warp_scale = compose_warp_scale; out.warp_kind = kind;
    if (timelapse) timelapse->dst_roi = tl_type == MIS_TIMELAPSE_CROP ? resultRoiIntersection(corners, sizes) : pano;     // :1197
    int btype = 0, bands = 0;
    float sharp = 0;
    MisBlender* blender = nullptr;
    if (!timelapse) {
        mis_blend_config(cfg_.blend_type, cfg_.blend_strength, pano.width, pano.height, &btype, &bands, &sharp);
        if (btype == MIS_BLEND_MULTI_BAND) std::cout << "Multi-band blender, number of bands: " << bands << std::endl;
        else if (btype == MIS_BLEND_FEATHER) std::cout << "Feather blender, sharpness: " << sharp << std::endl;
        check(mis_blender_create(ctx_, btype, bands, sharp, &blender), "mis_blender_create");
        check(mis_blender_prepare(blender, corners.data(), sizes.data(), kept), "mis_blender_prepare");
    }
    // ---- seam-scale pass (:604-622 resize, :973-990 warp, :1002-1023 exposure compensator, :1029-1065 seam finder) ----
    const bool seam_step = cfg_.expos_comp_type != "no" || seam.find;
    MisCompensator* compensator = nullptr;
    std::vector<MisImage> masks_warped(kept);
    if (seam_step) {
        const double seam_scale = std::min(1.0, std::sqrt(cfg_.seam_megapix * 1e6 / ((double)W * H)));
        const float swa = (float)(seam_scale / work_scale);   // seam_work_aspect (:607)
        const float seam_warp_scale = warped_image_scale * swa;
        std::vector<MisImage> images_warped(kept);
        std::vector<MisPoint> seam_corners(kept);
        for (int k = 0; k < kept; k++) {
            MisImage full = view(frames[out.indices[k]]), img{};
            if (seam_scale < 1.0) check(mis_resize_linear_exact(ctx_, &full, 0, 0, seam_scale, seam_scale, &img), "mis_resize_linear_exact");
            else img = full;
            std::array<float, 9> Ks_ = Ks[k];
            Ks_[0] *= swa; Ks_[2] *= swa; Ks_[4] *= swa; Ks_[5] *= swa;
            check(mis_warper_warp(ctx_, kind, &img, seam_warp_scale, Ks_.data(), Rs[k].data(), MIS_INTER_LINEAR, MIS_BORDER_REFLECT, &images_warped[k], &seam_corners[k]),
                  "mis_warper_warp (seam scale)");
            std::vector<uint8_t> ones((size_t)img.width * img.height, 255);
            MisImage m{ones.data(), img.width, img.height, 1, (size_t)img.width, MIS_U8, MIS_MEM_HOST};
            MisPoint tl;
            check(mis_warper_warp(ctx_, kind, &m, seam_warp_scale, Ks_.data(), Rs[k].data(), MIS_INTER_NEAREST, MIS_BORDER_CONSTANT, &masks_warped[k], &tl),
                  "mis_warper_warp (seam-scale mask)");
            if (seam_scale < 1.0) mis_image_free(ctx_, &img);
        }
        if (expos_kind != MIS_EXPOS_NO) {
            MisCompensatorParams cp;
            mis_compensator_default_params(&cp);      // 64 x 64 blocks, 2 filtering passes (:1014-1016)
            cp.type = expos_kind;
            cp.nr_feeds = cfg_.expos_comp_nr_feeds;
            check(mis_compensator_create_ex(ctx_, &cp, &compensator), "mis_compensator_create_ex");
            check(mis_compensator_feed(compensator, seam_corners.data(), images_warped.data(), masks_warped.data(), kept), "mis_compensator_feed");
        }
        if (seam.find) check(seam.find(ctx_, seam_corners.data(), images_warped.data(), masks_warped.data(), kept), seam.what);
        for (auto& im : images_warped) mis_image_free(ctx_, &im);
    }
    if (timelapse) {
        // ---- the timelapser as the sink (:1194-1215): no blender, one registered frame per kept image ----
        for (auto& m : masks_warped) if (m.data) mis_image_free(ctx_, &m);      // the seam-scale masks fed the compensator; nothing else reads them
        const MisRect dr = timelapse->dst_roi;
        timelapse->frames.assign(kept, HostImage{dr.width, dr.height, 3, {}});
        for (auto& f : timelapse->frames) f.data.resize((size_t)dr.width * dr.height * 3);
        std::vector<MisImage> srcs(kept);
        for (int k = 0; k < kept; k++) {
            MisImage full = view(frames[out.indices[k]]);
            if (compose_resized) { srcs[k] = MisImage{}; check(mis_resize_linear_exact(ctx_, &full, 0, 0, compose_scale, compose_scale, &srcs[k]), "mis_resize_linear_exact (compose scale)"); }
            else srcs[k] = full;
        }
        auto free_srcs = [&]() { if (compose_resized) for (auto& s : srcs) mis_image_free(ctx_, &s); };
        if (expos_kind == MIS_EXPOS_NO || expos_kind == MIS_EXPOS_GAIN || expos_kind == MIS_EXPOS_CHANNELS) {
            // scalar gains: warp -> gains -> canvas -> 8U of all frames in one launch per 16 frames
            std::vector<double> gains((size_t)kept * 3);
            for (int k = 0; compensator && k < kept; k++) check(mis_compensator_gains(compensator, k, &gains[3 * (size_t)k]), "mis_compensator_gains");
            std::vector<float> Kf((size_t)kept * 9), Rf((size_t)kept * 9);
            std::vector<MisRect> rois(kept);
            std::vector<MisImage> dsts(kept);
            for (int k = 0; k < kept; k++) {
                std::copy(cKs[k].begin(), cKs[k].end(), Kf.begin() + 9 * (size_t)k);
                std::copy(Rs[k].begin(), Rs[k].end(), Rf.begin() + 9 * (size_t)k);
                rois[k] = {corners[k].x, corners[k].y, sizes[k].width, sizes[k].height};
                dsts[k] = view(timelapse->frames[k]);
            }
            const int rc = mis_timelapse_warp_batch(ctx_, kind, srcs.data(), kept, compose_warp_scale, Kf.data(), Rf.data(), rois.data(), &dr, compensator ? gains.data() : nullptr,
                                                    dsts.data(), MIS_U8);
            free_srcs();
            if (compensator) mis_compensator_destroy(compensator);
            check(rc, "mis_timelapse_warp_batch");
        } else {
            // a gain map per frame: the warped frame is stored, multiplied, placed and clamped, frame by frame
            Timelapser timelapser(ctx_, cfg_.timelapse_type);
            timelapser.initialize(corners, sizes);
            for (int k = 0; k < kept; k++) {
                MisImage img_warped_s{}, mask_warped{};
                MisPoint tl;
                check(mis_warper_warp_fused(ctx_, kind, &srcs[k], compose_warp_scale, cKs[k].data(), Rs[k].data(), &img_warped_s, &mask_warped, &tl), "mis_warper_warp_fused");
                check(mis_compensator_apply(compensator, k, &img_warped_s), "mis_compensator_apply");   // :1162
                const std::vector<int16_t>& dst = timelapser.process(img_warped_s, tl);                  // :1203-1204
                mis_image_free(ctx_, &img_warped_s);
                mis_image_free(ctx_, &mask_warped);
                for (size_t i = 0; i < dst.size(); i++) timelapse->frames[k].data[i] = (uint8_t)std::clamp<int>(dst[i], 0, 255);     // :1214
            }
            free_srcs();
            mis_compensator_destroy(compensator);
        }
        out.t_compositing = now() - t;
        std::cout << "Compositing, time: " << out.t_compositing << " sec" << std::endl;
        return out;
    }
    for (int k = 0; k < kept; k++) {
        std::cout << "Compositing image #" << out.indices[k] + 1 << std::endl;
        MisImage full = view(frames[out.indices[k]]), src{}, img_warped_s{}, mask_warped{};
        if (compose_resized) check(mis_resize_linear_exact(ctx_, &full, 0, 0, compose_scale, compose_scale, &src), "mis_resize_linear_exact (compose scale)");
        else src = full;
        MisPoint tl;
        check(mis_warper_warp_fused(ctx_, kind, &src, compose_warp_scale, cKs[k].data(), Rs[k].data(), &img_warped_s, &mask_warped, &tl), "mis_warper_warp_fused");
        if (compose_resized) mis_image_free(ctx_, &src);
        if (compensator) check(mis_compensator_apply(compensator, k, &img_warped_s), "mis_compensator_apply");   // :1162
        if (seam_step) {
            check(mis_seam_mask_apply(ctx_, &masks_warped[k], &mask_warped), "mis_seam_mask_apply");                // :1169-1171
            mis_image_free(ctx_, &masks_warped[k]);
        }
        check(mis_blender_feed(blender, &img_warped_s, &mask_warped, tl), "mis_blender_feed");
        mis_image_free(ctx_, &img_warped_s);
        mis_image_free(ctx_, &mask_warped);
    }
    if (compensator) mis_compensator_destroy(compensator);
    std::vector<int16_t> res16((size_t)pano.width * pano.height * 3);
    out.mask.width = pano.width; out.mask.height = pano.height; out.mask.channels = 1;
    out.mask.data.resize((size_t)pano.width * pano.height);
    MisImage result{res16.data(), pano.width, pano.height, 3, (size_t)pano.width * 6, MIS_S16, MIS_MEM_HOST};
    MisImage result_mask{out.mask.data.data(), pano.width, pano.height, 1, (size_t)pano.width, MIS_U8, MIS_MEM_HOST};
    check(mis_blender_blend(blender, &result, &result_mask), "mis_blender_blend");
    mis_blender_destroy(blender);
    out.t_compositing = now() - t;
    std::cout << "Compositing, time: " << out.t_compositing << " sec" << std::endl;
    // imwrite converts the 16S result with saturate_cast<uchar>
    out.pano.width = pano.width; out.pano.height = pano.height; out.pano.channels = 3;
    out.pano.data.resize(res16.size());
    for (size_t i = 0; i < res16.size(); i++) out.pano.data[i] = (uint8_t)std::clamp<int>(res16[i], 0, 255);
    return out;
}

HostImage renderView(MisContext* ctx, const StitchResult& result, const float K[9], const float R[9], int width, int height) {
    if (width <= 0 || height <= 0) throw std::runtime_error("renderView: the view size must be positive");
    HostImage view;
    view.width = width; view.height = height; view.channels = 3;
    view.data.resize((size_t)width * height * 3);
    const MisImage src{const_cast<uint8_t*>(result.pano.data.data()), result.pano.width, result.pano.height, 3, (size_t)result.pano.width * 3, MIS_U8, MIS_MEM_HOST};
    MisImage dst{view.data.data(), width, height, 3, (size_t)width * 3, MIS_U8, MIS_MEM_HOST};
    if (mis_warper_warp_backward(ctx, result.warp_kind, &src, result.pano_tl, result.warp_scale, K, R, MIS_INTER_LINEAR, MIS_BORDER_CONSTANT, width, height, &dst, nullptr) != MIS_OK)
        throw std::runtime_error(std::string("mis_warper_warp_backward failed: ") + mis_last_error(ctx));
    return view;
}

}  // namespace mis
