// job_core.cpp -- see job_core.hpp.
#include "job_core.hpp"
#include <algorithm>
#include <numeric>

namespace mis {

static float median_focal(const std::vector<CameraParams>& cams, const std::vector<int>& idx) {
    // image_stitching.cpp:884-895: median of the kept cameras' focals (mean of the middle two for an even count), as float
    std::vector<double> f;
    for (int i : idx) f.push_back(cams[i].focal);
    std::sort(f.begin(), f.end());
    return f.size() % 2 == 1 ? static_cast<float>(f[f.size() / 2]) : static_cast<float>(f[f.size() / 2 - 1] + f[f.size() / 2]) * 0.5f;
}

void JobCore::Hook::fire(void* self_) {
    Hook* self = static_cast<Hook*>(self_);
    self->ran_ = true;
    try { self->body_(); } catch (const std::exception& e) { self->error_ = e.what(); }
}

void JobCore::Hook::arm(std::function<void()> body) {
    body_ = std::move(body);
    ran_ = false;
    error_.clear();
}

void JobCore::Hook::finish() {
    if (!ran_) fire(this);
    if (!error_.empty()) throw std::runtime_error(error_);
}

void JobCore::check(MisContext* c, int rc, const char* what) const {
    if (rc != MIS_OK) throw std::runtime_error(std::string(what) + " failed" + where_ + ": " + mis_last_error(c));
}

JobCore::JobCore(const char* who, std::string where, int device, void* main_stream, int width, int height, const std::vector<CameraParams>& cameras,
                 const StitchConfig& cfg)
    : w_(width), h_(height), n_((int)cameras.size()), wg_(work_geometry(cfg, width, height)), cams_(cameras), cfg_(cfg), everyone_(n_), mstream_(main_stream),
      where_(std::move(where)) {
    std::iota(everyone_.begin(), everyone_.end(), 0);
    if (wg_.scale != 1.0) {
        for (auto& c : cams_) { c.focal *= wg_.scale; c.ppx *= wg_.scale; c.ppy *= wg_.scale; }
        compose_work_aspect_ = 1.0 / wg_.scale;
    }
    try {
        if (cfg_.features_type != "orb" || cfg_.ba_cost_func != "no" || cfg_.expos_comp_type != "no" || cfg_.seam_find_type != "no")
            throw std::runtime_error(std::string(who) + " runs the hot path (ORB, supplied cameras, no seam-scale step); use mis::Stitcher for the other options");
        if (cfg_.timelapse)     // the jobs end in the blender; the timelapser is another sink
            throw std::runtime_error(std::string(who) + " blends a panorama; timelapse = true (the timelapse output) is mis::Stitcher::timelapse");
        if (mode_is_scans(cfg_.mode))       // the jobs speculate the composition from supplied cameras; the scans mode has none
            throw std::runtime_error(std::string(who) + " runs supplied cameras only; the scans mode is mis::Stitcher's");
        if (estimator_is_homography(cfg_.estimator_type))      // likewise: an estimator's cameras exist only after the matcher has returned (a name that is no estimator is refused as mis::Stitcher refuses it)
            throw std::runtime_error(std::string(who) + " runs supplied cameras only; estimator_type '" + cfg_.estimator_type + "' is mis::Stitcher's");
        kind_ = warp_kind(cfg_.warp_type);
        check_range_width(cfg_.range_width);
        model_ = matcher_model(cfg_.matcher_type, cfg_.range_width);
        if (mis_context_create(device, mstream_, &ctx_) != MIS_OK) throw std::runtime_error("mis_context_create failed: no HIP device (there is no CPU fallback)");
        check(ctx_, mis_stream_create(device, 0, &cstream_), "mis_stream_create");
        if (mis_context_create(device, cstream_, &cctx_) != MIS_OK) throw std::runtime_error("mis_context_create (compose stream) failed");
        MisOrbParams op;
        mis_orb_default_params(&op);
        check(ctx_, mis_orb_create(ctx_, &op, wg_.width, wg_.height, &orb_), "mis_orb_create");
    } catch (...) {
        release();
        throw;
    }
    Ks_.resize((size_t)n_ * 9); Rs_.resize((size_t)n_ * 9);
    for (int i = 0; i < n_; i++) {
        CameraParams cc = cams_[i];
        if (compose_work_aspect_ != 1.0) { cc.focal *= compose_work_aspect_; cc.ppx *= compose_work_aspect_; cc.ppy *= compose_work_aspect_; }
        const Mat3<float> K = cc.K().cast<float>(), R = cams_[i].R.cast<float>();
        std::copy(K.m.begin(), K.m.end(), Ks_.begin() + 9 * i);
        std::copy(R.m.begin(), R.m.end(), Rs_.begin() + 9 * i);
    }
    // A plane warp refuses the roi of a frame turned behind the panorama plane, even one the pruning will drop: when the all-frames
    // rois fail, the jobs compose the kept set after pruning instead of speculating (only a refused roi among the kept frames is an
    // error).  Cameras only, so it is decided here; the spherical roi is never refused.
    if (kind_ != MIS_WARP_SPHERICAL) {
        const float scale = warp_scale(everyone_);
        MisRect r;
        // (a roi that scans every source pixel: the batch entry runs that on the device, one call for all frames)
        if (MIS_WARP_ROI_IS_FULL_SCAN(kind_)) {
            std::vector<MisRect> rr((size_t)n_);
            spec_ok_ = n_ == 0 || mis_warper_roi_batch(cctx_, kind_, scale, w_, h_, n_, Ks_.data(), Rs_.data(), rr.data()) == MIS_OK;
        } else
            for (int i = 0; i < n_ && spec_ok_; i++) spec_ok_ = mis_warper_roi(kind_, scale, w_, h_, &Ks_[9 * i], &Rs_[9 * i], &r) == MIS_OK;
    }
}

JobCore::~JobCore() { release(); }

float JobCore::warp_scale(const std::vector<int>& idx) const {
    const float scale = median_focal(cams_, idx);
    return compose_work_aspect_ != 1.0 ? scale * static_cast<float>(compose_work_aspect_) : scale;
}

const MisImage* JobCore::work_frames(const std::vector<MisImage>& frames) {
    if (wg_.scale == 1.0 || frames.empty()) return frames.data();
    if (work_.size() < frames.size()) work_.resize(frames.size(), MisImage{});
    check(ctx_, mis_resize_linear_exact_batch(ctx_, frames.data(), (int)frames.size(), 0, 0, wg_.scale, wg_.scale, work_.data()), "mis_resize_linear_exact_batch");
    return work_.data();
}

// a context is destroyed before its stream (its destruction synchronises that stream)
void JobCore::release() {
    if (cctx_) mis_context_synchronize(cctx_);
    if (ctx_) mis_context_synchronize(ctx_);
    if (!pairwise_.empty()) mis_matches_free(pairwise_.data(), (int)pairwise_.size());
    if (ctx_) for (auto& im : work_) mis_image_free(ctx_, &im);
    if (blender_) mis_blender_destroy(blender_);
    if (orb_) mis_orb_destroy(orb_);
    if (cctx_) mis_context_destroy(cctx_);
    if (ctx_) mis_context_destroy(ctx_);
    if (cstream_) mis_stream_destroy(cstream_);
    if (mstream_) mis_stream_destroy(mstream_);
}

void JobCore::synchronize() {
    check(ctx_, mis_context_synchronize(ctx_), "mis_context_synchronize");
    check(cctx_, mis_context_synchronize(cctx_), "mis_context_synchronize (compose)");
}

JobCore::Compose JobCore::prepare(const std::vector<int>& idx) {
    const int m = (int)idx.size();
    const float scale = warp_scale(idx);
    std::vector<float> Ks((size_t)m * 9), Rs((size_t)m * 9);
    for (int k = 0; k < m; k++) {
        std::copy(Ks_.begin() + 9 * idx[k], Ks_.begin() + 9 * idx[k] + 9, Ks.begin() + 9 * k);
        std::copy(Rs_.begin() + 9 * idx[k], Rs_.begin() + 9 * idx[k] + 9, Rs.begin() + 9 * k);
    }
    rois_.assign(m, MisRect{});
    check(cctx_, mis_warper_roi_batch(cctx_, kind_, scale, w_, h_, m, Ks.data(), Rs.data(), rois_.data()), "mis_warper_roi_batch");
    std::vector<MisPoint> corners(m);
    std::vector<MisSize> sizes(m);
    for (int k = 0; k < m; k++) { corners[k] = {rois_[k].x, rois_[k].y}; sizes[k] = {rois_[k].width, rois_[k].height}; }
    Compose c;
    check(cctx_, mis_result_roi(corners.data(), sizes.data(), m, &c.pano), "mis_result_roi");
    check(cctx_, mis_blend_config(cfg_.blend_type, cfg_.blend_strength, c.pano.width, c.pano.height, &c.type, &c.bands, &c.sharp), "mis_blend_config");
    if (!blender_ || c.type != key_.type || c.bands != key_.bands || c.sharp != key_.sharp) {      // band count / sharpness are creation parameters
        if (blender_) { mis_blender_destroy(blender_); blender_ = nullptr; }
        check(cctx_, mis_blender_create(cctx_, c.type, c.bands, c.sharp, &blender_), "mis_blender_create");
    }
    key_ = c;
    check(cctx_, mis_blender_prepare(blender_, corners.data(), sizes.data(), m), "mis_blender_prepare");
    return c;
}

void JobCore::fence_knn() {
    const int rc = mis_match_knn_fence(ctx_, cstream_, mis_match_sequence(ctx_), 0);
    if (rc < 0) check(ctx_, rc, "mis_match_knn_fence");
}

void JobCore::arm_knn_ahead() {
    check(ctx_, mis_orb_arm_knn_ahead(orb_, n_, nullptr, cfg_.range_width, 0, 1), "mis_orb_arm_knn_ahead");
}

void JobCore::compose(const std::vector<MisImage>& frames, const std::vector<int>& frame_ids, const std::vector<int>& idx) {
    std::vector<MisImage> fr;
    std::vector<float> Ks, Rs;
    std::vector<MisRect> rois;
    for (size_t q = 0; q < frame_ids.size(); q++) {
        const auto it = std::find(idx.begin(), idx.end(), frame_ids[q]);
        if (it == idx.end()) continue;
        fr.push_back(frames[q]);
        Ks.insert(Ks.end(), Ks_.begin() + 9 * frame_ids[q], Ks_.begin() + 9 * frame_ids[q] + 9);
        Rs.insert(Rs.end(), Rs_.begin() + 9 * frame_ids[q], Rs_.begin() + 9 * frame_ids[q] + 9);
        rois.push_back(rois_[it - idx.begin()]);
    }
    if (fr.empty()) return;     // every frame of a rank was pruned: nothing to warp or feed (the exchanges around still run)
    check(cctx_, mis_compose_frames_kind(blender_, kind_, fr.data(), (int)fr.size(), warp_scale(idx), Ks.data(), Rs.data(), rois.data()),
          "mis_compose_frames_kind");
}

MisMatchParams JobCore::reset_matches() {
    if (!pairwise_.empty()) { mis_matches_free(pairwise_.data(), (int)pairwise_.size()); pairwise_.clear(); }
    pairwise_.assign((size_t)n_ * n_, MisMatchesInfo{});
    return match_params(model_, cfg_.match_conf);
}

}  // namespace mis
