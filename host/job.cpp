// job.cpp -- see job.hpp.
#include "job.hpp"
#include <cstring>

namespace mis {

StitchJob::StitchJob(int device, int width, int height, const std::vector<CameraParams>& cameras, const StitchConfig& cfg)
    : JobCore("mis::StitchJob", "", device, nullptr, width, height, cameras, cfg) {}

StitchJob::~StitchJob() {
    mis_image_free(cctx_, &pano_);      // (synchronises the compose stream)
    mis_image_free(cctx_, &mask_);
}

void StitchJob::finalize() {
    // the result images are reused while the panorama keeps its size
    if (pano_.data && (pano_.width != key_.pano.width || pano_.height != key_.pano.height)) { mis_image_free(cctx_, &pano_); mis_image_free(cctx_, &mask_); pano_ = MisImage{}; mask_ = MisImage{}; }
    if (!pano_.data) { pano_ = MisImage{}; mask_ = MisImage{}; pano_.mem = mask_.mem = MIS_MEM_DEVICE; }
    check(cctx_, mis_blender_blend(blender_, &pano_, &mask_), "mis_blender_blend");
}

JobOutput StitchJob::run(const std::vector<MisImage>& frames) {
    if ((int)frames.size() != n_) throw std::runtime_error("StitchJob::run: one frame per camera");
    JobOutput out;
    // the compose stream is non-blocking: order it behind whatever produced the frames on the main context's stream
    check(cctx_, mis_context_wait(cctx_, ctx_), "mis_context_wait");
    // sizing + zeroing of the panorama pyramids depends on the cameras only: it runs from the finder's hook, once the feature batch is
    // enqueued (warpRoi ends in a synchronisation of the compose stream: in front of the features it kept the main stream idle)
    const MisImage* work = work_frames(frames);       // (:602, one launch on the main stream)
    prep_.arm([this] { if (spec_ok_) prepare(everyone_); });
    check(ctx_, mis_orb_on_enqueued(orb_, &Hook::fire, &prep_), "mis_orb_on_enqueued");
    arm_knn_ahead();        // the matcher below takes this batch as it is: its 2-NN pass goes in behind the batch
    // ---- features (:567-622) ----
    std::vector<MisFeatures> feats(n_);
    std::memset(feats.data(), 0, sizeof(MisFeatures) * n_);
    const int rc_f = mis_orb_detect_batch(orb_, work, n_, feats.data());
    mis_orb_on_enqueued(orb_, nullptr, nullptr);
    check(ctx_, rc_f, "mis_orb_detect_batch");
    prep_.finish();
    for (int i = 0; i < n_; i++) { feats[i].img_idx = i; out.num_features.push_back(feats[i].n); }
    // ---- matching (:647-653) with the speculative composition (all frames) enqueued from its hook ----
    const MisMatchParams mp = reset_matches();
    match_.arm([this, &frames] {
        if (!spec_ok_) return;      // a refused all-frames roi: the kept set is composed after the pruning
        fence_knn();
        compose(frames, everyone_, everyone_);
        finalize();
    });
    check(ctx_, mis_match_on_enqueued(ctx_, &Hook::fire, &match_), "mis_match_on_enqueued");
    const int rc = mis_match_pairs_model(ctx_, feats.data(), n_, &mp, model_, nullptr, cfg_.range_width, 0, 1, pairwise_.data());
    mis_match_on_enqueued(ctx_, nullptr, nullptr);
    for (auto& f : feats) mis_features_free(ctx_, &f);
    check(ctx_, rc, "mis_match_pairs_model");
    match_.finish();
    // ---- pruning (:215-278) ----
    out.confidence.resize((size_t)n_ * n_);
    for (int k = 0; k < n_ * n_; k++) out.confidence[k] = pairwise_[k].confidence;
    std::vector<int> idx(n_);
    int kept = 0;
    check(ctx_, mis_leave_biggest_component(pairwise_.data(), n_, cfg_.conf_thresh, idx.data(), &kept), "mis_leave_biggest_component");
    idx.resize(kept);
    if (kept < 2) throw std::runtime_error("Need more images");
    out.indices = idx;
    out.speculation_kept = spec_ok_ && kept == n_;
    if (!out.speculation_kept) {
        // a frame was dropped (or nothing was speculated): the panorama of the kept set (its own scale, roi and band count) replaces the speculated one
        prepare(idx);
        compose(frames, everyone_, idx);
        finalize();
    }
    check(cctx_, mis_context_synchronize(cctx_), "mis_context_synchronize (compose)");
    out.pano = pano_; out.mask = mask_;
    out.num_bands = key_.bands; out.pano_width = key_.pano.width; out.pano_height = key_.pano.height;
    out.matches = pairwise_;
    return out;
}

}  // namespace mis
