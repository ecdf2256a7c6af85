// job_core.hpp -- what the two C++ jobs over frames in HBM share: mis::StitchJob (job.hpp, one process) and mis::ShardedJob
// (sharded_job.hpp, N ranks).  The core holds the contexts and streams, the ORB finder, the cameras as the warper takes them, the
// blender with its sizing (prepare) and the batched warp + feed (compose), and keeps the library hooks' bookkeeping.  The flows
// themselves -- matcher call, exchanges, finalise -- stay in the two jobs.
#pragma once
#include <functional>
#include <string>
#include <vector>
#include "stitcher.hpp"

namespace mis {

// What a job's run returns.  Every field but `matches` is filled by both jobs, on every rank.
struct JobOutput {
    std::vector<int> indices;         // frames kept by the pruning
    std::vector<double> confidence;   // n x n (the sharded job: summed over the ranks)
    std::vector<int> num_features;    // all n frames
    MisImage pano{}, mask{};          // device: 16SC3 panorama and 8U mask, owned by the job (valid until its next run)
    int num_bands = 0, pano_width = 0, pano_height = 0;
    bool speculation_kept = false;    // the composition enqueued under the matcher was the final one
    // mis::StitchJob: n x n (host arrays owned by the library; released by the job's next run).  mis::ShardedJob: empty (a rank
    // holds only the pairs it matched)
    std::vector<MisMatchesInfo> matches;
};

class JobCore {
protected:
    struct Compose { int type = 0, bands = 0; float sharp = 0; MisRect pano{}; };

    // One of the library's "on enqueued" hooks.  arm() before the call, hand the library &Hook::fire with the hook as user data,
    // finish() after it: the body runs exactly once, inside the call or -- a call that returned before its hook -- from finish(),
    // and an exception it throws (which must not cross the C ABI) is rethrown by finish().
    class Hook {
    public:
        static void fire(void* self);
        void arm(std::function<void()> body);
        void finish();
    private:
        std::function<void()> body_;
        bool ran_ = false;
        std::string error_;
    };

    // who: the job's name in the configuration error; where: appended to check()'s messages (" on rank r", or nothing).
    // main_stream: the main context's stream -- nullptr for the null stream, or one the job created with mis_stream_create, which
    // the core then owns.  The core creates the compose stream.
    JobCore(const char* who, std::string where, int device, void* main_stream, int width, int height, const std::vector<CameraParams>& cameras,
            const StitchConfig& cfg);
    ~JobCore();
    JobCore(const JobCore&) = delete;
    JobCore& operator=(const JobCore&) = delete;

    void check(MisContext* c, int rc, const char* what) const;
    void synchronize();
    // warpRoi of the frames `idx` at the scale of that set, panorama roi, blender sizing + prepare -- on the compose stream
    Compose prepare(const std::vector<int>& idx);
    // the compose stream queued behind the 2-NN pass of the matcher call in flight (from the matcher's hook)
    void fence_knn();
    // a job that matches its finder's own output next, on one rank: the next feature batch (of all n frames) enqueues the matcher's
    // 2-NN pass behind its kernels (mis_orb_arm_knn_ahead); the matcher call adopts it
    void arm_knn_ahead();
    // the frames at work scale (:589-603): resized in one launch into images the core keeps from its first run on (allocated by the
    // library then; an allocation per run would synchronise the device); the frames themselves when the work scale is 1
    const MisImage* work_frames(const std::vector<MisImage>& frames);
    // the warper's scale for the frames `idx`: median focal of their work-unit cameras times (float)compose_work_aspect (:884-895, :1116)
    float warp_scale(const std::vector<int>& idx) const;
    // batched fused warp + feed (rois_ from prepare(idx)) of the frames among `frame_ids` that are in `idx`; frames[q] is frame
    // frame_ids[q].  Both lists ascend, so the frames go in `idx` order.
    void compose(const std::vector<MisImage>& frames, const std::vector<int>& frame_ids, const std::vector<int>& idx);
    // the previous run's pair records released, n x n empty ones in their place; the matcher's parameters
    MisMatchParams reset_matches();

    int w_, h_, n_;
    WorkGeometry wg_;                 // work scale and work image size (features_[i].img_size, the finder's size)
    double compose_work_aspect_ = 1;  // compose_scale / work_scale with compose_scale = 1 (:1113)
    std::vector<CameraParams> cams_;  // in work units: focal, ppx, ppy times work_scale (:635-637)
    std::vector<MisImage> work_;      // work frames (device), kept between runs
    StitchConfig cfg_;
    std::vector<int> everyone_;       // 0 .. n-1
    int kind_ = MIS_WARP_SPHERICAL;   // the warper (cfg_.warp_type)
    int model_ = MIS_MATCH_HOMOGRAPHY;   // the matcher's motion model (cfg_.matcher_type): both are accepted
    bool spec_ok_ = true;             // warpRoi of ALL frames succeeds: the composition may be speculated (see JobCore::JobCore)
    void* mstream_ = nullptr;         // main stream (nullptr: the null stream): features, matcher, the feature all-gather
    void* cstream_ = nullptr;         // compose stream: warp, feed, blend (and the sharded job's blend exchange)
    MisContext* ctx_ = nullptr;
    MisContext* cctx_ = nullptr;
    MisOrb* orb_ = nullptr;
    MisBlender* blender_ = nullptr;
    Compose key_{};
    std::vector<float> Ks_, Rs_;      // n x 9 each (float, as main() hands them to the warper): the compositing loop's, intrinsics times compose_work_aspect (:1122-1125)
    std::vector<MisRect> rois_;       // of the frames of the current composition (position in idx)
    std::vector<MisMatchesInfo> pairwise_;

private:
    void release();
    std::string where_;
};

}  // namespace mis
