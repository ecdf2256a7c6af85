// job.hpp -- the hot path of the reference's main() (image_stitching/image_stitching.cpp:567-1228) as ONE job over frames that
// are already resident in HBM, in C++ over the C ABI of libmistitch: the flow bench.py times through
// image_stitching_amd/distributed.py (StitchJob.run on one rank), re-authored for a C++ host.
//
//   blender sizing + zeroing on the compose stream (cameras only)                      :1119-1140, :1175-1192
//   ORB of all frames in one batched call                                              :567-622
//   all-pairs matching; from the matcher's own hook (mis_match_on_enqueued: the calling thread is idle there)
//     the composition of ALL frames is enqueued on the compose stream behind the 2-NN pass (mis_match_knn_fence):
//     batched fused warp + feed (mis_compose_frames) and the collapse (mis_blender_blend)       :647-653, :1086-1228
//   pruning (myLeaveBiggestComponent); when a frame was dropped the composition is redone for the kept set      :215-278
// The result stays in HBM (MisImage with mem = MIS_MEM_DEVICE).  The main context runs on the null stream.  Contexts, finder,
// blender sizing and the warp + feed are mis::JobCore's (job_core.hpp), shared with mis::ShardedJob; this file is the flow.
#pragma once
#include <vector>
#include "job_core.hpp"

namespace mis {

class StitchJob : private JobCore {
public:
    StitchJob(int device, int width, int height, const std::vector<CameraParams>& cameras, const StitchConfig& cfg = StitchConfig());
    ~StitchJob();
    // frames: n device-resident 8UC3 images of the job's size, complete on the main context's stream (or synchronised)
    JobOutput run(const std::vector<MisImage>& frames);
    using JobCore::synchronize;
    MisContext* context() const { return ctx_; }           // features + matcher
    MisContext* compose_context() const { return cctx_; }  // warp + blend (own stream)

private:
    void finalize();

    MisImage pano_{}, mask_{};
    Hook prep_, match_;     // the finder's hook (mis_orb_on_enqueued): prepare() under the feature stage; the matcher's: the composition
};

}  // namespace mis
