// sharded_job.hpp -- ONE panorama job spread over N ranks (one process per GPU) from a C++ host: the hot path of the reference's
// main() (image_stitching/image_stitching.cpp:567-1228) with the three exchange steps of SURVEY section 8(e), RCCL called directly.
//
//   stage                      partition                          exchange (mis::Communicator: RCCL, or host-staged for rehearsals)
//   detect + describe (:613)   frames, a contiguous block / rank  --
//   match + RANSAC (:653)      pairs dealt round-robin            all-gather of {counts, keypoints, descriptors} before it
//   pruning (:215-278)         replicated (n <= 64)               sum of the n x n confidence matrix (every pair has one owner)
//   warp + feed (:1154-1218)   frames (the same blocks)           --
//   blend (:1225)              column strips of the panorama      all-to-all of pyramid rectangles (rank -> strip owner), then an
//                                                                 all-gather of the finished strips
// The flow, the strip plan and the order of the f32 additions are those of image_stitching_amd/distributed.py (StitchJob with
// world_size > 1): the two hosts produce the same panorama byte for byte (tests/test_host_cpp.py).  The composition of a rank's own
// frames is speculated under the matcher (all frames kept is the rule) and redone for the kept set when the pruning drops one.
// Contexts, finder, blender sizing and the warp + feed are mis::JobCore's (job_core.hpp), shared with mis::StitchJob; this file is
// the sharded flow: the exchanges, the strip plan and the finalise.  Both streams are the job's own.
#pragma once
#include <memory>
#include <vector>
#include "comm.hpp"
#include "job_core.hpp"

namespace mis {

std::vector<int> frame_block(int n, int rank, int world);     // contiguous block of frame indices owned by `rank`

class ShardedJob : private JobCore {
public:
    // device: this rank's GPU; cameras: all n; comm: rank / world of the job
    ShardedJob(int device, int width, int height, const std::vector<CameraParams>& cameras, Communicator& comm, const StitchConfig& cfg = StitchConfig());
    ~ShardedJob();
    const std::vector<int>& my_frames() const { return mine_; }
    // frames: this rank's block (my_frames() order), device-resident 8UC3 of the job's size, complete on the main stream (or synchronised)
    JobOutput run(const std::vector<MisImage>& frames);
    using JobCore::synchronize;

private:
    struct DevBuf { void* p = nullptr; size_t bytes = 0; };
    void* reserve(DevBuf& b, size_t bytes);
    void prepare_multi_band(const std::vector<int>& idx);
    void exchange_finalize(const std::vector<int>& idx);

    Communicator& comm_;
    std::vector<int> mine_;
    DevBuf kps_send_, desc_send_, kps_all_, desc_all_, strip_mine_, strips_all_, pano_buf_, mask_buf_;
    std::vector<DevBuf> send_, recv_;
    MisImage pano_{}, mask_{};        // views of pano_buf_ / mask_buf_
    Hook prep_, match_;
};

}  // namespace mis
