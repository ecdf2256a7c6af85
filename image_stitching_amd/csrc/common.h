// common.h -- internal declarations shared by the libmistitch.so translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "../../include/mistitch.h"

// per-context caches that outlive a call (grow-only device workspaces); freed with the context
struct MisWorkspace {
    virtual ~MisWorkspace() {}
};

struct MisContext {
    int device = 0;
    int num_cu = 256;   // compute units of the device (persistent kernels size their grids from it)
    MisWorkspace* match_ws = nullptr;
    MisWorkspace* resize_ws = nullptr;    // device coefficient tables of mis_resize_linear_exact_batch, one per geometry (imgops.hip)
    // recycled device blocks (size, pointer): feature sets are allocated and released every frame, and a
    // hipFree would synchronise the whole device each time
    std::vector<std::pair<size_t, void*>> pool;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // grow-only scratch for host<->device staging
    void* stage = nullptr;
    size_t stage_bytes = 0;
    // The context's two auxiliary streams (non-blocking, created on first use).  Every stage that forks work off the
    // context's stream takes them from here -- the SIFT finder's lanes, then the matcher's side chains -- so a job owns
    // four streams in all (this one, the two auxiliaries, the caller's compose stream): one per hardware queue of the
    // runtime's default of four, whichever stage is running.
    hipStream_t aux[2] = {nullptr, nullptr};
    // pinned, device-visible host block of mis_warp_roi_batch (jobs in, extremes out)
    void* roi_pinned = nullptr;
    size_t roi_pinned_bytes = 0;
    void* host_stage = nullptr;      // pinned host scratch of host-logic entries (mis_seam_dp): grow-only, see mis_host_stage
    size_t host_stage_bytes = 0;
    // the last mis_seam_graphcut call's counts (seam_gc.hip): pairs, levels, grid nodes, the round-set cap, global relabels, relabel
    // sweeps, then the round sets of every level
    std::vector<int> gc_stats;
    // the last device crop's counts (crop.hip): kernel launches, doubling rounds, border pixels, the chosen contour's points
    std::vector<int> crop_stats;
};

int mis_set_error(MisContext* ctx, int code, const char* fmt, ...);
int mis_host_stage(MisContext* ctx, size_t bytes, void** out);   // pinned scratch of at least `bytes` (valid until the next call)
int mis_dev_stage(MisContext* ctx, size_t bytes, void** out);    // the same in device memory
// (errs: the context that gets the error text when it is not ctx -- a block taken from another context's pool on a thread of its own)
int mis_pool_alloc(MisContext* ctx, size_t bytes, void** out, size_t* got, MisContext* errs = nullptr);
int mis_aux_stream(MisContext* ctx, int k, hipStream_t* out);   // k = 0, 1
void mis_pool_free(MisContext* ctx, void* p, size_t bytes);
// Feature blocks (features.hip): a feature set owns one device block from ctx's pool of recycled blocks, registered so that
// mis_features_free recycles it.  mis_feat_block_alloc gives a bare block (the SIFT finders lay out their own two regions);
// mis_feat_alloc lays out [keypoints][descriptors][count] for `cap` features, every region 256-byte aligned, the count one int
// on the device that the finder's kernels publish (mis_feat_count).
int mis_feat_block_alloc(MisContext* ctx, size_t bytes, void** out, MisContext* errs = nullptr);
struct MisFeatLayout { size_t desc_off, count_off, bytes; };
MisFeatLayout mis_feat_layout(int cap, int desc_cols, int desc_dtype);
int mis_feat_alloc(MisContext* ctx, int cap, int desc_cols, int desc_dtype, MisFeatures* f);
int* mis_feat_count(const MisFeatures* f, int cap);
// The Hamming 2-NN pass enqueued ahead of the matcher call (match.hip).  mis_knn_ahead_enqueue: the expansion and the 2-NN pass
// of the selected pairs (mask / range_width / rank / world as in mis_match_pairs_select) of a batch of n feature blocks whose
// keypoint counts are still on the device only -- block i holds at most caps[i] features and its finder publishes the count at
// counts[i] (device) --, on ctx's stream, planned from the capacities; it does nothing where the pass on the matrix cores does
// not apply.  mis_knn_ahead_confirm: the batch now has its counts on the host (feats[i].n): the next matcher call of ctx may
// adopt the pass.  mis_knn_ahead_drop: nobody will (owner != NULL: only if that block belongs to the pass).  Not adopting a
// pass is always correct: its results are read by no one.
int mis_knn_ahead_enqueue(MisContext* ctx, const MisFeatures* feats, int n, const int* caps, int* const* counts, const uint8_t* mask, int range_width,
                          int rank, int world);
void mis_knn_ahead_confirm(MisContext* ctx, const MisFeatures* feats, int n);
void mis_knn_ahead_drop(MisContext* ctx, const void* owner);

// DpSeamFinder::computeGradients of n 8UC3 device frames in one launch on ctx's stream (seam_grad.hip): gx / gy are f32 planes of
// the frame's size on the device, strides in bytes (the planes' multiples of 4).  Nothing is checked here: the entries do.
struct MisSeamGradJob { const uint8_t* src; size_t ss; float* gx; size_t gxs; float* gy; size_t gys; int w, h; };
int mis_seam_grad_enqueue(MisContext* ctx, const MisSeamGradJob* jobs, int n);

// the text mis_jpeg_last_error() returns to the calling thread (jpeg.hip): set by the context-free JPEG entries
void mis_jpeg_set_last_error(const char* text);

#define MIS_HIP(ctx, call)                                                                           \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return mis_set_error((ctx), MIS_E_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                                 __FILE__, __LINE__);                                                  \
    } while (0)

#define MIS_CHECK(ctx, cond, code, ...)                              \
    do {                                                             \
        if (!(cond)) return mis_set_error((ctx), (code), __VA_ARGS__); \
    } while (0)

static inline size_t mis_dtype_size(int dtype) { return dtype == MIS_U8 ? 1 : (dtype == MIS_S16 ? 2 : 4); }
static inline size_t mis_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Device view of a caller's image for the length of a scope: the caller's device pointer, or a staged device copy of a host
// buffer.  Whatever the view allocated and did not hand over in commit() is freed when it goes out of scope, after a wait for
// the context's stream, so an early return drops nothing.
struct DevView {
    void* data = nullptr;
    size_t stride = 0;
    DevView() = default;
    DevView(const DevView&) = delete;
    DevView& operator=(const DevView&) = delete;
    ~DevView();
    int read(MisContext* ctx, const MisImage* img);     // host images are uploaded
    // Output of the given geometry: the caller's device buffer, a device twin of a host buffer, or (data == NULL) a device
    // allocation entered into *img, which is the caller's only after commit(): without it *img goes back to what it was.
    int write(MisContext* ctx, MisImage* img, int width, int height, int channels, int dtype);
    int read_write(MisContext* ctx, MisImage* img);     // read(), and commit() copies a host image back
    int commit();                                       // copy a host output back and free its twin; hand a fresh allocation over
private:
    MisContext* ctx_ = nullptr;
    MisImage* out_ = nullptr;       // what commit() copies back to
    MisImage entry_{};              // *out_ before a fresh allocation was entered into it
    bool staged_ = false, fresh_ = false;
};

// A device block from the context's pool for the length of a scope.  It goes back to the pool on every way out, after a wait for
// the context's stream: an error path may leave work on the block in flight.  release() hands it back at once, without the wait,
// for a caller whose remaining work on the block is already enqueued: the pool's next user is ordered behind it on the stream.
struct PoolBlock {
    MisContext* ctx; void* p = nullptr; size_t got = 0;
    explicit PoolBlock(MisContext* c) : ctx(c) {}
    PoolBlock(const PoolBlock&) = delete;
    PoolBlock& operator=(const PoolBlock&) = delete;
    ~PoolBlock() { if (p) { hipStreamSynchronize(ctx->stream); release(); } }
    int alloc(size_t bytes) { const int rc = mis_pool_alloc(ctx, bytes, &p, &got); if (rc != MIS_OK) p = nullptr; return rc; }
    void release() { if (p) mis_pool_free(ctx, p, got); p = nullptr; }
};

// a HIP event that is destroyed with its scope
struct OwnedEvent {
    hipEvent_t ev = nullptr;
    OwnedEvent() = default; OwnedEvent(const OwnedEvent&) = delete;
    ~OwnedEvent() { if (ev) hipEventDestroy(ev); }
    hipError_t ready(unsigned flags = hipEventDisableTiming) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
};

