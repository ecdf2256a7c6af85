/*
 * mistitch.h -- C ABI of libmistitch.so: the MI355X-native (gfx950 / HIP) stitching hot path.
 *
 * The reference (a1q123456/image_stitching) has no FFI of its own: image_stitching.h is an empty
 * stub (image_stitching/image_stitching.h:1-8) and the hot path is the set of cv::detail calls
 * main() makes.  Every entry point below replaces one of those call sites (cited per function);
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes, no C++ / torch types.
 *  - every function returns int: MIS_OK (0) or a negative MIS_E_* code; mis_last_error() gives text.
 *    Nothing throws across the ABI (the reference's OpenCV calls throw cv::Exception instead).
 *  - one MisContext = one HIP device + one stream; calls on a context are serialised by the caller.
 *  - image buffers are described by MisImage; `mem` says whether `data` is a host or a device
 *    pointer.  Device pointers are used in place (zero copy); host pointers are staged through HBM.
 *  - outputs whose `data` is NULL on entry are allocated by the library (in HBM) and released with
 *    mis_image_free(); otherwise they must have exactly the required size.
 *  - there is NO CPU fallback: without a HIP device mis_context_create() fails.
 */
#ifndef MISTITCH_H
#define MISTITCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIS_OK 0
#define MIS_E_INVALID (-1)     /* bad argument */
#define MIS_E_HIP (-2)         /* HIP runtime error */
#define MIS_E_NOMEM (-3)
#define MIS_E_OVERFLOW (-4)    /* an internal candidate buffer was too small for the input */
#define MIS_E_STATE (-5)       /* call order violated (e.g. feed before prepare) */
#define MIS_E_UNSUPPORTED (-6)
#define MIS_E_INTERNAL (-7)    /* a bounded iteration reached its cap (mis_seam_graphcut); nothing was written */
#define MIS_FENCE_TIMEOUT 1     /* mis_match_knn_fence only, not an error: the matcher call did not show up within the timeout, nothing was queued */

enum { MIS_MEM_HOST = 0, MIS_MEM_DEVICE = 1 };
enum { MIS_U8 = 0, MIS_S16 = 1, MIS_F32 = 2 };
enum { MIS_INTER_NEAREST = 0, MIS_INTER_LINEAR = 1 };          /* cv::INTER_NEAREST / INTER_LINEAR */
enum { MIS_BORDER_CONSTANT = 0, MIS_BORDER_REFLECT = 2 };       /* cv::BORDER_CONSTANT / BORDER_REFLECT */
/* the warper kinds of the reference's GPU branch (warp_type, image_stitching.cpp:917-969), its Mercator warper (:961-962) and its
 * fisheye (:941-942) and stereographic (:943-944) warpers; the float maps are those of OpenCV's Spherical / Cylindrical / Plane (T = 0) /
 * Mercator / Fisheye / Stereographic projectors, CPU path.  The first four have a separable backward ray (column and row tables, no
 * transcendental per pixel); the fisheye and stereographic maps are polar and are evaluated per output pixel.
 * Kinds 8 .. 11: the compressed-rectilinear (:945-948) and Panini (:953-956) warpers, one kind per (A, B) setting the reference offers
 * (the entries have no slot for the two parameters).  Their backward map is half separable: the horizontal angle depends on the
 * column only, the vertical one on the pixel.  Kinds 6, 7 and 12 are not assigned.
 * Kind 13: cv::detail::AffineWarper (:935-936), the plane warper with a translation.  Its `R` argument is the 3x3 homogeneous affine
 * H of AffineWarper::warp(src, K, H, ...): getRTfromHomogeneous splits it into the plane projector's R (H without its translation
 * column, transposed) and T = -(R T0).  Same separable tables as the plane, the two subtractions of T folded into them. */
enum { MIS_WARP_SPHERICAL = 0, MIS_WARP_CYLINDRICAL = 1, MIS_WARP_PLANE = 2, MIS_WARP_MERCATOR = 3, MIS_WARP_FISHEYE = 4, MIS_WARP_STEREOGRAPHIC = 5,
       MIS_WARP_COMPRESSED_PLANE_A2B1 = 8, MIS_WARP_COMPRESSED_PLANE_A15B1 = 9, MIS_WARP_PANINI_A2B1 = 10, MIS_WARP_PANINI_A15B1 = 11,
       MIS_WARP_AFFINE = 13 };
/* the kinds the library builds: every entry that takes a kind answers MIS_E_UNSUPPORTED ("unknown warp kind") for any other value */
#define MIS_WARP_KIND_IS_KNOWN(kind) (((kind) >= MIS_WARP_SPHERICAL && (kind) <= MIS_WARP_STEREOGRAPHIC) || \
                                      ((kind) >= MIS_WARP_COMPRESSED_PLANE_A2B1 && (kind) <= MIS_WARP_PANINI_A15B1) || (kind) == MIS_WARP_AFFINE)
/* the kinds whose warper has no detectResultRoi of its own: RotationWarperBase::detectResultRoi projects EVERY source pixel forward.
 * For these mis_warper_roi is O(width * height) on the host and mis_warper_roi_batch a grid-wide reduction on the device. */
#define MIS_WARP_ROI_IS_FULL_SCAN(kind) (((kind) >= MIS_WARP_MERCATOR && (kind) <= MIS_WARP_STEREOGRAPHIC) || \
                                        ((kind) >= MIS_WARP_COMPRESSED_PLANE_A2B1 && (kind) <= MIS_WARP_PANINI_A15B1))
enum { MIS_BLEND_NO = 0, MIS_BLEND_FEATHER = 1, MIS_BLEND_MULTI_BAND = 2 }; /* cv::detail::Blender::NO/FEATHER/MULTI_BAND */

typedef struct MisContext MisContext;
typedef struct MisOrb MisOrb;
typedef struct MisBlender MisBlender;

typedef struct { int x, y; } MisPoint;
typedef struct { int width, height; } MisSize;
typedef struct { int x, y, width, height; } MisRect;

typedef struct {
    void* data;
    int width, height, channels;
    size_t stride; /* bytes between rows */
    int dtype;     /* MIS_U8 / MIS_S16 / MIS_F32 */
    int mem;       /* MIS_MEM_HOST / MIS_MEM_DEVICE */
} MisImage;

/* ---------------------------------------------------------------- context ------------------- */
/* `stream` is a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL is the device's
 * default (null) stream.  All work of the context is enqueued on that stream. */
int mis_context_create(int device, void* stream, MisContext** out);
/* A non-blocking HIP stream for a second context on the same device (priority > 0: background work that yields
 * to the default-priority streams, < 0: urgent, 0: normal).  Pass the handle as `stream` to mis_context_create. */
int mis_stream_create(int device, int priority, void** stream);
int mis_stream_destroy(void* stream);
int mis_context_destroy(MisContext* ctx);
int mis_context_synchronize(MisContext* ctx);
/* Device-side ordering between two contexts of one device: work enqueued on `ctx` after this call starts only after everything
 * enqueued on `other` before it has finished (an event on other's stream; the host does not wait).  What the job does at its
 * entry between the stream that produced the frames and its compose stream. */
int mis_context_wait(MisContext* ctx, MisContext* other);
const char* mis_last_error(const MisContext* ctx);
const char* mis_version(void);
int mis_image_free(MisContext* ctx, MisImage* img);

/* ---------------------------------------------------------------- features ------------------ */
/* cv::KeyPoint as ImageFeatures::keypoints carries it (class_id is never read by the reference). */
typedef struct {
    float x, y, size, angle, response;
    int octave;
} MisKeyPoint;

/* ORB::create(nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel, WTA_K, scoreType,
 * patchSize, fastThreshold) -- replaces image_stitching/image_stitching.cpp:545.  Supported:
 * first_level 0, wta_k 2, score_type 0 (HARRIS_SCORE) or 1 (FAST_SCORE), patch_size 2 .. 40 except 31 (OpenCV's fixed
 * bit_pattern_31_), nlevels <= 16, at most 1920 keypoints in any level's budget (4000 at 1.2 x 8 levels gives level 0 869), and no
 * pyramid level of size zero: mis_orb_create (for the maximum size) and mis_orb_detect* (for the frame's) refuse the others with
 * MIS_E_UNSUPPORTED. */
typedef struct {
    int nfeatures;
    float scale_factor;
    int nlevels, edge_threshold, first_level, wta_k, score_type, patch_size, fast_threshold;
} MisOrbParams;

/* cv::detail::ImageFeatures (image_stitching.cpp:537): keypoints + descriptors stay in HBM. */
typedef struct {
    int img_idx;
    int img_w, img_h;
    int n;                    /* number of keypoints */
    MisKeyPoint* keypoints;   /* device, n entries */
    void* descriptors;        /* device, n x desc_cols of desc_dtype (ORB: 32 x u8) */
    int desc_cols, desc_dtype;
    void* owner_;             /* internal */
} MisFeatures;

void mis_orb_default_params(MisOrbParams* p); /* the reference's values (image_stitching.cpp:545) */
int mis_orb_create(MisContext* ctx, const MisOrbParams* p, int max_width, int max_height, MisOrb** out);
int mis_orb_destroy(MisOrb* orb);
/* computeImageFeatures(finder, img, features[i]) -- replaces image_stitching.cpp:613.
 * `bgr` is 8UC3 interleaved BGR.  Keypoints are ordered by level, then response (descending), y, x. */
int mis_orb_detect(MisOrb* orb, const MisImage* bgr, MisFeatures* out);
/* same, for a batch of frames of one size with a single host synchronisation at the end */
int mis_orb_detect_batch(MisOrb* orb, const MisImage* bgr, int n_images, MisFeatures* out);
/* One-shot hook of this finder's NEXT mis_orb_detect_batch call: fn(user) runs on the calling thread once the batch's device work
 * is enqueued and before the call waits for it (fn = NULL clears a pending hook).  The job sizes its blender there (warpRoi of all
 * cameras: a kernel and a synchronisation on the compose stream), under the feature stage instead of in front of it. */
int mis_orb_on_enqueued(MisOrb* orb, void (*fn)(void*), void* user);
/* One-shot arm of this finder's NEXT mis_orb_detect_batch call, for a batch of n frames that the matcher of the finder's context
 * will match with this selection (mask: n x n or NULL, range_width, rank, world: as in mis_match_pairs_select; the mask is copied).
 * The batch then enqueues the matcher's descriptor expansion and Hamming 2-NN pass of the selected pairs behind its own kernels, on
 * the context's stream, while the keypoint counts are still on the device -- the device no longer idles while the host fetches
 * the counts, returns and enters the matcher.  The next matcher call of that context ADOPTS the pass when its feature list is
 * exactly the batch's output (the same MisFeatures, unmodified, in the same order), its selection is the armed one, world is 1
 * and every frame has between 1 and 8192 keypoints; it then runs its ratio test and RANSAC chains on the pass's results.  In every
 * other case -- another list, order or selection, an empty frame, a batch of another size or of more than 64 frames, blocks that
 * hold more than 8192 features, an error or overflow in the batch, a
 * feature set of the batch freed, another batch in between -- the pass is dropped and the matcher call runs its own: ignoring
 * the pass is always correct, and the results are the same either way.  n <= 0 disarms. */
int mis_orb_arm_knn_ahead(MisOrb* orb, int n, const uint8_t* mask, int range_width, int rank, int world);
int mis_features_download(MisContext* ctx, const MisFeatures* f, MisKeyPoint* kps_host, void* desc_host);
/* wrap caller-provided (host) keypoints/descriptors as device-resident features */
int mis_features_upload(MisContext* ctx, int img_w, int img_h, int n, const MisKeyPoint* kps_host,
                        const void* desc_host, int desc_cols, int desc_dtype, MisFeatures* out);
int mis_features_free(MisContext* ctx, MisFeatures* f);
/* m feature sets into two dense device arrays (frame i at kps_dst + i * cap * 24 and desc_dst + i * cap * row_bytes, tails
 * zeroed): the send buffers of the descriptor all-gather of a sharded job; device-to-device, no host copy */
int mis_features_pack(MisContext* ctx, const MisFeatures* feats, int m, int cap, int row_bytes, void* kps_dst, void* desc_dst);
/* 2-D device-to-device copy on the context's stream (a rank's finished column strip into the assembled panorama) */
int mis_copy_2d(MisContext* ctx, void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width_bytes, size_t height);
/* stage intermediates of the last mis_orb_detect (host copies, for parity tests):
 * which = 0 gray level (tight w*h), 1 NMS-surviving FAST score map, 2 blurred bordered level */
int mis_orb_debug_level(MisOrb* orb, int level, int which, uint8_t* host_out, int* width, int* height);

/* ---------------------------------------------------------------- matching ------------------ */
/* BestOf2NearestMatcher(try_cuda, match_conf, num_matches_thresh1 = 6, num_matches_thresh2 = 6)
 * -- replaces image_stitching.cpp:647; findHomography defaults (RANSAC, 3.0, 2000, 0.995). */
typedef struct {
    float match_conf;
    int num_matches_thresh1, num_matches_thresh2;
    double ransac_thresh;
    int max_iters;
    double confidence;
} MisMatchParams;

typedef struct { int query_idx, train_idx, img_idx; float distance; } MisDMatch; /* cv::DMatch */

/* cv::detail::MatchesInfo (image_stitching.cpp:642); arrays are host memory owned by the library */
typedef struct {
    int src_img_idx, dst_img_idx;
    int n_matches;
    MisDMatch* matches;
    uint8_t* inliers_mask; /* n_matches entries, NULL when RANSAC did not run */
    int num_inliers;
    int has_H;
    double H[9];
    double confidence;
} MisMatchesInfo;

void mis_match_default_params(MisMatchParams* p);
/* (*matcher)(features, pairwise_matches) -- replaces image_stitching.cpp:653.  `out` is an n*n
 * row-major array (diagonal entries stay default-initialised, (j,i) mirrors (i,j) with H^-1). */
int mis_match_all_pairs(MisContext* ctx, const MisFeatures* feats, int n, const MisMatchParams* p, MisMatchesInfo* out);
/* sharded form: only the pairs with (pair_index % world_size) == rank are matched (others left default) */
int mis_match_pairs_sharded(MisContext* ctx, const MisFeatures* feats, int n, const MisMatchParams* p, int rank,
                            int world_size, MisMatchesInfo* out);
/* BestOf2NearestRangeMatcher(range_width, ...) and the pair mask of FeaturesMatcher::operator() -- replaces
 * image_stitching.cpp:646-649.  A pair (i, j), i < j, is matched iff both frames have keypoints, `mask` is NULL or
 * mask[i*n + j] != 0 (n*n row-major; only the strict upper triangle is read), and range_width == -1 or j < i + range_width
 * (2: adjacent frames only; 1: nothing).  The selected pairs keep their row-major order and are dealt
 * (selected_pair_index % world_size) == rank; every other entry stays default-initialised.  range_width must be -1 or >= 1.
 * mis_match_all_pairs and mis_match_pairs_sharded are the (NULL, -1) case. */
int mis_match_pairs_select(MisContext* ctx, const MisFeatures* feats, int n, const MisMatchParams* p, const uint8_t* mask,
                           int range_width, int rank, int world_size, MisMatchesInfo* out);
/* The matcher's motion model -- the matcher_type switch of image_stitching.cpp:64, :644-649.  MIS_MATCH_HOMOGRAPHY:
 * BestOf2NearestMatcher / BestOf2NearestRangeMatcher, the three entries above.  MIS_MATCH_AFFINE_PARTIAL:
 * AffineBestOf2NearestMatcher(full_affine = false, try_cuda, match_conf) of :644-645 -- the same 2-NN and ratio test; the points are
 * the keypoint positions as they are (not shifted by half the image size); cv::estimateAffinePartial2D (RANSAC, threshold 3,
 * 2000 iterations, confidence 0.99, 10 refinement iterations) in place of findHomography; num_inliers is its mask's count and
 * confidence = num_inliers / (8 + 0.3 matches) WITHOUT the "> 3" zeroing; no |det H| test, no second estimation; H is
 * [a -b tx; b a ty] with the last row exactly (0, 0, 1), the mirrored entry holds its inverse. */
enum { MIS_MATCH_HOMOGRAPHY = 0, MIS_MATCH_AFFINE_PARTIAL = 1 };
/* AffineBestOf2NearestMatcher's defaults (:645 with match_conf as mis_match_default_params has it): threshold 3.0, 2000 iterations,
 * confidence 0.99, num_matches_thresh1 6.  num_matches_thresh2 is ignored for this model. */
void mis_match_affine_default_params(MisMatchParams* p);
/* mis_match_pairs_select with the model (:644-649): the pair mask, range_width and the sharding are orthogonal to it.  An unknown
 * model returns MIS_E_UNSUPPORTED.  For MIS_MATCH_AFFINE_PARTIAL mis_match_knn_fence releases at the end of the 2-NN pass. */
int mis_match_pairs_model(MisContext* ctx, const MisFeatures* feats, int n, const MisMatchParams* p, int model, const uint8_t* mask,
                          int range_width, int rank, int world_size, MisMatchesInfo* out);
int mis_matches_free(MisMatchesInfo* m, int count);
/* Ordering aid for a caller that overlaps other device work with a matcher call made by another host thread (the
 * job's speculative composition): mis_match_sequence = number of matcher calls this context has started;
 * mis_match_knn_fence(ctx, stream, mis_match_sequence(ctx) + 1 taken BEFORE the other thread calls the matcher, ms)
 * makes `stream` wait for the point of that call behind which other work shares the device well: by default the first draw of
 * the side RANSAC chain, 0.55 ms behind the 2-NN pass (the chains' kernels are few large workgroups that wait for room once another
 * stream's grids fill the compute units; from that point on they hold theirs). */
long long mis_match_sequence(MisContext* ctx);
int mis_match_knn_fence(MisContext* ctx, void* stream, long long target_seq, int timeout_ms);
/* The same without a second host thread: a one-shot hook of this context's NEXT matcher call.  fn(user) runs on the thread that
 * calls mis_match_all_pairs / mis_match_pairs_sharded / mis_match_pairs_select, once all of the call's device work is enqueued and before the call waits
 * for the device (the ~5 ms in which that thread is idle); inside it mis_match_knn_fence(ctx, stream, mis_match_sequence(ctx), 0)
 * returns at once and queues `stream` behind the 2-NN pass.  The hook is not called when the matcher call fails earlier. */
int mis_match_on_enqueued(MisContext* ctx, void (*fn)(void*), void* user);
/* diagnostics: the number of this context's matcher calls that adopted a 2-NN pass enqueued ahead (mis_orb_arm_knn_ahead) */
long long mis_debug_knn_ahead_adopted(MisContext* ctx);
/* test aid: the 2-NN pass enqueued ahead, with counts of the caller's choice.  feats[i] is a set made by mis_features_upload whose
 * n is its block's capacity (all of its rows are uploaded); counts[i], 0 .. that capacity, is written into the block's device
 * count slot on the context's stream, the pass is enqueued from the capacities and those slots with this selection (mask,
 * range_width, rank, world: as in mis_orb_arm_knn_ahead), feats[i].n becomes counts[i] and the pass is confirmed -- what
 * mis_orb_detect_batch does behind its gather.  The caller then hands the same structs to a matcher entry.  MIS_E_INVALID: a
 * null pointer, a count below 0 or above its capacity; where the finder would enqueue nothing, so does this, and returns MIS_OK. */
int mis_debug_knn_ahead(MisContext* ctx, MisFeatures* feats, int n, const int* counts, const uint8_t* mask, int range_width, int rank,
                        int world);
/* exact 2-NN (distance, trainIdx) for one direction; results in host memory (stage test hook).  Binary sets are 32 bytes wide
 * (ORB) or 61 (AKAZE's 486-bit MLDB, the last byte's top two bits clear): the matcher entries above and this one take either, and
 * every set of a call must have one width (MIS_E_INVALID otherwise).  61-byte sets run a vector-pipe kernel of their own; the
 * 32-byte kernels and their selection do not see them. */
int mis_knn2(MisContext* ctx, const MisFeatures* query, const MisFeatures* train, int* idx2_host, float* dist2_host);
/* cv::findHomography(src, dst, mask, RANSAC, thresh, max_iters, confidence) on host point lists */
int mis_find_homography(MisContext* ctx, const float* src_xy, const float* dst_xy, int n, double thresh, int max_iters,
                        double confidence, double H[9], uint8_t* mask, int* ok);
/* cv::estimateAffinePartial2D(src, dst, mask, RANSAC, thresh, max_iters, confidence, refine_iters) on host point lists -- the
 * estimator of AffineBestOf2NearestMatcher::match (image_stitching.cpp:644-645); M = [a -b tx; b a ty] row-major.  *ok = 0: no
 * model (M zeroed, mask zeroed).  refine_iters 0 returns the RANSAC model itself. */
int mis_estimate_affine_partial(MisContext* ctx, const float* src_xy, const float* dst_xy, int n, double thresh, int max_iters,
                                double confidence, int refine_iters, double M[6], uint8_t* mask, int* ok);
/* myLeaveBiggestComponent -- replaces image_stitching.cpp:215-278 (host logic on the matcher output) */
int mis_leave_biggest_component(const MisMatchesInfo* pairwise, int n, float conf_threshold, int* indices, int* n_indices);
/* the same on the bare n x n confidence matrix (row-major; what a sharded job has after its all-reduce) */
int mis_leave_biggest_component_conf(const double* confidence, int n, float conf_threshold, int* indices, int* n_indices);

/* ---------------------------------------------------------------- camera refinement --------- */
/* cv::detail::CameraParams (focal, aspect, ppx, ppy, R, t) as the reference fills it (image_stitching.cpp:485-517) */
typedef struct {
    double focal, aspect, ppx, ppy;
    double R[9];   /* row-major */
    double t[3];
} MisCameraParams;
/* (*adjuster)(features, pairwise_matches, cameras) with makePtr<detail::BundleAdjusterReproj>(), setConfThresh,
 * setRefinementMask -- replaces image_stitching.cpp:681-712.  Host logic (as in OpenCV): Levenberg-Marquardt over 7
 * parameters per camera on the inlier correspondences of the pairs above conf_thresh; refine_mask = the reference's
 * ba_refine_mask string ("xxxxx"); the rotations are normalised to the centre of the maximum spanning tree. */
int mis_bundle_adjust_reproj(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh,
                             const char* refine_mask, MisCameraParams* cameras);
/* (*adjuster)(features, pairwise_matches, cameras) with makePtr<detail::BundleAdjusterRay>(), setConfThresh -- replaces
 * image_stitching.cpp:683-684 (ba_cost_func = "ray").  Levenberg-Marquardt over 4 parameters per camera (focal, rotation vector)
 * on the rays of the inlier correspondences of the pairs above conf_thresh: 3 errors per correspondence, sqrt(f_i f_j) times the
 * difference of the two unit rays, K taken from the features' image sizes.  No refinement mask; ppx, ppy, aspect and t come back
 * as given.  The solver is host logic; the errors, the central-difference Jacobian (step 1e-3) and the per-pair sums of the
 * normal equations are evaluated by kernels on the context's stream, reading the keypoints in the features' device arrays.  The
 * match indices are validated on the host first.  The rotations are normalised to the centre of the maximum spanning tree. */
int mis_bundle_adjust_ray(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh,
                          MisCameraParams* cameras);
/* (*adjuster)(features, pairwise_matches, cameras) with makePtr<detail::BundleAdjusterAffinePartial>(), setConfThresh -- replaces
 * image_stitching.cpp:685-686 (ba_cost_func = "affine"; reached through the scans mode, not through that name).  Levenberg-Marquardt
 * over 4 parameters per camera, (a, b, tx, ty) = (R[0,0], R[1,0], R[0,2], R[1,2]) of the float32 R, H = [a -b tx; b a ty; 0 0 1]: 2
 * errors per inlier correspondence of the pairs above conf_thresh, p2 - (H_i^-1 H_j) p1 (invertAffineTransform in double).  On return
 * R = the float32 H of the refined four values, normalised to the centre of the maximum spanning tree; focal, aspect, ppx, ppy and t
 * come back as given.  The solver is host logic; the errors, the central-difference Jacobian (step 1e-4) and the per-pair sums of
 * the normal equations are evaluated by kernels on the context's stream, reading the keypoints in the features' device arrays.
 * The match indices are validated on the host first. */
int mis_bundle_adjust_affine_partial(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh,
                                     MisCameraParams* cameras);
/* estimator = makePtr<detail::AffineBasedEstimator>(); (*estimator)(features, pairwise_matches, cameras): every camera a default
 * CameraParams (focal 1, aspect 1, ppx = ppy = 0, t = 0), R chained along the maximum spanning tree on num_inliers, breadth-first
 * from its centre: R_to = R_from * H(from, to) in double, handed on as float32 values.  Host logic; it never fails. */
int mis_estimate_affine_cameras(const MisMatchesInfo* pairwise, int n, MisCameraParams* cameras);
/* detail::focalsFromHomography(H, f0, f1, f0_ok, f1_ok) (stitching/src/autocalib.cpp): the focal lengths of the source (f0) and the
 * destination (f1) view that a homography in centred coordinates between two views of a rotating camera implies, in IEEE double
 * as SURVEY Appendix A.16 writes them out.  Zero denominators are not special-cased (H = I and a pure roll give ok = 0 through
 * NaN comparisons; an infinite quotient gives f = inf with ok = 1).  A focal whose ok is 0 is returned as 0. */
int mis_focals_from_homography(const double H[9], double* f0, double* f1, int* f0_ok, int* f1_ok);
/* detail::estimateFocal(features, pairwise_matches, focals): sqrt(f0 f1) of every ordered pair with has_H whose two focals are ok;
 * with at least n - 1 (and at least one) such candidates every focal is their median, otherwise sum(width + height) / n.
 * img_sizes: the sizes of the images the features were found on (MisFeatures.img_w, img_h: work scale); focals: n doubles. */
int mis_estimate_focal(const MisMatchesInfo* pairwise, int n, const MisSize* img_sizes, double* focals);
/* estimator = makePtr<detail::HomographyBasedEstimator>(); (*estimator)(features, pairwise_matches, cameras): what
 * Stitcher::create(PANORAMA) runs when no cameras are supplied.  Every camera a default CameraParams (aspect 1, t = 0) with the
 * focal of mis_estimate_focal; R chained along the maximum spanning tree on num_inliers, breadth-first from its centre:
 * R_to = R_from * K_from^-1 * H(from, to)^-1 * K_to in double, not orthonormalised, handed on as float32 values; ppx, ppy = half
 * the image size.  Host logic, no context; it never fails.  MIS_E_INVALID: a null pointer, n < 1 or a non-positive size. */
int mis_estimate_homography_cameras(const MisMatchesInfo* pairwise, int n, const MisSize* img_sizes, MisCameraParams* cameras);
/* waveCorrect(rmats, wave_correct) -- replaces image_stitching.cpp:718-726; rmats: n x 9 doubles in place; kind 0 = HORIZ, 1 = VERT */
int mis_wave_correct(double* rmats, int n, int kind);

/* ---------------------------------------------------------------- warp ---------------------- */
/* warper->warpRoi(sz, K, R) -- replaces image_stitching.cpp:1138 (K, R: 3x3 f32 row-major) */
int mis_warp_roi(float scale, int src_width, int src_height, const float K[9], const float R[9], MisRect* roi);
/* the loop `for i: sizes[i], corners[i] = warper->warpRoi(sz, K_i, R_i)` of image_stitching.cpp:1119-1140 in one call:
 * the 2(W+H) border projections of every frame run in one small kernel (one workgroup per frame) instead of on the host;
 * Ks, Rs: n x 9 floats.  Same rois as n calls of mis_warp_roi (nothing is cached between calls in either form). */
int mis_warp_roi_batch(MisContext* ctx, float scale, int src_width, int src_height, int n, const float* Ks, const float* Rs, MisRect* rois);
/* warper->warp(src, K, R, interp, border, dst) -- replaces image_stitching.cpp:985, :988, :1154, :1159.
 * u8 source with 1 or 3 channels; (INTER_LINEAR, BORDER_REFLECT) or (INTER_NEAREST, BORDER_CONSTANT). */
int mis_warp_spherical(MisContext* ctx, const MisImage* src, float scale, const float K[9], const float R[9], int interp,
                       int border, MisImage* dst, MisPoint* tl);
/* fused compose-scale warp: image (LINEAR, REFLECT) converted to 16SC3 plus the validity mask
 * (NEAREST, CONSTANT of an all-255 mask) in one pass -- replaces :1154 + :1157-1159 + :1164. */
int mis_warp_spherical_fused(MisContext* ctx, const MisImage* src_bgr, float scale, const float K[9], const float R[9],
                             MisImage* dst_s16x3, MisImage* dst_mask, MisPoint* tl);
/* the same with the roi already known (the value mis_warp_roi / mis_warp_roi_batch returned for exactly these scale, K, R and
 * source size): skips the border walk the reference repeats inside warp() -- the compose loop's form (:1138 then :1154). */
int mis_warp_spherical_fused_roi(MisContext* ctx, const MisImage* src_bgr, float scale, const float K[9], const float R[9],
                                 const MisRect* roi, MisImage* dst_s16x3, MisImage* dst_mask, MisPoint* tl);
/* the fused warps of n frames (the loop :1086-1220 for all of them) in one grid per 16 frames: the results of n
 * mis_warp_spherical_fused_roi calls (dsts[i] / dmasks[i]: caller's buffers or NULL data as there), without a launch of its own per
 * frame -- a 4K frame alone fills and drains the device for a quarter of its launch */
int mis_warp_spherical_fused_batch(MisContext* ctx, const MisImage* srcs_u8x3, int n, float scale, const float* Ks, const float* Rs, const MisRect* rois,
                                   MisImage* dsts_s16x3, MisImage* dmasks_u8, MisPoint* tls);
/* measurement aid (bench.py): the batch launched `repeats` times between two HIP events on the context's stream; *avg_us = one pass */
int mis_warp_spherical_fused_batch_timed(MisContext* ctx, const MisImage* srcs_u8x3, int n, float scale, const float* Ks, const float* Rs,
                                         const MisRect* rois, MisImage* dsts_s16x3, MisImage* dmasks_u8, MisPoint* tls, int repeats, float* avg_us);
/* measurement aid: the same warp with the main kernel launched `repeats` times back to back on the context's
 * stream between two HIP events; *avg_us = average kernel duration (bench.py's roofline leg: no host gaps). */
int mis_warp_spherical_fused_timed(MisContext* ctx, const MisImage* src_bgr, float scale, const float K[9], const float R[9],
                                   MisImage* dst_s16x3, MisImage* dst_mask, MisPoint* tl, int repeats, float* avg_us);
/* The warpers of any kind (MIS_WARP_*): warper_creator = makePtr<{Spherical,Cylindrical,Plane}WarperGpu>() or
 * makePtr<{Mercator,Fisheye,Stereographic}Warper>() of image_stitching.cpp:917-969, then create(scale) (:973, :1117).  Each entry is the spherical one above with the kind added; the
 * spherical entries are these with MIS_WARP_SPHERICAL.  An unknown kind returns MIS_E_UNSUPPORTED.
 * Departures from OpenCV, each where OpenCV returns a meaningless rectangle: a plane roi with a corner behind the panorama plane
 * (z_ <= 0) and a cylindrical, Mercator, fisheye or stereographic roi with a non-finite extreme (Mercator: a source pixel at the
 * lower pole projects to v = -inf; stereographic: a source pixel next to the ray (0, -1, 0) has 1 - cos v_ = 0 under a non-zero
 * sin v_ and projects to +-inf, the pixel exactly on it gives 0 / 0 = NaN and is skipped) return MIS_E_INVALID.  A roi whose width or height does not fit an int (any kind) is MIS_E_INVALID too, never a
 * wrapped size. */
/* warper->warpRoi(sz, K, R) -- replaces :1138.  Plane: the four corners (PlaneWarper::detectResultRoi); cylindrical: the border.
 * Mercator: cv::MercatorWarper has no detectResultRoi of its own, so RotationWarperBase projects EVERY source pixel forward and
 * takes the four extremes; this context-free entry does the same in a plain host loop and is O(width * height) for that kind (a
 * 4K frame: 8.3 M projections).  mis_warper_roi_batch and every entry with a context run that scan on the device.  Fisheye,
 * stereographic, compressed-plane and Panini: the same (MIS_WARP_ROI_IS_FULL_SCAN).  A compressed-plane frame with a ray at
 * u_ = +-90 degrees (1 / cosf(u_) infinite) is MIS_E_INVALID like the Mercator pole. */
int mis_warper_roi(int kind, float scale, int src_width, int src_height, const float K[9], const float R[9], MisRect* roi);
/* the warpRoi loop of :1119-1140 in one call (one small kernel; the same rois as mis_warper_roi; the message names a refused frame).
 * Mercator, fisheye, stereographic: one grid-wide reduction over all pixels of all n frames, still one launch and one stream
 * synchronisation. */
int mis_warper_roi_batch(MisContext* ctx, int kind, float scale, int src_width, int src_height, int n, const float* Ks, const float* Rs,
                         MisRect* rois);
/* warper->warp(src, K, R, interp, border, dst) -- replaces :985, :988, :1154, :1159 (u8, 1 or 3 channels) */
int mis_warper_warp(MisContext* ctx, int kind, const MisImage* src, float scale, const float K[9], const float R[9], int interp,
                    int border, MisImage* dst, MisPoint* tl);
/* the same with the roi mis_warper_roi / mis_warper_roi_batch gave for these parameters (the Mercator roi is a scan of every source
 * pixel: a caller that sized dst from the roi passes it on instead of having it computed again) */
int mis_warper_warp_roi(MisContext* ctx, int kind, const MisImage* src, float scale, const float K[9], const float R[9], const MisRect* roi,
                        int interp, int border, MisImage* dst, MisPoint* tl);
/* fused compose-scale warp -- replaces :1154 + :1157-1159 + :1164.  (Fisheye and stereographic: mapBackward per output pixel,
 * atan2 / sqrt / atan / two sincos, in a kernel of its own; the same contract and the same sampling.  Compressed-plane and Panini:
 * the column terms once per column and tile, an atan and a sincos per pixel, in a kernel of their own.) */
int mis_warper_warp_fused(MisContext* ctx, int kind, const MisImage* src_bgr, float scale, const float K[9], const float R[9],
                          MisImage* dst_s16x3, MisImage* dst_mask, MisPoint* tl);
/* the same with the roi mis_warper_roi gave for these parameters (:1138 then :1154) */
int mis_warper_warp_fused_roi(MisContext* ctx, int kind, const MisImage* src_bgr, float scale, const float K[9], const float R[9],
                              const MisRect* roi, MisImage* dst_s16x3, MisImage* dst_mask, MisPoint* tl);
/* the fused warps of n frames (the loop :1086-1220) in one grid per 16 frames: the results of n mis_warper_warp_fused_roi calls */
int mis_warper_warp_fused_batch(MisContext* ctx, int kind, const MisImage* srcs_u8x3, int n, float scale, const float* Ks, const float* Rs,
                                const MisRect* rois, MisImage* dsts_s16x3, MisImage* dmasks_u8, MisPoint* tls);
/* ---- the warper's point, map and backward methods ----
 * warper->warpPoint(pt, K, R) (direction MIS_MAP_FORWARD: setCameraParams, then mapForward(pt.x, pt.y)) and
 * warper->warpPointBackward(pt, K, R) (MIS_MAP_BACKWARD: mapBackward at float coordinates; the kinds that test z > 0 give (-1, -1),
 * the plane and affine kinds divide whatever the sign) for n points.  xy_in / xy_out: host arrays of n (x, y) pairs
 * (they may be the same array).  ctx NULL: a host loop over the library's mapForward and over the operation sequences its warp
 * kernels evaluate for mapBackward; with a context: one point per lane of a kernel on the context's stream.  The two agree in every
 * bit (NaN payloads aside).  The affine kind takes H for R.  n == 0: MIS_OK, nothing read or written.  MIS_E_UNSUPPORTED: an unknown
 * kind; MIS_E_INVALID: a null pointer, scale <= 0, n < 0, another direction, with a context more than 2^27 points in one call. */
enum { MIS_MAP_FORWARD = 0, MIS_MAP_BACKWARD = 1 };
int mis_warper_warp_points(MisContext* ctx_or_null, int kind, float scale, const float K[9], const float R[9], int direction,
                           const float* xy_in, float* xy_out, int n);
/* warper->buildMaps(src_size, K, R, xmap, ymap): mapBackward(u, v) for every integer (u, v) of the warp roi into two
 * 1-channel MIS_F32 device images of the roi's size (any row pitch that is a multiple of 4; data == NULL: the library allocates) --
 * the maps the warp kernels evaluate in registers, bit for bit.  roi_or_null: the roi mis_warper_roi / mis_warper_roi_batch gave for
 * these parameters (nothing is scanned again), or NULL (computed here).  roi_out (may be NULL): that roi, (x, y, width, height) with
 * the maps' size; OpenCV returns Rect(tl, br), one less in both directions (A.17).  Refused before anything is launched or
 * allocated: an unknown kind (MIS_E_UNSUPPORTED); null pointers, sizes <= 0, scale <= 0, maps of another geometry, a refused roi
 * (MIS_E_INVALID). */
int mis_warper_build_maps(MisContext* ctx, int kind, float scale, int src_width, int src_height, const float K[9], const float R[9],
                          const MisRect* roi_or_null, MisImage* xmap_f32, MisImage* ymap_f32, MisRect* roi_out);
/* warper->warpBackward(src, K, R, interp, border, dst_size, dst), generalised: src (8UC1 or 8UC3, 2 .. 32767 on a side)
 * is any image whose top-left pixel lies at src_tl in the warper's plane -- a warped frame with its roi's corner (OpenCV's call, which
 * also asserts src's size to be the roi's), or a panorama with result_roi's corner.  For every pixel (x, y) of the dst_width x
 * dst_height view: (u, v) = mapForward(x, y), xmap = u - src_tl.x, ymap = v - src_tl.y (float32), dst = remap(src, xmap, ymap).
 * (interp, border): (LINEAR, REFLECT), (NEAREST, CONSTANT 0) or (LINEAR, CONSTANT 0: remap's INTER_BITS = 5 quantisation and Q15
 * weights, a tap outside src contributing 0); anything else is MIS_E_UNSUPPORTED.  dst_mask_or_null: 255 where the nearest source
 * pixel of the map coordinate lies inside src (warpBackward of an all-255 mask with (NEAREST, CONSTANT)).  dst / mask: 8U buffers of
 * the view's size at any pitch, or data == NULL (the library allocates).  Taps past src are border: nothing wraps at the +-180 degree
 * seam.  A 16SC3 blend result is converted to 8U by the caller, as for imwrite.  Refused before anything is launched or allocated:
 * an unknown kind or MIS_WARP_AFFINE, whose warper does not override warpBackward (MIS_E_UNSUPPORTED); null pointers, sizes <= 0,
 * scale <= 0 (MIS_E_INVALID). */
int mis_warper_warp_backward(MisContext* ctx, int kind, const MisImage* src, MisPoint src_tl, float scale, const float K[9], const float R[9],
                             int interp, int border, int dst_width, int dst_height, MisImage* dst, MisImage* dst_mask_or_null);
/* n views (Ks, Rs: n x 9 floats; dst_sizes[i]: view i's size) out of one source: the results of n
 * mis_warper_warp_backward calls, the tiles of up to 16 views in one one-dimensional grid.  masks_or_null: n masks or NULL.  n == 0:
 * MIS_OK; n < 0: MIS_E_INVALID.  Every view is checked before the first output is touched; the error text names a refused view. */
int mis_warper_warp_backward_batch(MisContext* ctx, int kind, const MisImage* src, MisPoint src_tl, float scale, int n, const float* Ks,
                                   const float* Rs, const MisSize* dst_sizes, int interp, int border, MisImage* dsts, MisImage* masks_or_null);
/* test aid: out[i] = f(in[i]) for one of the library's float32 functions (dev_math.h), evaluated on the host (ctx NULL) or in a
 * one-thread-per-element kernel on the context's stream (in / out are host arrays either way).  fn: MIS_MATH_*. */
enum { MIS_MATH_LOG = 0, MIS_MATH_TAN = 1, MIS_MATH_SINH = 2, MIS_MATH_ASIN = 3, MIS_MATH_ATAN = 4, MIS_MATH_EXP = 5 };
int mis_debug_math_f32(MisContext* ctx_or_null, int fn, const float* in, float* out, int n);
/* test aid: out[i] = f(a[i]) or f(a[i], b[i]) for every other function of dev_math.h and for the raw float32 sqrtf(x), 1.0f / x and
 * a / b, evaluated as mis_debug_math_f32 evaluates: on the host (ctx NULL) or in a one-thread-per-element kernel on the context's
 * stream (at most 2^20 elements per call then); a, b and out are host arrays.  The element types follow fn:
 *   SIN .. RCP                float -> float           (b unused; sin and cos through mis_sincosf)
 *   ATAN2, FAST_ATAN2, DIV    (float a, float b) -> float:  atan2(y = a, x = b), fastAtan2(y = a, x = b), a / b
 *   ROUND_F .. FLOOR_F        float -> int
 *   SAT_SHORT                 int -> int
 *   REFLECT101 .. REFLECT1    (int p = a, int len = b) -> int
 *   LOG_D                     double -> double
 *   ROUND_D                   double -> int */
enum { MIS_MATHX_SIN = 0, MIS_MATHX_COS = 1, MIS_MATHX_ACOS = 2, MIS_MATHX_SQRT = 3, MIS_MATHX_RCP = 4, MIS_MATHX_ATAN2 = 5,
       MIS_MATHX_FAST_ATAN2 = 6, MIS_MATHX_DIV = 7, MIS_MATHX_ROUND_F = 8, MIS_MATHX_ROUND_SAT_F = 9, MIS_MATHX_FLOOR_F = 10,
       MIS_MATHX_SAT_SHORT = 11, MIS_MATHX_REFLECT101 = 12, MIS_MATHX_REFLECT = 13, MIS_MATHX_REFLECT1 = 14, MIS_MATHX_LOG_D = 15,
       MIS_MATHX_ROUND_D = 16 };
int mis_debug_math(MisContext* ctx_or_null, int fn, const void* a, const void* b_or_null, void* out, int n);
/* test aid: mapBackward of a compressed-plane / Panini kind for every pixel of roi (at most 2^24 pixels) -> the source coordinates
 * xy[(row * roi->width + column) * 2 + {0, 1}] (a host array).  ctx NULL: the reference's operation sequence, unsplit, per pixel on
 * the host; with a context: the warp kernels' tile walk, which evaluates the column terms once per column.  The two must agree in
 * every bit.  Another kind: MIS_E_UNSUPPORTED. */
int mis_debug_warper_map_f32(MisContext* ctx_or_null, int kind, float scale, const float K[9], const float R[9], const MisRect* roi, float* xy);

/* ---------------------------------------------------------------- SIFT ---------------------- */
/* SIFT::create() -- replaces image_stitching/image_stitching.cpp:559 (features_type == "sift").  Defaults of the
 * reference: nfeatures 0 (only value supported), nOctaveLayers 3, contrastThreshold 0.04, edgeThreshold 10, sigma 1.6.
 * n_octave_layers 1 .. 8, sigma > 0.5.  A Gaussian kernel is never truncated: GaussianBlur's ksize = cvRound(8 s + 1) | 1 of the
 * base blur and of every incremental sigma must not exceed 127 taps (n_octave_layers 1 at sigma 1.6 needs 91, 3 at sigma 8.1 needs
 * 127); a parameter set that needs more returns MIS_E_UNSUPPORTED. */
typedef struct {
    int nfeatures, n_octave_layers;
    double contrast_threshold, edge_threshold, sigma;
} MisSiftParams;
typedef struct MisSift MisSift;
void mis_sift_default_params(MisSiftParams* p);
int mis_sift_create(MisContext* ctx, const MisSiftParams* params /* NULL = defaults */, int max_width, int max_height, MisSift** out);
int mis_sift_destroy(MisSift* sift);
/* computeImageFeatures(finder, img, features) -- replaces image_stitching.cpp:613 for the SIFT finder: keypoints in the
 * order of KeyPointsFilter::removeDuplicatedSorted, descriptors n x 128 f32 with integer values 0..255 (feeds K8). */
int mis_sift_detect(MisSift* sift, const MisImage* bgr, MisFeatures* out);
/* n frames of one size, two in flight (second scale space allocated on first use); out[i].img_idx = i as at :614 */
int mis_sift_detect_batch(MisSift* sift, const MisImage* bgr, int n_images, MisFeatures* out);
/* test aid: one image of the Gaussian (dog = 0) or DoG (dog = 1) pyramid of `bgr`, copied to host_out (may be NULL) */
int mis_sift_debug_level(MisSift* sift, const MisImage* bgr, int octave, int layer, int dog, float* host_out, int* width, int* height);
/* counters of this finder's last mis_sift_detect: extrema candidates, raw keypoints, keypoints after duplicate removal, refined candidates */
int mis_sift_debug_counts(MisSift* sift, unsigned* counts4);

/* ---------------------------------------------------------------- AKAZE --------------------- */
/* AKAZE::create() -- replaces image_stitching/image_stitching.cpp:547-550 (features_type == "akaze").  The definition is SURVEY
 * Appendix A.19.  Defaults: threshold 0.001, 4 octaves, 4 layers an octave, max_points -1 (all; > 0: the max_points keypoints of
 * highest response), the rotation-invariant MLDB descriptor at full size (486 bits in 61 bytes) over 3 channels, PM-G2
 * diffusivity.  Every other descriptor kind, size, channel count or diffusivity: MIS_E_UNSUPPORTED.  1 .. 6 octaves, 1 .. 8 layers,
 * at most 32 levels. */
enum { MIS_AKAZE_DESCRIPTOR_KAZE_UPRIGHT = 2, MIS_AKAZE_DESCRIPTOR_KAZE = 3, MIS_AKAZE_DESCRIPTOR_MLDB_UPRIGHT = 4, MIS_AKAZE_DESCRIPTOR_MLDB = 5 };
enum { MIS_AKAZE_DIFF_PM_G1 = 0, MIS_AKAZE_DIFF_PM_G2 = 1, MIS_AKAZE_DIFF_WEICKERT = 2, MIS_AKAZE_DIFF_CHARBONNIER = 3 };
typedef struct {
    float threshold;
    int n_octaves, n_octave_layers, max_points;
    int descriptor_type, descriptor_size, descriptor_channels, diffusivity;
} MisAkazeParams;
typedef struct MisAkaze MisAkaze;
void mis_akaze_default_params(MisAkazeParams* p);       /* image_stitching.cpp:547-550 */
int mis_akaze_create(MisContext* ctx, const MisAkazeParams* params /* NULL = defaults */, int max_width, int max_height, MisAkaze** out);   /* :547-550 */
int mis_akaze_destroy(MisAkaze* akaze);                 /* :547-550 (the finder's lifetime) */
/* computeImageFeatures(finder, img, features) -- :613 for the finder of :547-550: keypoints in (level, y, x) order, descriptors
 * n x 61 MIS_U8 (the top two bits of byte 60 are 0).  A frame with more candidates than the finder's capacity (one per 32 pixels,
 * at least 16384) is refused with MIS_E_OVERFLOW and the count, never truncated. */
int mis_akaze_detect(MisAkaze* akaze, const MisImage* bgr, MisFeatures* out);
/* n frames, one after the other (:547-550, :613-614): out[i].img_idx = i */
int mis_akaze_detect_batch(MisAkaze* akaze, const MisImage* bgr, int n_images, MisFeatures* out);
/* test aids of the finder of :547-550, all about its LAST detect.  debug_level: plane `which` (0 Lt, 1 Lsmooth, 2 flow, 3 Lx, 4 Ly,
 * 5 Ldet) of a level, copied to host_out (may be NULL: only the size).  debug_counts: candidates, after suppression, after
 * refinement, the k-contrast's float bits.  debug_class_ids: the keypoints' levels (cv::KeyPoint::class_id, which MisKeyPoint does
 * not carry).  debug_fed: the reordered FED steps into a level (taus may be NULL; level 0 has none). */
int mis_akaze_debug_level(MisAkaze* akaze, int level, int which, float* host_out, int* width, int* height);
int mis_akaze_debug_counts(MisAkaze* akaze, unsigned* counts4);
int mis_akaze_debug_class_ids(MisAkaze* akaze, int* host_out, int capacity);
int mis_akaze_debug_fed(MisAkaze* akaze, int level, float* taus, int* n);

/* ---------------------------------------------------------------- image operators ----------- */
/* cv::resize(src, dst, dsize, fx, fy, INTER_LINEAR_EXACT) -- replaces image_stitching.cpp:580 (work scale), :619 (seam
 * scale), :1144 (compose scale).  8UC1 / 8UC3.  dst_w, dst_h > 0: that size (scale = dsize / ssize); otherwise
 * dsize = (cvRound(w * fx), cvRound(h * fy)) and the coordinate scale is exactly 1/fx, 1/fy, as in resize(). */
int mis_resize_linear_exact(MisContext* ctx, const MisImage* src, int dst_w, int dst_h, double fx, double fy, MisImage* dst);
/* The work-scale resize of every frame of a job in one launch -- replaces the loop body image_stitching.cpp:589-603
 * (work_megapix < 0: work_scale = 1, the frame is used as it is; otherwise work_scale = min(1, sqrt(work_megapix * 1e6 / area))
 * from the first frame and cv::resize(full_img, img, Size(), work_scale, work_scale, INTER_LINEAR_EXACT) for every frame, with no
 * |scale - 1| > 0.1 test).  What follows from the work scale is the caller's: features carry the work size (:613), seam_work_aspect =
 * seam_scale / work_scale (:607), cameras *= work_scale before matching (:635-637), compose_work_aspect = compose_scale /
 * work_scale (:1113-1125).
 * n images of one size and type (8UC1 / 8UC3) -> n images; the size / factor rules and the 8.8 fixed-point arithmetic of
 * mis_resize_linear_exact, bit for bit.  Outputs follow the library's convention (data == NULL: allocated in HBM, kept by the
 * caller for the next call; otherwise exactly the destination size).  The coefficient tables are cached on the device per
 * geometry (grow-only, released with the context): with device images a call that finds its geometry uploads nothing and never
 * waits for the stream; the first call of a geometry uploads through the context's pinned staging and waits for that copy.
 * Host images are accepted as the single entry accepts them (staged through HBM, a copy and a wait per image).
 * Images of different size or type, n <= 0, null pointers: MIS_E_INVALID; other types than 8UC1 / 8UC3: MIS_E_UNSUPPORTED. */
int mis_resize_linear_exact_batch(MisContext* ctx, const MisImage* srcs, int n, int dst_w, int dst_h, double fx, double fy, MisImage* dsts);
/* cv::rotate(src, dst, code) -- replaces image_stitching.cpp:571 (ROTATE_90_CLOCKWISE = 0), :576 (ROTATE_180 = 1);
 * 2 = ROTATE_90_COUNTERCLOCKWISE.  8UC1 / 8UC3. */
int mis_rotate(MisContext* ctx, const MisImage* src, int rotate_code, MisImage* dst);
/* dilate(masks_warped[i], 3x3) -> resize(to mask_warped.size(), INTER_LINEAR_EXACT) -> mask_warped &= ... in one
 * pass -- replaces image_stitching.cpp:1169-1171.  Both 8UC1; mask_warped is updated in place. */
int mis_seam_mask_apply(MisContext* ctx, const MisImage* seam_mask_warped, MisImage* mask_warped);

/* ---- exposure compensation and seam finders between warp and blend ----
 * Replaces ExposureCompensator::createDefault(expos_comp_type) with setNrFeeds(expos_comp_nr_feeds),
 * setNrGainsFilteringIterations(2), setBlockSize(64, 64) (image_stitching.cpp:73-76, :1002-1016),
 * compensator->feed(corners, images_warped, masks_warped) (:1023) and
 * compensator->apply(img_idx, corners[img_idx], img_warped, mask_warped) (:1162).
 * Images are 8UC3, masks 8UC1 (255 = valid), host or device.
 * The types are cv::detail::ExposureCompensator's, with OpenCV's values: GAIN (one gain per frame), GAIN_BLOCKS (one per block,
 * smoothed into a map), CHANNELS (one gain per frame and colour channel), CHANNELS_BLOCKS (a three-channel map).  NO needs no
 * object.  The similarity threshold of OpenCV 4.x stays at its default of 1 (no similarity masks): it is not built.
 * The caller's images: with more than one feed OpenCV multiplies the images it was given by the previous feed's gains (GAIN and
 * GAIN_BLOCKS edit the caller's seam-scale images, the channel types edit extracted copies).  This library works on private device
 * copies for every type: mis_compensator_feed NEVER alters the caller's images or masks, whatever nr_feeds is. */
#define MIS_EXPOS_NO 0
#define MIS_EXPOS_GAIN 1
#define MIS_EXPOS_GAIN_BLOCKS 2
#define MIS_EXPOS_CHANNELS 3
#define MIS_EXPOS_CHANNELS_BLOCKS 4
typedef struct {
    int type;                            /* MIS_EXPOS_* (not NO) */
    int nr_feeds;                        /* >= 1: feeds k > 0 run on the images multiplied by the gains of feed k - 1; the result is the product */
    int block_width, block_height;       /* block types only */
    int nr_gain_filtering_iterations;    /* block types only */
} MisCompensatorParams;
typedef struct MisCompensator MisCompensator;
/* the reference's values: GAIN_BLOCKS, 1 feed, 64 x 64 blocks, 2 filtering passes */
void mis_compensator_default_params(MisCompensatorParams* params);
/* type NO, an unknown type or nr_feeds < 1: MIS_E_INVALID */
int mis_compensator_create_ex(MisContext* ctx, const MisCompensatorParams* params, MisCompensator** out);
/* {GAIN_BLOCKS, 1 feed, the given blocks and passes} */
int mis_compensator_create(MisContext* ctx, int block_width, int block_height, int nr_gain_filtering_iterations, MisCompensator** out);
int mis_compensator_destroy(MisCompensator* c);
int mis_compensator_feed(MisCompensator* c, const MisPoint* corners, const MisImage* images, const MisImage* masks, int n);
/* gains of one image after the feed: GAIN the gain three times, CHANNELS B, G, R; block types: MIS_E_UNSUPPORTED */
int mis_compensator_gains(const MisCompensator* c, int index, double gains[3]);
/* smoothed gain map of one image (one float per block, row-major); map_host may be NULL to query the grid size.
 * One-channel maps only: MIS_E_UNSUPPORTED for CHANNELS_BLOCKS and for the types without a map */
int mis_compensator_gain_map(const MisCompensator* c, int index, float* map_host, int capacity, int* blocks_x, int* blocks_y);
/* the same for GAIN_BLOCKS (*channels = 1) and CHANNELS_BLOCKS (*channels = 3, interleaved B, G, R per block); capacity in floats */
int mis_compensator_gain_map_channels(const MisCompensator* c, int index, float* map_host, int capacity, int* blocks_x, int* blocks_y, int* channels);
/* image *= gains, in place; 8UC3, or the 16SC3 image the fused warp produces (values 0..255) */
int mis_compensator_apply(MisCompensator* c, int index, MisImage* image);
/* Test hook: the overlap statistics of frames i and j in the LAST feed of a GAIN (channel 0) or CHANNELS (channel 0..2 = B, G, R)
 * compensator: N_ij = max(1, intersect count), I_ij and I_ji; all 0 when the frames' rectangles do not intersect.  Block types:
 * MIS_E_UNSUPPORTED. */
int mis_compensator_debug_stats(const MisCompensator* c, int i, int j, int channel, int* N, double* I_ij, double* I_ji);
/* VoronoiSeamFinder::find (seam_find_type "voronoi", image_stitching.cpp:1031): masks (8UC1) are edited in place.
 * "no" (NoSeamFinder) needs no call; the reference's default, DpSeamFinder(COLOR) ("dp_color"), is mis_seam_dp below. */
int mis_seam_voronoi(MisContext* ctx, const MisPoint* corners, MisImage* masks, int n);
/* seam_finder = makePtr<detail::DpSeamFinder>(DpSeamFinder::COLOR); seam_finder->find(images_warped_f, corners, masks_warped)
 * -- replaces image_stitching.cpp:1056-1057, :1065 (the reference's default seam finder, "dp_color").  images: the seam-scale
 * warped 8UC3 images (converted to float inside, as :992-994 does); masks: 8U, edited in place.  Host logic on copies of the
 * (~0.1 MP) images; device or host buffers.  cost_func: MIS_SEAM_DP_COLOR only; any other value is MIS_E_UNSUPPORTED here
 * (DpSeamFinder::COLOR_GRAD is the entry of its own below, mis_seam_dp_colorgrad). */
#define MIS_SEAM_DP_COLOR 0
int mis_seam_dp(MisContext* ctx, const MisPoint* corners, const MisImage* images, MisImage* masks, int n, int cost_func);
/* seam_finder = makePtr<detail::DpSeamFinder>(DpSeamFinder::COLOR_GRAD) -- image_stitching.cpp:1057-1058, :1065 ("dp_colorgrad").
 * Inputs, checks, pair order and mask write-back as mis_seam_dp; the colour cost of a cut is divided by 1 + the four absolute
 * Sobel derivatives across it.  The derivatives are made once per frame by one kernel launch (mis_seam_gradients' kernel) on the
 * gathered device copies and come to the host in the finder's one staged copy; host images are uploaded for it. */
int mis_seam_dp_colorgrad(MisContext* ctx, const MisPoint* corners, const MisImage* images, MisImage* masks, int n);
/* DpSeamFinder::computeGradients for n images in one launch; images: 8UC3, device or host; gradx / grady: f32 x 1 of the same
 * sizes, device or host.  Host inputs are uploaded; there is one arithmetic, the kernel's (float32, no FMA: csrc/seam_grad.hip).
 * n == 0: MIS_OK.  A size, type or channel mismatch: MIS_E_INVALID, nothing written. */
int mis_seam_gradients(MisContext* ctx, const MisImage* images, int n, MisImage* gradx, MisImage* grady);
/* seam_finder = makePtr<detail::GraphCutSeamFinder(Gpu)>(COST_COLOR, terminal_cost, bad_region_penalty); seam_finder->find(...)
 * -- image_stitching.cpp:1037-1054, :1065 (the reference's try_cuda seam finder; OpenCV's defaults are 10000 and 1000).  Inputs
 * and checks as mis_seam_dp: seam-scale 8UC3 images, 8U masks edited in place, device or host buffers; a size, type or channel
 * mismatch is MIS_E_INVALID with nothing written, n == 0 is MIS_OK.  Per overlapping pair, in PairwiseSeamFinder::run order
 * (i, then j > i), a maximum flow on the roi grown by 10 pixels decides which image keeps each pixel; the definition with its
 * integer capacities is SURVEY.md appendix A.13, the kernels are csrc/seam_gc.hip (device push-relabel; the labels are the
 * minimal source side, a property of the input).  cost_type: MIS_SEAM_GC_COST_COLOR; MIS_SEAM_GC_COST_COLOR_GRAD is refused by
 * name with MIS_E_UNSUPPORTED, any other value is MIS_E_INVALID.  terminal_cost / bad_region_penalty: finite and >= 0, and small
 * enough that a node's four edges and its terminal stay below 2^31 together, else MIS_E_INVALID.  The solver's launches are
 * bounded: a pair that has not finished within the cap returns MIS_E_INTERNAL with the pair named, the masks untouched. */
#define MIS_SEAM_GC_COST_COLOR 0
#define MIS_SEAM_GC_COST_COLOR_GRAD 1
int mis_seam_graphcut(MisContext* ctx, const MisPoint* corners, const MisImage* images, MisImage* masks, int n,
                      int cost_type, float terminal_cost, float bad_region_penalty);
/* Test aid: the graph of pair (i, j), 0 <= i < j < n, built and cut with the default costs on the masks AS GIVEN (no earlier pair
 * has edited them; nothing is written to them) -> its integer capacities towards the right and the lower neighbour (0 in the
 * last column / row), its terminals (> 0 source, < 0 sink) and its labels (1: in the minimal source side), row-major planes of
 * grid_w x grid_h nodes, the 10-pixel gap included.  grid_w / grid_h are always written; capacity_elems == 0 asks for them alone;
 * planes that hold fewer than grid_w * grid_h elements, or images that do not overlap: MIS_E_INVALID. */
int mis_seam_graphcut_debug_pair(MisContext* ctx, const MisPoint* corners, const MisImage* images, const MisImage* masks, int n, int i, int j,
                                 int32_t* cap_right, int32_t* cap_down, int32_t* terminals, uint8_t* labels, size_t capacity_elems,
                                 int* grid_w, int* grid_h);
/* The counts of the context's last mis_seam_graphcut call: overlapping pairs, dependency levels, grid nodes, the cap on a level's
 * round sets, global relabels, relabel sweeps, then the round sets each level used.  *count: how many there are; out takes the
 * first `capacity` of them. */
int mis_seam_graphcut_stats(const MisContext* ctx, int* out, int capacity, int* count);

/* ---------------------------------------------------------------- blend --------------------- */
/* reference-side blender sizing, image_stitching.cpp:1176-1190: returns the blend type to use in
 * *type_out and fills num_bands (MULTI_BAND) or sharpness (FEATHER) */
int mis_blend_config(int blend_type, float blend_strength, int pano_width, int pano_height, int* type_out, int* num_bands,
                     float* sharpness);
int mis_result_roi(const MisPoint* corners, const MisSize* sizes, int n, MisRect* roi); /* cv::detail::resultRoi */
/* Blender::createDefault(type) + setNumBands / setSharpness -- replaces :1175, :1183, :1189 */
int mis_blender_create(MisContext* ctx, int type, int num_bands, float sharpness, MisBlender** out);
int mis_blender_destroy(MisBlender* b);
int mis_blender_prepare(MisBlender* b, const MisPoint* corners, const MisSize* sizes, int n); /* :1192 */
int mis_blender_num_bands(const MisBlender* b);
/* blender->feed(img_warped_s [16SC3], mask_warped [8U], corners[i]) -- replaces :1218 */
int mis_blender_feed(MisBlender* b, const MisImage* img_s16x3, const MisImage* mask_u8, MisPoint tl);
/* the feeds of n frames of the loop :1086-1220 in one call: the result of mis_blender_feed(imgs[0], ...) ... mis_blender_feed(imgs[n-1], ...)
 * in that order, bit for bit; the multi-band blender builds the frames' Gaussian pyramids together (one launch per level for all
 * frames instead of one per level and frame) before it accumulates the Laplacians frame by frame */
int mis_blender_feed_batch(MisBlender* b, const MisImage* imgs_s16x3, const MisImage* masks_u8, const MisPoint* tls, int n);
/* blender->blend(result, result_mask) -- replaces :1225 */
int mis_blender_blend(MisBlender* b, MisImage* dst_s16x3, MisImage* dst_mask);
/* blend() for the panorama columns x0 .. x1 - 1 only (relative to the result roi; x1 is clipped to its width): the same values
 * as those columns of mis_blender_blend's result, computed from the accumulators of that strip + a halo of two columns per
 * level.  A rank that owns a column strip of the panorama finalises only that strip. */
int mis_blender_blend_columns(MisBlender* b, int x0, int x1, MisImage* dst_s16x3, MisImage* dst_mask);
/* Multi-GPU blend exchange (replaces nothing in the single-process reference: its feed loop :1218 adds every frame into one
 * pyramid; N ranks add theirs into N pyramids and exchange rectangles).  A rectangle of accumulator level `level`,
 * columns x0 .. x1 - 1, rows y0 .. y1 - 1, lives in a byte buffer at `offset`: 16SC3 Laplacian sums row by row (6 B per pixel,
 * the block rounded up to 16 B), then the f32 weight sums (4 B per pixel, rounded up to 16 B).
 *   pack: accumulators -> buffer;   add: accumulators += buffer (16-bit sums wrap: any order gives the same bits; f32 sums are
 *   added in call order);   zero: accumulators = 0.   All on the blender's stream, device buffers. */
typedef struct { int level, x0, y0, x1, y1; unsigned long long offset; } MisLevelRect;
int mis_blender_pack_rects(MisBlender* b, const MisLevelRect* rects, int n, void* dev_buf, size_t bytes);
int mis_blender_add_rects(MisBlender* b, const MisLevelRect* rects, int n, const void* dev_buf, size_t bytes);
int mis_blender_zero_rects(MisBlender* b, const MisLevelRect* rects, int n);
/* The per-frame body of the compositing loop for n frames in one call: fused warp of frames[i] with (Ks + 9 i, Rs + 9 i)
 * at `scale` into library-owned device blocks of size rois[i] (= mis_warp_roi of the frame), then feed -- replaces
 * image_stitching.cpp:1154-1164 and :1218 for every image of the loop at :1086.  Same results as the single calls. */
int mis_compose_frames(MisBlender* b, const MisImage* frames, int n, float scale, const float* Ks, const float* Rs, const MisRect* rois);
/* the same with a warper kind (MIS_WARP_*) -- the compositing loop under warp_type (image_stitching.cpp:917-969, :1154-1164, :1218) */
int mis_compose_frames_kind(MisBlender* b, int kind, const MisImage* frames, int n, float scale, const float* Ks, const float* Rs,
                            const MisRect* rois);
/* the rectangle of the (padded) panorama a feed of a width x height frame at `tl` touches: MultiBandBlender::feed's tile
 * (frame + 3 * 2^bands margin, clipped, aligned to 2^bands); P_b of SURVEY 8(d) = tile.width * tile.height */
int mis_blender_feed_rect(const MisBlender* b, int width, int height, MisPoint tl, MisRect* tile);
/* accumulated pyramid level before blend() (host copies, parity tests / multi-GPU reduction hooks) */
int mis_blender_level_info(const MisBlender* b, int level, int* width, int* height, void** lap_dev, void** weight_dev);

/* ---------------------------------------------------------------- timelapse ----------------- */
/* The compositing loop's other sink (image_stitching.cpp:82 `timelapse`, :79 timelapse_type = Timelapser::CROP, :1083, :1194-1215):
 * every frame is warped into one common canvas and written out as a registered frame of its own ("fixed_<name>"), nothing is
 * blended.  SURVEY appendix A.18 has the semantics. */
enum { MIS_TIMELAPSE_AS_IS = 0, MIS_TIMELAPSE_CROP = 1 };      /* cv::detail::Timelapser::AS_IS / CROP */
typedef struct MisTimelapser MisTimelapser;
/* cv::detail::resultRoiIntersection(corners, sizes) -- what TimelapserCrop::initialize (:1197) sizes its canvas with:
 * Rect(tl = (max x_i, max y_i), br = (min (x_i + w_i), min (y_i + h_i))).  Host only, no context.  MIS_E_INVALID: a null pointer,
 * n < 1, an empty intersection (width or height <= 0; OpenCV fails in Mat::create there). */
int mis_result_roi_intersection(const MisPoint* corners, const MisSize* sizes, int n, MisRect* roi);
/* timelapser = Timelapser::createDefault(timelapse_type) -- replaces :1083 (the declaration) and :1196.  Another type: MIS_E_INVALID. */
int mis_timelapser_create(MisContext* ctx, int type, MisTimelapser** out);
int mis_timelapser_destroy(MisTimelapser* t);
/* timelapser->initialize(corners, sizes) -- replaces :1197: dst_roi = resultRoi (AS_IS, mis_result_roi) or resultRoiIntersection
 * (CROP); an empty intersection is MIS_E_INVALID with the rectangle named, a canvas of 2^31 pixels or more too. */
int mis_timelapser_initialize(MisTimelapser* t, const MisPoint* corners, const MisSize* sizes, int n);
int mis_timelapser_dst_roi(const MisTimelapser* t, MisRect* roi);      /* before initialize: MIS_E_STATE */
/* timelapser->process(img_warped_s, Mat::ones(...), corners[img_idx]) then getDst() -- replaces :1203-1204: the 16SC3 canvas of
 * dst_roi's size set to 0, then every pixel of img whose panorama position tl + (x, y) lies in dst_roi copied to it, in one pass
 * (one write per canvas pixel).  The reference's mask is all ones and is not an argument.  dst: the caller's 16SC3 buffer of the
 * canvas's size at any 2-byte aligned pitch, or data == NULL (the library allocates).  img may lie anywhere, wholly outside
 * included (the canvas is then all 0). */
int mis_timelapser_process(MisTimelapser* t, const MisImage* img_s16x3, MisPoint tl, MisImage* dst_s16x3);
/* The loop body :1154-1164 + :1203-1204 (+ the 16S -> 8U conversion of imwrite, :1214) for n frames in one launch per 16 frames:
 * canvas i = Timelapser::process of { mis_warper_warp_fused_roi(srcs[i], Ks + 9 i, Rs + 9 i, rois[i]), then -- gains given --
 * mis_compensator_apply of a GAIN / CHANNELS compensator whose mis_compensator_gains(i) are gains[3 i ..] } into dst_roi, bit for
 * bit, but a canvas pixel is mapped only where it lies in rois[i] (with CROP: nowhere else), no mask plane is produced and no
 * warped frame is stored.  rois[i]: what mis_warper_roi gave for frame i; dst_roi: mis_result_roi (AS_IS) or
 * mis_result_roi_intersection (CROP) of the rois, or any other rectangle.  dst_format: MIS_S16 (16SC3, getDst's) or MIS_U8 (packed
 * 8UC3 BGR, saturate_cast<uchar> of it: what mis_jpeg_encode_batch reads).  dsts[i]: a buffer of dst_roi's size in that format at
 * any pitch, or data == NULL (the library allocates).  All kinds mis_warper_warp_fused_batch accepts; the affine kind takes H for R.
 * Refused before anything is allocated or launched: an unknown kind (MIS_E_UNSUPPORTED); null pointers, n < 1, scale <= 0, an
 * empty dst_roi, a canvas of 2^31 pixels or more, another format, a non-finite gain, and by name ("frame <i>: ...") a source that
 * is not 8UC3 of 2 .. 32767 on a side, an empty roi, an output of another geometry (MIS_E_INVALID). */
int mis_timelapse_warp_batch(MisContext* ctx, int kind, const MisImage* srcs_u8x3, int n, float scale, const float* Ks, const float* Rs,
                             const MisRect* rois, const MisRect* dst_roi, const double* gains_or_null, MisImage* dsts, int dst_format);
/* measurement aid (tools/timelapse_bench.py; :1203-1214): the batch launched `repeats` times between two HIP events on the context's
 * stream; *avg_us = one pass over all n frames */
int mis_timelapse_warp_batch_timed(MisContext* ctx, int kind, const MisImage* srcs_u8x3, int n, float scale, const float* Ks, const float* Rs,
                                   const MisRect* rois, const MisRect* dst_roi, const double* gains_or_null, MisImage* dsts, int dst_format,
                                   int repeats, float* avg_us);

/* ---------------------------------------------------------------- JPEG ingest ---------------- */
/* imread("<k>.jpg") -- replaces image_stitching.cpp:569 (cv::imread with IMREAD_COLOR: 8UC3 BGR, a grey file gives B = G = R).
 * Baseline (SOF0, Huffman, 8-bit) streams of 1 or 3 components in one interleaved scan, luma sampled 1x1, 2x1 or 2x2 with 1x1
 * chroma; restart markers, custom Huffman tables and fill bytes are handled.  The result is bit for bit libjpeg-turbo's default
 * decode (JDCT_ISLOW, fancy upsampling), which is cv::imread's.  The entropy decode runs on host threads (frames and restart
 * intervals side by side), dequantisation + inverse DCT, upsampling and colour conversion on the device.
 * MIS_E_UNSUPPORTED, by name: progressive (SOF2), extended / lossless / hierarchical SOFs, arithmetic coding, 12-bit precision,
 * 16-bit quantisation tables, 4 components, multi-scan or non-interleaved files, any other sampling layout (4:4:0, 4:1:1, 4:4:4
 * written as all-2x2, ...), and a block whose coefficients are beyond the bound of the 32-bit inverse DCT (jpeg_core.h: no
 * encoder makes one).  MIS_E_INVALID: a truncated stream (libjpeg pads a truncated scan with zeros; this decoder refuses it), a
 * missing table, a zero run past coefficient 63, a Huffman code that is not in the table, a wrong restart index or count, a zero
 * dimension, width * height >= 2^31.  A refused stream writes nothing.  No EXIF-orientation rotation (the reference rotates by
 * isPortrait itself, :570-577). */
typedef struct {
    int width, height, components;
    int h[4], v[4];             /* the sampling factors of each component as the frame header writes them */
    int restart_interval;       /* MCUs between restart markers, 0: none */
} MisJpegInfo;
/* the frame header of a stream: host logic, no context and no device.  The text of a refusal: mis_jpeg_last_error(), of the
 * calling thread's last context-free JPEG call. */
int mis_jpeg_info(const void* data, size_t bytes, MisJpegInfo* out);
const char* mis_jpeg_last_error(void);
/* One frame / n frames of any sizes and layouts in one pass: one upload, one set of two launches for all n.  Outputs follow the
 * library's convention (data == NULL: allocated in HBM; otherwise exactly width x height, 8UC3, host or device, any stride >= 3 *
 * width).  A refused stream anywhere in a batch refuses the whole call before anything is launched or allocated; the error text
 * names the frame ("frame <i>: ..."). */
int mis_jpeg_decode(MisContext* ctx, const void* data, size_t bytes, MisImage* dst_bgr);
int mis_jpeg_decode_batch(MisContext* ctx, const void* const* datas, const size_t* bytes, int n, MisImage* dsts_bgr);
/* the same call with its parts timed (tools/jpeg_decode_bench.py): ms[0] the header pass and ms[1] the entropy decode on the host
 * clock, ms[2] the upload, ms[3] the IDCT launch and ms[4] the upsampling + colour launch between events on the stream */
int mis_jpeg_decode_batch_timed(MisContext* ctx, const void* const* datas, const size_t* bytes, int n, MisImage* dsts_bgr, float ms[5]);
/* the host layer alone: the quantised coefficient blocks of one component as the entropy decoder hands them to the device (int16,
 * natural order, 64 per block, the plane of (MCUs_y * V) x (MCUs_x * H) blocks row by row) and its quantisation table in natural
 * order.  No context and no device.  capacity (in coefficients) smaller than the plane: MIS_E_INVALID. */
int mis_jpeg_debug_coefficients(const void* data, size_t bytes, int component, int16_t* out, size_t capacity, uint16_t qtable[64]);

/* ---------------------------------------------------------------- JPEG output ---------------- */
/* imwrite("result.jpg", result) -- replaces image_stitching.cpp:1228 (cv::imwrite with its defaults: quality 95, 4:2:0, standard
 * Huffman tables, a JFIF 1.01 header).  The whole file is byte for byte what libjpeg-turbo writes from the same pixels (JDCT_ISLOW).
 * Colour conversion, chroma downsampling, forward DCT and quantisation run on the device (edges are replicated by clamped reads,
 * dummy blocks of a partial MCU are filled there too); one copy brings the quantised coefficients to the host, whose threads
 * Huffman-code chunks of whole MCU rows (whole restart intervals when there is an interval) side by side; the chunks are joined at
 * bit granularity and FF bytes stuffed after the join, so the stream does not depend on the number of threads.
 * MIS_E_UNSUPPORTED, by name: a 1- or 4-channel source, any other sampling (MIS_JPEG_440, MIS_JPEG_411, ...).  Optimised Huffman
 * tables and progressive streams are not written: the parameters have no field for them.  MIS_E_INVALID: a zero or negative size, a
 * dimension above 65535, a quality outside 0 .. 100, a restart interval outside 0 .. 65535. */
enum { MIS_JPEG_420 = 0, MIS_JPEG_422 = 1, MIS_JPEG_444 = 2, MIS_JPEG_440 = 3, MIS_JPEG_411 = 4 };
typedef struct {
    int quality;          /* 1 .. 100, 0: the default 95 (cv::imwrite's) */
    int sampling;         /* MIS_JPEG_420 (the default), MIS_JPEG_422, MIS_JPEG_444 */
    int restart_interval; /* MCUs between restart markers, 0: none */
} MisJpegEncodeParams;
typedef struct { uint8_t* data; size_t bytes; } MisJpegStream;   /* host memory the library owns: mis_jpeg_stream_free */
/* One image / n images of any sizes in one pass (image_stitching.cpp:1228): one upload of the argument table, one set of two
 * launches and one download for all n.  Sources are 8UC3 BGR in host or device memory with any stride >= 3 * width; params == NULL
 * means all defaults.  A refused image anywhere in a batch refuses the whole call before anything is launched or allocated; the
 * error text names the frame ("frame <i>: ...").  On success every outs[i] holds a whole file. */
int mis_jpeg_encode(MisContext* ctx, const MisImage* src_bgr, const MisJpegEncodeParams* params, MisJpegStream* out);
int mis_jpeg_encode_batch(MisContext* ctx, const MisImage* srcs_bgr, int n, const MisJpegEncodeParams* params, MisJpegStream* outs);
/* the same call with its parts timed (tools/jpeg_encode_bench.py; image_stitching.cpp:1228): ms[0] the upload of the argument table
 * and the two launches, ms[1] the download of the coefficients, both between events on the stream; ms[2] the entropy coding of the
 * chunks, ms[3] the join with byte stuffing, ms[4] the headers, on the host clock */
int mis_jpeg_encode_batch_timed(MisContext* ctx, const MisImage* srcs_bgr, int n, const MisJpegEncodeParams* params, MisJpegStream* outs, float ms[5]);
/* frees a stream of the entries above and of mis_jpeg_debug_entropy_encode and clears it (image_stitching.cpp:1228); NULL or an empty
 * stream is fine */
int mis_jpeg_stream_free(MisJpegStream* s);
/* the host layer alone (the entropy coder of image_stitching.cpp:1228's imwrite), no context and no device: the coefficient planes
 * of a w x h image in the layout of mis_jpeg_debug_coefficients (dummy blocks filled) -> the whole file, coded in `chunks` chunks
 * (clamped to 1 .. the number of MCU rows or restart intervals).  The text of a refusal: mis_jpeg_last_error(). */
int mis_jpeg_debug_entropy_encode(const int16_t* const coef[3], int w, int h, const MisJpegEncodeParams* params, int chunks, MisJpegStream* out);
/* the device layer alone (the transform of image_stitching.cpp:1228's imwrite): the coefficient plane of one component as the kernels
 * wrote it (int16, natural order, 64 per block, (MCUs_y * V) x (MCUs_x * H) blocks row by row) and its quantisation table in natural
 * order.  capacity (in coefficients) smaller than the plane: MIS_E_INVALID. */
int mis_jpeg_debug_encode_coefficients(MisContext* ctx, const MisImage* src_bgr, const MisJpegEncodeParams* params, int component,
                                       int16_t* out, size_t capacity, uint16_t qtable[64]);

/* ---------------------------------------------------------------- cropper -------------------- */
/* crop(cv::Mat& source) -- replaces image_stitching/cropper.cpp:124-209 (API in cropper.h) on the device: the rectangle the host
 * cropper (host/cropper.cpp, image_stitching_amd/cropper.py) finds, bit for bit, without the image leaving the device.  The steps
 * of :128-158 (grey > 0 with the integer grey formula, findContours RETR_EXTERNAL + CHAIN_APPROX_NONE, the first contour of maximal
 * point count, drawContours FILLED, the contour's coordinates sorted by x and by y) and the shrink loop of :160-200 with
 * checkInteriorExterior (:6-112) all run as kernels; one count and the result block cross to the host.
 * src: 8UC1 or 8UC3 (BGR) in DEVICE memory, `row_stride` bytes a row (any value >= width * channels: a view into a larger image
 * works).  rect_out = (x, y, width, height); *status_out = 0 ok, 1 "the image is empty" (no foreground: cropper.cpp would fail on
 * contours[0]), 2 "no interior rectangle found" (the lists crossed on an empty rectangle); with 1 and 2 the rectangle is all zero
 * or empty and the call itself succeeds.  MIS_E_INVALID: a null pointer, a size <= 0, channels not 1 or 3, a stride below a row,
 * (width + 2) * (height + 2) >= 2^28 (the cropper's 32-bit state indices).  Other approximation modes than CHAIN_APPROX_NONE and
 * contour hierarchies are not built. */
int mis_crop_rect(MisContext* ctx, const void* src, int width, int height, int channels, size_t row_stride, int rect_out[4], int* status_out);
/* measurement aid (tools/crop_device_bench.py; cropper.cpp:124-209): the same call with events between its stages on the context's
 * stream.  ms[0] the mask, ms[1] the foreground labelling, ms[2] the background labelling, ms[3] the border slots and the read of
 * their count, ms[4] successor table and start states, ms[5] the doubling rounds, ms[6] counts, winner and walls, ms[7] the fill's
 * labelling, ms[8] the two prefix counts, ms[9] the shrink loop. */
enum { MIS_CROP_STAGES = 10 };
int mis_crop_rect_timed(MisContext* ctx, const void* src, int width, int height, int channels, size_t row_stride, int rect_out[4], int* status_out,
                        float ms[MIS_CROP_STAGES]);
/* the same (cropper.cpp:124-209) and source(croppingMask).copyTo(dst) (:202-207): the rectangle's pixels packed from dst's first
 * byte on, `dst_stride` bytes a row.  dst: DEVICE memory of the source's size (height rows of dst_stride >= width * channels bytes:
 * the rectangle is known on the device only when the copy is enqueued).  Nothing is copied unless the status is 0.  A caller that
 * can use a strided view of src needs no copy: mis_crop_rect. */
int mis_crop(MisContext* ctx, const void* src, int width, int height, int channels, size_t row_stride, void* dst, size_t dst_stride, int rect_out[4],
             int* status_out);
/* test hook for the stages of cropper.cpp:132-158: the chosen contour's point count and first pixel in raster order (y * width + x;
 * 0 and -1 without a contour), the histograms of its points' x (width entries) and y (height entries) with multiplicity -- the
 * sorted lists of :150-158 in counted form -- and the filled contour mask of :146-148 (width * height bytes, 0 / 255), all to HOST
 * memory. */
int mis_crop_debug_contour(MisContext* ctx, const void* src, int width, int height, int channels, size_t row_stride, int* count_out, int* first_out,
                           int32_t* xhist, int32_t* yhist, uint8_t* cmask_out);
/* the last crop call's counts (cropper.cpp:124-209 takes one pass; this takes launches): kernel launches, pointer-doubling rounds
 * (ceil(log2(8 * border pixels))), border pixels, the chosen contour's points.  *count = how many there are; at most `capacity`
 * are written. */
int mis_crop_stats(const MisContext* ctx, int* out, int capacity, int* count);

#ifdef __cplusplus
}
#endif
#endif
