// motion_affine.hip -- the affine family's motion estimation, what Stitcher::create(SCANS) puts in place
// of the homography estimator and the rotation adjusters:
//   estimator = makePtr<AffineBasedEstimator>()                                      (host: motion_host.h)
//   (*adjuster)(features, pairwise_matches, cameras) with BundleAdjusterAffinePartial  image_stitching/image_stitching.cpp:685-686
// The adjuster's solver is the host's (ba_affine_solve.h over ba_ray_solve.h and motion_host.h: CvLevMarq, the Jacobi SVD solve of
// the 4n x 4n system); what grows with the number of inlier matches runs on the device, once per evaluation, on the context's
// stream (ba_eval_device.h, shared with the ray adjuster):
//   ba_eval_kernel<BaAffineObsModel>   one thread per observation: its 2 errors and, in the Jacobian state, its 2 x 8 Jacobian entries
//   ba_normal_kernel<2>                one workgroup per edge: the 44 ordered sums of the edge's normal equations over 2 count rows
// The keypoints are read where the finder left them, in the features' device arrays.  The arithmetic is ba_affine.h's.
#include "ba_affine_solve.h"
#include "ba_eval_device.h"

extern "C" int mis_bundle_adjust_affine_partial(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh,
                                                MisCameraParams* cameras) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, features && pairwise && cameras && n >= 2, MIS_E_INVALID, "null argument or fewer than two cameras");
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    BaDeviceEval<BaAffineObsModel> ev;
    return ba_affine_solve(ctx, features, pairwise, n, conf_thresh, cameras, ev);
}

extern "C" int mis_estimate_affine_cameras(const MisMatchesInfo* pairwise, int n, MisCameraParams* cameras) {
    if (!pairwise || !cameras || n < 1) return MIS_E_INVALID;
    estimate_affine_cameras(n, pairwise, cameras);
    return MIS_OK;
}
