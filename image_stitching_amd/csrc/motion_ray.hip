// motion_ray.hip -- BundleAdjusterRay: the adjuster behind ba_cost_func = "ray"
//   (*adjuster)(features, pairwise_matches, cameras) with BundleAdjusterRay        image_stitching/image_stitching.cpp:683-684
// The solver is the host's (ba_ray_solve.h over motion_host.h: CvLevMarq, the Jacobi SVD solve of the 4n x 4n system); what
// grows with the number of inlier matches runs here, once per evaluation, on the context's stream:
//   ba_eval_kernel<BaRayObsModel>   one thread per observation: its 3 errors and, in the Jacobian state, its 3 x 8 Jacobian entries
//   ba_normal_kernel<3>             one workgroup per edge, one thread per entry of the edge's 8 x 8 block of J^T J (upper triangle)
//                                   and of J^T err: a sequential sum over the edge's rows in ascending order
// (ba_eval_device.h: the kernels and the evaluator are shared with the affine-partial adjuster of motion_affine.hip).  The
// keypoints are read where the finder left them, in the features' device arrays.  The arithmetic is ba_ray.h's.
#include "ba_ray_solve.h"
#include "ba_eval_device.h"

extern "C" int mis_bundle_adjust_ray(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh, MisCameraParams* cameras) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, features && pairwise && cameras && n >= 2, MIS_E_INVALID, "null argument or fewer than two cameras");
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    BaDeviceEval<BaRayObsModel> ev;
    return ba_ray_solve(ctx, features, pairwise, n, conf_thresh, cameras, ev);
}
