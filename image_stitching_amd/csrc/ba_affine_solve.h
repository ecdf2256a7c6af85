// ba_affine_solve.h -- BundleAdjusterAffinePartial's host side (recalled from OpenCV 4.5 stitching/src/motion_estimators.cpp,
// SURVEY.md A.15): BundleAdjusterBase(4 parameters per camera, 2 errors per match).  The edge and observation tables, the ordered
// combine of the per-edge normal equations, the CvLevMarq loop, its termination and the normalisation to the spanning tree's
// centre are ba_ray_solve.h's ba_obs_solve; this header brings the adjuster's model: which four numbers of a camera are refined,
// a camera's record, and how they are written back.  The refinement mask is ignored, as there.
#pragma once
#include "ba_affine.h"
#include "ba_ray_solve.h"

namespace {

struct BaAffineModel : BaAffineObsModel {
    static constexpr double STEP = BA_AFFINE_STEP;
    static const char* tag() { return "affine"; }
    // setUpInitialCameraParams: (a, b, tx, ty) = (R(0,0), R(1,0), R(0,2), R(1,2)) of the CV_32F rotation
    static void start(const MisCameraParams& c, double* q) {
        q[0] = (double)(float)c.R[0]; q[1] = (double)(float)c.R[3]; q[2] = (double)(float)c.R[2]; q[3] = (double)(float)c.R[5];
    }
    static void record(const double* q, const MisFeatures&, double* rec) { ba_affine_record(q, rec); }
    // obtainRefinedCameraParams: R = eye(3, CV_32F) with the four values written as floats; focal, aspect, ppx, ppy and t stay
    static void refined(const double* q, MisCameraParams* c) {
        const float a = (float)q[0], b = (float)q[1], tx = (float)q[2], ty = (float)q[3];
        const double R[9] = {a, -b, tx, b, a, ty, 0., 0., 1.};
        for (int k = 0; k < 9; k++) c->R[k] = R[k];
    }
};

template <class Eval>
int ba_affine_solve(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh, MisCameraParams* cameras, Eval& ev) {
    return ba_obs_solve<BaAffineModel>(ctx, features, pairwise, n, conf_thresh, cameras, ev);
}

}  // namespace
