// ba_ray_solve.h -- BundleAdjusterRay's host side (recalled from OpenCV 4.5 stitching/src/motion_estimators.cpp):
// the edge and observation tables, the camera records of every evaluation, the ordered combine of the per-edge normal
// equations and the CvLevMarq loop.  What evaluates the observations is the caller's `Eval`: the kernels of motion_ray.hip in the
// library, plain loops over the same ba_ray.h functions in tests/harness/ba_ray_host_harness.cpp.
//
//   struct Eval {
//       int prepare(MisContext*, const MisFeatures*, int n, const std::vector<BaRayEdge>&, const std::vector<BaRayObs>&);
//       double* records();      // where the host writes the 9 n x 10 doubles of an evaluation
//       // evaluates the records; afterwards err() holds the 3 total errors and, with jac, partials() the 44 sums of every edge
//       int run(MisContext*, bool jac);
//       const double* err(); const double* partials();
//   };
// The loop itself (ba_obs_solve) is shared with BundleAdjusterAffinePartial (ba_affine_solve.h), which has 4 parameters per
// camera too: what an adjuster brings is its MODEL -- the observation model of ba_ray.h / ba_affine.h plus, on the host,
//       static constexpr double STEP;                                           // central-difference step
//       static const char* tag();                                               // for the trace line
//       static void start(const MisCameraParams&, double q[4]);                 // setUpInitialCameraParams
//       static void record(const double q[4], const MisFeatures&, double* rec); // the camera record of parameters q
//       static void refined(const double q[4], MisCameraParams*);               // obtainRefinedCameraParams
#pragma once
#include "ba_ray.h"
#include "motion_host.h"

namespace {

// record of a camera with parameters (focal, rotation vector) = q: H = R K^-1, K = [[f, 0, w/2], [0, f, h/2], [0, 0, 1]]
void ba_ray_record(const double* q, int img_w, int img_h, double* rec) {
    double R[9], Ki[9];
    rodrigues_to_mat(q + 1, R);
    const double K[9] = {q[0], 0, img_w * 0.5, 0, q[0], img_h * 0.5, 0, 0, 1};
    inv3(K, Ki);
    mul3(R, Ki, rec);
    rec[9] = q[0];
}

struct BaRayModel : BaRayObsModel {
    static constexpr double STEP = BA_RAY_STEP;
    static const char* tag() { return "ray"; }
    // focal as given, R projected on SO(3) and turned into a rotation vector
    static void start(const MisCameraParams& c, double* q) { q[0] = c.focal; ba_start_rvec(c.R, q + 1); }
    static void record(const double* q, const MisFeatures& f, double* rec) { ba_ray_record(q, f.img_w, f.img_h, rec); }
    // focal and R; ppx, ppy, aspect and t stay as given
    static void refined(const double* q, MisCameraParams* c) { c->focal = q[0]; ba_refined_R(q + 1, c->R); }
};

template <class MODEL, class Eval>
int ba_obs_solve(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh, MisCameraParams* cameras, Eval& ev) {
    constexpr int REC = MODEL::REC, ERRS = MODEL::ERRS;
    // leave only consistent image pairs; every index is checked here, before anything reads a keypoint through it
    std::vector<BaRayEdge> edges;
    std::vector<BaRayObs> obs;
    for (int i = 0; i < n - 1; i++)
        for (int j = i + 1; j < n; j++) {
            const MisMatchesInfo& mi = pairwise[i * n + j];
            if (!(mi.confidence > conf_thresh)) continue;
            const int first = (int)obs.size();
            for (int k = 0; k < mi.n_matches; k++) {
                if (!mi.inliers_mask || !mi.inliers_mask[k]) continue;
                const MisDMatch& m = mi.matches[k];
                MIS_CHECK(ctx, m.query_idx >= 0 && m.query_idx < features[i].n && m.train_idx >= 0 && m.train_idx < features[j].n, MIS_E_INVALID,
                          "match indices of pair (%d, %d) exceed the feature counts", i, j);
                obs.push_back({(int)edges.size(), m.query_idx, m.train_idx});
            }
            edges.push_back({i, j, first, (int)obs.size() - first});
        }
    const int total = (int)obs.size(), ne = (int)edges.size();
    MIS_CHECK(ctx, total > 0, MIS_E_INVALID, "bundle adjustment: no image pair above the confidence threshold");
    // setUpInitialCameraParams
    std::vector<double> cam((size_t)n * 4);
    for (int i = 0; i < n; i++) MODEL::start(cameras[i], &cam[i * 4]);
    if (int rc = ev.prepare(ctx, features, n, edges, obs)) return rc;

    LevMarq solver(n * 4, total * ERRS, 1000, DBL_EPSILON, false);   // TermCriteria(EPS + COUNT, 1000, DBL_EPSILON); no host J
    solver.param = cam;
    int evals = 0;
    const bool trace = getenv("MIS_BA_TRACE") != nullptr;
    for (;;) {
        bool want_J, want_err;
        const bool proceed = solver.update(want_J, want_err);
        if (trace) fprintf(stderr, "[ba %s] state %d iters %d lambdaLg10 %d prevErr %.17g err %.17g evaluations %d observations %d\n", MODEL::tag(), solver.state, solver.iters, solver.lambdaLg10, solver.prevErrNorm, solver.errNorm, evals, total);
        cam = solver.param;
        if (!proceed || !want_err) break;
        double* rec = ev.records();
        for (int c = 0; c < n; c++) MODEL::record(&cam[c * 4], features[c], rec + (size_t)c * REC);
        if (want_J)
            for (int c = 0; c < n; c++)
                for (int p = 0; p < 4; p++)
                    for (int s = 0; s < 2; s++) {
                        double q[4] = {cam[c * 4], cam[c * 4 + 1], cam[c * 4 + 2], cam[c * 4 + 3]};
                        q[p] = s ? q[p] + MODEL::STEP : q[p] - MODEL::STEP;
                        MODEL::record(q, features[c], rec + (size_t)ba_ray_slot(n, c, p, s) * REC);
                    }
        if (int rc = ev.run(ctx, want_J)) return rc;
        evals++;
        memcpy(solver.err.data(), ev.err(), sizeof(double) * (size_t)total * ERRS);
        if (want_J) {
            // JtJ(a, b) = sum over the edges that hold both columns' cameras, ascending, from +0; the same for JtErr
            std::fill(solver.JtJ.v.begin(), solver.JtJ.v.end(), 0.);
            std::fill(solver.JtErr.begin(), solver.JtErr.end(), 0.);
            const double* P = ev.partials();
            for (int e = 0; e < ne; e++)
                for (int t = 0; t < BA_RAY_CHAINS; t++) {
                    int a, b;
                    ba_ray_chain(t, &a, &b);
                    const int ga = 4 * (a < 4 ? edges[e].i : edges[e].j) + (a & 3);
                    const double v = P[(size_t)e * BA_RAY_CHAINS + t];
                    if (b < 0) solver.JtErr[ga] += v;
                    else solver.JtJ(ga, 4 * (b < 4 ? edges[e].i : edges[e].j) + (b & 3)) += v;
                }
        }
    }
    for (double v : cam) MIS_CHECK(ctx, std::isfinite(v), MIS_E_INVALID, "bundle adjustment diverged (non-finite camera parameter)");
    // obtainRefinedCameraParams
    for (int i = 0; i < n; i++) MODEL::refined(&cam[i * 4], &cameras[i]);
    ba_normalise_to_centre(n, pairwise, cameras);
    return MIS_OK;
}

template <class Eval>
int ba_ray_solve(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh, MisCameraParams* cameras, Eval& ev) {
    return ba_obs_solve<BaRayModel>(ctx, features, pairwise, n, conf_thresh, cameras, ev);
}

}  // namespace
