// motion.hip -- camera refinement between matching and warping, host logic of the library:
//   (*adjuster)(features, pairwise_matches, cameras) with BundleAdjusterReproj   image_stitching/image_stitching.cpp:681-712
//   waveCorrect(rmats, WAVE_CORRECT_HORIZ)                                       image_stitching/image_stitching.cpp:718-726
//   (*estimator)(features, pairwise_matches, cameras) with HomographyBasedEstimator   image_stitching/image_stitchin3g.cpp:746-779
// The reference runs both on the CPU inside OpenCV (stitching/src/motion_estimators.cpp, calib3d CvLevMarq, core
// JacobiSVD / Jacobi eigen, calib3d Rodrigues); restated here from the published algorithms with the reference's precisions: the
// cameras' rotations are CV_32F (image_stitching.cpp:626-634), the solver state is CV_64F, the refined rotations leave as CV_32F
// and wave correction runs in CV_32F.  PARITY UNPINNED (OpenCV absent offline); bit-exact against the oracle's independent
// restatement (oracle/mo_motion.c, tests/test_motion_gpu.py).
// No kernels: the data is a few thousand inlier correspondences and 7 parameters per camera.
#include "motion_host.h"

namespace {

// ---------------------------------------------------------------- BundleAdjusterReproj ----------
struct Edge { int i, j; };
struct Obs { float x1, y1, x2, y2; };   // inlier correspondence of an edge: keypoint of image i, keypoint of image j

struct Adjuster {
    int n = 0;
    std::vector<Edge> edges;
    std::vector<std::vector<Obs>> obs;    // per edge
    int total = 0;
    std::vector<double> cam;              // 7 per camera: focal, ppx, ppy, aspect, rvec
    uint8_t refine[5] = {1, 1, 1, 1, 1};   // focal, skew (unused), ppx, aspect, ppy  -- ba_refine_mask "xxxxx"

    std::vector<int> edge_m;                  // first observation of every edge (set by index_edges)
    std::vector<std::vector<int>> cam_edges;  // per camera: the edges it is part of, ascending
    void index_edges() {
        edge_m.assign(edges.size(), 0);
        cam_edges.assign(n, {});
        int m = 0;
        for (size_t e = 0; e < edges.size(); e++) { edge_m[e] = m; m += (int)obs[e].size(); cam_edges[edges[e].i].push_back((int)e); cam_edges[edges[e].j].push_back((int)e); }
    }
    void calc_error(std::vector<double>& err) const { calc_error_at(cam, err, nullptr); }
    // only: the edges to evaluate (the other rows of err are left as they are); nullptr: all, err is resized and zeroed first
    void calc_error_at(const std::vector<double>& cam, std::vector<double>& err, const std::vector<int>* only) const {
        if (!only) err.assign((size_t)total * 2, 0.);
        const size_t ne = only ? only->size() : edges.size();
        for (size_t q = 0; q < ne; q++) {
            const size_t e = only ? (size_t)(*only)[q] : q;
            int m = edge_m[e];
            const int i = edges[e].i, j = edges[e].j;
            const double f1 = cam[i * 7], f2 = cam[j * 7], ppx1 = cam[i * 7 + 1], ppx2 = cam[j * 7 + 1], ppy1 = cam[i * 7 + 2], ppy2 = cam[j * 7 + 2];
            const double a1 = cam[i * 7 + 3], a2 = cam[j * 7 + 3];
            double R1[9], R2[9], R2i[9];
            rodrigues_to_mat(&cam[i * 7 + 4], R1);
            rodrigues_to_mat(&cam[j * 7 + 4], R2);
            const double K1[9] = {f1, 0, ppx1, 0, f1 * a1, ppy1, 0, 0, 1}, K2[9] = {f2, 0, ppx2, 0, f2 * a2, ppy2, 0, 0, 1};
            double K1i[9], H[9];
            inv3(K1, K1i);
            inv3(R2, R2i);
            mul3(K2, R2i, H); mul3(H, R1, H); mul3(H, K1i, H);      // H1to2 = K2 * R2^-1 * R1 * K1^-1
            for (const Obs& o : obs[e]) {
                const double x = H[0] * o.x1 + H[1] * o.y1 + H[2], y = H[3] * o.x1 + H[4] * o.y1 + H[5], z = H[6] * o.x1 + H[7] * o.y1 + H[8];
                err[2 * m] = o.x2 - x / z;
                err[2 * m + 1] = o.y2 - y / z;
                m++;
            }
        }
    }
    void calc_jacobian(Mat& J) {
        const double step = 1e-4;
        // columns: 0 focal, 1 ppx, 2 ppy, 3 aspect, 4..6 rotation; refinement mask positions (0,0) (0,2) (1,2) (1,1).  A column is a pair
        // of error evaluations at its own perturbed copy of the cameras: one column per host thread at a time
        const bool on[7] = {(bool)refine[0], (bool)refine[2], (bool)refine[4], (bool)refine[3], true, true, true};
        // (only the rows of the pairs the column's camera is part of are evaluated and written: elsewhere the two evaluations are
        // identical, their difference is +0, and J was zeroed by the solver before this call)
        ba_parallel_for(7 * n, [&](int col) {
            if (!on[col % 7]) return;
            const std::vector<int>& mine = cam_edges[col / 7];
            std::vector<double> c = cam, e1((size_t)total * 2), e2((size_t)total * 2);
            const double val = c[col];
            c[col] = val - step; calc_error_at(c, e1, &mine);
            c[col] = val + step; calc_error_at(c, e2, &mine);
            for (int e : mine)
                for (int k = 2 * edge_m[e]; k < 2 * (edge_m[e] + (int)obs[e].size()); k++) J(k, col) = (e2[k] - e1[k]) / (2 * step);
        });
    }
};

inline float hypot_cv(float a, float b) {   // cv::hypot(float, float)
    a = std::fabs(a); b = std::fabs(b);
    if (a > b) { b /= a; return a * std::sqrt(1 + b * b); }
    if (b > 0) { a /= b; return b * std::sqrt(1 + a * a); }
    return 0;
}

// cv::eigen of a symmetric n x n CV_32F matrix (core/src/lapack.cpp JacobiImpl_<float>): cyclic pivoting on the largest
// off-diagonal element of the upper triangle (row / column maxima kept in indR / indC), eigenvalues descending, eigenvectors as rows
void jacobi_eigen_f32(float* A, int n, float* W, float* V) {
    const float eps = FLT_EPSILON;
    std::vector<int> indR(n), indC(n);
    for (int i = 0; i < n; i++) { for (int j = 0; j < n; j++) V[i * n + j] = 0; V[i * n + i] = 1; }
    auto row_max = [&](int k) { int m = k + 1; float mv = std::fabs(A[n * k + m]); for (int i = k + 2; i < n; i++) { const float val = std::fabs(A[n * k + i]); if (mv < val) mv = val, m = i; } return m; };
    auto col_max = [&](int k) { int m = 0; float mv = std::fabs(A[k]); for (int i = 1; i < k; i++) { const float val = std::fabs(A[n * i + k]); if (mv < val) mv = val, m = i; } return m; };
    for (int k = 0; k < n; k++) {
        W[k] = A[(n + 1) * k];
        if (k < n - 1) indR[k] = row_max(k);
        if (k > 0) indC[k] = col_max(k);
    }
    if (n > 1)
        for (int iters = 0; iters < n * n * 30; iters++) {
            int k = 0;
            float mv = std::fabs(A[indR[0]]);
            for (int i = 1; i < n - 1; i++) { const float val = std::fabs(A[n * i + indR[i]]); if (mv < val) mv = val, k = i; }
            int l = indR[k];
            for (int i = 1; i < n; i++) { const float val = std::fabs(A[n * indC[i] + i]); if (mv < val) mv = val, k = indC[i], l = i; }
            const float p = A[n * k + l];
            if (std::fabs(p) <= eps) break;
            const float y = (float)((W[l] - W[k]) * 0.5);
            float t = std::fabs(y) + hypot_cv(p, y);
            float sn = hypot_cv(p, t);
            const float c = t / sn;
            sn = p / sn; t = (p / t) * p;
            if (y < 0) sn = -sn, t = -t;
            A[n * k + l] = 0;
            W[k] -= t; W[l] += t;
            auto rot = [&](float& v0, float& v1) { const float a0 = v0, b0 = v1; v0 = a0 * c - b0 * sn; v1 = a0 * sn + b0 * c; };
            for (int i = 0; i < k; i++) rot(A[n * i + k], A[n * i + l]);
            for (int i = k + 1; i < l; i++) rot(A[n * k + i], A[n * i + l]);
            for (int i = l + 1; i < n; i++) rot(A[n * k + i], A[n * l + i]);
            for (int i = 0; i < n; i++) rot(V[n * k + i], V[n * l + i]);
            for (int j = 0; j < 2; j++) {
                const int idx = j == 0 ? k : l;
                if (idx < n - 1) indR[idx] = row_max(idx);
                if (idx > 0) indC[idx] = col_max(idx);
            }
        }
    for (int k = 0; k < n - 1; k++) {
        int m = k;
        for (int i = k + 1; i < n; i++) if (W[m] < W[i]) m = i;
        if (k != m) { std::swap(W[m], W[k]); for (int i = 0; i < n; i++) std::swap(V[n * m + i], V[n * k + i]); }
    }
}

}  // namespace

extern "C" int mis_bundle_adjust_reproj(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh,
                                        const char* refine_mask, MisCameraParams* cameras) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, features && pairwise && cameras && n >= 2, MIS_E_INVALID, "null argument or fewer than two cameras");
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    Adjuster ad;
    ad.n = n;
    if (refine_mask && strlen(refine_mask) >= 5)
        for (int k = 0; k < 5; k++) ad.refine[k] = refine_mask[k] == 'x';
    // keypoints of every image to the host (a few hundred KB)
    std::vector<std::vector<MisKeyPoint>> kps(n);
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; i++) {
        kps[i].resize((size_t)std::max(features[i].n, 0));
        if (features[i].n > 0) MIS_HIP(ctx, hipMemcpy(kps[i].data(), features[i].keypoints, sizeof(MisKeyPoint) * (size_t)features[i].n, hipMemcpyDeviceToHost));
    }
    // setUpInitialCameraParams: R projected on SO(3) through its SVD, then Rodrigues
    ad.cam.assign((size_t)n * 7, 0.);
    for (int i = 0; i < n; i++) {
        ad.cam[i * 7] = cameras[i].focal; ad.cam[i * 7 + 1] = cameras[i].ppx; ad.cam[i * 7 + 2] = cameras[i].ppy; ad.cam[i * 7 + 3] = cameras[i].aspect;
        ba_start_rvec(cameras[i].R, &ad.cam[i * 7 + 4]);
    }
    // leave only consistent image pairs
    for (int i = 0; i < n - 1; i++)
        for (int j = i + 1; j < n; j++) {
            const MisMatchesInfo& mi = pairwise[i * n + j];
            if (!(mi.confidence > conf_thresh)) continue;
            std::vector<Obs> ob;
            for (int k = 0; k < mi.n_matches; k++) {
                if (!mi.inliers_mask || !mi.inliers_mask[k]) continue;
                const MisDMatch& m = mi.matches[k];
                MIS_CHECK(ctx, m.query_idx >= 0 && m.query_idx < (int)kps[i].size() && m.train_idx >= 0 && m.train_idx < (int)kps[j].size(), MIS_E_INVALID,
                          "match indices of pair (%d, %d) exceed the feature counts", i, j);
                ob.push_back({kps[i][m.query_idx].x, kps[i][m.query_idx].y, kps[j][m.train_idx].x, kps[j][m.train_idx].y});
            }
            ad.edges.push_back({i, j});
            ad.total += (int)ob.size();
            ad.obs.push_back(std::move(ob));
        }
    MIS_CHECK(ctx, ad.total > 0, MIS_E_INVALID, "bundle adjustment: no image pair above the confidence threshold");
    ad.index_edges();
    LevMarq solver(n * 7, ad.total * 2, 1000, DBL_EPSILON);   // TermCriteria(EPS + COUNT, 1000, DBL_EPSILON)
    solver.param = ad.cam;
    {
        // the rows of an edge (two per observation, in edge order) depend on the parameters of its two cameras only
        std::vector<std::vector<std::pair<int, int>>> cam_rows(n);
        int row = 0;
        for (size_t e = 0; e < ad.edges.size(); e++) {
            const int r1 = row + 2 * (int)ad.obs[e].size();
            for (int c : {ad.edges[e].i, ad.edges[e].j}) {
                auto& v = cam_rows[c];
                if (!v.empty() && v.back().second == row) v.back().second = r1; else v.emplace_back(row, r1);
            }
            row = r1;
        }
        solver.col_rows.resize((size_t)n * 7);
        for (int c = 0; c < n; c++) for (int j = 0; j < 7; j++) solver.col_rows[c * 7 + j] = cam_rows[c];
    }
    const bool trace = getenv("MIS_BA_TRACE") != nullptr;
    for (;;) {
        bool want_J, want_err;
        const bool proceed = solver.update(want_J, want_err);
        if (trace) fprintf(stderr, "[ba] state %d iters %d lambdaLg10 %d prevErr %.17g err %.17g p0 %.17g p4 %.17g\n", solver.state, solver.iters, solver.lambdaLg10, solver.prevErrNorm, solver.errNorm, solver.param[0], solver.param[4]);
        ad.cam = solver.param;
        if (!proceed || !want_err) break;
        if (want_J) ad.calc_jacobian(solver.J);
        if (want_err) ad.calc_error(solver.err);
    }
    for (double v : ad.cam) MIS_CHECK(ctx, std::isfinite(v), MIS_E_INVALID, "bundle adjustment diverged (non-finite camera parameter)");
    // obtainRefinedCameraParams
    for (int i = 0; i < n; i++) {
        cameras[i].focal = ad.cam[i * 7]; cameras[i].ppx = ad.cam[i * 7 + 1]; cameras[i].ppy = ad.cam[i * 7 + 2]; cameras[i].aspect = ad.cam[i * 7 + 3];
        ba_refined_R(&ad.cam[i * 7 + 4], cameras[i].R);
    }
    ba_normalise_to_centre(n, pairwise, cameras);
    return MIS_OK;
}

// detail::waveCorrect (motion_estimators.cpp): kind 0 = WAVE_CORRECT_HORIZ, 1 = WAVE_CORRECT_VERT; rmats: n x 9 doubles holding the
// CV_32F rotations the reference passes (image_stitching.cpp:720-722); everything in float as there, results returned in place
extern "C" int mis_wave_correct(double* rmats, int n, int kind) {
    if (!rmats || n < 1 || (kind != 0 && kind != 1)) return MIS_E_INVALID;
    if (n <= 1) return MIS_OK;
    std::vector<float> R((size_t)n * 9);
    for (int i = 0; i < 9 * n; i++) R[i] = (float)rmats[i];
    float moment[9] = {0};
    for (int i = 0; i < n; i++) {
        const float col[3] = {R[9 * i], R[9 * i + 3], R[9 * i + 6]};   // col(0): the camera's x axis
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) moment[a * 3 + b] += col[a] * col[b];
    }
    float evals[3], evecs[9];
    jacobi_eigen_f32(moment, 3, evals, evecs);
    float rg1[3], img_k[3] = {0, 0, 0};
    memcpy(rg1, kind == 0 ? evecs + 6 : evecs, sizeof(rg1));   // HORIZ: the eigenvector of the smallest eigenvalue; VERT: of the largest
    for (int i = 0; i < n; i++) { img_k[0] += R[9 * i + 2]; img_k[1] += R[9 * i + 5]; img_k[2] += R[9 * i + 8]; }   // sum of the z axes
    float rg0[3] = {rg1[1] * img_k[2] - rg1[2] * img_k[1], rg1[2] * img_k[0] - rg1[0] * img_k[2], rg1[0] * img_k[1] - rg1[1] * img_k[0]};
    const double rg0n = std::sqrt((double)rg0[0] * rg0[0] + (double)rg0[1] * rg0[1] + (double)rg0[2] * rg0[2]);
    if (rg0n <= DBL_MIN) return MIS_OK;
    for (float& v : rg0) v = (float)(v * (1. / rg0n));    // rg0 /= norm: scaled by the reciprocal, in double
    const float rg2[3] = {rg0[1] * rg1[2] - rg0[2] * rg1[1], rg0[2] * rg1[0] - rg0[0] * rg1[2], rg0[0] * rg1[1] - rg0[1] * rg1[0]};
    double conf = 0;
    for (int i = 0; i < n; i++) {
        const float* g = kind == 0 ? rg0 : rg1;     // Mat::dot on CV_32F: products and sum in double
        const double d = (double)g[0] * R[9 * i] + (double)g[1] * R[9 * i + 3] + (double)g[2] * R[9 * i + 6];
        conf += kind == 0 ? d : -d;
    }
    if (conf < 0) { for (float& v : rg0) v *= -1; for (float& v : rg1) v *= -1; }
    const float Rg[9] = {rg0[0], rg0[1], rg0[2], rg1[0], rg1[1], rg1[2], rg2[0], rg2[1], rg2[2]};
    for (int i = 0; i < n; i++) {
        float o[9];
        mul3(Rg, &R[9 * i], o);
        for (int k = 0; k < 9; k++) rmats[9 * i + k] = o[k];
    }
    return MIS_OK;
}

// ---------------------------------------------------------------- HomographyBasedEstimator ------
// estimator = makePtr<detail::HomographyBasedEstimator>(); (*estimator)(features, pairwise_matches, cameras), what
// Stitcher::create(PANORAMA) runs ahead of the ray adjuster.  Host logic (motion_host.h), no context:
// O(n^2) closed forms on nine doubles and a tree walk -- a launch would cost more than the work.
static bool sizes_ok(const MisSize* s, int n) {
    for (int i = 0; i < n; i++) if (s[i].width <= 0 || s[i].height <= 0) return false;
    return true;
}
extern "C" int mis_focals_from_homography(const double H[9], double* f0, double* f1, int* f0_ok, int* f1_ok) {
    if (!H || !f0 || !f1 || !f0_ok || !f1_ok) return MIS_E_INVALID;
    bool ok0, ok1;
    focals_from_homography(H, *f0, *f1, ok0, ok1);
    *f0_ok = ok0; *f1_ok = ok1;
    return MIS_OK;
}
extern "C" int mis_estimate_focal(const MisMatchesInfo* pairwise, int n, const MisSize* img_sizes, double* focals) {
    if (!pairwise || !img_sizes || !focals || n < 1 || !sizes_ok(img_sizes, n)) return MIS_E_INVALID;
    estimate_focal(n, pairwise, img_sizes, focals);
    return MIS_OK;
}
extern "C" int mis_estimate_homography_cameras(const MisMatchesInfo* pairwise, int n, const MisSize* img_sizes, MisCameraParams* cameras) {
    if (!pairwise || !img_sizes || !cameras || n < 1 || !sizes_ok(img_sizes, n)) return MIS_E_INVALID;
    estimate_homography_cameras(n, pairwise, img_sizes, cameras);
    return MIS_OK;
}
