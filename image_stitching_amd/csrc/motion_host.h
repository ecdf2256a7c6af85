// motion_host.h -- host pieces shared by the bundle adjusters (motion.hip: reprojection cost; motion_ray.hip: ray cost; motion_affine.hip:
// the affine-partial cost and the affine estimator) and the homography-based estimator with its focal estimation: small dense
// linear algebra, the Jacobi SVD and its solve, the Rodrigues pair, the CvLevMarq state machine and the spanning tree's centres.
// Restated from the published algorithms with the reference's precisions (see motion.hip).  Everything sits in an unnamed
// namespace: each translation unit that includes this header gets its own copy.
#pragma once
#include "common.h"
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <thread>
#include <vector>

namespace {

// ---------------------------------------------------------------- small dense linear algebra ---
struct Mat {
    int r = 0, c = 0;
    std::vector<double> v;
    Mat() {}
    Mat(int r_, int c_) : r(r_), c(c_), v((size_t)r_ * c_, 0.) {}
    double& operator()(int i, int j) { return v[(size_t)i * c + j]; }
    double operator()(int i, int j) const { return v[(size_t)i * c + j]; }
};

// 3x3 product: the written-out sums of OpenCV's small-matrix path, in the matrix type
template <typename T>
void mul3(const T* a, const T* b, T* o) {   // o = a * b (3x3)
    T t[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) t[i * 3 + j] = a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j] + a[i * 3 + 2] * b[6 + j];
    memcpy(o, t, sizeof(t));
}
// determinant / inverse: cofactors in double for either matrix type, the result stored in the matrix type (cv::determinant / cv::invert, 3x3)
template <typename T>
double det3(const T* a) {
    return a[0] * ((double)a[4] * a[8] - (double)a[5] * a[7]) - a[1] * ((double)a[3] * a[8] - (double)a[5] * a[6]) + a[2] * ((double)a[3] * a[7] - (double)a[4] * a[6]);
}
template <typename T>
bool inv3(const T* a, T* o) {
    double d = det3(a);
    if (d == 0) return false;
    d = 1. / d;
    const double t[9] = {((double)a[4] * a[8] - (double)a[5] * a[7]) * d, ((double)a[2] * a[7] - (double)a[1] * a[8]) * d, ((double)a[1] * a[5] - (double)a[2] * a[4]) * d,
                         ((double)a[5] * a[6] - (double)a[3] * a[8]) * d, ((double)a[0] * a[8] - (double)a[2] * a[6]) * d, ((double)a[2] * a[3] - (double)a[0] * a[5]) * d,
                         ((double)a[3] * a[7] - (double)a[4] * a[6]) * d, ((double)a[1] * a[6] - (double)a[0] * a[7]) * d, ((double)a[0] * a[4] - (double)a[1] * a[3]) * d};
    for (int i = 0; i < 9; i++) o[i] = (T)t[i];
    return true;
}

template <typename T> struct SvdTraits;
template <> struct SvdTraits<double> { static double eps() { return DBL_EPSILON * 10; } static double minval() { return DBL_MIN; } };
template <> struct SvdTraits<float> { static float eps() { return FLT_EPSILON * 2; } static double minval() { return FLT_MIN; } };

// core/src/lapack.cpp JacobiSVDImpl_<T>: one-sided Jacobi on the rows of At (n rows of length m); W = singular
// values (descending), rows of At become the left vectors scaled to unit length, Vt the right vectors.  The squared norms and
// the rotation angle are computed in double for either T, the rotations themselves in T.
template <typename T>
void jacobi_svd(T* At, int astep, T* Wout, T* Vt, int vstep, int m, int n) {
    const T eps = SvdTraits<T>::eps();
    const double minval = SvdTraits<T>::minval();
    std::vector<double> W(n);
    const int max_iter = std::max(m, 30);
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const T t = At[i * astep + k]; sd += (double)t * t; }
        W[i] = sd;
        for (int k = 0; k < n; k++) Vt[i * vstep + k] = 0;
        Vt[i * vstep + i] = 1;
    }
    for (int iter = 0; iter < max_iter; iter++) {
        bool changed = false;
        for (int i = 0; i < n - 1; i++)
            for (int j = i + 1; j < n; j++) {
                T *Ai = At + i * astep, *Aj = At + j * astep;
                double a = W[i], p = 0, b = W[j];
                for (int k = 0; k < m; k++) p += (double)Ai[k] * Aj[k];
                if (std::abs(p) <= eps * std::sqrt((double)a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = hypot((double)p, beta);
                T c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (T)std::sqrt(delta / gamma);
                    c = (T)(p / (gamma * s * 2));
                } else {
                    c = (T)std::sqrt((gamma + beta) / (gamma * 2));
                    s = (T)(p / (gamma * c * 2));
                }
                a = b = 0;
                for (int k = 0; k < m; k++) {
                    const T t0 = c * Ai[k] + s * Aj[k], t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0; Aj[k] = t1;
                    a += (double)t0 * t0; b += (double)t1 * t1;
                }
                W[i] = a; W[j] = b;
                changed = true;
                T *Vi = Vt + i * vstep, *Vj = Vt + j * vstep;
                for (int k = 0; k < n; k++) {
                    const T t0 = c * Vi[k] + s * Vj[k], t1 = -s * Vi[k] + c * Vj[k];
                    Vi[k] = t0; Vj[k] = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; i++) {
        double sd = 0;
        for (int k = 0; k < m; k++) { const T t = At[i * astep + k]; sd += (double)t * t; }
        W[i] = std::sqrt(sd);
    }
    for (int i = 0; i < n - 1; i++) {
        int j = i;
        for (int k = i + 1; k < n; k++) if (W[j] < W[k]) j = k;
        if (i != j) {
            std::swap(W[i], W[j]);
            for (int k = 0; k < m; k++) std::swap(At[i * astep + k], At[j * astep + k]);
            for (int k = 0; k < n; k++) std::swap(Vt[i * vstep + k], Vt[j * vstep + k]);
        }
    }
    for (int i = 0; i < n; i++) {
        Wout[i] = (T)W[i];
        const T s = (T)(W[i] > minval ? 1 / W[i] : 0.);   // (degenerate directions: zeroed; the random completion of
        for (int k = 0; k < m; k++) At[i * astep + k] *= s;   //  OpenCV only matters for full bases, not for solve)
    }
}

// cv::solve(A, b, x, DECOMP_SVD) for a square system: SVD of A, then SVBkSb with the threshold 2 eps sum(w)
bool solve_svd(const Mat& A, const std::vector<double>& b, std::vector<double>& x) {
    const int n = A.r;
    // JacobiSVD works on the transposed matrix: rows of At = columns of A; A = U diag(w) Vt with At rows -> u_i
    Mat At(n, n), Vt(n, n);
    for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) At(i, j) = A(j, i);
    std::vector<double> w(n);
    jacobi_svd(At.v.data(), n, w.data(), Vt.v.data(), n, n, n);
    // after the call: At(i, :) = i-th left singular vector (as a row), Vt(i, :) = i-th right singular vector
    double thr = 0;
    for (int i = 0; i < n; i++) thr += w[i];
    thr *= 2 * DBL_EPSILON;
    x.assign(n, 0.);
    for (int i = 0; i < n; i++) {
        if (!(w[i] > thr)) continue;
        double s = 0;
        for (int k = 0; k < n; k++) s += At(i, k) * b[k];
        s /= w[i];
        for (int k = 0; k < n; k++) x[k] += s * Vt(i, k);
    }
    return true;
}

// 3x3 SVD through the same routine: R = U diag(w) Vt  (u, vt as 3x3 row-major)
template <typename T>
void svd3(const T* R, T* u, T* w, T* vt) {
    T At[9], Vt[9];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) At[i * 3 + j] = R[j * 3 + i];
    jacobi_svd(At, 3, w, Vt, 3, 3, 3);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { u[j * 3 + i] = At[i * 3 + j]; vt[i * 3 + j] = Vt[i * 3 + j]; }
}

// calib3d Rodrigues: rotation vector -> matrix
void rodrigues_to_mat(const double* r, double* R) {
    const double theta = std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    if (theta < DBL_EPSILON) { double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}; memcpy(R, I, sizeof(I)); return; }
    // cos and sin of one angle through ONE sincos call, as the oracle does: gcc merges separate calls into sincos, clang does not,
    // and glibc's sincos differs from its cos / sin in the last place for some arguments (found on a 6-camera scene: one float ulp in R)
    double c, s;
    ::sincos(theta, &s, &c);
    const double c1 = 1. - c, it = 1 / theta;
    const double x = r[0] * it, y = r[1] * it, z = r[2] * it;
    const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
    const double rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; k++) R[k] = c * I[k] + c1 * rrt[k] + s * rx[k];
}
// matrix -> rotation vector (cvRodrigues2 projects the matrix on SO(3) through its SVD first)
void rodrigues_to_vec(const double* Rin, double* r) {
    double U[9], W[3], Vt[9], R[9];
    svd3(Rin, U, W, Vt);
    mul3(U, Vt, R);
    double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = std::sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
    double c = (R[0] + R[4] + R[8] - 1) * 0.5;
    c = c > 1. ? 1. : (c < -1. ? -1. : c);
    double theta = std::acos(c);
    if (s < 1e-5) {
        if (c > 0) { r[0] = r[1] = r[2] = 0; return; }
        double t;
        t = (R[0] + 1) * 0.5; rx = std::sqrt(std::max(t, 0.));
        t = (R[4] + 1) * 0.5; ry = std::sqrt(std::max(t, 0.)) * (R[1] < 0 ? -1. : 1.);
        t = (R[8] + 1) * 0.5; rz = std::sqrt(std::max(t, 0.)) * (R[2] < 0 ? -1. : 1.);
        if (std::fabs(rx) < std::fabs(ry) && std::fabs(rx) < std::fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
        theta /= std::sqrt(rx * rx + ry * ry + rz * rz);
        r[0] = rx * theta; r[1] = ry * theta; r[2] = rz * theta;
        return;
    }
    double vth = 1 / (2 * s);
    vth *= theta;
    r[0] = rx * vth; r[1] = ry * vth; r[2] = rz * vth;
}

// Host threads for the two loops that make bundle adjustment slow at 16 x 4K (round 4: 3.7 s per job on one thread; every item is
// computed as before -- each sum walks its terms in the same order -- so the results are the same bits)
template <class F>
static void ba_parallel_for(int n, F f) {
    const int nt = std::max(1, std::min<int>({n, 16, (int)std::thread::hardware_concurrency()}));
    if (nt == 1) { for (int i = 0; i < n; i++) f(i); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back([=]() { for (int i = t; i < n; i += nt) f(i); });
    for (auto& x : th) x.join();
}

// ---------------------------------------------------------------- CvLevMarq ---------------------
// calib3d compat_ptsetreg.cpp: the state machine of the Levenberg-Marquardt solver BundleAdjusterBase drives
struct LevMarq {
    enum { DONE = 0, STARTED = 1, CALC_J = 2, CHECK_ERR = 3 };
    int nparams, nerrs, max_iter, state = STARTED, iters = 0, lambdaLg10 = -3;
    double epsilon, prevErrNorm = DBL_MAX, errNorm = 0;
    std::vector<double> param, prevParam, err, JtErr;
    Mat J, JtJ;
    std::vector<std::vector<std::pair<int, int>>> col_rows;      // optional: per column of J, the row ranges [first, second) that can be non-zero
    // host_J = false: there is no host J; whenever update() asks for J the caller fills JtJ (upper triangle) and JtErr itself
    bool host_J;
    LevMarq(int np, int ne, int maxit, double eps, bool host_J_ = true)
        : nparams(np), nerrs(ne), max_iter(maxit), epsilon(eps), param(np, 0.), prevParam(np, 0.), err(ne, 0.), JtErr(np, 0.), J(host_J_ ? ne : 0, host_J_ ? np : 0), JtJ(np, np), host_J(host_J_) {}
    void step() {
        const double lambda = std::exp(lambdaLg10 * std::log(10.));
        Mat A = JtJ;
        for (int i = 0; i < nparams; i++) for (int j = 0; j < i; j++) A(i, j) = A(j, i);   // completeSymm (upper -> lower)
        for (int i = 0; i < nparams; i++) A(i, i) *= 1. + lambda;
        std::vector<double> d;
        solve_svd(A, JtErr, d);
        if (getenv("MIS_BA_TRACE")) {      // diagnostics: bit checksums of the step's system and its solution (the oracle prints the same)
            unsigned long long ha = 0, hb = 0, hd = 0, t;
            for (size_t q = 0; q < A.v.size(); q++) { memcpy(&t, &A.v[q], 8); ha += t * (q + 1); }
            for (int q = 0; q < nparams; q++) { memcpy(&t, &JtErr[q], 8); hb += t * (unsigned long long)(q + 1); memcpy(&t, &d[q], 8); hd += t * (unsigned long long)(q + 1); }
            fprintf(stderr, "[ba] step lambdaLg10 %d A %016llx JtErr %016llx delta %016llx\n", lambdaLg10, ha, hb, hd);
        }
        for (int i = 0; i < nparams; i++) param[i] = prevParam[i] - d[i];
    }
    // normL2Sqr<double, double>: groups of four, as the unrolled loop of core's stat code adds them
    static double l2sqr(const double* a, const double* b, int n) {
        double s = 0;
        int i = 0;
        for (; i <= n - 4; i += 4) {
            const double v0 = a[i] - (b ? b[i] : 0.), v1 = a[i + 1] - (b ? b[i + 1] : 0.), v2 = a[i + 2] - (b ? b[i + 2] : 0.), v3 = a[i + 3] - (b ? b[i + 3] : 0.);
            s += v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3;
        }
        for (; i < n; i++) { const double v = a[i] - (b ? b[i] : 0.); s += v * v; }
        return s;
    }
    static double norm2(const std::vector<double>& a) { return std::sqrt(l2sqr(a.data(), nullptr, (int)a.size())); }
    // returns proceed; want_J / want_err tell the caller what to compute for `param`
    bool update(bool& want_J, bool& want_err) {
        want_J = want_err = false;
        if (state == DONE) return false;
        if (state == STARTED) {
            std::fill(J.v.begin(), J.v.end(), 0.); std::fill(err.begin(), err.end(), 0.);
            want_J = want_err = true; state = CALC_J;
            return true;
        }
        if (state == CALC_J) {
            // JtJ = J^T J (upper triangle), JtErr = J^T err: every entry the same sequential sum over the rows of J as before, one row of
            // JtJ per host thread.  col_rows (set by the caller): per column the row ranges outside which the column is exactly zero -- a
            // camera's parameters only move the errors of the pairs the camera is part of, and a central difference of two identical
            // evaluations is +0 --; a product with such a zero is +-0 and adding it leaves a sum that is not -0 unchanged, so the sums
            // walk the intersection of the two columns' ranges only (16 cameras: 60 x fewer terms).  Without col_rows: all rows, read
            // from a transposed copy (J's columns are 8 nparams bytes apart).
            if (!host_J) {
                // JtJ and JtErr are the caller's
            } else if (!col_rows.empty()) {
                ba_parallel_for(nparams, [&](int i) {
                    const auto& ri = col_rows[i];
                    for (int j = i; j < nparams; j++) {
                        const auto& rj = col_rows[j];
                        double s = 0;
                        size_t a = 0, b = 0;
                        while (a < ri.size() && b < rj.size()) {      // sorted, disjoint ranges: their intersection in row order
                            const int lo = std::max(ri[a].first, rj[b].first), hi = std::min(ri[a].second, rj[b].second);
                            for (int k = lo; k < hi; k++) s += J(k, i) * J(k, j);
                            if (ri[a].second < rj[b].second) a++; else b++;
                        }
                        JtJ(i, j) = s;
                    }
                    double s = 0;
                    for (const auto& r : ri)
                        for (int k = r.first; k < r.second; k++) s += J(k, i) * err[k];
                    JtErr[i] = s;
                });
            } else {
                const size_t ne = (size_t)nerrs;
                std::vector<double> Jt((size_t)nparams * ne);
                ba_parallel_for(nparams, [&](int i) { double* o = Jt.data() + (size_t)i * ne; for (int k = 0; k < nerrs; k++) o[k] = J(k, i); });
                ba_parallel_for(nparams, [&](int i) {
                    const double* a = Jt.data() + (size_t)i * ne;
                    for (int j = i; j < nparams; j++) {
                        const double* b = Jt.data() + (size_t)j * ne;
                        double s = 0;
                        for (int k = 0; k < nerrs; k++) s += a[k] * b[k];
                        JtJ(i, j) = s;
                    }
                    double s = 0;
                    for (int k = 0; k < nerrs; k++) s += a[k] * err[k];
                    JtErr[i] = s;
                });
            }
            prevParam = param;
            step();
            if (iters == 0) prevErrNorm = norm2(err);
            std::fill(err.begin(), err.end(), 0.);
            want_err = true; state = CHECK_ERR;
            return true;
        }
        errNorm = norm2(err);
        if (errNorm > prevErrNorm) {
            if (++lambdaLg10 <= 16) {
                step();
                std::fill(err.begin(), err.end(), 0.);
                want_err = true; state = CHECK_ERR;
                return true;
            }
        }
        lambdaLg10 = std::max(lambdaLg10 - 1, -16);
        // cvNorm(param, prevParam, CV_RELATIVE_L2)
        const double change = std::sqrt(l2sqr(param.data(), prevParam.data(), nparams)) / (std::sqrt(l2sqr(prevParam.data(), nullptr, nparams)) + DBL_EPSILON);
        if (++iters >= max_iter || change < epsilon) { state = DONE; return true; }
        prevErrNorm = errNorm;
        std::fill(J.v.begin(), J.v.end(), 0.);
        want_J = want_err = true; state = CALC_J;
        return true;
    }
};

// stitching/src/motion_estimators.cpp findMaxSpanningTree: Kruskal on num_inliers (descending), then the tree's centres
// (tree: optionally the spanning tree's adjacency lists, neighbours in the order the edges were added)
void max_spanning_tree_centers(int n, const MisMatchesInfo* pm, std::vector<int>& centers, std::vector<std::vector<int>>* tree = nullptr) {
    struct GE { int from, to; float w; };
    std::vector<GE> all;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            if (pm[i * n + j].has_H == 0) continue;
            const float w = (float)pm[i * n + j].num_inliers;
            all.push_back({i, j, w});
        }
    std::stable_sort(all.begin(), all.end(), [](const GE& a, const GE& b) { return a.w > b.w; });
    std::vector<int> parent(n), rnk(n, 0);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int e) { int s = e; while (s != parent[s]) s = parent[s]; while (e != parent[e]) { int nx = parent[e]; parent[e] = s; e = nx; } return s; };
    std::vector<std::vector<int>> adj(n);
    std::vector<int> power(n, 0);
    for (const GE& e : all) {
        int c1 = find(e.from), c2 = find(e.to);
        if (c1 == c2) continue;
        if (rnk[c1] < rnk[c2]) parent[c1] = c2; else if (rnk[c2] < rnk[c1]) parent[c2] = c1; else { parent[c1] = c2; rnk[c2]++; }
        adj[e.from].push_back(e.to); adj[e.to].push_back(e.from);
        power[e.from]++; power[e.to]++;
    }
    std::vector<int> leafs;
    for (int i = 0; i < n; i++) if (power[i] == 1) leafs.push_back(i);
    // distance from every leaf (BFS); the centres minimise the maximum distance to a leaf
    std::vector<int> max_dists(n, 0);
    for (int leaf : leafs) {
        std::vector<int> dist(n, -1), q{leaf};
        dist[leaf] = 0;
        for (size_t h = 0; h < q.size(); h++) for (int v : adj[q[h]]) if (dist[v] < 0) { dist[v] = dist[q[h]] + 1; q.push_back(v); }
        for (int i = 0; i < n; i++) if (dist[i] >= 0) max_dists[i] = std::max(max_dists[i], dist[i]);
    }
    int mn = max_dists.empty() ? 0 : *std::min_element(max_dists.begin(), max_dists.end());
    centers.clear();
    for (int i = 0; i < n; i++) if (max_dists[i] == mn) centers.push_back(i);
    if (tree) *tree = adj;
}

// AffineBasedEstimator::estimate: every camera a default CameraParams (focal 1, aspect 1, ppx = ppy = 0, R = I,
// t = 0); the maximum spanning tree on num_inliers walked breadth-first from its first centre, R_to = R_from * H(from, to) in
// double.  It never fails; cameras no tree edge reaches keep R = I.  R is handed on as CV_32F values (the Stitcher's convertTo).
void estimate_affine_cameras(int n, const MisMatchesInfo* pm, MisCameraParams* cameras) {
    for (int i = 0; i < n; i++) {
        MisCameraParams& c = cameras[i];
        c.focal = 1.; c.aspect = 1.; c.ppx = 0.; c.ppy = 0.;
        for (int k = 0; k < 9; k++) c.R[k] = (k % 4 == 0) ? 1. : 0.;
        c.t[0] = c.t[1] = c.t[2] = 0.;
    }
    std::vector<int> centers;
    std::vector<std::vector<int>> tree;
    max_spanning_tree_centers(n, pm, centers, &tree);
    if (!centers.empty()) {
        std::vector<char> was((size_t)n, 0);
        std::vector<int> q{centers[0]};
        was[centers[0]] = 1;
        for (size_t h = 0; h < q.size(); h++) {
            const int from = q[h];
            for (int to : tree[from]) {
                if (was[to]) continue;
                mul3(cameras[from].R, pm[from * n + to].H, cameras[to].R);
                was[to] = 1;
                q.push_back(to);
            }
        }
    }
    for (int i = 0; i < n; i++) for (int k = 0; k < 9; k++) cameras[i].R[k] = (double)(float)cameras[i].R[k];
}

// stitching/src/autocalib.cpp focalsFromHomography: the two focal lengths a homography between two views of a
// rotating camera implies, f0 of the source and f1 of the destination view, each from two closed forms.  Zero denominators are
// not special-cased: H = I or a pure roll gives NaN, every comparison with NaN is false, so ok = false; an infinite v gives
// f = inf with ok = true.  The choice between v1 and v2 is made AFTER the swap, as OpenCV makes it.  A focal that is not ok is 0.
inline bool focal_from_forms(double d1, double d2, double v1, double v2, double& f) {
    if (v1 < v2) std::swap(v1, v2);
    if (v1 > 0 && v2 > 0) f = std::sqrt(std::abs(d1) > std::abs(d2) ? v1 : v2);
    else if (v1 > 0) f = std::sqrt(v1);
    else { f = 0.; return false; }
    return true;
}
void focals_from_homography(const double* h, double& f0, double& f1, bool& f0_ok, bool& f1_ok) {
    double d1 = h[6] * h[7];
    double d2 = (h[7] - h[6]) * (h[7] + h[6]);
    double v1 = -(h[0] * h[1] + h[3] * h[4]) / d1;
    double v2 = (h[0] * h[0] + h[3] * h[3] - h[1] * h[1] - h[4] * h[4]) / d2;
    f1_ok = focal_from_forms(d1, d2, v1, v2, f1);
    d1 = h[0] * h[3] + h[1] * h[4];
    d2 = h[0] * h[0] + h[1] * h[1] - h[3] * h[3] - h[4] * h[4];
    v1 = -h[2] * h[5] / d1;
    v2 = (h[5] * h[5] - h[2] * h[2]) / d2;
    f0_ok = focal_from_forms(d1, d2, v1, v2, f0);
}

// autocalib.cpp estimateFocal: sqrt(f0 f1) of every ordered pair with has_H whose two focals are ok; with at least n - 1 such
// candidates every focal is their median (even count: the mean of the two middle ones), otherwise -- and with no candidate at all,
// which OpenCV reaches for n = 1 and then reads outside its vector -- the "naive approach": the sum of (width + height) over n.
void estimate_focal(int n, const MisMatchesInfo* pm, const MisSize* sizes, double* focals, std::vector<double>* candidates = nullptr) {
    std::vector<double> all;
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            const MisMatchesInfo& m = pm[i * n + j];
            if (m.has_H == 0) continue;
            double f0, f1;
            bool ok0, ok1;
            focals_from_homography(m.H, f0, f1, ok0, ok1);
            if (ok0 && ok1) all.push_back(std::sqrt(f0 * f1));
        }
    if (candidates) *candidates = all;
    double f;
    if (!all.empty() && (int)all.size() >= n - 1) {
        std::sort(all.begin(), all.end());
        f = all.size() % 2 == 1 ? all[all.size() / 2] : (all[all.size() / 2 - 1] + all[all.size() / 2]) * 0.5;
    } else {
        double s = 0;
        for (int i = 0; i < n; i++) s += sizes[i].width + sizes[i].height;
        f = s / n;
    }
    for (int i = 0; i < n; i++) focals[i] = f;
}

// HomographyBasedEstimator::estimate: default cameras (aspect 1, ppx = ppy = 0, R = I, t = 0) with the focal of
// estimate_focal; the maximum spanning tree walked breadth-first from its first centre, per tree edge
// R_to = R_from * (K_from^-1 * H(from, to)^-1 * K_to) in double (cv::invert's 3x3 cofactors; a singular matrix inverts to zero),
// not orthonormalised; then ppx += 0.5 * width, ppy += 0.5 * height: the matcher's homographies are in centred coordinates.  It
// never fails; cameras no tree edge reaches keep R = I.  R is handed on as CV_32F values (the Stitcher's convertTo).
void estimate_homography_cameras(int n, const MisMatchesInfo* pm, const MisSize* sizes, MisCameraParams* cameras) {
    std::vector<double> focals((size_t)n);
    estimate_focal(n, pm, sizes, focals.data());
    for (int i = 0; i < n; i++) {
        MisCameraParams& c = cameras[i];
        c.focal = focals[i]; c.aspect = 1.; c.ppx = 0.; c.ppy = 0.;
        for (int k = 0; k < 9; k++) c.R[k] = (k % 4 == 0) ? 1. : 0.;
        c.t[0] = c.t[1] = c.t[2] = 0.;
    }
    std::vector<int> centers;
    std::vector<std::vector<int>> tree;
    max_spanning_tree_centers(n, pm, centers, &tree);
    if (!centers.empty()) {
        auto Kof = [](const MisCameraParams& c, double* K) {
            const double k[9] = {c.focal, 0., c.ppx, 0., c.focal * c.aspect, c.ppy, 0., 0., 1.};
            memcpy(K, k, sizeof(k));
        };
        std::vector<char> was((size_t)n, 0);
        std::vector<int> q{centers[0]};
        was[centers[0]] = 1;
        for (size_t h = 0; h < q.size(); h++) {
            const int from = q[h];
            for (int to : tree[from]) {
                if (was[to]) continue;
                double Kf[9], Kt[9], Kfi[9], Hi[9], rel[9];
                Kof(cameras[from], Kf);
                Kof(cameras[to], Kt);
                if (!inv3(Kf, Kfi)) std::fill(Kfi, Kfi + 9, 0.);
                if (!inv3(pm[from * n + to].H, Hi)) std::fill(Hi, Hi + 9, 0.);
                mul3(Kfi, Hi, rel);
                mul3(rel, Kt, rel);
                mul3(cameras[from].R, rel, cameras[to].R);
                was[to] = 1;
                q.push_back(to);
            }
        }
    }
    for (int i = 0; i < n; i++) {
        cameras[i].ppx += 0.5 * sizes[i].width;
        cameras[i].ppy += 0.5 * sizes[i].height;
        for (int k = 0; k < 9; k++) cameras[i].R[k] = (double)(float)cameras[i].R[k];
    }
}


// setUpInitialCameraParams of both adjusters, the rotation part: the reference's cameras carry CV_32F rotations
// (image_stitching.cpp:626-634): SVD, u * vt and the sign fix in float, Rodrigues in double on the float matrix, the rotation
// vector stored as CV_32F
void ba_start_rvec(const double* Rin, double* rvec) {
    float Rf[9], u[9], w[3], vt[9], R[9];
    for (int k = 0; k < 9; k++) Rf[k] = (float)Rin[k];
    svd3(Rf, u, w, vt);
    mul3(u, vt, R);
    if (det3(R) < 0) for (float& v : R) v *= -1;
    double Rd[9], rv[3];
    for (int k = 0; k < 9; k++) Rd[k] = R[k];
    rodrigues_to_vec(Rd, rv);
    for (int k = 0; k < 3; k++) rvec[k] = (double)(float)rv[k];
}
// obtainRefinedCameraParams, the rotation part: Rodrigues in double, then R.convertTo(tmp, CV_32F)
void ba_refined_R(const double* rvec, double* Rout) {
    double R[9];
    rodrigues_to_mat(rvec, R);
    for (int k = 0; k < 9; k++) Rout[k] = (double)(float)R[k];
}
// normalise the motion to the centre image of the maximum spanning tree: R_i = R_c^-1 * R_i on the CV_32F matrices
void ba_normalise_to_centre(int n, const MisMatchesInfo* pairwise, MisCameraParams* cameras) {
    std::vector<int> centers;
    max_spanning_tree_centers(n, pairwise, centers);
    if (centers.empty()) return;
    float Rc[9], Rinv[9];
    for (int k = 0; k < 9; k++) Rc[k] = (float)cameras[centers[0]].R[k];
    if (!inv3(Rc, Rinv)) return;
    for (int i = 0; i < n; i++) {
        float Ri[9], Ro[9];
        for (int k = 0; k < 9; k++) Ri[k] = (float)cameras[i].R[k];
        mul3(Rinv, Ri, Ro);
        for (int k = 0; k < 9; k++) cameras[i].R[k] = Ro[k];
    }
}

}  // namespace
