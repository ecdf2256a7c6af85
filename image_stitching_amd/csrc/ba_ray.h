// ba_ray.h -- BundleAdjusterRay's per-observation arithmetic, defined once for the kernels of motion_ray.hip and for host code
// (the host twin of tests/harness/ba_ray_host_harness.cpp).  Plain double + - * / sqrt in the association written here; the
// library is built with -ffp-contract=off, so both sides round every operation the same way.
//
// A camera RECORD is ten doubles: H = R K^-1 (row-major) and the focal length.  Record c (c < n) holds camera c at the
// current parameters; record ba_ray_slot(n, c, p, s) holds camera c with its parameter p (0 focal, 1..3 rotation vector) moved
// by -step (s = 0) or +step (s = 1).  sin / cos stay on the host: the records are computed there.
#pragma once
#include "dev_math.h"

#define BA_RAY_REC 10          // doubles per camera record
#define BA_RAY_JCOLS 8         // non-zero Jacobian entries of an error row: 4 of camera i, then 4 of camera j
#define BA_RAY_PAIRS 36        // entries a <= b of an edge's 8 x 8 block of J^T J
#define BA_RAY_CHAINS 44       // ... and the 8 of J^T err: sequential sums per edge
#define BA_RAY_STEP 1e-3       // central-difference step of BundleAdjusterRay::calcJacobian

struct BaRayEdge { int i, j, first, count; };     // cameras i < j, the edge's first observation and how many it has
struct BaRayObs { int edge, q, t; };              // keypoint q of image i, keypoint t of image j

MIS_HD int ba_ray_slot(int n, int c, int p, int s) { return n + (c * 4 + p) * 2 + s; }

// the unit ray of pixel (px, py) through H
MIS_HD void ba_ray_dir(const double* H, double px, double py, double* r) {
    const double x = (H[0] * px + H[1] * py) + H[2];
    const double y = (H[3] * px + H[4] * py) + H[5];
    const double z = (H[6] * px + H[7] * py) + H[8];
    const double len = sqrt((x * x + y * y) + z * z);
    r[0] = x / len; r[1] = y / len; r[2] = z / len;
}
MIS_HD double ba_ray_mult(double fi, double fj) { return sqrt(fi * fj); }
MIS_HD double ba_ray_err(double mult, double r1, double r2) { return mult * (r1 - r2); }
// calcDeriv: (err(+step) - err(-step)) / (2 step)
MIS_HD double ba_ray_deriv(double e_plus, double e_minus) { return (e_plus - e_minus) / (2 * BA_RAY_STEP); }

// One observation: its 3 errors and, with jac != nullptr, its 3 x 8 Jacobian entries (row k at jac + 8 k).
// rec: the records (9 n of them when jac is wanted, else n); (x1, y1) the keypoint of image i, (x2, y2) of image j.
MIS_HD void ba_ray_observation(const double* rec, int n, int i, int j, double x1, double y1, double x2, double y2, double* err, double* jac) {
    const double* Hi = rec + (size_t)i * BA_RAY_REC;
    const double* Hj = rec + (size_t)j * BA_RAY_REC;
    double r1[3], r2[3];
    ba_ray_dir(Hi, x1, y1, r1);
    ba_ray_dir(Hj, x2, y2, r2);
    const double mult = ba_ray_mult(Hi[9], Hj[9]);
#pragma unroll
    for (int k = 0; k < 3; k++) err[k] = ba_ray_err(mult, r1[k], r2[k]);
    if (!jac) return;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const double* Hm = rec + (size_t)ba_ray_slot(n, i, p, 0) * BA_RAY_REC;
        const double* Hp = rec + (size_t)ba_ray_slot(n, i, p, 1) * BA_RAY_REC;
        double rm[3], rp[3];
        ba_ray_dir(Hm, x1, y1, rm);
        ba_ray_dir(Hp, x1, y1, rp);
        const double mm = ba_ray_mult(Hm[9], Hj[9]), mp = ba_ray_mult(Hp[9], Hj[9]);
#pragma unroll
        for (int k = 0; k < 3; k++) jac[k * BA_RAY_JCOLS + p] = ba_ray_deriv(ba_ray_err(mp, rp[k], r2[k]), ba_ray_err(mm, rm[k], r2[k]));
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const double* Hm = rec + (size_t)ba_ray_slot(n, j, p, 0) * BA_RAY_REC;
        const double* Hp = rec + (size_t)ba_ray_slot(n, j, p, 1) * BA_RAY_REC;
        double rm[3], rp[3];
        ba_ray_dir(Hm, x2, y2, rm);
        ba_ray_dir(Hp, x2, y2, rp);
        const double mm = ba_ray_mult(Hi[9], Hm[9]), mp = ba_ray_mult(Hi[9], Hp[9]);
#pragma unroll
        for (int k = 0; k < 3; k++) jac[k * BA_RAY_JCOLS + 4 + p] = ba_ray_deriv(ba_ray_err(mp, r1[k], rp[k]), ba_ray_err(mm, r1[k], rm[k]));
    }
}

// What the shared evaluators (ba_eval_device.h, the host twins) need to know of an adjuster: record size, errors per observation
// and the observation itself.  ba_affine.h has the affine-partial adjuster's.
struct BaRayObsModel {
    enum { REC = BA_RAY_REC, ERRS = 3 };
    static MIS_HD void observation(const double* rec, int n, int i, int j, double x1, double y1, double x2, double y2, double* err, double* jac) {
        ba_ray_observation(rec, n, i, j, x1, y1, x2, y2, err, jac);
    }
};

// Chain t of an edge's normal equations: t < 36 the entry (a, b), a <= b, of the 8 x 8 block in row-major order of the upper
// triangle; t >= 36 the entry a = t - 36 of J^T err.
MIS_HD void ba_ray_chain(int t, int* a, int* b) {
    if (t >= BA_RAY_PAIRS) { *a = t - BA_RAY_PAIRS; *b = -1; return; }
    int row = 0, left = t;
    while (left >= BA_RAY_JCOLS - row) { left -= BA_RAY_JCOLS - row; row++; }      // at most 7 steps
    *a = row; *b = row + left;
}
// One term of a chain: the product is rounded, then added
MIS_HD double ba_ray_accumulate(double s, double ja, double other) { return s + ja * other; }
