// ba_affine.h -- BundleAdjusterAffinePartial's per-observation arithmetic, defined once for the kernels of
// motion_affine.hip and for host code (the host twin of tests/harness/ba_affine_host_harness.cpp).  Plain double + - * / in the
// association written here; the library is built with -ffp-contract=off, so both sides round every operation the same way.
//
// A camera's parameters are (a, b, tx, ty): H = [a -b tx; b a ty; 0 0 1].  A camera RECORD is ten doubles: the four parameters
// and the 2 x 3 inverse of H by invertAffineTransform (row-major).  Record c (c < n) holds camera c at the current parameters;
// record ba_ray_slot(n, c, p, s) holds camera c with its parameter p moved by -step (s = 0) or +step (s = 1).
// The edge / observation tables, the 8 Jacobian columns of an error row and the 44 chains of an edge are the ray adjuster's
// (ba_ray.h): both adjusters have 4 parameters per camera.
#pragma once
#include "ba_ray.h"

#define BA_AFFINE_REC 10       // doubles per camera record: a, b, tx, ty, then the inverse's two rows
#define BA_AFFINE_STEP 1e-4    // central-difference step of BundleAdjusterAffinePartial::calcJacobian

// the record of parameters q: invertAffineTransform in double -- D = a11 a22 - a12 a21, D = D != 0 ? 1 / D : 0 (a = b = 0 gives
// the zero matrix, not a division by zero)
MIS_HD void ba_affine_record(const double* q, double* rec) {
    const double a11 = q[0], a12 = -q[1], a21 = q[1], a22 = q[0], b1 = q[2], b2 = q[3];
    double D = a11 * a22 - a12 * a21;
    D = D != 0. ? 1. / D : 0.;
    const double A11 = a22 * D, A22 = a11 * D, A12 = -a12 * D, A21 = -a21 * D;
    rec[0] = q[0]; rec[1] = q[1]; rec[2] = q[2]; rec[3] = q[3];
    rec[4] = A11; rec[5] = A12; rec[6] = -A11 * b1 - A12 * b2;
    rec[7] = A21; rec[8] = A22; rec[9] = -A21 * b1 - A22 * b2;
}

// The two errors of one correspondence under H = H1^-1 H2: the upper two rows of the 3 x 3 product with every term of its sums
// written out, k = 0, 1, 2 in ascending order ((A_r0 B_0c + A_r1 B_1c) + A_r2 B_2c; the third row of both factors is 0 0 1),
// then p2 - H p1 with H p1 = (H_r0 x + H_r1 y) + H_r2.
// ri: the record whose inverse is H1^-1; rj: the record whose parameters are H2.
MIS_HD void ba_affine_err(const double* ri, const double* rj, double x1, double y1, double x2, double y2, double* err) {
    const double* A = ri + 4;                                       // 2 x 3
    const double a = rj[0], b = rj[1], tx = rj[2], ty = rj[3];      // B = [a -b tx; b a ty; 0 0 1]
    const double H00 = (A[0] * a + A[1] * b) + A[2] * 0., H01 = (A[0] * -b + A[1] * a) + A[2] * 0., H02 = (A[0] * tx + A[1] * ty) + A[2] * 1.;
    const double H10 = (A[3] * a + A[4] * b) + A[5] * 0., H11 = (A[3] * -b + A[4] * a) + A[5] * 0., H12 = (A[3] * tx + A[4] * ty) + A[5] * 1.;
    err[0] = x2 - ((H00 * x1 + H01 * y1) + H02);
    err[1] = y2 - ((H10 * x1 + H11 * y1) + H12);
}
// calcDeriv: (err(+step) - err(-step)) / (2 step)
MIS_HD double ba_affine_deriv(double e_plus, double e_minus) { return (e_plus - e_minus) / (2 * BA_AFFINE_STEP); }

// One observation: its 2 errors and, with jac != nullptr, its 2 x 8 Jacobian entries (row k at jac + 8 k): columns 0..3 the
// parameters of camera i, 4..7 those of camera j.
// rec: the records (9 n of them when jac is wanted, else n); (x1, y1) the keypoint of image i, (x2, y2) of image j.
MIS_HD void ba_affine_observation(const double* rec, int n, int i, int j, double x1, double y1, double x2, double y2, double* err, double* jac) {
    const double* Ri = rec + (size_t)i * BA_AFFINE_REC;
    const double* Rj = rec + (size_t)j * BA_AFFINE_REC;
    ba_affine_err(Ri, Rj, x1, y1, x2, y2, err);
    if (!jac) return;
#pragma unroll
    for (int p = 0; p < 4; p++) {
        double em[2], ep[2];
        ba_affine_err(rec + (size_t)ba_ray_slot(n, i, p, 0) * BA_AFFINE_REC, Rj, x1, y1, x2, y2, em);
        ba_affine_err(rec + (size_t)ba_ray_slot(n, i, p, 1) * BA_AFFINE_REC, Rj, x1, y1, x2, y2, ep);
        jac[p] = ba_affine_deriv(ep[0], em[0]);
        jac[BA_RAY_JCOLS + p] = ba_affine_deriv(ep[1], em[1]);
    }
#pragma unroll
    for (int p = 0; p < 4; p++) {
        double em[2], ep[2];
        ba_affine_err(Ri, rec + (size_t)ba_ray_slot(n, j, p, 0) * BA_AFFINE_REC, x1, y1, x2, y2, em);
        ba_affine_err(Ri, rec + (size_t)ba_ray_slot(n, j, p, 1) * BA_AFFINE_REC, x1, y1, x2, y2, ep);
        jac[4 + p] = ba_affine_deriv(ep[0], em[0]);
        jac[BA_RAY_JCOLS + 4 + p] = ba_affine_deriv(ep[1], em[1]);
    }
}

struct BaAffineObsModel {
    enum { REC = BA_AFFINE_REC, ERRS = 2 };
    static MIS_HD void observation(const double* rec, int n, int i, int j, double x1, double y1, double x2, double y2, double* err, double* jac) {
        ba_affine_observation(rec, n, i, j, x1, y1, x2, y2, err, jac);
    }
};
