// Test harness (not shipped): the host twin of the affine-partial bundle adjuster (csrc/motion_affine.hip) and the affine
// estimator.  The library evaluates the observations with kernels (ba_eval_device.h); here the same ba_affine.h functions run in
// plain loops on host keypoints, with the two-level sums as the library defines them (per edge a sequential sum over its rows
// from +0, the edges combined in ascending order by ba_ray_solve.h's ba_obs_solve), and drive the same solver
// (ba_affine_solve.h).  Compiled for the CPU; tests/test_refimpl_ba_affine_cpu.py builds and drives it (tests/ba_affine_twin.py),
// tests/test_ba_affine_gpu.py compares the device with it bit for bit.  With BA_AFFINE_HARNESS_MAIN it is a stand-alone program
// that runs a small fixed problem (for sanitizer builds on the CPU).
#include <cstdarg>
#include <cstring>
#include "../../image_stitching_amd/csrc/ba_affine_solve.h"

int mis_set_error(MisContext* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    fprintf(stderr, "mis error %d: %s\n", code, buf);
    return code;
}

namespace {
struct HostEval {
    static constexpr int ERRS = BaAffineObsModel::ERRS;
    const MisFeatures* features = nullptr;
    int n = 0;
    std::vector<BaRayEdge> edges;
    std::vector<BaRayObs> obs;
    std::vector<double> rec, errv, jac, part;
    int prepare(MisContext*, const MisFeatures* f, int n_, const std::vector<BaRayEdge>& e, const std::vector<BaRayObs>& o) {
        features = f; n = n_; edges = e; obs = o;
        rec.assign((size_t)9 * n * BA_AFFINE_REC, 0.); errv.assign(obs.size() * ERRS, 0.); jac.assign(obs.size() * ERRS * BA_RAY_JCOLS, 0.);
        part.assign(edges.size() * BA_RAY_CHAINS, 0.);
        return MIS_OK;
    }
    double* records() { return rec.data(); }
    const double* err() const { return errv.data(); }
    const double* partials() const { return part.data(); }
    int run(MisContext*, bool want_jac) {
        for (size_t m = 0; m < obs.size(); m++) {
            const BaRayEdge& e = edges[obs[m].edge];
            const MisKeyPoint& k1 = features[e.i].keypoints[obs[m].q];      // host arrays here
            const MisKeyPoint& k2 = features[e.j].keypoints[obs[m].t];
            ba_affine_observation(rec.data(), n, e.i, e.j, (double)k1.x, (double)k1.y, (double)k2.x, (double)k2.y, &errv[m * ERRS],
                                  want_jac ? &jac[m * ERRS * BA_RAY_JCOLS] : nullptr);
        }
        if (!want_jac) return MIS_OK;
        for (size_t e = 0; e < edges.size(); e++)
            for (int t = 0; t < BA_RAY_CHAINS; t++) {
                int a, b;
                ba_ray_chain(t, &a, &b);
                double s = 0.;
                for (size_t k = (size_t)ERRS * edges[e].first; k < (size_t)ERRS * (edges[e].first + edges[e].count); k++)
                    s = ba_ray_accumulate(s, jac[k * BA_RAY_JCOLS + a], b < 0 ? errv[k] : jac[k * BA_RAY_JCOLS + b]);
                part[e * BA_RAY_CHAINS + t] = s;
            }
        return MIS_OK;
    }
};
}  // namespace

extern "C" int dbg_bundle_adjust_affine_partial(const MisFeatures* f, const MisMatchesInfo* pm, int n, float conf, MisCameraParams* cams) {
    MisContext ctx;
    if (!(f && pm && cams && n >= 2)) return mis_set_error(&ctx, MIS_E_INVALID, "null argument or fewer than two cameras");
    HostEval ev;
    return ba_affine_solve(&ctx, f, pm, n, conf, cams, ev);
}

extern "C" int dbg_estimate_affine_cameras(const MisMatchesInfo* pm, int n, MisCameraParams* cams) {
    if (!pm || !cams || n < 1) return MIS_E_INVALID;
    estimate_affine_cameras(n, pm, cams);
    return MIS_OK;
}

#ifdef BA_AFFINE_HARNESS_MAIN
// three cameras in a chain under known similarities, 40 matches per edge, from perturbed cameras: estimator, then adjuster
int main() {
    const int n = 3, per = 40;
    const double truth[n][4] = {{1, 0, 0, 0}, {0.99, 0.08, 120, -15}, {0.97, -0.11, 250, 20}};
    std::vector<MisKeyPoint> kps[n];
    std::vector<MisDMatch> matches[n * n];
    std::vector<uint8_t> masks[n * n];
    std::vector<MisMatchesInfo> pm((size_t)n * n);
    memset(pm.data(), 0, sizeof(MisMatchesInfo) * pm.size());
    unsigned seed = 12345;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (double)(seed >> 8) / (double)(1u << 24); };
    for (int i = 0; i + 1 < n; i++) {
        const int j = i + 1;
        double ri[BA_AFFINE_REC], rj[BA_AFFINE_REC];
        ba_affine_record(truth[i], ri);
        ba_affine_record(truth[j], rj);
        for (int k = 0; k < per; k++) {
            MisKeyPoint a; memset(&a, 0, sizeof(a));
            MisKeyPoint b = a;
            a.x = (float)(rnd() * 640); a.y = (float)(rnd() * 360);
            double zero[2];
            ba_affine_err(ri, rj, a.x, a.y, 0., 0., zero);      // err = 0 - H p1
            b.x = (float)-zero[0]; b.y = (float)-zero[1];
            MisDMatch m; memset(&m, 0, sizeof(m));
            m.query_idx = (int)kps[i].size(); m.train_idx = (int)kps[j].size();
            kps[i].push_back(a); kps[j].push_back(b);
            matches[i * n + j].push_back(m);
            std::swap(m.query_idx, m.train_idx);
            matches[j * n + i].push_back(m);
        }
        for (int s = 0; s < 2; s++) {
            const int a = s ? j : i, b = s ? i : j;
            MisMatchesInfo& e = pm[a * n + b];
            masks[a * n + b].assign(per, 1);
            e.src_img_idx = a; e.dst_img_idx = b; e.n_matches = per; e.num_inliers = per + i; e.has_H = 1; e.confidence = 2.0;
            double ra[BA_AFFINE_REC];
            ba_affine_record(truth[a], ra);
            const double* q = truth[b];
            const double* A = ra + 4;
            const double H[9] = {A[0] * q[0] + A[1] * q[1], A[0] * -q[1] + A[1] * q[0], A[0] * q[2] + A[1] * q[3] + A[2],
                                 A[3] * q[0] + A[4] * q[1], A[3] * -q[1] + A[4] * q[0], A[3] * q[2] + A[4] * q[3] + A[5], 0, 0, 1};
            memcpy(e.H, H, sizeof(H));
        }
    }
    std::vector<MisFeatures> f(n);
    memset(f.data(), 0, sizeof(MisFeatures) * n);
    for (int i = 0; i < n; i++) { f[i].img_idx = i; f[i].img_w = 640; f[i].img_h = 360; f[i].n = (int)kps[i].size(); f[i].keypoints = kps[i].data(); }
    for (int k = 0; k < n * n; k++) { pm[k].matches = matches[k].empty() ? nullptr : matches[k].data(); pm[k].inliers_mask = masks[k].empty() ? nullptr : masks[k].data(); }
    std::vector<MisCameraParams> cams(n);
    if (dbg_estimate_affine_cameras(pm.data(), n, cams.data()) != MIS_OK) return 1;
    for (int i = 0; i < n; i++) { cams[i].R[0] += 0.01 * i; cams[i].R[4] += 0.01 * i; cams[i].R[2] += 3.0 * i; }
    if (dbg_bundle_adjust_affine_partial(f.data(), pm.data(), n, 1.0f, cams.data()) != MIS_OK) return 2;
    // the middle camera is the tree's centre: the others relative to it
    double r1[BA_AFFINE_REC];
    ba_affine_record(truth[1], r1);
    const double want_tx = r1[4] * truth[2][2] + r1[5] * truth[2][3] + r1[6];
    printf("camera 2: a %.6f b %.6f tx %.3f (truth %.3f) ty %.3f\n", cams[2].R[0], cams[2].R[3], cams[2].R[2], want_tx, cams[2].R[5]);
    return std::fabs(cams[2].R[2] - want_tx) < 0.05 ? 0 : 3;
}
#endif
