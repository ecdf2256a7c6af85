// Test harness (not shipped): the host twin of the ray bundle adjuster (csrc/motion_ray.hip).  The library evaluates the
// observations with kernels; here the same ba_ray.h functions run in plain loops on host keypoints, with the two-level sums as the
// library defines them (per edge a sequential sum over its rows from +0, the edges combined in ascending order by
// ba_ray_solve.h), and drive the same solver (ba_ray_solve.h over motion_host.h).  Compiled for the CPU;
// tests/test_refimpl_motion_ray_cpu.py builds and drives it, tests/test_refimpl_motion_ray_gpu.py compares the device with it bit for bit.
#include <cstdarg>
#include <cstring>
#include "../../image_stitching_amd/csrc/ba_ray_solve.h"

int mis_set_error(MisContext* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
    fprintf(stderr, "mis error %d: %s\n", code, buf);
    return code;
}

namespace {
struct HostEval {
    const MisFeatures* features = nullptr;
    int n = 0;
    std::vector<BaRayEdge> edges;
    std::vector<BaRayObs> obs;
    std::vector<double> rec, errv, jac, part;
    int prepare(MisContext*, const MisFeatures* f, int n_, const std::vector<BaRayEdge>& e, const std::vector<BaRayObs>& o) {
        features = f; n = n_; edges = e; obs = o;
        rec.assign((size_t)9 * n * BA_RAY_REC, 0.); errv.assign(obs.size() * 3, 0.); jac.assign(obs.size() * 3 * BA_RAY_JCOLS, 0.); part.assign(edges.size() * BA_RAY_CHAINS, 0.);
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
            ba_ray_observation(rec.data(), n, e.i, e.j, (double)k1.x, (double)k1.y, (double)k2.x, (double)k2.y, &errv[m * 3], want_jac ? &jac[m * 3 * BA_RAY_JCOLS] : nullptr);
        }
        if (!want_jac) return MIS_OK;
        for (size_t e = 0; e < edges.size(); e++)
            for (int t = 0; t < BA_RAY_CHAINS; t++) {
                int a, b;
                ba_ray_chain(t, &a, &b);
                double s = 0.;
                for (size_t k = (size_t)3 * edges[e].first; k < (size_t)3 * (edges[e].first + edges[e].count); k++)
                    s = ba_ray_accumulate(s, jac[k * BA_RAY_JCOLS + a], b < 0 ? errv[k] : jac[k * BA_RAY_JCOLS + b]);
                part[e * BA_RAY_CHAINS + t] = s;
            }
        return MIS_OK;
    }
};
}  // namespace

extern "C" int dbg_bundle_adjust_ray(const MisFeatures* f, const MisMatchesInfo* pm, int n, float conf, MisCameraParams* cams) {
    MisContext ctx;
    if (!(f && pm && cams && n >= 2)) return mis_set_error(&ctx, MIS_E_INVALID, "null argument or fewer than two cameras");
    HostEval ev;
    return ba_ray_solve(&ctx, f, pm, n, conf, cams, ev);
}
