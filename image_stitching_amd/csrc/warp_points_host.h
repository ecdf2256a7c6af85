// warp_points_host.h -- warpPoint / warpPointBackward of every warper kind for one point, on the host and on the device (SURVEY
// Appendix A.17), and the host loop of mis_warper_warp_points (ctx NULL).  Included by warp_back.hip and, as a program of its own,
// by tests/harness/warp_points_host_harness.cpp (the host compiler alone builds it: nothing here needs a device).
#pragma once
#include "warp_shared.h"

namespace {

// everything mapForward and mapBackward of one (kind, scale, K, R) need; small enough to be a kernel argument
struct PointMap {
    float fwd[9];   // r_kinv (mapForward)
    float bwd[9];   // k_rinv (mapBackward)
    float scale, a, b;
    float t[3];     // PlaneProjector::t of the affine kind, else 0
    int kind;
};
PointMap point_map_of(const Projector& p) {
    PointMap m;
    for (int i = 0; i < 9; i++) { m.fwd[i] = p.r_kinv[i]; m.bwd[i] = p.k_rinv[i]; }
    m.scale = p.scale; m.a = p.a; m.b = p.b; m.kind = p.kind;
    for (int i = 0; i < 3; i++) m.t[i] = p.t[i];
    return m;
}

// mapBackward(u, v) of a half-separable kind at one point: the column terms and the pixel's rest, as col_tile evaluates them
template <int FAM>
MIS_HD void col_point(const float* m, float scale, float pa, float pb, float u, float v, float* x, float* y) {
    const ColTerms ct = col_hoist<FAM>(scale, pa, pb, u);
    float sinv, cosv;
    col_pixel<FAM>(ct, pb, v / scale, &sinv, &cosv);
    map_backward(FAM, m, ct.sl, ct.cl, cosv, sinv, x, y);
}

// mapBackward(u, v) of any kind at float coordinates, on the host and on the device: the warp kernels' sequences, so an integer
// (u, v) gives the very floats those kernels sample at.  t0, t1: the affine kind's translation (its t2 is +-0, see WarpArgs).
MIS_HD void map_backward_any(int kind, const float* m, float scale, float pa, float pb, float t0, float t1, float u, float v, float* x, float* y) {
    if (kind == MIS_WARP_FISHEYE || kind == MIS_WARP_STEREOGRAPHIC) map_backward_polar(kind, m, scale, u, v, x, y);
    else if (kind >= MIS_WARP_COMPRESSED_PLANE_A2B1 && kind <= MIS_WARP_COMPRESSED_PLANE_A15B1) col_point<MIS_WARP_COMPRESSED_PLANE_A2B1>(m, scale, pa, pb, u, v, x, y);
    else if (kind >= MIS_WARP_PANINI_A2B1 && kind <= MIS_WARP_PANINI_A15B1) col_point<MIS_WARP_PANINI_A2B1>(m, scale, pa, pb, u, v, x, y);
    else {
        float su, cu, s, c;
        col_terms(kind, scale, u, t0, &su, &cu);
        row_terms(kind, scale, v, t1, &s, &c);
        map_backward(kind, m, su, cu, s, c, x, y);
    }
}

// one point of warpPoint (backward == 0) or warpPointBackward
MIS_HD void warp_point(const PointMap& p, int backward, float x, float y, float* ox, float* oy) {
    if (backward) map_backward_any(p.kind, p.bwd, p.scale, p.a, p.b, p.t[0], p.t[1], x, y, ox, oy);
    else map_forward(p.kind, p.fwd, p.scale, x, y, ox, oy, p.a, p.b, p.t);
}

// the host path of mis_warper_warp_points (in and out may be the same array)
void warp_points_host(const PointMap& pm, int backward, const float* xy_in, float* xy_out, int n) {
    for (int i = 0; i < n; i++) {
        const float x = xy_in[2 * (size_t)i], y = xy_in[2 * (size_t)i + 1];
        warp_point(pm, backward, x, y, &xy_out[2 * (size_t)i], &xy_out[2 * (size_t)i + 1]);
    }
}

}  // namespace
