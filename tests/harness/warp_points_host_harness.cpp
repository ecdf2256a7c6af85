// warp_points_host_harness.cpp -- the host path of mis_warper_warp_points (image_stitching_amd/csrc/warp_points_host.h: the source
// warp_back.hip compiles for the host loop and for warp_points_kernel) as a program of its own, built by the host compiler alone.
//
//   warp_points_host_harness
//        both directions of every warper kind over the special points: the poles of the spherical family (the rays (0, +-1, 0)),
//        z = 0 (rays in the camera's own plane and the panorama plane's horizon), the origin of the polar kinds, NaN, +-inf and
//        +-FLT_MAX coordinates, with cameras that look along the axis, at the pole and backwards, and in-place (out == in).
//        Asserted: every call returns, the in-place call (out == in) gives the bits of the call with separate arrays, and the
//        spherical warper-plane point on the axis of a camera turned by 180 degrees maps to exactly (-1, -1).  Printed, not
//        compared: the number of backward points answered (-1, -1) and a checksum of the bit patterns.  Ends with "special points
//        OK".  Built with -fsanitize=address,undefined this is the memory-safety and undefined-behaviour check of the host path
//        (float -> int conversions, shifts, array bounds): that run is what the program is for.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../image_stitching_amd/csrc/warp_points_host.h"

static const int KINDS[11] = {MIS_WARP_SPHERICAL, MIS_WARP_CYLINDRICAL, MIS_WARP_PLANE, MIS_WARP_MERCATOR, MIS_WARP_FISHEYE, MIS_WARP_STEREOGRAPHIC,
                              MIS_WARP_COMPRESSED_PLANE_A2B1, MIS_WARP_COMPRESSED_PLANE_A15B1, MIS_WARP_PANINI_A2B1, MIS_WARP_PANINI_A15B1, MIS_WARP_AFFINE};

static void rot_x(double deg, float R[9]) {
    const double c = cos(deg * M_PI / 180), s = sin(deg * M_PI / 180);
    const double r[9] = {1, 0, 0, 0, c, -s, 0, s, c};
    for (int i = 0; i < 9; i++) R[i] = (float)r[i];
}
static void rot_y(double deg, float R[9]) {
    const double c = cos(deg * M_PI / 180), s = sin(deg * M_PI / 180);
    const double r[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    for (int i = 0; i < 9; i++) R[i] = (float)r[i];
}

int main() {
    const float f = 100.f, scale = 100.f;
    const float K[9] = {f, 0, 32, 0, f, 24, 0, 0, 1};
    const float inf = INFINITY, nan = NAN, big = 3.4028234e38f, pi_s = 3.14159265358979323846f * scale;
    // forward: pixels (the principal point = the axis, the pole under a 90 degree pitch, huge and non-finite pixels)
    // backward: warper-plane points (the origin = the polar kinds' centre, u = +-pi scale = the seam, v = 0 and pi scale = the spherical
    // poles, u = pi / 2 scale = z 0 for an unrotated camera)
    std::vector<float> pts = {32, 24, 0, 0, 63, 47, 32, -1e6f, 32, 1e6f, -1e6f, 24, 1e6f, 24, 0.f, pi_s, 0.f, 0.f, pi_s, pi_s / 2, -pi_s, pi_s / 2,
                              pi_s / 2, pi_s / 2, -pi_s / 2, 0.f, 1e-30f, -1e-30f, nan, 0, 0, nan, nan, nan, inf, 0, 0, -inf, inf, inf, -inf, inf, big, big, -big, big, big, -big};
    const int n = (int)pts.size() / 2;
    float Rs[5][9];
    rot_x(0, Rs[0]); rot_x(90, Rs[1]); rot_x(-90, Rs[2]); rot_y(180, Rs[3]); rot_y(90, Rs[4]);
    unsigned sum = 0;
    long behind = 0, total = 0;
    for (int kind : KINDS)
        for (int r = 0; r < 5; r++) {
            float H[9];
            memcpy(H, Rs[r], sizeof(H));
            if (kind == MIS_WARP_AFFINE) { H[2] = 12.5f; H[5] = -7.25f; H[6] = 0; H[7] = 0; H[8] = 1; }    // a homogeneous 2-D transform
            Projector p;
            projector_set(&p, kind, scale, K, H);
            const PointMap pm = point_map_of(p);
            for (int backward = 0; backward < 2; backward++) {
                std::vector<float> out(pts.size(), 123.f), inplace = pts;
                warp_points_host(pm, backward, pts.data(), out.data(), n);
                warp_points_host(pm, backward, inplace.data(), inplace.data(), n);
                if (memcmp(out.data(), inplace.data(), sizeof(float) * out.size()) != 0) { printf("kind %d: in-place differs\n", kind); return 1; }
                for (int i = 0; i < n; i++) {
                    unsigned bx, by;
                    memcpy(&bx, &out[2 * i], 4); memcpy(&by, &out[2 * i + 1], 4);
                    sum = sum * 31u + (out[2 * i] == out[2 * i] ? bx : 0x7fc00000u);
                    sum = sum * 31u + (out[2 * i + 1] == out[2 * i + 1] ? by : 0x7fc00000u);
                    total++;
                    if (backward && out[2 * i] == -1.f && out[2 * i + 1] == -1.f) behind++;
                }
                // the roi code walks the same mapForward: a refusal is an answer, a crash is not
                int tlx, tly, brx, bry;
                if (!backward) detect_result_roi(&p, 64, 48, &tlx, &tly, &brx, &bry);
            }
        }
    // a camera turned by 180 degrees sees the warper-plane origin of the z-testing kinds behind it
    float back[2], origin[2] = {0.f, pi_s / 2};
    Projector p;
    projector_set(&p, MIS_WARP_SPHERICAL, scale, K, Rs[3]);
    warp_points_host(point_map_of(p), 1, origin, back, 1);
    if (back[0] != -1.f || back[1] != -1.f) { printf("spherical: a point behind the camera maps to (%g, %g)\n", back[0], back[1]); return 1; }
    printf("points %ld, behind %ld, checksum %08x\nspecial points OK\n", total, behind, sum);
    return 0;
}
