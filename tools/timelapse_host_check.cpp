// timelapse_host_check.cpp -- the host part of csrc/timelapse.hip under a sanitizer, as a stand-alone program: resultRoiIntersection on
// extreme and random rectangles against a 64-bit restatement, and every argument check of the timelapser and of the fused batch
// entries (each is refused before a device call, so no GPU is needed and none is touched).  Build and run (host code only is
// instrumented; the device code of the unit is compiled and never launched):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
//         -I image_stitching_amd/csrc tools/timelapse_host_check.cpp image_stitching_amd/csrc/timelapse.hip image_stitching_amd/csrc/context.hip \
//         -o /tmp/timelapse_host_check && ASAN_OPTIONS=detect_leaks=0 /tmp/timelapse_host_check
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#include "common.h"

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
    } while (0)

static bool restated(const std::vector<MisPoint>& c, const std::vector<MisSize>& s, MisRect* r) {
    long long x0 = LLONG_MIN, y0 = LLONG_MIN, x1 = LLONG_MAX, y1 = LLONG_MAX;
    for (size_t i = 0; i < c.size(); i++) {
        x0 = std::max<long long>(x0, c[i].x); y0 = std::max<long long>(y0, c[i].y);
        x1 = std::min<long long>(x1, (long long)c[i].x + s[i].width); y1 = std::min<long long>(y1, (long long)c[i].y + s[i].height);
    }
    if (x1 - x0 <= 0 || y1 - y0 <= 0 || x1 - x0 > INT_MAX || y1 - y0 > INT_MAX) return false;
    *r = {(int)x0, (int)y0, (int)(x1 - x0), (int)(y1 - y0)};
    return true;
}

int main() {
    std::mt19937 rng(79);
    const int extremes[] = {INT_MIN, INT_MIN + 1, -1, 0, 1, INT_MAX - 1, INT_MAX};
    for (int round = 0; round < 20000; round++) {
        const int n = 1 + (int)(rng() % 6);
        std::vector<MisPoint> c(n);
        std::vector<MisSize> s(n);
        for (int i = 0; i < n; i++) {
            if (round % 3 == 0) { c[i] = {extremes[rng() % 7], extremes[rng() % 7]}; s[i] = {extremes[rng() % 7], extremes[rng() % 7]}; }
            else { c[i] = {(int)(rng() % 400) - 200, (int)(rng() % 400) - 200}; s[i] = {(int)(rng() % 300), (int)(rng() % 300)}; }
        }
        MisRect want{7, 7, 7, 7}, got{7, 7, 7, 7};
        const bool ok = restated(c, s, &want);
        const int rc = mis_result_roi_intersection(c.data(), s.data(), n, &got);
        EXPECT((rc == MIS_OK) == ok);
        EXPECT(got.x == want.x && got.y == want.y && got.width == want.width && got.height == want.height);
    }
    MisRect r;
    MisPoint p{0, 0};
    MisSize z{4, 4};
    EXPECT(mis_result_roi_intersection(nullptr, &z, 1, &r) == MIS_E_INVALID && mis_result_roi_intersection(&p, nullptr, 1, &r) == MIS_E_INVALID);
    EXPECT(mis_result_roi_intersection(&p, &z, 0, &r) == MIS_E_INVALID && mis_result_roi_intersection(&p, &z, 1, nullptr) == MIS_E_INVALID);

    // the argument checks: a context object that no device call ever reads
    MisContext ctx;
    MisTimelapser* t = nullptr;
    EXPECT(mis_timelapser_create(nullptr, MIS_TIMELAPSE_CROP, &t) == MIS_E_INVALID && mis_timelapser_create(&ctx, 2, &t) == MIS_E_INVALID && !t);
    EXPECT(mis_timelapser_create(&ctx, MIS_TIMELAPSE_CROP, nullptr) == MIS_E_INVALID);
    EXPECT(mis_timelapser_create(&ctx, MIS_TIMELAPSE_CROP, &t) == MIS_OK && t);
    EXPECT(mis_timelapser_dst_roi(t, &r) == MIS_E_STATE && mis_timelapser_dst_roi(nullptr, &r) == MIS_E_INVALID);
    int16_t px[4 * 4 * 3] = {};
    MisImage img{px, 4, 4, 3, 24, MIS_S16, MIS_MEM_HOST}, dst{};
    EXPECT(mis_timelapser_process(t, &img, p, &dst) == MIS_E_STATE && !dst.data);
    const MisPoint apart[2] = {{0, 0}, {50, 0}};
    const MisSize ten[2] = {{10, 10}, {10, 10}};
    EXPECT(mis_timelapser_initialize(t, apart, ten, 2) == MIS_E_INVALID && std::string(mis_last_error(&ctx)).find("tl = (50, 0), br = (10, 10)") != std::string::npos);
    EXPECT(mis_timelapser_initialize(t, nullptr, ten, 2) == MIS_E_INVALID && mis_timelapser_initialize(t, apart, ten, 0) == MIS_E_INVALID);
    const MisPoint far_[2] = {{INT_MIN, INT_MIN}, {INT_MAX - 5, INT_MAX - 5}};
    const MisSize five[2] = {{5, 5}, {5, 5}};
    EXPECT(mis_timelapser_initialize(t, far_, five, 2) == MIS_E_INVALID);
    {   // the union of the same extremes (AS_IS) is refused too, not wrapped
        MisTimelapser* u = nullptr;
        EXPECT(mis_timelapser_create(&ctx, MIS_TIMELAPSE_AS_IS, &u) == MIS_OK);
        EXPECT(mis_timelapser_initialize(u, far_, five, 2) == MIS_E_INVALID);
        EXPECT(mis_timelapser_initialize(u, apart, ten, 2) == MIS_OK && mis_timelapser_dst_roi(u, &r) == MIS_OK && r.x == 0 && r.y == 0 && r.width == 60 && r.height == 10);
        mis_timelapser_destroy(u);
    }
    const MisPoint near_[2] = {{0, 0}, {5, 5}};
    EXPECT(mis_timelapser_initialize(t, near_, ten, 2) == MIS_OK && mis_timelapser_dst_roi(t, &r) == MIS_OK && r.x == 5 && r.y == 5 && r.width == 5 && r.height == 5);
    MisImage wrong{px, 4, 4, 3, 24, MIS_S16, MIS_MEM_HOST};
    EXPECT(mis_timelapser_process(t, &img, p, &wrong) == MIS_E_INVALID && mis_timelapser_process(t, nullptr, p, &dst) == MIS_E_INVALID);
    MisImage u8img{px, 4, 4, 3, 12, MIS_U8, MIS_MEM_HOST};
    EXPECT(mis_timelapser_process(t, &u8img, p, &dst) == MIS_E_INVALID && !dst.data);
    EXPECT(mis_timelapser_destroy(t) == MIS_OK && mis_timelapser_destroy(nullptr) == MIS_OK);

    uint8_t src_px[4 * 4 * 3] = {};
    MisImage srcs[2] = {{src_px, 4, 4, 3, 12, MIS_U8, MIS_MEM_HOST}, {src_px, 4, 4, 3, 12, MIS_U8, MIS_MEM_HOST}};
    MisImage dsts[2] = {};
    const float K[18] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 1};
    MisRect rois[2] = {{0, 0, 4, 4}, {1, 1, 4, 4}}, canvas{1, 1, 3, 3};
    auto call = [&](int kind, const MisImage* s, int n, float scale, const float* Ks, const float* Rs, const MisRect* ro, const MisRect* dr, const double* g, MisImage* d, int fmt) {
        const int rc = mis_timelapse_warp_batch(&ctx, kind, s, n, scale, Ks, Rs, ro, dr, g, d, fmt);
        float us = 0;
        EXPECT(mis_timelapse_warp_batch_timed(&ctx, kind, s, n, scale, Ks, Rs, ro, dr, g, d, fmt, 2, &us) == rc);
        EXPECT(!dsts[0].data && !dsts[1].data);
        return rc;
    };
    EXPECT(call(7, srcs, 2, 1.f, K, K, rois, &canvas, nullptr, dsts, MIS_U8) == MIS_E_UNSUPPORTED);
    EXPECT(call(0, nullptr, 2, 1.f, K, K, rois, &canvas, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    EXPECT(call(0, srcs, 2, 1.f, nullptr, K, rois, &canvas, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    EXPECT(call(0, srcs, 2, 1.f, K, nullptr, rois, &canvas, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    EXPECT(call(0, srcs, 2, 1.f, K, K, nullptr, &canvas, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    EXPECT(call(0, srcs, 2, 1.f, K, K, rois, nullptr, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    EXPECT(call(0, srcs, 2, 1.f, K, K, rois, &canvas, nullptr, nullptr, MIS_U8) == MIS_E_INVALID);
    EXPECT(call(0, srcs, 0, 1.f, K, K, rois, &canvas, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    EXPECT(call(0, srcs, 2, 0.f, K, K, rois, &canvas, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    EXPECT(call(0, srcs, 2, 1.f, K, K, rois, &canvas, nullptr, dsts, MIS_F32) == MIS_E_INVALID);
    const MisRect empty{0, 0, 0, 3}, huge{0, 0, 65536, 32768}, off{INT_MAX - 2, 0, 3, 3};
    EXPECT(call(0, srcs, 2, 1.f, K, K, rois, &empty, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    EXPECT(call(0, srcs, 2, 1.f, K, K, rois, &huge, nullptr, dsts, MIS_U8) == MIS_E_INVALID && std::string(mis_last_error(&ctx)).find("too many pixels") != std::string::npos);
    EXPECT(call(0, srcs, 2, 1.f, K, K, rois, &off, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    MisRect bad_rois[2] = {{0, 0, 4, 4}, {1, 1, 0, 4}};
    EXPECT(call(0, srcs, 2, 1.f, K, K, bad_rois, &canvas, nullptr, dsts, MIS_U8) == MIS_E_INVALID && std::string(mis_last_error(&ctx)).find("frame 1: empty roi") != std::string::npos);
    MisImage grey[2] = {srcs[0], {src_px, 4, 4, 1, 4, MIS_U8, MIS_MEM_HOST}};
    EXPECT(call(0, grey, 2, 1.f, K, K, rois, &canvas, nullptr, dsts, MIS_U8) == MIS_E_INVALID && std::string(mis_last_error(&ctx)).find("frame 1: ") != std::string::npos);
    const double nan_gains[6] = {1, 1, 1, 1, std::nan(""), 1};
    EXPECT(call(0, srcs, 2, 1.f, K, K, rois, &canvas, nan_gains, dsts, MIS_U8) == MIS_E_INVALID && std::string(mis_last_error(&ctx)).find("frame 1: gain 1") != std::string::npos);
    uint8_t out_px[4 * 4 * 3] = {};
    MisImage wrong_dsts[2] = {{}, {out_px, 4, 3, 3, 12, MIS_U8, MIS_MEM_HOST}};
    EXPECT(mis_timelapse_warp_batch(&ctx, 0, srcs, 2, 1.f, K, K, rois, &canvas, nullptr, wrong_dsts, MIS_U8) == MIS_E_INVALID && !wrong_dsts[0].data);
    float us = 0;
    EXPECT(mis_timelapse_warp_batch_timed(&ctx, 0, srcs, 2, 1.f, K, K, rois, &canvas, nullptr, dsts, MIS_U8, 0, &us) == MIS_E_INVALID);
    EXPECT(mis_timelapse_warp_batch_timed(&ctx, 0, srcs, 2, 1.f, K, K, rois, &canvas, nullptr, dsts, MIS_U8, 2, nullptr) == MIS_E_INVALID);
    EXPECT(mis_timelapse_warp_batch(nullptr, 0, srcs, 2, 1.f, K, K, rois, &canvas, nullptr, dsts, MIS_U8) == MIS_E_INVALID);
    std::printf(failures ? "timelapse host check: %d FAILED\n" : "timelapse host check OK\n", failures);
    return failures ? 1 : 0;
}
