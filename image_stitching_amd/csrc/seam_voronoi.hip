// seam_voronoi.hip -- VoronoiSeamFinder, the reference's seam_find_type "voronoi" (SURVEY row N1b):
//   seam_finder = makePtr<detail::VoronoiSeamFinder>()                    image_stitching/image_stitching.cpp:1031
//   seam_finder->find(images_warped_f, corners, masks_warped)             image_stitching/image_stitching.cpp:1065
// The images are not looked at.  Per overlapping pair, in PairwiseSeamFinder::run order (the pair plan of seam_plan.h; its levels
// are not used: the pairs follow each other on the stream, a mask edited by one pair is the input of the next): both masks cut over
// the shared rectangle grown by a gap of 10, the exact L1 distance transform of either unique part, and the pixel goes to the image
// whose unique part is nearer.  Pinned to the independent reference of tests/test_refimpl_expos_gpu.py.
#include "common.h"
#include "seam_plan.h"
#include <vector>

namespace {

struct MaskDesc { const uint8_t* msk; size_t mstride; int cx, cy, w, h; };      // a mask on the device, its corner and size

// VoronoiSeamFinder::findInPair: cut both masks over the shared rectangle grown by `gap`; unique = mask minus the collision
__global__ __launch_bounds__(256) void vor_cut_kernel(MaskDesc A, MaskDesc B, int x0, int y0, int W, int H, int gap, uint8_t* __restrict__ u1, uint8_t* __restrict__ u2) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int px = x0 - gap + x, py = y0 - gap + y;
    const int xa = px - A.cx, ya = py - A.cy, xb = px - B.cx, yb = py - B.cy;
    const uint8_t m1 = (xa >= 0 && ya >= 0 && xa < A.w && ya < A.h) ? A.msk[(size_t)ya * A.mstride + xa] : 0;
    const uint8_t m2 = (xb >= 0 && yb >= 0 && xb < B.w && yb < B.h) ? B.msk[(size_t)yb * B.mstride + xb] : 0;
    const bool collision = m1 && m2;
    // the transform below measures the distance to the nearest ZERO byte: zero where the unique mask is set
    u1[(size_t)y * W + x] = (m1 && !collision) ? 0 : 1;
    u2[(size_t)y * W + x] = (m2 && !collision) ? 0 : 1;
}
// exact L1 distance to the nearest zero byte: rows (both directions), then columns; one thread per line, both maps at once
constexpr int VINF = 1 << 29;
__global__ void vor_rows_kernel(const uint8_t* __restrict__ u1, const uint8_t* __restrict__ u2, int W, int H, int* __restrict__ d1, int* __restrict__ d2) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * H) return;
    const uint8_t* u = (t < H ? u1 : u2) + (size_t)(t % H) * W;
    int* d = (t < H ? d1 : d2) + (size_t)(t % H) * W;
    int run = VINF;
    for (int x = 0; x < W; x++) { run = u[x] ? min(run + 1, VINF) : 0; d[x] = run; }
    run = VINF;
    for (int x = W - 1; x >= 0; x--) { run = u[x] ? min(run + 1, VINF) : 0; d[x] = min(d[x], run); }
}
__global__ void vor_cols_kernel(int W, int H, int* __restrict__ d1, int* __restrict__ d2) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * W) return;
    int* d = (t < W ? d1 : d2) + (t % W);
    int run = VINF;
    for (int y = 0; y < H; y++) { run = min(min(run + 1, VINF), d[(size_t)y * W]); d[(size_t)y * W] = run; }
    run = VINF;
    for (int y = H - 1; y >= 0; y--) { run = min(min(run + 1, VINF), d[(size_t)y * W]); d[(size_t)y * W] = run; }
}
// seam = dist1 < dist2: the second image loses the pixel, otherwise the first does
__global__ __launch_bounds__(256) void vor_apply_kernel(MaskDesc A, MaskDesc B, uint8_t* __restrict__ ma, uint8_t* __restrict__ mb, int x0, int y0, int rw, int rh, int W,
                                                        int gap, const int* __restrict__ d1, const int* __restrict__ d2) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= rw) return;
    const size_t k = (size_t)(y + gap) * W + x + gap;
    if (d1[k] < d2[k]) mb[(size_t)(y0 - B.cy + y) * B.mstride + (x0 - B.cx + x)] = 0;
    else ma[(size_t)(y0 - A.cy + y) * A.mstride + (x0 - A.cx + x)] = 0;
}

}  // namespace

extern "C" int mis_seam_voronoi(MisContext* ctx, const MisPoint* corners, MisImage* masks, int n) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, corners && masks && n > 0, MIS_E_INVALID, "voronoi seams: null argument or no masks");
    for (int i = 0; i < n; i++)
        MIS_CHECK(ctx, masks[i].data && masks[i].dtype == MIS_U8 && masks[i].channels == 1, MIS_E_UNSUPPORTED, "voronoi seams: mask %d is not 8UC1", i);
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<DevView> dm(n);
    std::vector<MaskDesc> desc(n);
    std::vector<SeamFrame> frames(n);
    int rc = MIS_OK;
    for (int i = 0; i < n; i++) {
        if ((rc = dm[i].read_write(ctx, &masks[i])) != MIS_OK) return rc;
        desc[i] = {(const uint8_t*)dm[i].data, dm[i].stride, corners[i].x, corners[i].y, masks[i].width, masks[i].height};
        frames[i] = SeamFrame{corners[i].x, corners[i].y, masks[i].width, masks[i].height};
    }
    const int gap = 10;
    for (const SeamPair& sp : seam_plan(frames, SEAM_ORDER_RUN).pairs) {
        const int i = sp.i, j = sp.j, x0 = sp.roi.x0, y0 = sp.roi.y0;
        const int rw = sp.roi.x1 - x0, rh = sp.roi.y1 - y0, W = rw + 2 * gap, H = rh + 2 * gap;
        const size_t px = (size_t)W * H, bytes = mis_align_up(px, 256) * 2 + px * 2 * sizeof(int);
        void* buf = nullptr; size_t got = 0;
        if ((rc = mis_pool_alloc(ctx, bytes, &buf, &got)) != MIS_OK) return rc;
        uint8_t* u1 = (uint8_t*)buf; uint8_t* u2 = u1 + mis_align_up(px, 256);
        int* d1 = (int*)(u2 + mis_align_up(px, 256)); int* d2 = d1 + px;
        hipLaunchKernelGGL(vor_cut_kernel, dim3((W + 255) / 256, H), dim3(256), 0, ctx->stream, desc[i], desc[j], x0, y0, W, H, gap, u1, u2);
        hipLaunchKernelGGL(vor_rows_kernel, dim3((2 * H + 63) / 64), dim3(64), 0, ctx->stream, u1, u2, W, H, d1, d2);
        hipLaunchKernelGGL(vor_cols_kernel, dim3((2 * W + 63) / 64), dim3(64), 0, ctx->stream, W, H, d1, d2);
        hipLaunchKernelGGL(vor_apply_kernel, dim3((rw + 255) / 256, rh), dim3(256), 0, ctx->stream, desc[i], desc[j], (uint8_t*)dm[i].data, (uint8_t*)dm[j].data, x0, y0,
                           rw, rh, W, gap, d1, d2);
        mis_pool_free(ctx, buf, got);
        MIS_HIP(ctx, hipGetLastError());
    }
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = dm[i].commit();
    return rc;
}
