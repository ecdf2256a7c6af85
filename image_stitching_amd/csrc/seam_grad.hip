// seam_grad.hip -- DpSeamFinder::computeGradients (stitching/src/seam_finders.cpp) for every frame of a seam step in one launch:
//   cvtColor(image CV_32FC3, gray, COLOR_BGR2GRAY); Sobel(gray, gradx, CV_32F, 1, 0); Sobel(gray, grady, CV_32F, 0, 1)
// (3 x 3, scale 1, BORDER_REFLECT_101).  OpenCV recomputes the two planes for both images of every pair it processes; here they
// are made once per frame, on the device, and travel to the host with the seam step's one staged copy (seam.hip).
// The arithmetic is float32, every operation rounded, no FMA (the library builds with -ffp-contract=off):
//   g           = (B * 0.114f + G * 0.587f) + R * 0.299f
//   gradx(y, x) = (d(y - 1, x) + 2 d(y, x)) + d(y + 1, x),   d(y, x) = g(y, x + 1) - g(y, x - 1)
//   grady(y, x) = s(y + 1, x) - s(y - 1, x),                 s(y, x) = (g(y, x - 1) + 2 g(y, x)) + g(y, x + 1)
// -- OpenCV's separable row-then-column order as recalled; PARITY UNPINNED.  The independent numpy
// statement is tests/refimpl_seam_dp_grad.py, equal bit for bit in tests/test_seam_dp_grad_gpu.py.
#include "common.h"
#include "dev_math.h"

namespace {

constexpr int SG_TW = 64, SG_TH = 16;     // a block's tile: 64 x 4 threads, four rows each
constexpr int SG_ROWS = SG_TH / 4;
constexpr int SG_MAX = 32;                // frames per launch (the table travels as kernel arguments)
struct SeamGradArgs {
    const uint8_t* src[SG_MAX];
    float* gx[SG_MAX];
    float* gy[SG_MAX];
    int w[SG_MAX], h[SG_MAX];
    unsigned ss[SG_MAX], gxs[SG_MAX], gys[SG_MAX];      // row strides in bytes
};

// Frame on the grid's z; the grid covers the largest frame of the launch and a block outside its own frame leaves at once.
// The tile's grey values go through LDS with a one-pixel halo (each source pixel is converted once per tile); the halo of a
// tile on the frame's edge holds the reflected pixels, so the filter below knows no borders.
__global__ __launch_bounds__(256) void seam_grad_kernel(const SeamGradArgs A) {
    const int f = blockIdx.z;
    const int w = A.w[f], h = A.h[f];
    const int x0 = blockIdx.x * SG_TW, y0 = blockIdx.y * SG_TH;
    if (x0 >= w || y0 >= h) return;
    __shared__ float g[SG_TH + 2][SG_TW + 2];
    const uint8_t* __restrict__ src = A.src[f];
    const size_t ss = A.ss[f];
    for (int i = threadIdx.x; i < (SG_TH + 2) * (SG_TW + 2); i += 256) {
        const int ly = i / (SG_TW + 2), lx = i - ly * (SG_TW + 2);
        const int py = y0 - 1 + ly, px = x0 - 1 + lx;
        if (py > h || px > w) continue;     // (a ragged last tile: no pixel of the frame reads past its one-pixel border)
        const uint8_t* p = src + (size_t)mis_reflect101(py, h) * ss + (size_t)mis_reflect101(px, w) * 3;
        g[ly][lx] = ((float)p[0] * 0.114f + (float)p[1] * 0.587f) + (float)p[2] * 0.299f;
    }
    __syncthreads();
    const int tx = threadIdx.x & 63, ly0 = (threadIdx.x >> 6) * SG_ROWS;
    const int x = x0 + tx;
    if (x >= w || y0 + ly0 >= h) return;
    // the row pass of both filters on the thread's SG_ROWS + 2 rows, then the column pass
    float d[SG_ROWS + 2], s[SG_ROWS + 2];
#pragma unroll
    for (int r = 0; r < SG_ROWS + 2; r++) {
        const int ly = ly0 + r;             // <= SG_TH + 1
        const float a = g[ly][tx], b = g[ly][tx + 1], c = g[ly][tx + 2];
        d[r] = c - a;
        s[r] = (a + 2.f * b) + c;
    }
    float* __restrict__ gx = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(A.gx[f]) + (size_t)(y0 + ly0) * A.gxs[f]) + x;
    float* __restrict__ gy = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(A.gy[f]) + (size_t)(y0 + ly0) * A.gys[f]) + x;
#pragma unroll
    for (int r = 0; r < SG_ROWS; r++) {
        if (y0 + ly0 + r >= h) break;
        *reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(gx) + (size_t)r * A.gxs[f]) = (d[r] + 2.f * d[r + 1]) + d[r + 2];
        *reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(gy) + (size_t)r * A.gys[f]) = s[r + 2] - s[r];
    }
}

}  // namespace

int mis_seam_grad_enqueue(MisContext* ctx, const MisSeamGradJob* jobs, int n) {
    for (int b = 0; b < n; b += SG_MAX) {       // (a job's frames are one launch; more than SG_MAX frames take one per SG_MAX)
        const int m = n - b < SG_MAX ? n - b : SG_MAX;
        SeamGradArgs A;
        memset(&A, 0, sizeof(A));
        int mw = 0, mh = 0;
        for (int i = 0; i < m; i++) {
            const MisSeamGradJob& j = jobs[b + i];
            A.src[i] = j.src; A.gx[i] = j.gx; A.gy[i] = j.gy;
            A.w[i] = j.w; A.h[i] = j.h;
            A.ss[i] = (unsigned)j.ss; A.gxs[i] = (unsigned)j.gxs; A.gys[i] = (unsigned)j.gys;
            mw = j.w > mw ? j.w : mw; mh = j.h > mh ? j.h : mh;
        }
        const dim3 grid((mw + SG_TW - 1) / SG_TW, (mh + SG_TH - 1) / SG_TH, m), block(256);
        hipLaunchKernelGGL(seam_grad_kernel, grid, block, 0, ctx->stream, A);
        MIS_HIP(ctx, hipGetLastError());
    }
    return MIS_OK;
}

extern "C" int mis_seam_gradients(MisContext* ctx, const MisImage* images, int n, MisImage* gradx, MisImage* grady) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, n >= 0, MIS_E_INVALID, "seam gradients of %d images", n);
    if (n == 0) return MIS_OK;
    MIS_CHECK(ctx, images && gradx && grady, MIS_E_INVALID, "null argument");
    // everything is checked before anything is staged or written
    for (int i = 0; i < n; i++) {
        const MisImage& I = images[i];
        MIS_CHECK(ctx, I.data && I.dtype == MIS_U8 && I.channels == 3 && I.width > 0 && I.height > 0 && I.width < (1 << 22) && I.height < (1 << 22) &&
                           I.stride >= (size_t)I.width * 3 && I.stride <= 0xffffffffu, MIS_E_INVALID, "image %d: need an 8UC3 image", i);
        const MisImage* G[2] = {&gradx[i], &grady[i]};
        for (const MisImage* g : G)
            MIS_CHECK(ctx, g->data && g->dtype == MIS_F32 && g->channels == 1 && g->width == I.width && g->height == I.height && g->stride >= (size_t)I.width * 4 &&
                               g->stride <= 0xffffffffu && (g->mem != MIS_MEM_DEVICE || (((uintptr_t)g->data | g->stride) & 3) == 0), MIS_E_INVALID,
                      "image %d: need two f32 x 1 planes of the image's size (%dx%d), rows 4-byte aligned", i, I.width, I.height);
    }
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<DevView> din(n), dgx(n), dgy(n);
    std::vector<MisSeamGradJob> jobs((size_t)n);
    int rc = MIS_OK;
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = din[i].read(ctx, &images[i]);
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = dgx[i].write(ctx, &gradx[i], images[i].width, images[i].height, 1, MIS_F32);
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = dgy[i].write(ctx, &grady[i], images[i].width, images[i].height, 1, MIS_F32);
    if (rc != MIS_OK) return rc;
    for (int i = 0; i < n; i++)
        jobs[i] = MisSeamGradJob{(const uint8_t*)din[i].data, din[i].stride, (float*)dgx[i].data, dgx[i].stride, (float*)dgy[i].data, dgy[i].stride, images[i].width, images[i].height};
    rc = mis_seam_grad_enqueue(ctx, jobs.data(), n);
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = dgx[i].commit();
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = dgy[i].commit();
    return rc;
}
