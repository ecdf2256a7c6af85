// jpeg.hip -- imread of a baseline JPEG (image_stitching.cpp:569): the entropy decode on the host (jpeg_host.h, a serial bit stream
// per restart interval), dequantisation + inverse DCT, chroma upsampling and colour conversion on the device (the arithmetic of
// jpeg_core.h), bit for bit what libjpeg-turbo gives with its defaults -- what cv::imread returns.
//
// One call decodes n frames of any sizes and sampling layouts: the host threads write every frame's coefficient blocks into the
// context's pinned staging, one copy brings them and the argument table to the device, and two launches -- frame and component
// on the grid -- produce every frame.  The kernels use no atomics, and every trip count comes from the argument table, which
// holds only geometry that jpeg_parse has validated.
#include <algorithm>
#include <array>
#include <chrono>
#include "common.h"
#include "host_threads.h"
#include "jpeg_core.h"
#include "jpeg_host.h"

namespace {

// one frame of the device's argument table
struct JpegFrameArgs {
    const int16_t* coef[3];     // blocks of 64 in natural order, the component's plane row by row
    uint8_t* plane[3];          // component planes of bw * 8 x bh * 8 samples
    uint8_t* dst;               // 8UC3 BGR
    unsigned dst_stride, plane_stride[3];
    int w, h, ncomp;
    int bw[3], nblk[3];
    int cw, ch, rule;           // the chroma planes' real size and their upsampling rule (JPEG_UP_*)
    int dst_dwords;             // dst and its stride are multiples of 4: a thread stores a row of its tile as six dwords
    int q[3][64];               // quantisation tables, natural order
};

// One thread per block: the 64 coefficients live in registers (eight 16-byte loads), the quantisation table comes through the
// scalar cache (frame and component are uniform), the block's rows leave as eight 8-byte stores that consecutive threads --
// consecutive blocks of a block row -- write side by side.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const JpegFrameArgs* __restrict__ A) {
    const JpegFrameArgs& a = A[blockIdx.z];
    const int c = blockIdx.y;
    if (c >= a.ncomp) return;
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.nblk[c]) return;
    const int4* __restrict__ src = reinterpret_cast<const int4*>(a.coef[c] + (size_t)b * 64);
    const int* __restrict__ q = a.q[c];
    uint32_t ws[64];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int4 v = src[i];
        const int w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            ws[8 * i + 2 * k] = (uint32_t)((int)(int16_t)(w4[k] & 0xffff) * q[8 * i + 2 * k]);
            ws[8 * i + 2 * k + 1] = (uint32_t)((w4[k] >> 16) * q[8 * i + 2 * k + 1]);
        }
    }
    uint32_t row[8][2];
    jpeg_idct_block(ws, row);
    const int by = b / a.bw[c], bx = b - by * a.bw[c];
    uint8_t* out = a.plane[c] + (size_t)by * 8 * a.plane_stride[c] + (size_t)bx * 8;
#pragma unroll
    for (int y = 0; y < 8; y++) *reinterpret_cast<uint2*>(out + (size_t)y * a.plane_stride[c]) = make_uint2(row[y][0], row[y][1]);
}

// A thread produces a tile of 8 x 2 pixels: the luma samples are two 8-byte loads of the padded plane, the chroma samples come from
// the real chroma planes -- the h2v2 rule (4:2:0) a tile at a time (jpeg_h2v2_tile: 9 loads per plane), the other rules pixel by
// pixel --, 24 bytes per row leave as six dwords where the destination allows it.
__global__ __launch_bounds__(256) void jpeg_color_kernel(const JpegFrameArgs* __restrict__ A) {
    const JpegFrameArgs& a = A[blockIdx.z];
    const int x0 = (blockIdx.x * 64 + (threadIdx.x & 63)) * 8;
    const int y0 = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 2;
    if (x0 >= a.w || y0 >= a.h) return;
    const int nvalid = min(8, a.w - x0), nrows = min(2, a.h - y0);
    int cb[2][8], cr[2][8];
    if (a.ncomp == 3) {
        if (a.rule == JPEG_UP_H2V2) {
            jpeg_h2v2_tile(a.plane[1], a.plane_stride[1], a.cw, a.ch, x0, y0, cb);
            jpeg_h2v2_tile(a.plane[2], a.plane_stride[2], a.cw, a.ch, x0, y0, cr);
        } else {
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int k = 0; k < 8; k++) {       // (pixels past the image are computed on its last column / row and not stored)
                    const int xc = min(x0 + k, a.w - 1), yc = min(y0 + r, a.h - 1);
                    cb[r][k] = jpeg_upsample_at(a.plane[1], a.plane_stride[1], a.cw, a.ch, a.rule, xc, yc);
                    cr[r][k] = jpeg_upsample_at(a.plane[2], a.plane_stride[2], a.cw, a.ch, a.rule, xc, yc);
                }
        }
    }
#pragma unroll
    for (int r = 0; r < 2; r++) {
        if (r >= nrows) break;
        // (the plane is padded to whole blocks: the eight samples at x0 < w lie inside their row)
        const uint2 luma = *reinterpret_cast<const uint2*>(a.plane[0] + (size_t)(y0 + r) * a.plane_stride[0] + x0);
        unsigned px[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int yy = ((k < 4 ? luma.x : luma.y) >> (8 * (k & 3))) & 255;
            px[k] = a.ncomp == 1 ? (unsigned)yy * 0x010101u : jpeg_ycc_to_bgr(yy, cb[r][k], cr[r][k]);
        }
        uint8_t* out = a.dst + (size_t)(y0 + r) * a.dst_stride + (size_t)x0 * 3;
        if (a.dst_dwords && nvalid == 8) {
            unsigned* o32 = reinterpret_cast<unsigned*>(out);
#pragma unroll
            for (int g = 0; g < 2; g++) {
                o32[3 * g] = px[4 * g] | (px[4 * g + 1] << 24);
                o32[3 * g + 1] = (px[4 * g + 1] >> 8) | (px[4 * g + 2] << 16);
                o32[3 * g + 2] = (px[4 * g + 2] >> 16) | (px[4 * g + 3] << 8);
            }
        } else {
            for (int k = 0; k < nvalid; k++) {
                out[3 * k] = (uint8_t)px[k]; out[3 * k + 1] = (uint8_t)(px[k] >> 8); out[3 * k + 2] = (uint8_t)(px[k] >> 16);
            }
        }
    }
}

thread_local std::string g_jpeg_error;      // of the context-free entries

int free_error(const JpegError& e) { g_jpeg_error = e.text; return e.code; }

// the restart intervals of all frames on host threads: a frame's intervals in up to 16 runs, the runs handed out in order
struct EntropyTask { int frame; size_t first, count; };

int entropy_all(const uint8_t* const* datas, const std::vector<JpegHeader>& H, const std::vector<std::vector<JpegSegment>>& segs,
                const std::vector<std::array<int16_t*, 3>>& planes, int* bad_frame, JpegError* err) {
    std::vector<EntropyTask> tasks;
    for (int f = 0; f < (int)H.size(); f++) {
        const size_t ns = segs[f].size(), run = (ns + 15) / 16;
        for (size_t s = 0; s < ns; s += run) tasks.push_back({f, s, std::min(run, ns - s)});
    }
    std::vector<JpegError> errs(tasks.size());
    run_on_host_threads(tasks.size(), [&](size_t t) {
        const EntropyTask& k = tasks[t];
        jpeg_entropy(datas[k.frame], H[k.frame], segs[k.frame], k.first, k.count, planes[k.frame].data(), &errs[t]);
    });
    for (size_t t = 0; t < tasks.size(); t++)
        if (errs[t].code != JPEG_OK) { *bad_frame = tasks[t].frame; *err = errs[t]; return errs[t].code; }
    return JPEG_OK;
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// ms (optional): host milliseconds of the header pass and of the entropy decode, device milliseconds (events) of the upload, the
// IDCT launch and the upsampling + colour launch
int decode_batch(MisContext* ctx, const void* const* datas, const size_t* bytes, int n, MisImage* dsts, float* ms);

}  // namespace

extern "C" const char* mis_jpeg_last_error(void) { return g_jpeg_error.c_str(); }

void mis_jpeg_set_last_error(const char* text) { g_jpeg_error = text; }

extern "C" int mis_jpeg_info(const void* data, size_t bytes, MisJpegInfo* out) {
    JpegError e;
    if (!data || !out) return free_error((jpeg_fail(&e, JPEG_INVALID, "jpeg: null argument"), e));
    JpegHeader H;
    if (jpeg_parse((const uint8_t*)data, bytes, &H, &e) != JPEG_OK) return free_error(e);
    memset(out, 0, sizeof(*out));
    out->width = H.width; out->height = H.height; out->components = H.ncomp; out->restart_interval = H.restart_interval;
    for (int c = 0; c < H.ncomp; c++) { out->h[c] = H.file_h[c]; out->v[c] = H.file_v[c]; }
    g_jpeg_error.clear();
    return MIS_OK;
}

extern "C" int mis_jpeg_debug_coefficients(const void* data, size_t bytes, int component, int16_t* out, size_t capacity, uint16_t qtable[64]) {
    JpegError e;
    if (!data || !out || !qtable) return free_error((jpeg_fail(&e, JPEG_INVALID, "jpeg: null argument"), e));
    JpegHeader H;
    std::vector<JpegSegment> segs;
    const uint8_t* d = (const uint8_t*)data;
    if (jpeg_parse(d, bytes, &H, &e) != JPEG_OK || jpeg_segments(d, bytes, H, &segs, &e) != JPEG_OK) return free_error(e);
    if (component < 0 || component >= H.ncomp) return free_error((jpeg_fail(&e, JPEG_INVALID, "jpeg: component %d of %d", component, H.ncomp), e));
    if (capacity < H.blocks(component) * 64)
        return free_error((jpeg_fail(&e, JPEG_INVALID, "jpeg: component %d has %zu coefficients, capacity %zu", component, H.blocks(component) * 64, capacity), e));
    std::vector<std::vector<int16_t>> store(H.ncomp);
    int16_t* planes[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < H.ncomp; c++) { store[c].resize(H.blocks(c) * 64); planes[c] = store[c].data(); }
    if (jpeg_entropy(d, H, segs, 0, segs.size(), planes, &e) != JPEG_OK) return free_error(e);
    memcpy(out, planes[component], H.blocks(component) * 64 * sizeof(int16_t));
    memcpy(qtable, H.q[H.tq[component]], 64 * sizeof(uint16_t));
    g_jpeg_error.clear();
    return MIS_OK;
}

extern "C" int mis_jpeg_decode_batch(MisContext* ctx, const void* const* datas, const size_t* bytes, int n, MisImage* dsts) {
    if (!ctx) return MIS_E_INVALID;
    return decode_batch(ctx, datas, bytes, n, dsts, nullptr);
}

extern "C" int mis_jpeg_decode_batch_timed(MisContext* ctx, const void* const* datas, const size_t* bytes, int n, MisImage* dsts, float ms[5]) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, ms, MIS_E_INVALID, "jpeg: null argument");
    return decode_batch(ctx, datas, bytes, n, dsts, ms);
}

namespace {
int decode_batch(MisContext* ctx, const void* const* datas, const size_t* bytes, int n, MisImage* dsts, float* ms) {
    MIS_CHECK(ctx, datas && bytes && dsts, MIS_E_INVALID, "jpeg: null argument");
    auto t0 = std::chrono::steady_clock::now();
    MIS_CHECK(ctx, n > 0 && n <= 65535, MIS_E_INVALID, "jpeg: a batch of %d frames (1 .. 65535)", n);
    // headers and scan structure of every frame, then the outputs: everything is checked before anything is staged or allocated
    std::vector<JpegHeader> H(n);
    std::vector<std::vector<JpegSegment>> segs(n);
    JpegError e;
    for (int i = 0; i < n; i++) MIS_CHECK(ctx, datas[i], MIS_E_INVALID, "jpeg: frame %d: null data", i);
    {
        std::vector<JpegError> errs(n);     // (the scan for markers reads every byte: the frames side by side)
        run_on_host_threads((size_t)n, [&](size_t i) {
            const uint8_t* d = (const uint8_t*)datas[i];
            if (jpeg_parse(d, bytes[i], &H[i], &errs[i]) == JPEG_OK) jpeg_segments(d, bytes[i], H[i], &segs[i], &errs[i]);
        });
        for (int i = 0; i < n; i++)
            if (errs[i].code != JPEG_OK) return mis_set_error(ctx, errs[i].code, "frame %d: %s", i, errs[i].text);
    }
    if (ms) ms[0] = (float)ms_since(t0);
    for (int i = 0; i < n; i++) {
        const MisImage& d = dsts[i];
        if (!d.data) continue;
        MIS_CHECK(ctx, d.width == H[i].width && d.height == H[i].height && d.channels == 3 && d.dtype == MIS_U8, MIS_E_INVALID,
                  "jpeg: output %d is %dx%dx%d dtype %d, the frame decodes to %dx%dx3 dtype %d", i, d.width, d.height, d.channels, d.dtype, H[i].width, H[i].height, MIS_U8);
        MIS_CHECK(ctx, d.stride >= (size_t)d.width * 3 && d.stride <= 0xffffffffu, MIS_E_INVALID, "jpeg: bad output stride (%d)", i);
    }
    // one layout for the pinned staging and the device block: [argument table][coefficients of every frame and component], then, on
    // the device only, the component planes
    const size_t args_bytes = mis_align_up((size_t)n * sizeof(JpegFrameArgs), 256);
    std::vector<std::array<size_t, 3>> coef_off(n), plane_off(n);
    size_t off = args_bytes;
    for (int i = 0; i < n; i++)
        for (int c = 0; c < H[i].ncomp; c++) { coef_off[i][c] = off; off += mis_align_up(H[i].blocks(c) * 64 * sizeof(int16_t), 256); }
    const size_t upload_bytes = off;
    for (int i = 0; i < n; i++)
        for (int c = 0; c < H[i].ncomp; c++) { plane_off[i][c] = off; off += mis_align_up(H[i].blocks(c) * 64, 256); }
    const size_t total_bytes = off;
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    void* hs = nullptr;
    if (int rc = mis_host_stage(ctx, upload_bytes, &hs)) return rc;
    uint8_t* host = (uint8_t*)hs;
    std::vector<std::array<int16_t*, 3>> planes(n);
    for (int i = 0; i < n; i++)
        for (int c = 0; c < 3; c++) planes[i][c] = c < H[i].ncomp ? (int16_t*)(host + coef_off[i][c]) : nullptr;
    int bad = 0;
    t0 = std::chrono::steady_clock::now();
    if (entropy_all((const uint8_t* const*)datas, H, segs, planes, &bad, &e) != JPEG_OK) return mis_set_error(ctx, e.code, "frame %d: %s", bad, e.text);
    if (ms) ms[1] = (float)ms_since(t0);

    OwnedEvent ev[4];
    if (ms)
        for (OwnedEvent& v : ev) MIS_HIP(ctx, v.ready(hipEventDefault));
    PoolBlock blk(ctx);
    if (int rc = blk.alloc(total_bytes)) return rc;
    uint8_t* dev = (uint8_t*)blk.p;
    std::vector<DevView> dout(n);
    int rc = MIS_OK, maxw = 0, maxh = 0, maxblk = 0;
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = dout[i].write(ctx, &dsts[i], H[i].width, H[i].height, 3, MIS_U8);
    if (rc != MIS_OK) return rc;
    JpegFrameArgs* A = (JpegFrameArgs*)host;
    memset(A, 0, args_bytes);
    for (int i = 0; i < n; i++) {
        JpegFrameArgs& a = A[i];
        const JpegHeader& h = H[i];
        for (int c = 0; c < h.ncomp; c++) {
            a.coef[c] = (const int16_t*)(dev + coef_off[i][c]);
            a.plane[c] = dev + plane_off[i][c];
            a.plane_stride[c] = (unsigned)h.bw[c] * 8u;
            a.bw[c] = h.bw[c];
            a.nblk[c] = (int)h.blocks(c);
            for (int k = 0; k < 64; k++) a.q[c][k] = h.q[h.tq[c]][k];
            maxblk = std::max(maxblk, a.nblk[c]);
        }
        a.dst = (uint8_t*)dout[i].data; a.dst_stride = (unsigned)dout[i].stride;
        a.w = h.width; a.h = h.height; a.ncomp = h.ncomp;
        a.cw = h.cw; a.ch = h.ch; a.rule = h.rule;
        a.dst_dwords = (((uintptr_t)dout[i].data | dout[i].stride) & 3) == 0;
        maxw = std::max(maxw, h.width); maxh = std::max(maxh, h.height);
    }
    if (ms) MIS_HIP(ctx, hipEventRecord(ev[0].ev, ctx->stream));
    MIS_HIP(ctx, hipMemcpyAsync(dev, host, upload_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (ms) MIS_HIP(ctx, hipEventRecord(ev[1].ev, ctx->stream));
    const JpegFrameArgs* dA = (const JpegFrameArgs*)dev;
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((maxblk + 255) / 256, 3, n), dim3(256), 0, ctx->stream, dA);
    MIS_HIP(ctx, hipGetLastError());
    if (ms) MIS_HIP(ctx, hipEventRecord(ev[2].ev, ctx->stream));
    hipLaunchKernelGGL(jpeg_color_kernel, dim3(((maxw + 7) / 8 + 63) / 64, (maxh + 7) / 8, n), dim3(256), 0, ctx->stream, dA);
    MIS_HIP(ctx, hipGetLastError());
    if (ms) MIS_HIP(ctx, hipEventRecord(ev[3].ev, ctx->stream));
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = dout[i].commit();
    if (rc != MIS_OK) return rc;
    // the staging is the next call's to overwrite: the copy has to be over before this one returns
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ms)
        for (int k = 0; k < 3; k++) MIS_HIP(ctx, hipEventElapsedTime(&ms[2 + k], ev[k].ev, ev[k + 1].ev));
    blk.release();
    return MIS_OK;
}
}  // namespace

extern "C" int mis_jpeg_decode(MisContext* ctx, const void* data, size_t bytes, MisImage* dst_bgr) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, data && dst_bgr, MIS_E_INVALID, "jpeg: null argument");
    const int rc = mis_jpeg_decode_batch(ctx, &data, &bytes, 1, dst_bgr);
    return rc;
}
