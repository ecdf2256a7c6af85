// jpeg_enc.hip -- imwrite of a baseline JPEG (image_stitching.cpp:1228): colour conversion, chroma downsampling, forward DCT and
// quantisation on the device (the arithmetic of jpeg_enc_core.h), the Huffman coding on host threads (jpeg_enc_host.h: chunks of
// whole MCU rows, joined at bit granularity), byte for byte what libjpeg-turbo writes with its defaults -- what cv::imwrite writes.
//
// One call encodes n images of any sizes and samplings: one upload of the argument table, two launches -- frame on the grid; one
// thread per luma block, one per pair of chroma blocks -- and one copy of every coefficient into the context's pinned staging.
// The source is read twice (once for luma, once for both chroma components) and no Y / Cb / Cr plane exists in memory; edges are
// replicated by clamped reads; every coefficient is written once, in natural order (the layout of mis_jpeg_debug_coefficients, which
// the host coder reads through the zig-zag table).  Dummy blocks are filled here, by the thread that owns them.  The kernels use
// no atomics, and every trip count comes from the argument table, which holds only geometry that jpeg_enc_check has validated.
#include <array>
#include <chrono>
#include <stdlib.h>
#include "common.h"
#include "host_threads.h"
#include "jpeg_enc_core.h"
#include "jpeg_enc_host.h"

namespace {

// one frame of the device's argument table
struct JpegEncFrameArgs {
    const uint8_t* src;         // 8UC3 BGR
    size_t stride;
    int16_t* coef[3];           // blocks of 64 in natural order, the component's plane row by row
    int w, h, hmax, vmax;
    int bw[3], bh[3], wb[3], hb[3];
    int src_dwords;             // src and its stride are multiples of 4: a thread loads a whole row of its block as dwords
    uint32_t recip[2][64], half[2][64];     // per table (0 luminance, 1 chrominance): jpeg_enc_divisor of every entry, natural order
};

// N pixels of one row from column x0 (a multiple of 8) on, B | G << 8 | R << 16 each, columns past the image replicating its last
template <int N>
__device__ __forceinline__ void load_pixels(const uint8_t* __restrict__ row, int x0, int w, bool dwords, unsigned px[N]) {
    if (dwords && x0 + N <= w) {
        const unsigned* __restrict__ p = reinterpret_cast<const unsigned*>(row + (size_t)x0 * 3);
#pragma unroll
        for (int g = 0; g < N / 4; g++) {
            const unsigned d0 = p[3 * g], d1 = p[3 * g + 1], d2 = p[3 * g + 2];
            px[4 * g] = d0 & 0xffffffu;
            px[4 * g + 1] = (d0 >> 24) | ((d1 & 0xffffu) << 8);
            px[4 * g + 2] = (d1 >> 16) | ((d2 & 0xffu) << 16);
            px[4 * g + 3] = d2 >> 8;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) {
            const uint8_t* q = row + (size_t)min(x0 + k, w - 1) * 3;
            px[k] = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
        }
    }
}

// the 64 quantised coefficients of one block leave as eight 16-byte stores
__device__ __forceinline__ void store_block(int16_t* __restrict__ dst, const int x[64]) {
    uint4* __restrict__ o = reinterpret_cast<uint4*>(dst);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int* v = x + 8 * r;
        o[r] = make_uint4(((unsigned)v[0] & 0xffffu) | ((unsigned)v[1] << 16), ((unsigned)v[2] & 0xffffu) | ((unsigned)v[3] << 16),
                          ((unsigned)v[4] & 0xffffu) | ((unsigned)v[5] << 16), ((unsigned)v[6] & 0xffffu) | ((unsigned)v[7] << 16));
    }
}

// One thread per block of the luma plane, consecutive threads consecutive blocks of a block row.  A dummy block transforms the
// block whose DC it repeats (jpeg_enc_dummy_source) and keeps the DC alone.
__global__ __launch_bounds__(256) void jpeg_enc_luma_kernel(const JpegEncFrameArgs* __restrict__ A) {
    const JpegEncFrameArgs& a = A[blockIdx.z];
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.bw[0] * a.bh[0]) return;
    const int j = b / a.bw[0], i = b - j * a.bw[0];
    const bool dummy = i >= a.wb[0] || j >= a.hb[0];
    int si = i, sj = j;
    if (dummy) jpeg_enc_dummy_source(i, j, a.wb[0], a.hb[0], a.hmax, &si, &sj);
    int x[64];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        unsigned px[8];
        load_pixels<8>(a.src + (size_t)min(sj * 8 + r, a.h - 1) * a.stride, si * 8, a.w, a.src_dwords != 0, px);
#pragma unroll
        for (int k = 0; k < 8; k++) x[8 * r + k] = jpeg_enc_y((int)(px[k] >> 16), (int)((px[k] >> 8) & 255u), (int)(px[k] & 255u));
    }
    jpeg_fdct_quant_block(x, a.recip[0], a.half[0]);
    if (dummy) {
#pragma unroll
        for (int k = 1; k < 64; k++) x[k] = 0;
    }
    store_block(a.coef[0] + (size_t)b * 64, x);
}

// the Cb and Cr samples of one chroma block (i, j), sample k as cb | cr << 16: jcsample.c's h2v2 (FX = FY = 2), h2v1 (FX = 2) or a copy.
// The last input column is replicated, the last input row up to a multiple of FY only; below that the last downsampled row repeats.
template <int FX, int FY>
__device__ __forceinline__ void chroma_samples(const JpegEncFrameArgs& a, int i, int j, unsigned s[64]) {
    const int ch = (a.h + FY - 1) / FY;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int dy = min(j * 8 + r, ch - 1);
        int cb[8 * FX], cr[8 * FX];
#pragma unroll
        for (int k = 0; k < 8 * FX; k++) cb[k] = cr[k] = 0;
#pragma unroll
        for (int t = 0; t < FY; t++) {
            unsigned px[8 * FX];
            load_pixels<8 * FX>(a.src + (size_t)min(dy * FY + t, a.h - 1) * a.stride, i * 8 * FX, a.w, a.src_dwords != 0, px);
#pragma unroll
            for (int k = 0; k < 8 * FX; k++) {
                const int rr = (int)(px[k] >> 16), gg = (int)((px[k] >> 8) & 255u), bb = (int)(px[k] & 255u);
                cb[k] += jpeg_enc_cb(rr, gg, bb);
                cr[k] += jpeg_enc_cr(rr, gg, bb);
            }
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            int u, v;
            if (FX == 2 && FY == 2) {           // bias 1, 2, 1, 2, ... along the output row (block columns are even)
                u = (cb[2 * k] + cb[2 * k + 1] + 1 + (k & 1)) >> 2;
                v = (cr[2 * k] + cr[2 * k + 1] + 1 + (k & 1)) >> 2;
            } else if (FX == 2) {               // bias 0, 1, 0, 1, ...
                u = (cb[2 * k] + cb[2 * k + 1] + (k & 1)) >> 1;
                v = (cr[2 * k] + cr[2 * k + 1] + (k & 1)) >> 1;
            } else {
                u = cb[k]; v = cr[k];
            }
            s[8 * r + k] = (unsigned)u | ((unsigned)v << 16);
        }
    }
}

// One thread per block position of the chroma planes (they have no dummy blocks): it reads its 8 hmax x 8 vmax pixels once and
// writes the block of Cb and the block of Cr.
__global__ __launch_bounds__(256) void jpeg_enc_chroma_kernel(const JpegEncFrameArgs* __restrict__ A) {
    const JpegEncFrameArgs& a = A[blockIdx.z];
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= a.bw[1] * a.bh[1]) return;
    const int j = b / a.bw[1], i = b - j * a.bw[1];
    unsigned s[64];
    if (a.vmax == 2) chroma_samples<2, 2>(a, i, j, s);
    else if (a.hmax == 2) chroma_samples<2, 1>(a, i, j, s);
    else chroma_samples<1, 1>(a, i, j, s);
    int x[64];
#pragma unroll
    for (int k = 0; k < 64; k++) x[k] = (int)(s[k] & 0xffffu);
    jpeg_fdct_quant_block(x, a.recip[1], a.half[1]);
    store_block(a.coef[1] + (size_t)b * 64, x);
#pragma unroll
    for (int k = 0; k < 64; k++) x[k] = (int)(s[k] >> 16);
    jpeg_fdct_quant_block(x, a.recip[1], a.half[1]);
    store_block(a.coef[2] + (size_t)b * 64, x);
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

int free_error(const JpegError& e) { mis_jpeg_set_last_error(e.text); return e.code; }

JpegEncParams to_params(const MisJpegEncodeParams* p) { return p ? JpegEncParams{p->quality, p->sampling, p->restart_interval} : JpegEncParams{0, JPEG_ENC_420, 0}; }

int hand_over(const std::vector<uint8_t>& bytes, MisJpegStream* out) {
    out->data = (uint8_t*)malloc(bytes.size());
    if (!out->data) return MIS_E_NOMEM;
    memcpy(out->data, bytes.data(), bytes.size());
    out->bytes = bytes.size();
    return MIS_OK;
}

constexpr int JPEG_ENC_CHUNKS = 32;     // per frame at most: more chunks than host threads even out rows that code slowly

// Everything up to the coefficients in the pinned staging: checks, argument table, launches, download.  `planes` point into the
// staging, which is the next call's to overwrite.  ms (optional): the launches and the download between events.
int transform_batch(MisContext* ctx, const MisImage* srcs, int n, const MisJpegEncodeParams* params, std::vector<JpegEncGeom>* G, JpegEncParams* P,
                    std::vector<std::array<const int16_t*, 3>>* planes, float* ms) {
    MIS_CHECK(ctx, srcs, MIS_E_INVALID, "jpeg: null argument");
    MIS_CHECK(ctx, n > 0 && n <= 65535, MIS_E_INVALID, "jpeg: a batch of %d frames (1 .. 65535)", n);
    JpegError e;
    const JpegEncParams in = to_params(params);
    for (int i = 0; i < n; i++) {
        if (jpeg_enc_check(srcs[i].width, srcs[i].height, srcs[i].channels, srcs[i].dtype == MIS_U8, &in, P, &e) != JPEG_OK)
            return mis_set_error(ctx, e.code, "frame %d: %s", i, e.text);
        MIS_CHECK(ctx, srcs[i].data, MIS_E_INVALID, "frame %d: jpeg: null image data", i);
        MIS_CHECK(ctx, srcs[i].stride >= (size_t)srcs[i].width * 3, MIS_E_INVALID, "frame %d: jpeg: stride %zu smaller than a row", i, srcs[i].stride);
    }
    G->resize(n);
    planes->resize(n);
    // one layout for the pinned staging and the device block: [argument table][coefficients of every frame and component]
    const size_t args_bytes = mis_align_up((size_t)n * sizeof(JpegEncFrameArgs), 256);
    std::vector<std::array<size_t, 3>> coef_off(n);
    size_t off = args_bytes;
    for (int i = 0; i < n; i++) {
        (*G)[i] = jpeg_enc_geometry(srcs[i].width, srcs[i].height, P->sampling);
        for (int c = 0; c < 3; c++) { coef_off[i][c] = off; off += mis_align_up((*G)[i].blocks(c) * 64 * sizeof(int16_t), 256); }
    }
    const size_t total_bytes = off;
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    void* hs = nullptr;
    if (int rc = mis_host_stage(ctx, total_bytes, &hs)) return rc;
    uint8_t* host = (uint8_t*)hs;
    OwnedEvent ev[3];
    if (ms)
        for (OwnedEvent& v : ev) MIS_HIP(ctx, v.ready(hipEventDefault));
    PoolBlock blk(ctx);
    if (int rc = blk.alloc(total_bytes)) return rc;
    uint8_t* dev = (uint8_t*)blk.p;
    std::vector<DevView> din(n);
    for (int i = 0; i < n; i++)
        if (int rc = din[i].read(ctx, &srcs[i])) return rc;
    uint16_t q[2][64];
    for (int t = 0; t < 2; t++) jpeg_enc_qtable(P->quality, t, q[t]);
    JpegEncFrameArgs* A = (JpegEncFrameArgs*)host;
    memset(A, 0, args_bytes);
    size_t max_luma = 0, max_chroma = 0;
    for (int i = 0; i < n; i++) {
        JpegEncFrameArgs& a = A[i];
        const JpegEncGeom& g = (*G)[i];
        a.src = (const uint8_t*)din[i].data; a.stride = din[i].stride;
        a.w = g.w; a.h = g.h; a.hmax = g.hmax; a.vmax = g.vmax;
        for (int c = 0; c < 3; c++) {
            a.coef[c] = (int16_t*)(dev + coef_off[i][c]);
            (*planes)[i][c] = (const int16_t*)(host + coef_off[i][c]);
            a.bw[c] = g.bw[c]; a.bh[c] = g.bh[c]; a.wb[c] = g.wb[c]; a.hb[c] = g.hb[c];
        }
        a.src_dwords = (((uintptr_t)din[i].data | din[i].stride) & 3) == 0;
        for (int t = 0; t < 2; t++)
            for (int k = 0; k < 64; k++) jpeg_enc_divisor(q[t][k], &a.recip[t][k], &a.half[t][k]);
        max_luma = std::max(max_luma, g.blocks(0));
        max_chroma = std::max(max_chroma, g.blocks(1));
    }
    if (ms) MIS_HIP(ctx, hipEventRecord(ev[0].ev, ctx->stream));
    MIS_HIP(ctx, hipMemcpyAsync(dev, host, args_bytes, hipMemcpyHostToDevice, ctx->stream));
    const JpegEncFrameArgs* dA = (const JpegEncFrameArgs*)dev;
    hipLaunchKernelGGL(jpeg_enc_luma_kernel, dim3((unsigned)((max_luma + 255) / 256), 1, n), dim3(256), 0, ctx->stream, dA);
    MIS_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(jpeg_enc_chroma_kernel, dim3((unsigned)((max_chroma + 255) / 256), 1, n), dim3(256), 0, ctx->stream, dA);
    MIS_HIP(ctx, hipGetLastError());
    if (ms) MIS_HIP(ctx, hipEventRecord(ev[1].ev, ctx->stream));
    MIS_HIP(ctx, hipMemcpyAsync(host + args_bytes, dev + args_bytes, total_bytes - args_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (ms) MIS_HIP(ctx, hipEventRecord(ev[2].ev, ctx->stream));
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ms)
        for (int k = 0; k < 2; k++) MIS_HIP(ctx, hipEventElapsedTime(&ms[k], ev[k].ev, ev[k + 1].ev));
    blk.release();
    return MIS_OK;
}

int encode_batch(MisContext* ctx, const MisImage* srcs, int n, const MisJpegEncodeParams* params, MisJpegStream* outs, float* ms) {
    MIS_CHECK(ctx, outs, MIS_E_INVALID, "jpeg: null argument");
    std::vector<JpegEncGeom> G;
    std::vector<std::array<const int16_t*, 3>> planes;
    JpegEncParams P;
    if (int rc = transform_batch(ctx, srcs, n, params, &G, &P, &planes, ms)) return rc;
    static const JpegEncTables T;
    // every chunk of every frame on the host threads, then every frame's join
    auto t0 = std::chrono::steady_clock::now();
    std::vector<std::vector<JpegEncChunk>> chunks(n);
    struct Task { int frame; size_t chunk; };
    std::vector<Task> tasks;
    for (int i = 0; i < n; i++) {
        jpeg_enc_plan(G[i], P.restart_interval, JPEG_ENC_CHUNKS, &chunks[i]);
        for (size_t k = 0; k < chunks[i].size(); k++) tasks.push_back({i, k});
    }
    run_on_host_threads(tasks.size(), [&](size_t t) {
        const Task& k = tasks[t];
        jpeg_enc_code(planes[k.frame].data(), G[k.frame], P.restart_interval, T, &chunks[k.frame][k.chunk]);
    });
    for (const Task& k : tasks) {
        const JpegError& e = chunks[k.frame][k.chunk].err;
        if (e.code != JPEG_OK) return mis_set_error(ctx, e.code, "frame %d: %s", k.frame, e.text);
    }
    if (ms) ms[2] = (float)ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    std::vector<std::vector<uint8_t>> head(n);
    for (int i = 0; i < n; i++) jpeg_enc_headers(G[i], P, &head[i]);
    if (ms) ms[4] = (float)ms_since(t0);
    // the join: every chunk counts the bytes it owns, the counts place them in the file, every chunk writes its own
    t0 = std::chrono::steady_clock::now();
    std::vector<JpegEncJoin> J(n);
    for (int i = 0; i < n; i++) jpeg_enc_join_begin(chunks[i], P.restart_interval, &J[i]);
    run_on_host_threads(tasks.size(), [&](size_t t) { jpeg_enc_join_count(chunks[tasks[t].frame], &J[tasks[t].frame], tasks[t].chunk); });
    for (int i = 0; i < n; i++) jpeg_enc_join_layout(&J[i], head[i].size());
    std::vector<MisJpegStream> made(n, MisJpegStream{nullptr, 0});
    for (int i = 0; i < n; i++) {
        made[i].data = (uint8_t*)malloc(J[i].bytes);
        made[i].bytes = J[i].bytes;
        if (!made[i].data) {
            for (int k = 0; k < i; k++) mis_jpeg_stream_free(&made[k]);
            return mis_set_error(ctx, MIS_E_NOMEM, "jpeg: no host memory for a stream of %zu bytes", J[i].bytes);
        }
        memcpy(made[i].data, head[i].data(), head[i].size());
    }
    run_on_host_threads(tasks.size(), [&](size_t t) { jpeg_enc_join_write(chunks[tasks[t].frame], J[tasks[t].frame], tasks[t].chunk, made[tasks[t].frame].data); });
    for (int i = 0; i < n; i++) outs[i] = made[i];
    if (ms) ms[3] = (float)ms_since(t0);
    return MIS_OK;
}

}  // namespace

extern "C" int mis_jpeg_stream_free(MisJpegStream* s) {
    if (!s) return MIS_OK;
    free(s->data);
    s->data = nullptr;
    s->bytes = 0;
    return MIS_OK;
}

extern "C" int mis_jpeg_encode_batch(MisContext* ctx, const MisImage* srcs, int n, const MisJpegEncodeParams* params, MisJpegStream* outs) {
    if (!ctx) return MIS_E_INVALID;
    return encode_batch(ctx, srcs, n, params, outs, nullptr);
}

extern "C" int mis_jpeg_encode_batch_timed(MisContext* ctx, const MisImage* srcs, int n, const MisJpegEncodeParams* params, MisJpegStream* outs, float ms[5]) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, ms, MIS_E_INVALID, "jpeg: null argument");
    return encode_batch(ctx, srcs, n, params, outs, ms);
}

extern "C" int mis_jpeg_encode(MisContext* ctx, const MisImage* src_bgr, const MisJpegEncodeParams* params, MisJpegStream* out) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, src_bgr && out, MIS_E_INVALID, "jpeg: null argument");
    return encode_batch(ctx, src_bgr, 1, params, out, nullptr);
}

extern "C" int mis_jpeg_debug_entropy_encode(const int16_t* const coef[3], int w, int h, const MisJpegEncodeParams* params, int chunks, MisJpegStream* out) {
    JpegError e;
    if (!coef || !coef[0] || !coef[1] || !coef[2] || !out) return free_error((jpeg_fail(&e, JPEG_INVALID, "jpeg: null argument"), e));
    const JpegEncParams in = to_params(params);
    JpegEncParams P;
    if (jpeg_enc_check(w, h, 3, true, &in, &P, &e) != JPEG_OK) return free_error(e);
    std::vector<uint8_t> bytes;
    if (jpeg_enc_stream(coef, jpeg_enc_geometry(w, h, P.sampling), P, chunks, &bytes, &e) != JPEG_OK) return free_error(e);
    if (hand_over(bytes, out) != MIS_OK) return free_error((jpeg_fail(&e, MIS_E_NOMEM, "jpeg: no host memory for a stream of %zu bytes", bytes.size()), e));
    mis_jpeg_set_last_error("");
    return MIS_OK;
}

extern "C" int mis_jpeg_debug_encode_coefficients(MisContext* ctx, const MisImage* src_bgr, const MisJpegEncodeParams* params, int component,
                                                  int16_t* out, size_t capacity, uint16_t qtable[64]) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, src_bgr && out && qtable, MIS_E_INVALID, "jpeg: null argument");
    MIS_CHECK(ctx, component >= 0 && component < 3, MIS_E_INVALID, "jpeg: component %d of 3", component);
    // the capacity is checked against the geometry before anything is launched
    JpegError e;
    JpegEncParams P;
    const JpegEncParams in = to_params(params);
    if (jpeg_enc_check(src_bgr->width, src_bgr->height, src_bgr->channels, src_bgr->dtype == MIS_U8, &in, &P, &e) != JPEG_OK)
        return mis_set_error(ctx, e.code, "frame 0: %s", e.text);
    const size_t need = jpeg_enc_geometry(src_bgr->width, src_bgr->height, P.sampling).blocks(component) * 64;
    MIS_CHECK(ctx, capacity >= need, MIS_E_INVALID, "jpeg: component %d has %zu coefficients, capacity %zu", component, need, capacity);
    std::vector<JpegEncGeom> G;
    std::vector<std::array<const int16_t*, 3>> planes;
    if (int rc = transform_batch(ctx, src_bgr, 1, params, &G, &P, &planes, nullptr)) return rc;
    memcpy(out, planes[0][component], need * sizeof(int16_t));
    jpeg_enc_qtable(P.quality, component ? 1 : 0, qtable);
    return MIS_OK;
}
