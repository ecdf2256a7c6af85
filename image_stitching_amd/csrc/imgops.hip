// imgops.hip -- the small image operators either side of the hot path:
//   cv::resize(..., INTER_LINEAR_EXACT)   image_stitching/image_stitching.cpp:573-580 (work scale), :619 (seam scale),
//                                         :1144 (compose scale), :1170 (seam mask -> compose size)
//   cv::rotate(90 CW / 180 / 90 CCW)      image_stitching/image_stitching.cpp:571, :576
//   dilate(3x3) -> resize -> AND          image_stitching/image_stitching.cpp:1169-1171, fused into one kernel
//   cv::resize of every frame of a job      image_stitching/image_stitching.cpp:589-603 (work scale), one launch
// All of it is byte arithmetic bound by HBM: one thread per destination pixel (16 B of output per thread for
// the mask kernel; 4 pixels x 2 rows for the batched resize), coalesced along rows, coefficient tables built on the
// host exactly as resize() does.
#include "common.h"
#include "dev_math.h"
#include <vector>

namespace {

// resize.cpp: destination index i samples (i + 0.5) * scale - 0.5; 8.8 fixed-point weight of the right / lower
// tap; clamped to the first / last sample
void coeffs(int dlen, int slen, double scale, int* ofs, int* m1) {
    for (int i = 0; i < dlen; i++) {
        double v = ((double)i + 0.5) * scale - 0.5;
        int iv = (int)v; iv -= (iv > v);
        if (iv < 0) { ofs[i] = 0; m1[i] = 0; }
        else if (iv >= slen - 1) { ofs[i] = slen - 1; m1[i] = 0; }
        else { ofs[i] = iv; m1[i] = mis_round_d((v - (double)iv) * 256.0); }
    }
}

// device copy of {xofs[dw], xm1[dw], yofs[dh], ym1[dh]} in the context's grow-only scratch
int upload_tables(MisContext* ctx, int sw, int sh, int dw, int dh, double sx, double sy, const int** tab) {
    std::vector<int> h(2 * (size_t)dw + 2 * (size_t)dh);
    coeffs(dw, sw, sx, h.data(), h.data() + dw);
    coeffs(dh, sh, sy, h.data() + 2 * dw, h.data() + 2 * dw + dh);
    const size_t bytes = h.size() * sizeof(int);
    if (int rc = mis_dev_stage(ctx, bytes, (void**)tab)) return rc;
    // pageable source: the copy is complete for the host when the call returns, so `h` may go out of scope
    MIS_HIP(ctx, hipMemcpyAsync((void*)*tab, h.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MIS_OK;
}

template <int CN>
__global__ __launch_bounds__(256) void resize_exact_kernel(const uint8_t* __restrict__ src, int sw, int sh, size_t ss, uint8_t* __restrict__ dst, int dw,
                                                          int dh, size_t ds, const int* __restrict__ tab) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    const int *xo = tab, *xm = tab + dw, *yo = tab + 2 * dw, *ym = tab + 2 * dw + dh;
    const int x0 = xo[x], x1 = x0 + 1 < sw ? x0 + 1 : x0, mx1 = xm[x], mx0 = 256 - mx1;
    const int y0 = yo[y], y1 = y0 + 1 < sh ? y0 + 1 : y0, my1 = ym[y], my0 = 256 - my1;
    const uint8_t* r0 = src + (size_t)y0 * ss;
    const uint8_t* r1 = src + (size_t)y1 * ss;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        const unsigned h0 = (unsigned)r0[x0 * CN + c] * mx0 + (unsigned)r0[x1 * CN + c] * mx1;
        const unsigned h1 = (unsigned)r1[x0 * CN + c] * mx0 + (unsigned)r1[x1 * CN + c] * mx1;
        dst[(size_t)y * ds + (size_t)x * CN + c] = (uint8_t)((h0 * my0 + h1 * my1 + (1u << 15)) >> 16);
    }
}

template <int CN>
__global__ __launch_bounds__(256) void rotate_kernel(const uint8_t* __restrict__ src, int sw, int sh, size_t ss, int code, uint8_t* __restrict__ dst,
                                                    int dw, int dh, size_t ds) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= dw) return;
    int sx, sy;
    if (code == 0) { sx = y; sy = sh - 1 - x; }
    else if (code == 1) { sx = sw - 1 - x; sy = sh - 1 - y; }
    else { sx = sw - 1 - y; sy = x; }
    const uint8_t* s = src + (size_t)sy * ss + (size_t)sx * CN;
    uint8_t* d = dst + (size_t)y * ds + (size_t)x * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) d[c] = s[c];
}

// max over the 3x3 neighbourhood inside the image (the dilate border value never wins)
__device__ __forceinline__ unsigned dil3(const uint8_t* __restrict__ s, int w, int h, size_t ss, int x, int y) {
    unsigned m = 0;
    const int ya = y > 0 ? y - 1 : 0, yb = y + 1 < h ? y + 1 : h - 1, xa = x > 0 ? x - 1 : 0, xb = x + 1 < w ? x + 1 : w - 1;
    for (int yy = ya; yy <= yb; yy++)
        for (int xx = xa; xx <= xb; xx++) m = max(m, (unsigned)s[(size_t)yy * ss + xx]);
    return m;
}

// mask &= resize(dilate(seam)): 4 destination pixels per thread; the seam mask is ~0.1 MP and stays in L2
__global__ __launch_bounds__(256) void seam_mask_kernel(const uint8_t* __restrict__ seam, int sw, int sh, size_t ss, uint8_t* __restrict__ mask, int mw,
                                                       int mh, size_t ms, const int* __restrict__ tab) {
    const int xb = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y;
    if (xb >= mw) return;
    const int *xo = tab, *xm = tab + mw, *yo = tab + 2 * mw, *ym = tab + 2 * mw + mh;
    const int y0 = yo[y], y1 = y0 + 1 < sh ? y0 + 1 : y0, my1 = ym[y], my0 = 256 - my1;
    uint8_t* m = mask + (size_t)y * ms;
    for (int k = 0; k < 4 && xb + k < mw; k++) {
        const int x = xb + k;
        if (m[x] == 0) continue;   // x & 0 = 0
        const int x0 = xo[x], x1 = x0 + 1 < sw ? x0 + 1 : x0, mx1 = xm[x], mx0 = 256 - mx1;
        const unsigned h0 = dil3(seam, sw, sh, ss, x0, y0) * mx0 + dil3(seam, sw, sh, ss, x1, y0) * mx1;
        const unsigned h1 = dil3(seam, sw, sh, ss, x0, y1) * mx0 + dil3(seam, sw, sh, ss, x1, y1) * mx1;
        m[x] &= (uint8_t)((h0 * my0 + h1 * my1 + (1u << 15)) >> 16);
    }
}

// ---------------------------------------------------------------- batched resize (work scale) --
// mis_resize_linear_exact_batch: the frames of a job -> their work-scale images in one launch (image_stitching.cpp:589-603).
// The tables are packed (offset << 9 | weight of the right / lower tap, 0..256), x entries padded with zeros to a multiple of
// four so that a thread reads its four columns as one int4, then the y entries: {xt[dw4], yt[dh]}.
constexpr int RB_MAX = 32;       // frames per launch (pointers and strides travel as kernel arguments)
struct ResizeBatchArgs {
    const uint8_t* src[RB_MAX];
    uint8_t* dst[RB_MAX];
    unsigned ss[RB_MAX], ds[RB_MAX];
};

// grow-only cache of device tables, one per geometry; released with the context
struct ResizeTables : MisWorkspace {
    struct Entry { int sw, sh, dw, dh; double sx, sy; int* dev; };
    std::vector<Entry> entries;
    ~ResizeTables() override { for (Entry& e : entries) hipFree(e.dev); }
};

void packed_coeffs(int dlen, int slen, double scale, int* out) {
    std::vector<int> ofs(dlen), m1(dlen);
    coeffs(dlen, slen, scale, ofs.data(), m1.data());
    for (int i = 0; i < dlen; i++) out[i] = (ofs[i] << 9) | m1[i];
}

// a hit returns the cached pointer: no upload, no synchronisation.  A miss builds the tables in the context's pinned staging,
// uploads them to a block of their own and waits for that copy (the staging is anybody's after the call).
int cached_tables(MisContext* ctx, int sw, int sh, int dw, int dh, double sx, double sy, const int** tab) {
    if (!ctx->resize_ws) ctx->resize_ws = new ResizeTables();
    ResizeTables* ws = static_cast<ResizeTables*>(ctx->resize_ws);
    for (const ResizeTables::Entry& e : ws->entries)
        if (e.sw == sw && e.sh == sh && e.dw == dw && e.dh == dh && e.sx == sx && e.sy == sy) { *tab = e.dev; return MIS_OK; }
    const int dw4 = (dw + 3) & ~3;
    const size_t bytes = ((size_t)dw4 + (size_t)dh) * sizeof(int);
    void* hs = nullptr;
    if (int rc = mis_host_stage(ctx, bytes, &hs)) return rc;
    int* h = (int*)hs;
    packed_coeffs(dw, sw, sx, h);
    for (int i = dw; i < dw4; i++) h[i] = 0;
    packed_coeffs(dh, sh, sy, h + dw4);
    int* dev = nullptr;
    MIS_HIP(ctx, hipMalloc(&dev, bytes));
    hipError_t e = hipMemcpyAsync(dev, h, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { hipFree(dev); MIS_HIP(ctx, e); }
    ws->entries.push_back({sw, sh, dw, dh, sx, sy, dev});
    *tab = dev;
    return MIS_OK;
}

// A thread produces four consecutive destination pixels of ROWS rows: 12 bytes (8UC3) or 4 (8UC1) per row, stored as dwords.
// The two taps of a destination pixel are adjacent source pixels, 2 * CN contiguous bytes: with the dword that holds the first
// byte they lie inside NW aligned dwords (one dwordx3 / dwordx2 load per pixel, row and tap row instead of 2 * CN byte loads),
// and v_alignbyte brings them to bit 0.  The x entries are read once and serve all rows; every load of the thread is in flight
// before the first is used.  Pixels whose dwords would pass the end of a source row (the last two or three of a row), and
// images whose rows are not dword aligned, take byte loads packed into the same layout; a ragged last group stores bytes.
// flags: bit 0 every source base and stride is a multiple of 4, bit 1 every destination's is.
template <int CN, int ROWS>
__global__ __launch_bounds__(256) void resize_batch_kernel(const ResizeBatchArgs A, int sw, int sh, int dw, int dh, const int* __restrict__ tab, int flags) {
    constexpr int NW = CN == 3 ? 3 : 2;
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int ybase = __builtin_amdgcn_readfirstlane((blockIdx.y * 4 + (threadIdx.x >> 6)) * ROWS);
    if (x >= dw || ybase >= dh) return;
    const int f = blockIdx.z;
    const uint8_t* __restrict__ src = A.src[f];
    uint8_t* __restrict__ dst = A.dst[f];
    const size_t ss = A.ss[f], ds = A.ds[f];
    const int dw4 = (dw + 3) & ~3;
    const int* yt = tab + dw4;
    const int4 xt = *reinterpret_cast<const int4*>(tab + x);
    const int xe[4] = {xt.x, xt.y, xt.z, xt.w};
    const int nvalid = min(4, dw - x), nrows = min(ROWS, dh - ybase);
    int x0[4], mx1[4], al[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { x0[k] = xe[k] >> 9; mx1[k] = xe[k] & 511; al[k] = (x0[k] * CN) & ~3; }
    // (the zero padding past dw reads column 0: the largest offset of the four decides)
    const bool fast = (flags & 1) && max(max(al[0], al[1]), max(al[2], al[3])) + 4 * NW <= sw * CN;
    unsigned w[ROWS][2][4][NW];
    int my1[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        const int y = min(ybase + r, dh - 1);       // (rows past the image repeat its last row and are not stored)
        const int ye = yt[y], y0 = ye >> 9, y1 = y0 + 1 < sh ? y0 + 1 : y0;
        my1[r] = ye & 511;
        const uint8_t* rp[2] = {src + (size_t)y0 * ss, src + (size_t)y1 * ss};
        if (fast) {
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const unsigned* p = reinterpret_cast<const unsigned*>(rp[t] + al[k]);
#pragma unroll
                    for (int q = 0; q < NW; q++) w[r][t][k][q] = p[q];
                }
        } else {
#pragma unroll
            for (int t = 0; t < 2; t++)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const uint8_t* a = rp[t] + (size_t)x0[k] * CN;
                    const uint8_t* b = rp[t] + (size_t)(x0[k] + 1 < sw ? x0[k] + 1 : x0[k]) * CN;
                    if (CN == 3) {
                        w[r][t][k][0] = (unsigned)a[0] | ((unsigned)a[1] << 8) | ((unsigned)a[2] << 16) | ((unsigned)b[0] << 24);
                        w[r][t][k][1] = (unsigned)b[1] | ((unsigned)b[2] << 8);
                        w[r][t][k][NW - 1] = 0;
                    } else {
                        w[r][t][k][0] = (unsigned)a[0] | ((unsigned)b[0] << 8);
                        w[r][t][k][1] = 0;
                    }
                }
        }
    }
    const bool dwords = (flags & 2) && nvalid == 4;
#pragma unroll
    for (int r = 0; r < ROWS; r++) {
        if (r >= nrows) break;
        const unsigned my0 = 256 - my1[r];
        unsigned v[4][CN];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned o = fast ? (unsigned)(x0[k] * CN) & 3u : 0u, m1 = mx1[k], m0 = 256 - m1;
            unsigned lo[2], hi[2];      // bytes o .. o + 3 and o + 4 .. o + 7 of the loaded dwords, per tap row
#pragma unroll
            for (int t = 0; t < 2; t++) {
                lo[t] = __builtin_amdgcn_alignbyte(w[r][t][k][1], w[r][t][k][0], o);
                hi[t] = CN == 3 ? __builtin_amdgcn_alignbyte(w[r][t][k][NW - 1], w[r][t][k][1], o) : 0u;
            }
#pragma unroll
            for (int c = 0; c < CN; c++) {
                unsigned a[2], b[2];
#pragma unroll
                for (int t = 0; t < 2; t++) {
                    a[t] = (lo[t] >> (8 * c)) & 255u;
                    const int cb = CN + c;      // byte of the right tap
                    b[t] = (cb < 4 ? lo[t] >> (8 * cb) : hi[t] >> (8 * (cb - 4))) & 255u;
                }
                const unsigned h0 = a[0] * m0 + b[0] * m1, h1 = a[1] * m0 + b[1] * m1;
                v[k][c] = (h0 * my0 + h1 * (unsigned)my1[r] + (1u << 15)) >> 16;
            }
        }
        uint8_t* out = dst + (size_t)(ybase + r) * ds + (size_t)x * CN;
        if (dwords) {
            if (CN == 3) {
                unsigned* o32 = reinterpret_cast<unsigned*>(out);
                o32[0] = v[0][0] | (v[0][1] << 8) | (v[0][2] << 16) | (v[1][0] << 24);
                o32[1] = v[1][1] | (v[1][2] << 8) | (v[2][0] << 16) | (v[2][1] << 24);
                o32[2] = v[2][2] | (v[3][0] << 8) | (v[3][1] << 16) | (v[3][2] << 24);
            } else {
                *reinterpret_cast<unsigned*>(out) = v[0][0] | (v[1][0] << 8) | (v[2][0] << 16) | (v[3][0] << 24);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (k < nvalid)
#pragma unroll
                    for (int c = 0; c < CN; c++) out[k * CN + c] = (uint8_t)v[k][c];
        }
    }
}

}  // namespace

extern "C" int mis_resize_linear_exact(MisContext* ctx, const MisImage* src, int dst_w, int dst_h, double fx, double fy, MisImage* dst) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, src && dst && src->data, MIS_E_INVALID, "null image");
    MIS_CHECK(ctx, src->dtype == MIS_U8 && (src->channels == 1 || src->channels == 3), MIS_E_UNSUPPORTED, "resize: 8UC1 / 8UC3 only");
    const bool by_factor = !(dst_w > 0 && dst_h > 0);
    MIS_CHECK(ctx, !by_factor || (fx > 0 && fy > 0), MIS_E_INVALID, "resize needs a destination size or positive scale factors");
    // resize(): dsize = saturate_cast<int>(ssize * inv_scale) when empty; inv_scale = dsize / ssize when given
    const int dw = by_factor ? mis_round_d((double)src->width * fx) : dst_w, dh = by_factor ? mis_round_d((double)src->height * fy) : dst_h;
    MIS_CHECK(ctx, dw > 0 && dh > 0 && dw <= 65535 && dh <= 65535, MIS_E_INVALID, "resize destination %dx%d out of range", dw, dh);
    const double sx = by_factor ? 1.0 / fx : 1.0 / ((double)dw / (double)src->width);
    const double sy = by_factor ? 1.0 / fy : 1.0 / ((double)dh / (double)src->height);
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    DevView din, dout;
    int rc;
    if ((rc = din.read(ctx, src)) != MIS_OK) return rc;
    if ((rc = dout.write(ctx, dst, dw, dh, src->channels, MIS_U8)) != MIS_OK) return rc;
    const int* tab;
    if ((rc = upload_tables(ctx, src->width, src->height, dw, dh, sx, sy, &tab)) != MIS_OK) return rc;
    dim3 grid((dw + 255) / 256, dh), block(256);
    if (src->channels == 3)
        hipLaunchKernelGGL(resize_exact_kernel<3>, grid, block, 0, ctx->stream, (const uint8_t*)din.data, src->width, src->height, din.stride, (uint8_t*)dout.data, dw, dh, dout.stride, tab);
    else
        hipLaunchKernelGGL(resize_exact_kernel<1>, grid, block, 0, ctx->stream, (const uint8_t*)din.data, src->width, src->height, din.stride, (uint8_t*)dout.data, dw, dh, dout.stride, tab);
    MIS_HIP(ctx, hipGetLastError());
    return dout.commit();
}

extern "C" int mis_resize_linear_exact_batch(MisContext* ctx, const MisImage* srcs, int n, int dst_w, int dst_h, double fx, double fy, MisImage* dsts) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, srcs && dsts, MIS_E_INVALID, "null image array");
    MIS_CHECK(ctx, n > 0, MIS_E_INVALID, "resize batch of %d images", n);
    const MisImage& s0 = srcs[0];
    MIS_CHECK(ctx, s0.data && s0.width > 0 && s0.height > 0 && s0.width < (1 << 22) && s0.height < (1 << 22), MIS_E_INVALID, "null image or size out of range (0)");
    MIS_CHECK(ctx, s0.dtype == MIS_U8 && (s0.channels == 1 || s0.channels == 3), MIS_E_UNSUPPORTED, "resize: 8UC1 / 8UC3 only");
    const bool by_factor = !(dst_w > 0 && dst_h > 0);
    MIS_CHECK(ctx, !by_factor || (fx > 0 && fy > 0), MIS_E_INVALID, "resize needs a destination size or positive scale factors");
    // the size and scale rules of mis_resize_linear_exact (resize(); image_stitching.cpp:602 calls it by factor)
    const int dw = by_factor ? mis_round_d((double)s0.width * fx) : dst_w, dh = by_factor ? mis_round_d((double)s0.height * fy) : dst_h;
    MIS_CHECK(ctx, dw > 0 && dh > 0 && dw <= 65535 && dh <= 65535, MIS_E_INVALID, "resize destination %dx%d out of range", dw, dh);
    const double sx = by_factor ? 1.0 / fx : 1.0 / ((double)dw / (double)s0.width);
    const double sy = by_factor ? 1.0 / fy : 1.0 / ((double)dh / (double)s0.height);
    // everything is checked before anything is staged or allocated
    for (int i = 0; i < n; i++) {
        const MisImage &s = srcs[i], &d = dsts[i];
        MIS_CHECK(ctx, s.data, MIS_E_INVALID, "null image (%d)", i);
        MIS_CHECK(ctx, s.width == s0.width && s.height == s0.height && s.channels == s0.channels && s.dtype == s0.dtype, MIS_E_INVALID,
                  "resize batch: image %d is %dx%dx%d dtype %d, image 0 %dx%dx%d dtype %d", i, s.width, s.height, s.channels, s.dtype, s0.width, s0.height, s0.channels, s0.dtype);
        MIS_CHECK(ctx, s.stride >= (size_t)s0.width * s0.channels && s.stride <= 0xffffffffu, MIS_E_INVALID, "resize batch: bad stride (%d)", i);
        if (!d.data) continue;      // allocated below
        MIS_CHECK(ctx, d.width == dw && d.height == dh && d.channels == s0.channels && d.dtype == MIS_U8, MIS_E_INVALID,
                  "resize batch: output %d is %dx%dx%d dtype %d, expected %dx%dx%d dtype %d", i, d.width, d.height, d.channels, d.dtype, dw, dh, s0.channels, MIS_U8);
        MIS_CHECK(ctx, d.stride >= (size_t)dw * s0.channels && d.stride <= 0xffffffffu, MIS_E_INVALID, "resize batch: bad output stride (%d)", i);
    }
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    const int* tab;
    if (int rc = cached_tables(ctx, s0.width, s0.height, dw, dh, sx, sy, &tab)) return rc;
    // device images are used in place; host images are staged as mis_resize_linear_exact stages them (a copy and a wait each)
    std::vector<DevView> din(n), dout(n);
    int rc = MIS_OK, flags = 3;
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = din[i].read(ctx, &srcs[i]);
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = dout[i].write(ctx, &dsts[i], dw, dh, s0.channels, MIS_U8);
    constexpr int ROWS = 2;
    for (int b = 0; b < n && rc == MIS_OK; b += RB_MAX) {       // (a job's frames are one launch; more than RB_MAX frames take one per RB_MAX)
        const int m = n - b < RB_MAX ? n - b : RB_MAX;
        if (b == 0)
            for (int i = 0; i < n; i++) {
                if (((uintptr_t)din[i].data | din[i].stride) & 3) flags &= ~1;
                if (((uintptr_t)dout[i].data | dout[i].stride) & 3) flags &= ~2;
            }
        ResizeBatchArgs A;
        memset(&A, 0, sizeof(A));
        for (int i = 0; i < m; i++) {
            A.src[i] = (const uint8_t*)din[b + i].data; A.dst[i] = (uint8_t*)dout[b + i].data;
            A.ss[i] = (unsigned)din[b + i].stride; A.ds[i] = (unsigned)dout[b + i].stride;
        }
        const dim3 grid(((dw + 3) / 4 + 63) / 64, (dh + 4 * ROWS - 1) / (4 * ROWS), m), block(256);
        if (s0.channels == 3)
            hipLaunchKernelGGL((resize_batch_kernel<3, ROWS>), grid, block, 0, ctx->stream, A, s0.width, s0.height, dw, dh, tab, flags);
        else
            hipLaunchKernelGGL((resize_batch_kernel<1, ROWS>), grid, block, 0, ctx->stream, A, s0.width, s0.height, dw, dh, tab, flags);
        if (hipGetLastError() != hipSuccess) rc = mis_set_error(ctx, MIS_E_HIP, "resize batch: launch failed");
    }
    for (int i = 0; i < n && rc == MIS_OK; i++) rc = dout[i].commit();
    return rc;
}

extern "C" int mis_rotate(MisContext* ctx, const MisImage* src, int rotate_code, MisImage* dst) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, src && dst && src->data, MIS_E_INVALID, "null image");
    MIS_CHECK(ctx, src->dtype == MIS_U8 && (src->channels == 1 || src->channels == 3), MIS_E_UNSUPPORTED, "rotate: 8UC1 / 8UC3 only");
    MIS_CHECK(ctx, rotate_code >= 0 && rotate_code <= 2, MIS_E_INVALID, "rotate code must be 0 (90 CW), 1 (180) or 2 (90 CCW)");
    const int dw = rotate_code == 1 ? src->width : src->height, dh = rotate_code == 1 ? src->height : src->width;
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    DevView din, dout;
    int rc;
    if ((rc = din.read(ctx, src)) != MIS_OK) return rc;
    if ((rc = dout.write(ctx, dst, dw, dh, src->channels, MIS_U8)) != MIS_OK) return rc;
    dim3 grid((dw + 255) / 256, dh), block(256);
    if (src->channels == 3)
        hipLaunchKernelGGL(rotate_kernel<3>, grid, block, 0, ctx->stream, (const uint8_t*)din.data, src->width, src->height, din.stride, rotate_code, (uint8_t*)dout.data, dw, dh, dout.stride);
    else
        hipLaunchKernelGGL(rotate_kernel<1>, grid, block, 0, ctx->stream, (const uint8_t*)din.data, src->width, src->height, din.stride, rotate_code, (uint8_t*)dout.data, dw, dh, dout.stride);
    MIS_HIP(ctx, hipGetLastError());
    return dout.commit();
}

extern "C" int mis_seam_mask_apply(MisContext* ctx, const MisImage* seam, MisImage* mask) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, seam && mask && seam->data && mask->data, MIS_E_INVALID, "null image");
    MIS_CHECK(ctx, seam->dtype == MIS_U8 && seam->channels == 1 && mask->dtype == MIS_U8 && mask->channels == 1, MIS_E_UNSUPPORTED, "masks must be 8UC1");
    MIS_CHECK(ctx, seam->width > 0 && seam->height > 0 && mask->width > 0 && mask->height > 0, MIS_E_INVALID, "empty mask");
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    DevView ds, dm;
    int rc;
    if ((rc = ds.read(ctx, seam)) != MIS_OK || (rc = dm.read_write(ctx, mask)) != MIS_OK) return rc;
    const int* tab;
    const double sx = 1.0 / ((double)mask->width / (double)seam->width), sy = 1.0 / ((double)mask->height / (double)seam->height);
    if ((rc = upload_tables(ctx, seam->width, seam->height, mask->width, mask->height, sx, sy, &tab)) != MIS_OK) return rc;
    hipLaunchKernelGGL(seam_mask_kernel, dim3((mask->width + 1023) / 1024, mask->height), dim3(256), 0, ctx->stream, (const uint8_t*)ds.data, seam->width,
                       seam->height, ds.stride, (uint8_t*)dm.data, mask->width, mask->height, dm.stride, tab);
    MIS_HIP(ctx, hipGetLastError());
    return dm.commit();
}
