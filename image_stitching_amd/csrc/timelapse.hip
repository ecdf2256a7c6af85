// timelapse.hip -- the timelapse output mode: cv::detail::Timelapser / TimelapserCrop (image_stitching.cpp:79, :82, :1083, :1194-1215).
// The compositing loop's other sink: every frame is warped into ONE common canvas -- resultRoi of all frames (AS_IS) or their
// intersection (CROP) -- and written out as a registered frame of its own, with nothing blended.
//   mis_result_roi_intersection      cv::detail::resultRoiIntersection (host only)
//   MisTimelapser                    initialize / process / getDst on an already warped 16SC3 image (timelapse_place_kernel)
//   mis_timelapse_warp_batch         warp -> gains -> canvas of n frames in one launch per 16 frames (timelapse_warp_batch_kernel)
// Nothing here is new arithmetic: mapBackward is the operation sequence of the warp kernels (col_terms / row_terms / map_backward,
// map_backward_polar, col_hoist / col_pixel of warp_shared.h), the sample is sample_linear, the gain is unit_gain_kernel's
// saturate_cast<uchar>(cvRound((float)v * g)) of expos.hip.  What this unit adds is the walk over a canvas that is not the frame's roi.
#include "warp_shared.h"
#include <cmath>

namespace {

// A lane owns TL_LPX = 4 consecutive canvas pixels of one row: 16SC3 is 24 bytes (the compiler writes them as a dwordx4 and a dwordx2 store), 8UC3 is 12 bytes = one dwordx3 store, where
// the canvas rows are 4-byte aligned (elements otherwise and at the canvas's right edge); 32 lanes write a whole 768- / 384-byte run.
// A tile is 128 x TL_TH = 32 rows: a lane evaluates what depends on its columns alone once (the separable kinds' {su, cu}, the
// half-separable kinds' ColTerms) and walks rows (thread >> 5) + 8 k, as warp_maps_kernel does.  The polar kinds hoist nothing.
constexpr int TL_LPX = 4, TL_TW = 32 * TL_LPX, TL_ROWS = 4, TL_TH = 8 * TL_ROWS;
enum { TL_SEPARABLE = 0, TL_POLAR = 1, TL_COMPRESSED = 2, TL_PANINI = 3 };

struct alignas(4) Dwords3 { uint32_t a, b, c; };

// 4 pixels x 3 channels (values 0..255, or anything an int16 holds for the 16SC3 form) -> the canvas row at pixel gx0
template <bool U8>
__device__ __forceinline__ void store_px4(uint8_t* row, int gx0, int cw, bool wide, const int* p) {
    if (U8) {
        uint8_t* d = row + (size_t)gx0 * 3;
        if (wide && gx0 + TL_LPX <= cw) {
            Dwords3 q;
            q.a = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            q.b = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
            q.c = (uint32_t)p[8] | ((uint32_t)p[9] << 8) | ((uint32_t)p[10] << 16) | ((uint32_t)p[11] << 24);
            *reinterpret_cast<Dwords3*>(d) = q;
        } else {
            const int n = (cw - gx0 < TL_LPX ? cw - gx0 : TL_LPX) * 3;
#pragma unroll
            for (int i = 0; i < TL_LPX * 3; i++) if (i < n) d[i] = (uint8_t)p[i];
        }
    } else {
        uint8_t* d = row + (size_t)gx0 * 6;
        if (wide && gx0 + TL_LPX <= cw) {
            Dwords3 q, r;
            q.a = ((uint32_t)p[0] & 0xffffu) | ((uint32_t)p[1] << 16); q.b = ((uint32_t)p[2] & 0xffffu) | ((uint32_t)p[3] << 16);
            q.c = ((uint32_t)p[4] & 0xffffu) | ((uint32_t)p[5] << 16);
            r.a = ((uint32_t)p[6] & 0xffffu) | ((uint32_t)p[7] << 16); r.b = ((uint32_t)p[8] & 0xffffu) | ((uint32_t)p[9] << 16);
            r.c = ((uint32_t)p[10] & 0xffffu) | ((uint32_t)p[11] << 16);
            reinterpret_cast<Dwords3*>(d)[0] = q;
            reinterpret_cast<Dwords3*>(d)[1] = r;
        } else {
            const int n = (cw - gx0 < TL_LPX ? cw - gx0 : TL_LPX) * 3;
            int16_t* s = (int16_t*)d;
#pragma unroll
            for (int i = 0; i < TL_LPX * 3; i++) if (i < n) s[i] = (int16_t)p[i];
        }
    }
}

// ---- Timelapser::process: an already warped 16SC3 image placed into the canvas ----
// dst.setTo(0), then the copy of the part of img that lies in dst_roi, in one pass over the canvas: every canvas pixel is written
// once, the image's where it covers it, 0 elsewhere.  dx, dy = tl - dst_roi's corner (64-bit: any two ints).
struct PlaceArgs {
    const uint8_t* src; size_t sstride; int sw, sh;
    uint8_t* dst; size_t dstride; int cw, ch;
    long long dx, dy;
};
__global__ __launch_bounds__(256) void timelapse_place_kernel(PlaceArgs a) {
    const int gx0 = (int)blockIdx.x * TL_TW + ((int)threadIdx.x & 31) * TL_LPX, gy0 = (int)blockIdx.y * TL_TH + ((int)threadIdx.x >> 5);
    if (gx0 >= a.cw) return;
    const bool wide = (((uintptr_t)a.dst | a.dstride) & 3) == 0;
#pragma unroll 1
    for (int k = 0; k < TL_ROWS; k++) {
        const int gy = gy0 + 8 * k;
        if (gy >= a.ch) break;
        const long long sy = (long long)gy - a.dy;
        const bool row_in = sy >= 0 && sy < a.sh;
        const int16_t* srow = (const int16_t*)(a.src + (size_t)(row_in ? sy : 0) * a.sstride);
        int p[TL_LPX * 3];
#pragma unroll
        for (int i = 0; i < TL_LPX; i++) {
            const long long sx = (long long)(gx0 + i) - a.dx;
            const bool in = row_in && sx >= 0 && sx < a.sw;
            const int16_t* s = srow + (in ? sx : 0) * 3;
            p[3 * i] = in ? s[0] : 0; p[3 * i + 1] = in ? s[1] : 0; p[3 * i + 2] = in ? s[2] : 0;
        }
        store_px4<false>(a.dst + (size_t)gy * a.dstride, gx0, a.cw, wide, p);
    }
}

// ---- the fused batch: warp -> gains -> canvas, frame = grid z ----
// WarpArgs per frame: m = k_rinv, tlx / tly / dw / dh = the frame's warp roi, pa / pb = (A, B) or the affine (t0, t1), src, dst =
// the frame's canvas.  (cx, cy, cw, ch): dst_roi, the same for every frame.
struct TimelapseBatch {
    WarpArgs a[WB_MAX];
    float gain[WB_MAX][3];      // read only with has_gains
    int cx, cy, cw, ch, has_gains;
};

template <int CLASS, bool U8>
__global__ __launch_bounds__(256) void timelapse_warp_batch_kernel(TimelapseBatch b) {
    const WarpArgs& a = b.a[blockIdx.z];
    const int gx0 = (int)blockIdx.x * TL_TW + ((int)threadIdx.x & 31) * TL_LPX, gy0 = (int)blockIdx.y * TL_TH + ((int)threadIdx.x >> 5);
    if (gx0 >= b.cw) return;
    const bool wide = (((uintptr_t)a.dst | a.dstride) & 3) == 0;
    // the canvas columns of this lane in the frame's roi (64-bit: dst_roi and the roi are any rectangles)
    const long long rx0 = (long long)b.cx + gx0 - a.tlx, ry_off = (long long)b.cy - a.tly;
    bool col_in[TL_LPX], any_col = false;
    float su[TL_LPX], cu[TL_LPX];
    ColTerms ct[TL_LPX];
#pragma unroll
    for (int i = 0; i < TL_LPX; i++) {
        col_in[i] = rx0 + i >= 0 && rx0 + i < a.dw;
        any_col |= col_in[i];
        const float u = (float)(b.cx + gx0 + i);    // a column of the roi: the int sum cannot wrap; outside it the value is not used
        if (CLASS == TL_SEPARABLE) col_terms(a.kind, a.scale, u, a.pa, &su[i], &cu[i]);
        else if (CLASS == TL_COMPRESSED) ct[i] = col_hoist<MIS_WARP_COMPRESSED_PLANE_A2B1>(a.scale, a.pa, a.pb, u);
        else if (CLASS == TL_PANINI) ct[i] = col_hoist<MIS_WARP_PANINI_A2B1>(a.scale, a.pa, a.pb, u);
    }
    const float g0 = b.gain[blockIdx.z][0], g1 = b.gain[blockIdx.z][1], g2 = b.gain[blockIdx.z][2];
#pragma unroll 1
    for (int k = 0; k < TL_ROWS; k++) {
        const int gy = gy0 + 8 * k;
        if (gy >= b.ch) break;
        int p[TL_LPX * 3];
#pragma unroll
        for (int i = 0; i < TL_LPX * 3; i++) p[i] = 0;
        const long long ry = ry_off + gy;
        if (any_col && ry >= 0 && ry < a.dh) {
            const float v = (float)(b.cy + gy);
            float s = 0.f, c = 0.f;
            if (CLASS == TL_SEPARABLE) row_terms(a.kind, a.scale, v, a.pb, &s, &c);
            const float vp = v / a.scale;
#pragma unroll
            for (int i = 0; i < TL_LPX; i++) {
                if (!col_in[i]) continue;
                float x, y;
                if (CLASS == TL_SEPARABLE) map_backward(a.kind, a.m, su[i], cu[i], s, c, &x, &y);
                else if (CLASS == TL_POLAR) map_backward_polar(a.kind, a.m, a.scale, (float)(b.cx + gx0 + i), v, &x, &y);
                else {
                    constexpr int FAM = CLASS == TL_COMPRESSED ? MIS_WARP_COMPRESSED_PLANE_A2B1 : MIS_WARP_PANINI_A2B1;
                    float sinv, cosv;
                    col_pixel<FAM>(ct[i], a.pb, vp, &sinv, &cosv);
                    map_backward(FAM, a.m, ct[i].sl, ct[i].cl, cosv, sinv, &x, &y);
                }
                int q[3];
                sample_linear<3>(a.src, a.sstride, a.sw, a.sh, x, y, q);       // 0..255: the 16SC3 value of the fused warp
                if (b.has_gains) {      // mis_compensator_apply on a 16S value, GAIN / CHANNELS (unit_gain_kernel)
                    const int r0 = mis_round_f((float)q[0] * g0), r1 = mis_round_f((float)q[1] * g1), r2 = mis_round_f((float)q[2] * g2);
                    q[0] = r0 < 0 ? 0 : (r0 > 255 ? 255 : r0); q[1] = r1 < 0 ? 0 : (r1 > 255 ? 255 : r1); q[2] = r2 < 0 ? 0 : (r2 > 255 ? 255 : r2);
                }
                p[3 * i] = q[0]; p[3 * i + 1] = q[1]; p[3 * i + 2] = q[2];      // within 0..255 either way: saturate_cast<uchar> is the identity
            }
        }
        store_px4<U8>((uint8_t*)a.dst + (size_t)gy * a.dstride, gx0, b.cw, wide, p);
    }
}

int tl_class_of(int kind) {
    if (kind_polar(kind)) return TL_POLAR;
    if (col_kind_of(kind).family == MIS_WARP_COMPRESSED_PLANE_A2B1) return TL_COMPRESSED;
    if (col_kind_of(kind).family == MIS_WARP_PANINI_A2B1) return TL_PANINI;
    return TL_SEPARABLE;
}
template <bool U8>
void launch_batch(int cls, dim3 grid, hipStream_t stream, const TimelapseBatch& b) {
    const dim3 block(256);
    if (cls == TL_POLAR) hipLaunchKernelGGL((timelapse_warp_batch_kernel<TL_POLAR, U8>), grid, block, 0, stream, b);
    else if (cls == TL_COMPRESSED) hipLaunchKernelGGL((timelapse_warp_batch_kernel<TL_COMPRESSED, U8>), grid, block, 0, stream, b);
    else if (cls == TL_PANINI) hipLaunchKernelGGL((timelapse_warp_batch_kernel<TL_PANINI, U8>), grid, block, 0, stream, b);
    else hipLaunchKernelGGL((timelapse_warp_batch_kernel<TL_SEPARABLE, U8>), grid, block, 0, stream, b);
}

// cv::detail::resultRoiIntersection: tl = the largest corner, br = the smallest far corner (64-bit sums); *empty when they cross
int roi_intersection(const MisPoint* corners, const MisSize* sizes, int n, long long* x0, long long* y0, long long* x1, long long* y1) {
    if (!corners || !sizes || n < 1) return MIS_E_INVALID;
    *x0 = *y0 = LLONG_MIN; *x1 = *y1 = LLONG_MAX;
    for (int i = 0; i < n; i++) {
        *x0 = std::max(*x0, (long long)corners[i].x); *y0 = std::max(*y0, (long long)corners[i].y);
        *x1 = std::min(*x1, (long long)corners[i].x + sizes[i].width); *y1 = std::min(*y1, (long long)corners[i].y + sizes[i].height);
    }
    return MIS_OK;
}

// a caller's output canvas: data == NULL (the library allocates) or exactly the canvas's geometry
bool canvas_fits(const MisImage* im, int w, int h, int cn, int dtype) {
    return !im->data || (im->width == w && im->height == h && im->channels == cn && im->dtype == dtype && im->stride >= (size_t)w * cn * mis_dtype_size(dtype));
}

int warp_batch_impl(MisContext* ctx, int kind, const MisImage* srcs, int n, float scale, const float* Ks, const float* Rs, const MisRect* rois,
                    const MisRect* dst_roi, const double* gains, MisImage* dsts, int dst_format, int repeats, float* avg_us) {
    // ---- every check before anything is allocated or launched ----
    MIS_CHECK(ctx, MIS_WARP_KIND_IS_KNOWN(kind), MIS_E_UNSUPPORTED, "unknown warp kind %d", kind);
    MIS_CHECK(ctx, srcs && Ks && Rs && rois && dst_roi && dsts, MIS_E_INVALID, "timelapse_warp_batch: null argument");
    MIS_CHECK(ctx, n >= 1, MIS_E_INVALID, "timelapse_warp_batch: %d frames (at least one)", n);
    MIS_CHECK(ctx, scale > 0.f, MIS_E_INVALID, "scale must be positive");
    MIS_CHECK(ctx, dst_format == MIS_S16 || dst_format == MIS_U8, MIS_E_INVALID, "timelapse_warp_batch: output format %d (MIS_S16: 16SC3, MIS_U8: 8UC3)", dst_format);
    MIS_CHECK(ctx, dst_roi->width > 0 && dst_roi->height > 0, MIS_E_INVALID, "timelapse_warp_batch: empty dst_roi (%d, %d, %d x %d)", dst_roi->x, dst_roi->y,
              dst_roi->width, dst_roi->height);
    MIS_CHECK(ctx, (long long)dst_roi->width * dst_roi->height < (1ll << 31), MIS_E_INVALID, "timelapse_warp_batch: canvas %dx%d has too many pixels for one launch",
              dst_roi->width, dst_roi->height);
    MIS_CHECK(ctx, (long long)dst_roi->x + dst_roi->width <= INT_MAX && (long long)dst_roi->y + dst_roi->height <= INT_MAX, MIS_E_INVALID,
              "timelapse_warp_batch: dst_roi (%d, %d, %d x %d) does not fit int coordinates", dst_roi->x, dst_roi->y, dst_roi->width, dst_roi->height);
    const int cw = dst_roi->width, ch = dst_roi->height;
    for (int i = 0; i < n; i++) {
        const MisImage& s = srcs[i];
        MIS_CHECK(ctx, s.data && s.dtype == MIS_U8 && s.channels == 3, MIS_E_INVALID, "frame %d: the source must be an 8UC3 image", i);
        MIS_CHECK(ctx, s.width >= 2 && s.height >= 2 && s.width <= 32767 && s.height <= 32767, MIS_E_INVALID, "frame %d: source size %dx%d out of range", i, s.width, s.height);
        MIS_CHECK(ctx, s.stride >= (size_t)s.width * 3, MIS_E_INVALID, "frame %d: source stride smaller than a row", i);
        MIS_CHECK(ctx, rois[i].width > 0 && rois[i].height > 0, MIS_E_INVALID, "frame %d: empty roi", i);
        MIS_CHECK(ctx, (long long)rois[i].x + rois[i].width <= INT_MAX && (long long)rois[i].y + rois[i].height <= INT_MAX, MIS_E_INVALID,
                  "frame %d: roi (%d, %d, %d x %d) does not fit int coordinates", i, rois[i].x, rois[i].y, rois[i].width, rois[i].height);
        MIS_CHECK(ctx, canvas_fits(&dsts[i], cw, ch, 3, dst_format), MIS_E_INVALID, "frame %d: the output is not a %s image of the canvas's size %dx%d", i,
                  dst_format == MIS_U8 ? "8UC3" : "16SC3", cw, ch);
        if (gains)
            for (int k = 0; k < 3; k++) MIS_CHECK(ctx, std::isfinite(gains[3 * i + k]), MIS_E_INVALID, "frame %d: gain %d is not finite", i, k);
    }
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<WarpArgs> args((size_t)n);
    std::vector<DevView> din((size_t)n), dout((size_t)n);
    int rc;
    for (int i = 0; i < n; i++) {
        Projector p;
        projector_set(&p, kind, scale, Ks + 9 * i, Rs + 9 * i);
        WarpArgs& a = args[i];
        a = WarpArgs{};
        for (int k = 0; k < 9; k++) a.m[k] = p.k_rinv[k];
        a.kind = kind; a.scale = scale; a.pa = p.a; a.pb = p.b;
        if (kind == MIS_WARP_AFFINE) { a.pa = p.t[0]; a.pb = p.t[1]; }
        a.tlx = rois[i].x; a.tly = rois[i].y; a.dw = rois[i].width; a.dh = rois[i].height;
        a.sw = srcs[i].width; a.sh = srcs[i].height; a.cn = 3;
        if ((rc = din[i].read(ctx, &srcs[i])) != MIS_OK) return rc;
        if ((rc = dout[i].write(ctx, &dsts[i], cw, ch, 3, dst_format)) != MIS_OK) return rc;
        a.src = (const uint8_t*)din[i].data; a.sstride = din[i].stride;
        a.dst = dout[i].data; a.dstride = dout[i].stride;
    }
    const int cls = tl_class_of(kind);
    OwnedEvent e0, e1;
    if (avg_us) {
        MIS_HIP(ctx, e0.ready(hipEventDefault));
        MIS_HIP(ctx, e1.ready(hipEventDefault));
        MIS_HIP(ctx, hipEventRecord(e0.ev, ctx->stream));
    }
    for (int rep = 0; rep < repeats; rep++)
        for (int g0 = 0; g0 < n; g0 += WB_MAX) {
            const int ng = std::min(WB_MAX, n - g0);
            TimelapseBatch b;
            for (int k = 0; k < WB_MAX; k++) {
                const int i = g0 + (k < ng ? k : 0);
                b.a[k] = args[i];
                for (int c = 0; c < 3; c++) b.gain[k][c] = gains ? (float)gains[3 * i + c] : 1.f;
            }
            b.cx = dst_roi->x; b.cy = dst_roi->y; b.cw = cw; b.ch = ch; b.has_gains = gains ? 1 : 0;
            const dim3 grid((unsigned)((cw + TL_TW - 1) / TL_TW), (unsigned)((ch + TL_TH - 1) / TL_TH), (unsigned)ng);
            if (dst_format == MIS_U8) launch_batch<true>(cls, grid, ctx->stream, b);
            else launch_batch<false>(cls, grid, ctx->stream, b);
        }
    MIS_HIP(ctx, hipGetLastError());
    if (avg_us) {
        float ms = 0.f;
        MIS_HIP(ctx, hipEventRecord(e1.ev, ctx->stream));
        MIS_HIP(ctx, hipEventSynchronize(e1.ev));
        MIS_HIP(ctx, hipEventElapsedTime(&ms, e0.ev, e1.ev));
        *avg_us = ms * 1000.f / (float)repeats;
    }
    for (int i = 0; i < n; i++)
        if ((rc = dout[i].commit()) != MIS_OK) return rc;
    return MIS_OK;
}

}  // namespace

struct MisTimelapser {
    MisContext* ctx = nullptr;
    int type = MIS_TIMELAPSE_AS_IS;
    bool initialized = false;
    MisRect dst_roi{0, 0, 0, 0};
};

extern "C" int mis_result_roi_intersection(const MisPoint* corners, const MisSize* sizes, int n, MisRect* roi) {
    long long x0, y0, x1, y1;
    if (!roi || roi_intersection(corners, sizes, n, &x0, &y0, &x1, &y1) != MIS_OK) return MIS_E_INVALID;
    if (x1 - x0 <= 0 || y1 - y0 <= 0 || x1 - x0 > INT_MAX || y1 - y0 > INT_MAX) return MIS_E_INVALID;
    roi->x = (int)x0; roi->y = (int)y0; roi->width = (int)(x1 - x0); roi->height = (int)(y1 - y0);
    return MIS_OK;
}

extern "C" int mis_timelapser_create(MisContext* ctx, int type, MisTimelapser** out) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, out, MIS_E_INVALID, "null argument");
    MIS_CHECK(ctx, type == MIS_TIMELAPSE_AS_IS || type == MIS_TIMELAPSE_CROP, MIS_E_INVALID, "timelapser type %d: MIS_TIMELAPSE_AS_IS (0) or MIS_TIMELAPSE_CROP (1)", type);
    MisTimelapser* t = new MisTimelapser();
    t->ctx = ctx; t->type = type;
    *out = t;
    return MIS_OK;
}

extern "C" int mis_timelapser_destroy(MisTimelapser* t) {
    delete t;
    return MIS_OK;
}

extern "C" int mis_timelapser_initialize(MisTimelapser* t, const MisPoint* corners, const MisSize* sizes, int n) {
    if (!t) return MIS_E_INVALID;
    MisContext* ctx = t->ctx;
    MIS_CHECK(ctx, corners && sizes && n >= 1, MIS_E_INVALID, "timelapser initialize: null argument or no frames");
    for (int i = 0; i < n; i++) MIS_CHECK(ctx, sizes[i].width > 0 && sizes[i].height > 0, MIS_E_INVALID, "timelapser initialize: frame %d has an empty size", i);
    MisRect r;
    if (t->type == MIS_TIMELAPSE_CROP) {
        long long x0, y0, x1, y1;
        roi_intersection(corners, sizes, n, &x0, &y0, &x1, &y1);
        MIS_CHECK(ctx, x1 - x0 > 0 && y1 - y0 > 0, MIS_E_INVALID, "timelapser initialize: the frames' intersection Rect(tl = (%lld, %lld), br = (%lld, %lld)) is empty", x0, y0, x1, y1);
        MIS_CHECK(ctx, x1 - x0 <= INT_MAX && y1 - y0 <= INT_MAX, MIS_E_INVALID, "timelapser initialize: the frames' intersection does not fit an int size");
        r = {(int)x0, (int)y0, (int)(x1 - x0), (int)(y1 - y0)};
    } else {        // cv::detail::resultRoi: mis_result_roi's rectangle, its corner sums in 64 bits
        long long x0 = LLONG_MAX, y0 = LLONG_MAX, x1 = LLONG_MIN, y1 = LLONG_MIN;
        for (int i = 0; i < n; i++) {
            x0 = std::min(x0, (long long)corners[i].x); y0 = std::min(y0, (long long)corners[i].y);
            x1 = std::max(x1, (long long)corners[i].x + sizes[i].width); y1 = std::max(y1, (long long)corners[i].y + sizes[i].height);
        }
        MIS_CHECK(ctx, x1 - x0 <= INT_MAX && y1 - y0 <= INT_MAX, MIS_E_INVALID, "timelapser initialize: the frames' union does not fit an int size");
        r = {(int)x0, (int)y0, (int)(x1 - x0), (int)(y1 - y0)};
    }
    MIS_CHECK(ctx, (long long)r.width * r.height < (1ll << 31), MIS_E_INVALID, "timelapser initialize: canvas %dx%d has too many pixels for one launch", r.width, r.height);
    t->dst_roi = r;
    t->initialized = true;
    return MIS_OK;
}

extern "C" int mis_timelapser_dst_roi(const MisTimelapser* t, MisRect* roi) {
    if (!t) return MIS_E_INVALID;
    MIS_CHECK(t->ctx, roi, MIS_E_INVALID, "null argument");
    MIS_CHECK(t->ctx, t->initialized, MIS_E_STATE, "timelapser: dst_roi before initialize");
    *roi = t->dst_roi;
    return MIS_OK;
}

extern "C" int mis_timelapser_process(MisTimelapser* t, const MisImage* img, MisPoint tl, MisImage* dst) {
    if (!t) return MIS_E_INVALID;
    MisContext* ctx = t->ctx;
    MIS_CHECK(ctx, t->initialized, MIS_E_STATE, "timelapser: process before initialize");
    MIS_CHECK(ctx, img && dst, MIS_E_INVALID, "null argument");
    MIS_CHECK(ctx, img->data && img->dtype == MIS_S16 && img->channels == 3 && img->width > 0 && img->height > 0, MIS_E_INVALID, "timelapser process: the image must be 16SC3");
    MIS_CHECK(ctx, img->stride >= (size_t)img->width * 6 && img->stride % 2 == 0 && (uintptr_t)img->data % 2 == 0, MIS_E_INVALID,
              "timelapser process: image rows must be 2-byte aligned and at least a row long");
    const int cw = t->dst_roi.width, ch = t->dst_roi.height;
    MIS_CHECK(ctx, canvas_fits(dst, cw, ch, 3, MIS_S16), MIS_E_INVALID, "timelapser process: the output is not a 16SC3 image of the canvas's size %dx%d", cw, ch);
    MIS_CHECK(ctx, !dst->data || (dst->stride % 2 == 0 && (uintptr_t)dst->data % 2 == 0), MIS_E_INVALID, "timelapser process: output rows must be 2-byte aligned");
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    DevView din, dout;
    int rc;
    if ((rc = din.read(ctx, img)) != MIS_OK) return rc;
    if ((rc = dout.write(ctx, dst, cw, ch, 3, MIS_S16)) != MIS_OK) return rc;
    PlaceArgs a;
    a.src = (const uint8_t*)din.data; a.sstride = din.stride; a.sw = img->width; a.sh = img->height;
    a.dst = (uint8_t*)dout.data; a.dstride = dout.stride; a.cw = cw; a.ch = ch;
    a.dx = (long long)tl.x - t->dst_roi.x; a.dy = (long long)tl.y - t->dst_roi.y;
    hipLaunchKernelGGL(timelapse_place_kernel, dim3((unsigned)((cw + TL_TW - 1) / TL_TW), (unsigned)((ch + TL_TH - 1) / TL_TH)), dim3(256), 0, ctx->stream, a);
    MIS_HIP(ctx, hipGetLastError());
    return dout.commit();
}

extern "C" int mis_timelapse_warp_batch(MisContext* ctx, int kind, const MisImage* srcs, int n, float scale, const float* Ks, const float* Rs, const MisRect* rois,
                                        const MisRect* dst_roi, const double* gains, MisImage* dsts, int dst_format) {
    if (!ctx) return MIS_E_INVALID;
    return warp_batch_impl(ctx, kind, srcs, n, scale, Ks, Rs, rois, dst_roi, gains, dsts, dst_format, 1, nullptr);
}

extern "C" int mis_timelapse_warp_batch_timed(MisContext* ctx, int kind, const MisImage* srcs, int n, float scale, const float* Ks, const float* Rs, const MisRect* rois,
                                              const MisRect* dst_roi, const double* gains, MisImage* dsts, int dst_format, int repeats, float* avg_us) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, repeats >= 1 && avg_us, MIS_E_INVALID, "repeats must be >= 1 and avg_us non-null");
    return warp_batch_impl(ctx, kind, srcs, n, scale, Ks, Rs, rois, dst_roi, gains, dsts, dst_format, repeats, avg_us);
}
