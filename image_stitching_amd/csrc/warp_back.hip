// warp_back.hip -- the other half of cv::detail::RotationWarper: warpPoint / warpPointBackward
// (mis_warper_warp_points), buildMaps (mis_warper_build_maps) and warpBackward (mis_warper_warp_backward, _batch).
// Nothing here is new arithmetic: mapForward is map_forward of warp_shared.h (the function the rois are computed with), mapBackward the
// operation sequences the warp kernels evaluate in registers (col_terms / row_terms / map_backward, map_backward_polar, col_hoist /
// col_pixel), the 8-bit remap the samplers of the warp kernels.  What this unit adds is the walk over points, over a roi (two float
// planes out) and over a pinhole view (forward map per output pixel, gather from the warped source).
#include "warp_points_host.h"

namespace {

// one point per lane, either direction
constexpr int WARP_POINTS_MAX = 1 << 27;    // per call with a context: 2 GB of staging
__global__ __launch_bounds__(256) void warp_points_kernel(PointMap p, int backward, const float2* __restrict__ in, float2* __restrict__ out, int n) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= n) return;
    const float2 q = in[i];
    float2 r;
    warp_point(p, backward, q.x, q.y, &r.x, &r.y);
    out[i] = r;
}

// ---- buildMaps: the backward map of every roi pixel into two float planes ----
// A lane owns BK_LPX = 4 consecutive columns (one 16-byte store per plane and row where the planes' rows are 16-byte aligned, single
// floats otherwise and at the roi's right edge), 32 lanes a tile row of 128 columns = one whole 512-byte run per plane.  A tile is 128 x
// MP_TH = 32 rows; a lane evaluates what depends on its columns alone once (the separable kinds' {su, cu}, the half-separable kinds'
// ColTerms) and walks rows (thread >> 5) + 8 k, as col_tile does.  The polar kinds hoist nothing.
// WarpArgs: m = k_rinv, tlx / tly / dw / dh = the roi, pa / pb = (A, B) or the affine (t0, t1), dst / dstride = xmap, mask / mstride = ymap.
constexpr int BK_LPX = 4, BK_TW = 32 * BK_LPX, BK_TH = 8;
constexpr int MP_ROWS = 4, MP_TH = 8 * MP_ROWS;
enum { MAPS_SEPARABLE = 0, MAPS_POLAR = 1, MAPS_COMPRESSED = 2, MAPS_PANINI = 3 };
static long long maps_tiles_of(const WarpArgs& a) { return (long long)((a.dw + BK_TW - 1) / BK_TW) * ((a.dh + MP_TH - 1) / MP_TH); }

template <int CLASS>
__global__ __launch_bounds__(256) void warp_maps_kernel(WarpArgs a) {
    const int tile = (int)blockIdx.x;
    const int tiles_x = (a.dw + BK_TW - 1) / BK_TW;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int gx0 = tx * BK_TW + ((int)threadIdx.x & 31) * BK_LPX, gy0 = ty * MP_TH + ((int)threadIdx.x >> 5);
    if (gx0 >= a.dw || gy0 >= a.dh) return;
    const bool wide = ((((uintptr_t)a.dst | a.dstride | (uintptr_t)a.mask | a.mstride) & 15) == 0) && gx0 + BK_LPX <= a.dw;    // (gx0 * 4 bytes = 16 k)
    float su[BK_LPX], cu[BK_LPX];
    ColTerms ct[BK_LPX];
#pragma unroll
    for (int i = 0; i < BK_LPX; i++) {      // (columns past the roi are computed and not stored)
        const float u = (float)(a.tlx + gx0 + i);
        if (CLASS == MAPS_SEPARABLE) col_terms(a.kind, a.scale, u, a.pa, &su[i], &cu[i]);
        else if (CLASS == MAPS_COMPRESSED) ct[i] = col_hoist<MIS_WARP_COMPRESSED_PLANE_A2B1>(a.scale, a.pa, a.pb, u);
        else if (CLASS == MAPS_PANINI) ct[i] = col_hoist<MIS_WARP_PANINI_A2B1>(a.scale, a.pa, a.pb, u);
    }
#pragma unroll 1
    for (int k = 0; k < MP_ROWS; k++) {
        const int gy = gy0 + 8 * k;
        if (gy >= a.dh) break;
        const float v = (float)(a.tly + gy);
        float x[BK_LPX], y[BK_LPX];
        if (CLASS == MAPS_SEPARABLE) {
            float s, c;
            row_terms(a.kind, a.scale, v, a.pb, &s, &c);
#pragma unroll
            for (int i = 0; i < BK_LPX; i++) map_backward(a.kind, a.m, su[i], cu[i], s, c, &x[i], &y[i]);
        } else if (CLASS == MAPS_POLAR) {
#pragma unroll
            for (int i = 0; i < BK_LPX; i++) map_backward_polar(a.kind, a.m, a.scale, (float)(a.tlx + gx0 + i), v, &x[i], &y[i]);
        } else {
            constexpr int FAM = CLASS == MAPS_COMPRESSED ? MIS_WARP_COMPRESSED_PLANE_A2B1 : MIS_WARP_PANINI_A2B1;
            const float vp = v / a.scale;
#pragma unroll
            for (int i = 0; i < BK_LPX; i++) {
                float sinv, cosv;
                col_pixel<FAM>(ct[i], a.pb, vp, &sinv, &cosv);
                map_backward(FAM, a.m, ct[i].sl, ct[i].cl, cosv, sinv, &x[i], &y[i]);
            }
        }
        float* xr = (float*)((uint8_t*)a.dst + (size_t)gy * a.dstride) + gx0;
        float* yr = (float*)(a.mask + (size_t)gy * a.mstride) + gx0;
        if (wide) {
            *reinterpret_cast<float4*>(xr) = make_float4(x[0], x[1], x[2], x[3]);
            *reinterpret_cast<float4*>(yr) = make_float4(y[0], y[1], y[2], y[3]);
        } else {
            for (int i = 0; i < BK_LPX && gx0 + i < a.dw; i++) { xr[i] = x[i]; yr[i] = y[i]; }
        }
    }
}

// ---- warpBackward: a pinhole view rendered out of a warped image ----
// remap INTER_LINEAR, BORDER_CONSTANT(0) on u8: sample_linear's quantisation and weights; a tap outside the source contributes 0
template <int CN>
__device__ __forceinline__ void sample_linear_constant(const uint8_t* src, size_t stride, int sw, int sh, float x, float y, int* out) {
    int sxq = mis_round_sat_f(x * 32.f), syq = mis_round_sat_f(y * 32.f);
    int fx = sxq & 31, fy = syq & 31;
    int sx = mis_sat_short(sxq >> 5), sy = mis_sat_short(syq >> 5);
    const bool x0in = (unsigned)sx < (unsigned)sw, x1in = (unsigned)(sx + 1) < (unsigned)sw;
    const bool y0in = (unsigned)sy < (unsigned)sh, y1in = (unsigned)(sy + 1) < (unsigned)sh;
    // a tap that is outside takes weight 0 and reads pixel / row 0 instead (always a valid address)
    const int x0 = x0in ? sx : 0, x1 = x1in ? sx + 1 : 0, y0 = y0in ? sy : 0, y1 = y1in ? sy + 1 : 0;
    int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
    if (!(x0in && y0in)) w00 = 0;
    if (!(x1in && y0in)) w01 = 0;
    if (!(x0in && y1in)) w10 = 0;
    if (!(x1in && y1in)) w11 = 0;
    const uint8_t* r0 = src + (size_t)y0 * stride;
    const uint8_t* r1 = src + (size_t)y1 * stride;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        int s = r0[x0 * CN + c] * w00 + r0[x1 * CN + c] * w01 + r1[x0 * CN + c] * w10 + r1[x1 * CN + c] * w11;
        out[c] = (s + (1 << 14)) >> 15;  // always within 0..255
    }
}

enum { BACK_LINEAR_REFLECT = 0, BACK_NEAREST_CONSTANT = 1, BACK_LINEAR_CONSTANT = 2 };

// The forward map does not split by row and column (atan2, acos or asin, a square root, tan / log / sincos by kind), so this is the
// polar kernels' regime: issue bound, no tables, no LDS, the taps gathered from global memory through L2.  polar_fused_tile's walk: a
// lane owns BK_LPX = 4 consecutive pixels of one row -- 8UC3: 12 bytes = three whole dwords, 8UC1 and the mask: one dword each where
// the rows are 4-byte aligned; bytes otherwise and at the view's right edge --, 32 lanes a tile row, the four waves of a workgroup the 8
// rows of a 128 x 8 tile; tiles are numbered row-major over the view.
// WarpArgs: m = r_kinv, tlx / tly = the source's top-left in the warper's plane, dw / dh = the view, sw / sh = the source, pa / pb =
// (A, B); mask may be null.  KIND: the kind, for kinds 8 .. 11 the family's A2B1 kind.
// xmap = u - tl.x, ymap = v - tl.y in float32, as RotationWarperBase::warpBackward fills its maps.
template <int KIND, int CN, int MODE>
__device__ __forceinline__ void warp_back_tile(const WarpArgs& a, int tile) {
    const int tiles_x = (a.dw + BK_TW - 1) / BK_TW;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int gx0 = tx * BK_TW + ((int)threadIdx.x & 31) * BK_LPX, gy = ty * BK_TH + ((int)threadIdx.x >> 5);
    if (gx0 >= a.dw || gy >= a.dh) return;
    const float tlx = (float)a.tlx, tly = (float)a.tly, yv = (float)gy;
    uint8_t px[BK_LPX * CN], mk[BK_LPX];
#pragma unroll
    for (int i = 0; i < BK_LPX; i++) {      // (columns past the view are computed and not stored)
        float u, v;
        map_forward(KIND, a.m, a.scale, (float)(gx0 + i), yv, &u, &v, a.pa, a.pb);
        const float x = u - tlx, y = v - tly;
        int sx, sy;
        const bool in = nearest_inside(a.sw, a.sh, x, y, &sx, &sy);
        if (MODE == BACK_NEAREST_CONSTANT) {
#pragma unroll
            for (int c = 0; c < CN; c++) px[CN * i + c] = in ? a.src[(size_t)sy * a.sstride + (size_t)sx * CN + c] : (uint8_t)0;
        } else {
            int p[CN];
            if (MODE == BACK_LINEAR_REFLECT) sample_linear<CN>(a.src, a.sstride, a.sw, a.sh, x, y, p);
            else sample_linear_constant<CN>(a.src, a.sstride, a.sw, a.sh, x, y, p);
#pragma unroll
            for (int c = 0; c < CN; c++) px[CN * i + c] = (uint8_t)p[c];
        }
        mk[i] = in ? 255 : 0;
    }
    uint8_t* drow = (uint8_t*)a.dst + (size_t)gy * a.dstride + (size_t)gx0 * CN;     // gx0 * CN = 4 k (CN = 1) or 12 k
    const bool whole = gx0 + BK_LPX <= a.dw;
    if (whole && (((uintptr_t)a.dst | a.dstride) & 3) == 0) {
        uint32_t* d = (uint32_t*)drow;
#pragma unroll
        for (int k = 0; k < CN; k++)
            d[k] = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int i = 0; i < BK_LPX * CN && gx0 * CN + i < a.dw * CN; i++) drow[i] = px[i];
    }
    if (a.mask) {
        uint8_t* mrow = a.mask + (size_t)gy * a.mstride + gx0;
        if (whole && (((uintptr_t)a.mask | a.mstride) & 3) == 0)
            *(uint32_t*)mrow = (uint32_t)mk[0] | ((uint32_t)mk[1] << 8) | ((uint32_t)mk[2] << 16) | ((uint32_t)mk[3] << 24);
        else
            for (int i = 0; i < BK_LPX && gx0 + i < a.dw; i++) mrow[i] = mk[i];
    }
}
static long long back_tiles(int w, int h) { return (long long)((w + BK_TW - 1) / BK_TW) * ((h + BK_TH - 1) / BK_TH); }
static long long back_tiles_of(const WarpArgs& a) { return back_tiles(a.dw, a.dh); }

template <int KIND, int CN, int MODE>
__global__ __launch_bounds__(256) void warp_back_kernel(WarpArgs a) {
    warp_back_tile<KIND, CN, MODE>(a, (int)blockIdx.x);
}

// n views out of one source: the tiles of all views, view after view, in one one-dimensional grid (PolarBatch's layout)
struct BackBatch {
    WarpArgs a[WB_MAX];
    int wg_base[WB_MAX + 1];    // view k owns workgroups wg_base[k] .. wg_base[k + 1] - 1; views past the batch own none
};
template <int KIND, int CN, int MODE>
__global__ __launch_bounds__(256) void warp_back_batch_kernel(BackBatch b) {
    const int bid = (int)blockIdx.x;
    int fi = 0;
#pragma unroll
    for (int k = 1; k < WB_MAX; k++) fi += bid >= b.wg_base[k] ? 1 : 0;       // (uniform: scalar compares on the kernel arguments)
    warp_back_tile<KIND, CN, MODE>(b.a[fi], bid - b.wg_base[fi]);
}

// run-time (kind, channels, mode) -> the instantiation (kinds 8 .. 11 by family; kind 13 never gets here)
template <class F> void with_back_kind(int kind, F&& launch) {
    switch (kind) {
        case MIS_WARP_SPHERICAL: launch(int_c<MIS_WARP_SPHERICAL>{}); break;
        case MIS_WARP_CYLINDRICAL: launch(int_c<MIS_WARP_CYLINDRICAL>{}); break;
        case MIS_WARP_PLANE: launch(int_c<MIS_WARP_PLANE>{}); break;
        case MIS_WARP_MERCATOR: launch(int_c<MIS_WARP_MERCATOR>{}); break;
        case MIS_WARP_FISHEYE: launch(int_c<MIS_WARP_FISHEYE>{}); break;
        case MIS_WARP_STEREOGRAPHIC: launch(int_c<MIS_WARP_STEREOGRAPHIC>{}); break;
        default: with_col_kind(kind, launch);
    }
}
template <class F> void with_back_cn_mode(int cn, int mode, F&& launch) {
    if (cn == 3) {
        if (mode == BACK_LINEAR_REFLECT) launch(int_c<3>{}, int_c<BACK_LINEAR_REFLECT>{});
        else if (mode == BACK_NEAREST_CONSTANT) launch(int_c<3>{}, int_c<BACK_NEAREST_CONSTANT>{});
        else launch(int_c<3>{}, int_c<BACK_LINEAR_CONSTANT>{});
    } else {
        if (mode == BACK_LINEAR_REFLECT) launch(int_c<1>{}, int_c<BACK_LINEAR_REFLECT>{});
        else if (mode == BACK_NEAREST_CONSTANT) launch(int_c<1>{}, int_c<BACK_NEAREST_CONSTANT>{});
        else launch(int_c<1>{}, int_c<BACK_LINEAR_CONSTANT>{});
    }
}

// (interp, border) -> BACK_*; -1: not one of the three pairs
int back_mode_of(int interp, int border) {
    if (interp == MIS_INTER_LINEAR && border == MIS_BORDER_REFLECT) return BACK_LINEAR_REFLECT;
    if (interp == MIS_INTER_NEAREST && border == MIS_BORDER_CONSTANT) return BACK_NEAREST_CONSTANT;
    if (interp == MIS_INTER_LINEAR && border == MIS_BORDER_CONSTANT) return BACK_LINEAR_CONSTANT;
    return -1;
}

// What every view of a warpBackward call shares, checked before anything is launched or allocated.  `who`: "" or "view k: ".
int back_check_common(MisContext* ctx, int kind, const MisImage* src, float scale, int interp, int border, int* mode) {
    MIS_CHECK(ctx, MIS_WARP_KIND_IS_KNOWN(kind), MIS_E_UNSUPPORTED, "unknown warp kind %d", kind);
    MIS_CHECK(ctx, kind != MIS_WARP_AFFINE, MIS_E_UNSUPPORTED, "warp_backward: AffineWarper (kind %d) has no warpBackward of its own", kind);
    MIS_CHECK(ctx, src, MIS_E_INVALID, "null argument");
    MIS_CHECK(ctx, src->data, MIS_E_INVALID, "warp_backward: the source has no data");
    MIS_CHECK(ctx, src->dtype == MIS_U8 && (src->channels == 1 || src->channels == 3), MIS_E_UNSUPPORTED, "warp_backward source must be 8UC1 or 8UC3");
    MIS_CHECK(ctx, src->width >= 2 && src->height >= 2 && src->width <= 32767 && src->height <= 32767, MIS_E_INVALID,
              "source size %dx%d out of range", src->width, src->height);
    MIS_CHECK(ctx, scale > 0.f, MIS_E_INVALID, "scale must be positive");
    *mode = back_mode_of(interp, border);
    MIS_CHECK(ctx, *mode >= 0, MIS_E_UNSUPPORTED, "supported: (LINEAR, REFLECT), (NEAREST, CONSTANT) and (LINEAR, CONSTANT)");
    return MIS_OK;
}
// one view's outputs as the caller describes them: a buffer of the view's geometry, or data == NULL (the library allocates)
int back_check_view(MisContext* ctx, const char* who, int cn, int w, int h, const MisImage* dst, const MisImage* mask) {
    MIS_CHECK(ctx, w > 0 && h > 0, MIS_E_INVALID, "%sview size %dx%d must be positive", who, w, h);
    MIS_CHECK(ctx, (long long)w * h < (1ll << 31), MIS_E_INVALID, "%sview size %dx%d: too many pixels for one launch", who, w, h);
    MIS_CHECK(ctx, dst, MIS_E_INVALID, "%snull output image", who);
    auto fits = [&](const MisImage* im, int c) {
        return !im->data || (im->width == w && im->height == h && im->channels == c && im->dtype == MIS_U8 && im->stride >= (size_t)w * c);
    };
    MIS_CHECK(ctx, fits(dst, cn), MIS_E_INVALID, "%sthe output image is not 8U, %dx%d with %d channel(s)", who, w, h, cn);
    MIS_CHECK(ctx, !mask || fits(mask, 1), MIS_E_INVALID, "%sthe output mask is not 8UC1 of %dx%d", who, w, h);
    return MIS_OK;
}
void back_args_of(const Projector& p, const MisImage* src, MisPoint src_tl, int w, int h, WarpArgs* a) {
    for (int i = 0; i < 9; i++) a->m[i] = p.r_kinv[i];
    a->scale = p.scale; a->kind = p.kind; a->pa = p.a; a->pb = p.b;
    a->tlx = src_tl.x; a->tly = src_tl.y; a->dw = w; a->dh = h;
    a->sw = src->width; a->sh = src->height; a->cn = src->channels;
}

}  // namespace

extern "C" int mis_warper_warp_points(MisContext* ctx, int kind, float scale, const float K[9], const float R[9], int direction,
                                      const float* xy_in, float* xy_out, int n) {
    if (!MIS_WARP_KIND_IS_KNOWN(kind)) return ctx ? mis_set_error(ctx, MIS_E_UNSUPPORTED, "unknown warp kind %d", kind) : MIS_E_UNSUPPORTED;
    if (!K || !R || !(scale > 0.f) || n < 0 || (direction != MIS_MAP_FORWARD && direction != MIS_MAP_BACKWARD))
        return ctx ? mis_set_error(ctx, MIS_E_INVALID, "warp_points: null matrix, non-positive scale, negative count or unknown direction") : MIS_E_INVALID;
    if (n == 0) return MIS_OK;
    if (!xy_in || !xy_out) return ctx ? mis_set_error(ctx, MIS_E_INVALID, "null argument") : MIS_E_INVALID;
    // the device path stages 16 bytes per point and numbers its lanes in an int
    if (ctx) MIS_CHECK(ctx, n <= WARP_POINTS_MAX, MIS_E_INVALID, "warp_points: %d points in one call (at most %d with a context)", n, WARP_POINTS_MAX);
    Projector p;
    projector_set(&p, kind, scale, K, R);
    const PointMap pm = point_map_of(p);
    const int backward = direction == MIS_MAP_BACKWARD;
    if (!ctx) {
        warp_points_host(pm, backward, xy_in, xy_out, n);
        return MIS_OK;
    }
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = sizeof(float2) * (size_t)n;
    float2* d = nullptr;
    int rc;
    if ((rc = mis_dev_stage(ctx, 2 * bytes, (void**)&d)) != MIS_OK) return rc;
    MIS_HIP(ctx, hipMemcpyAsync(d, xy_in, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(warp_points_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, ctx->stream, pm, backward, (const float2*)d, d + n, n);
    MIS_HIP(ctx, hipGetLastError());
    MIS_HIP(ctx, hipMemcpyAsync(xy_out, d + n, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MIS_OK;
}

extern "C" int mis_warper_build_maps(MisContext* ctx, int kind, float scale, int src_w, int src_h, const float K[9], const float R[9],
                                     const MisRect* roi_or_null, MisImage* xmap, MisImage* ymap, MisRect* roi_out) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, MIS_WARP_KIND_IS_KNOWN(kind), MIS_E_UNSUPPORTED, "unknown warp kind %d", kind);
    MIS_CHECK(ctx, K && R && xmap && ymap, MIS_E_INVALID, "null argument");
    MIS_CHECK(ctx, src_w >= 1 && src_h >= 1 && src_w <= 32767 && src_h <= 32767, MIS_E_INVALID, "source size %dx%d out of range", src_w, src_h);
    MIS_CHECK(ctx, scale > 0.f, MIS_E_INVALID, "scale must be positive");
    MIS_CHECK(ctx, !roi_or_null || (roi_or_null->width > 0 && roi_or_null->height > 0), MIS_E_INVALID, "empty roi");
    MisRect r;
    int rc;
    if (roi_or_null) r = *roi_or_null;       // the roi mis_warper_roi gave for these parameters: nothing is scanned again
    else if (MIS_WARP_ROI_IS_FULL_SCAN(kind)) {
        if ((rc = mis_warper_roi_batch(ctx, kind, scale, src_w, src_h, 1, K, R, &r)) != MIS_OK) return rc;
    } else {
        MIS_CHECK(ctx, mis_warper_roi(kind, scale, src_w, src_h, K, R, &r) == MIS_OK, MIS_E_INVALID, "build_maps: the warp roi is refused (mis_warper_roi)");
    }
    MIS_CHECK(ctx, (long long)r.width * r.height < (1ll << 31), MIS_E_INVALID, "warp roi %dx%d: too many pixels for one launch", r.width, r.height);
    auto fits = [&](const MisImage* im) {
        return !im->data || (im->width == r.width && im->height == r.height && im->channels == 1 && im->dtype == MIS_F32 && im->stride >= sizeof(float) * (size_t)r.width &&
                             im->stride % 4 == 0 && (uintptr_t)im->data % 4 == 0);
    };
    MIS_CHECK(ctx, fits(xmap) && fits(ymap), MIS_E_INVALID, "build_maps: the maps must be 1-channel F32 images of the roi's size %dx%d with 4-byte aligned rows", r.width, r.height);
    Projector p;
    projector_set(&p, kind, scale, K, R);
    WarpArgs a = {};
    for (int i = 0; i < 9; i++) a.m[i] = p.k_rinv[i];
    a.kind = kind; a.scale = scale; a.pa = p.a; a.pb = p.b;
    if (kind == MIS_WARP_AFFINE) { a.pa = p.t[0]; a.pb = p.t[1]; }
    a.tlx = r.x; a.tly = r.y; a.dw = r.width; a.dh = r.height; a.sw = src_w; a.sh = src_h; a.cn = 1;
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    DevView dx, dy;
    if ((rc = dx.write(ctx, xmap, a.dw, a.dh, 1, MIS_F32)) != MIS_OK) return rc;
    if ((rc = dy.write(ctx, ymap, a.dw, a.dh, 1, MIS_F32)) != MIS_OK) return rc;
    MIS_CHECK(ctx, dx.stride % 4 == 0 && dy.stride % 4 == 0, MIS_E_INVALID, "build_maps: map rows must be 4-byte aligned");
    a.dst = dx.data; a.dstride = dx.stride; a.mask = (uint8_t*)dy.data; a.mstride = dy.stride;
    const dim3 grid((unsigned)maps_tiles_of(a)), block(256);
    if (kind_polar(kind)) hipLaunchKernelGGL(warp_maps_kernel<MAPS_POLAR>, grid, block, 0, ctx->stream, a);
    else if (col_kind_of(kind).family == MIS_WARP_COMPRESSED_PLANE_A2B1) hipLaunchKernelGGL(warp_maps_kernel<MAPS_COMPRESSED>, grid, block, 0, ctx->stream, a);
    else if (col_kind_of(kind).family == MIS_WARP_PANINI_A2B1) hipLaunchKernelGGL(warp_maps_kernel<MAPS_PANINI>, grid, block, 0, ctx->stream, a);
    else hipLaunchKernelGGL(warp_maps_kernel<MAPS_SEPARABLE>, grid, block, 0, ctx->stream, a);
    MIS_HIP(ctx, hipGetLastError());
    if ((rc = dx.commit()) != MIS_OK || (rc = dy.commit()) != MIS_OK) return rc;
    if (roi_out) *roi_out = r;
    return MIS_OK;
}

extern "C" int mis_warper_warp_backward(MisContext* ctx, int kind, const MisImage* src, MisPoint src_tl, float scale, const float K[9], const float R[9],
                                        int interp, int border, int dst_w, int dst_h, MisImage* dst, MisImage* dst_mask) {
    if (!ctx) return MIS_E_INVALID;
    int mode, rc;
    if ((rc = back_check_common(ctx, kind, src, scale, interp, border, &mode)) != MIS_OK) return rc;
    MIS_CHECK(ctx, K && R, MIS_E_INVALID, "null argument");
    if ((rc = back_check_view(ctx, "", src->channels, dst_w, dst_h, dst, dst_mask)) != MIS_OK) return rc;
    Projector p;
    projector_set(&p, kind, scale, K, R);
    WarpArgs a = {};
    back_args_of(p, src, src_tl, dst_w, dst_h, &a);
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    DevView din, dout, dm;
    if ((rc = din.read(ctx, src)) != MIS_OK) return rc;
    if ((rc = dout.write(ctx, dst, dst_w, dst_h, src->channels, MIS_U8)) != MIS_OK) return rc;
    if (dst_mask && (rc = dm.write(ctx, dst_mask, dst_w, dst_h, 1, MIS_U8)) != MIS_OK) return rc;
    a.src = (const uint8_t*)din.data; a.sstride = din.stride;
    a.dst = dout.data; a.dstride = dout.stride;
    a.mask = dst_mask ? (uint8_t*)dm.data : nullptr; a.mstride = dst_mask ? dm.stride : 0;
    const dim3 grid((unsigned)back_tiles_of(a)), block(256);
    with_back_kind(kind, [&](auto k) {
        with_back_cn_mode(src->channels, mode, [&](auto cn, auto m) {
            hipLaunchKernelGGL((warp_back_kernel<k.value, cn.value, m.value>), grid, block, 0, ctx->stream, a);
        });
    });
    MIS_HIP(ctx, hipGetLastError());
    if ((rc = dout.commit()) != MIS_OK) return rc;
    if (dst_mask && (rc = dm.commit()) != MIS_OK) return rc;
    return MIS_OK;
}

extern "C" int mis_warper_warp_backward_batch(MisContext* ctx, int kind, const MisImage* src, MisPoint src_tl, float scale, int n, const float* Ks, const float* Rs,
                                              const MisSize* dst_sizes, int interp, int border, MisImage* dsts, MisImage* masks) {
    if (!ctx) return MIS_E_INVALID;
    int mode, rc;
    if ((rc = back_check_common(ctx, kind, src, scale, interp, border, &mode)) != MIS_OK) return rc;
    MIS_CHECK(ctx, n >= 0, MIS_E_INVALID, "negative view count %d", n);
    if (n == 0) return MIS_OK;
    MIS_CHECK(ctx, Ks && Rs && dst_sizes && dsts, MIS_E_INVALID, "null argument");
    // every view is checked before the first output is touched
    long long group_tiles = 0;      // of the grid view i belongs to (WB_MAX views per grid)
    for (int i = 0; i < n; i++) {
        char who[32];
        snprintf(who, sizeof(who), "view %d: ", i);
        if ((rc = back_check_view(ctx, who, src->channels, dst_sizes[i].width, dst_sizes[i].height, &dsts[i], masks ? &masks[i] : nullptr)) != MIS_OK) return rc;
        group_tiles = (i % WB_MAX ? group_tiles : 0) + back_tiles(dst_sizes[i].width, dst_sizes[i].height);
        MIS_CHECK(ctx, group_tiles <= INT_MAX, MIS_E_INVALID, "%sviews %d..%d have too many tiles for one launch", who, i - i % WB_MAX, i);
    }
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    DevView din;
    if ((rc = din.read(ctx, src)) != MIS_OK) return rc;
    std::vector<WarpArgs> args((size_t)n);
    std::vector<DevView> dout((size_t)n), dm((size_t)n);
    for (int i = 0; i < n; i++) {
        Projector p;
        projector_set(&p, kind, scale, Ks + 9 * i, Rs + 9 * i);
        WarpArgs& a = args[i];
        a = WarpArgs{};
        back_args_of(p, src, src_tl, dst_sizes[i].width, dst_sizes[i].height, &a);
        if ((rc = dout[i].write(ctx, &dsts[i], a.dw, a.dh, src->channels, MIS_U8)) != MIS_OK) return rc;
        if (masks && (rc = dm[i].write(ctx, &masks[i], a.dw, a.dh, 1, MIS_U8)) != MIS_OK) return rc;
        a.src = (const uint8_t*)din.data; a.sstride = din.stride;
        a.dst = dout[i].data; a.dstride = dout[i].stride;
        a.mask = masks ? (uint8_t*)dm[i].data : nullptr; a.mstride = masks ? dm[i].stride : 0;
    }
    for (int g0 = 0; g0 < n; g0 += WB_MAX) {
        const int ng = std::min(WB_MAX, n - g0);
        BackBatch b;
        long long wg = 0;       // <= INT_MAX (checked with the views)
        for (int k = 0; k < WB_MAX; k++) {
            b.a[k] = args[g0 + (k < ng ? k : 0)];
            b.wg_base[k] = (int)wg;
            if (k < ng) wg += back_tiles_of(args[g0 + k]);
        }
        b.wg_base[WB_MAX] = (int)wg;
        with_back_kind(kind, [&](auto k) {
            with_back_cn_mode(src->channels, mode, [&](auto cn, auto m) {
                hipLaunchKernelGGL((warp_back_batch_kernel<k.value, cn.value, m.value>), dim3((unsigned)wg), dim3(256), 0, ctx->stream, b);
            });
        });
        MIS_HIP(ctx, hipGetLastError());
    }
    for (int i = 0; i < n; i++) {
        if ((rc = dout[i].commit()) != MIS_OK) return rc;
        if (masks && (rc = dm[i].commit()) != MIS_OK) return rc;
    }
    return MIS_OK;
}
