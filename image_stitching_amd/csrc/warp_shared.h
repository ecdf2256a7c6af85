// warp_shared.h -- the pieces warp.hip and warp_back.hip share: the projector (ProjectorBase::setCameraParams), mapForward of every
// kind, detectResultRoi, the kernel argument block, the backward maps of the separable, polar and half-separable kinds, the 8-bit remap
// samplers and the run-time kind -> template instantiation helpers.  Everything lives in the including unit's anonymous namespace.
#pragma once
#include "common.h"
#include "dev_math.h"
#include <algorithm>
#include <cfloat>
#include <climits>
#include <type_traits>
#include <vector>

namespace {

struct Projector {
    float scale;
    float k[9], rinv[9], r_kinv[9], k_rinv[9];
    int kind;   // MIS_WARP_*
    float a, b; // the (A, B) of a compressed-plane / Panini kind (col_kind_of), else 0
    float t[3]; // PlaneProjector::t of the affine kind (affine_rt), else 0
};

// the kinds on the plane projector: the four-corner roi, the divide by z whatever its sign
MIS_HD bool kind_planar(int kind) { return kind == MIS_WARP_PLANE || kind == MIS_WARP_AFFINE; }

// AffineWarper::getRTfromHomogeneous (stitching/src/warpers.cpp): T0 = (H02, H12, 0); R = H without those two, transposed;
// T = (R T0) * -1.  The float matrix product as projector_set's: double products and sums, one rounding to float.  T[2] is +-0.
static void affine_rt(const float H[9], float R[9], float T[3]) {
    const float t0[3] = {H[2], H[5], 0.f};
    float r[9];
    for (int i = 0; i < 9; i++) r[i] = H[i];
    r[2] = 0.f; r[5] = 0.f;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[i * 3 + j] = r[j * 3 + i];
    for (int i = 0; i < 3; i++) {
        double s = 0;
        for (int k = 0; k < 3; k++) s += (double)R[i * 3 + k] * (double)t0[k];
        T[i] = (float)s * -1.f;
    }
}

// the kinds whose backward map is evaluated per output pixel (no column / row tables)
static bool kind_polar(int kind) { return kind == MIS_WARP_FISHEYE || kind == MIS_WARP_STEREOGRAPHIC; }

// The half-separable kinds: kind -> {family, a, b}.  The kernels are instantiated per family and read a and b from their arguments;
// the template value of a family is its A2B1 kind.
struct ColKind { int family; float a, b; };     // family: MIS_WARP_COMPRESSED_PLANE_A2B1 or MIS_WARP_PANINI_A2B1; 0 = another kind
static ColKind col_kind_of(int kind) {
    switch (kind) {
        case MIS_WARP_COMPRESSED_PLANE_A2B1: return {MIS_WARP_COMPRESSED_PLANE_A2B1, 2.f, 1.f};
        case MIS_WARP_COMPRESSED_PLANE_A15B1: return {MIS_WARP_COMPRESSED_PLANE_A2B1, 1.5f, 1.f};
        case MIS_WARP_PANINI_A2B1: return {MIS_WARP_PANINI_A2B1, 2.f, 1.f};
        case MIS_WARP_PANINI_A15B1: return {MIS_WARP_PANINI_A2B1, 1.5f, 1.f};
        default: return {0, 0.f, 0.f};
    }
}
static bool kind_col(int kind) { return col_kind_of(kind).family != 0; }

// ProjectorBase::setCameraParams (stitching/src/warpers.cpp): float matrices, double intermediates
// The affine kind: `R` is the homogeneous H; the projector takes the R and T of affine_rt (so rinv is H without its translation
// column, the transpose of R and not its inverse -- as there).
void projector_set(Projector* p, int kind, float scale, const float K[9], const float R[9]) {
    double kinv[9], d;
    float kinv_f[9], r_affine[9];
    p->t[0] = p->t[1] = p->t[2] = 0.f;
    if (kind == MIS_WARP_AFFINE) { affine_rt(R, r_affine, p->t); R = r_affine; }
    p->kind = kind;
    p->scale = scale;
    p->a = col_kind_of(kind).a; p->b = col_kind_of(kind).b;
    for (int i = 0; i < 9; i++) p->k[i] = K[i];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) p->rinv[i * 3 + j] = R[j * 3 + i];
    auto KD = [&](int r, int c) { return (double)K[r * 3 + c]; };
    d = KD(0, 0) * (KD(1, 1) * KD(2, 2) - KD(1, 2) * KD(2, 1)) - KD(0, 1) * (KD(1, 0) * KD(2, 2) - KD(1, 2) * KD(2, 0)) +
        KD(0, 2) * (KD(1, 0) * KD(2, 1) - KD(1, 1) * KD(2, 0));
    if (d != 0.) d = 1. / d;
    kinv[0] = (KD(1, 1) * KD(2, 2) - KD(1, 2) * KD(2, 1)) * d;
    kinv[1] = (KD(0, 2) * KD(2, 1) - KD(0, 1) * KD(2, 2)) * d;
    kinv[2] = (KD(0, 1) * KD(1, 2) - KD(0, 2) * KD(1, 1)) * d;
    kinv[3] = (KD(1, 2) * KD(2, 0) - KD(1, 0) * KD(2, 2)) * d;
    kinv[4] = (KD(0, 0) * KD(2, 2) - KD(0, 2) * KD(2, 0)) * d;
    kinv[5] = (KD(0, 2) * KD(1, 0) - KD(0, 0) * KD(1, 2)) * d;
    kinv[6] = (KD(1, 0) * KD(2, 1) - KD(1, 1) * KD(2, 0)) * d;
    kinv[7] = (KD(0, 1) * KD(2, 0) - KD(0, 0) * KD(2, 1)) * d;
    kinv[8] = (KD(0, 0) * KD(1, 1) - KD(0, 1) * KD(1, 0)) * d;
    for (int i = 0; i < 9; i++) kinv_f[i] = (float)kinv[i];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0, t = 0;
            for (int k = 0; k < 3; k++) {
                s += (double)R[i * 3 + k] * (double)kinv_f[k * 3 + j];
                t += (double)K[i * 3 + k] * (double)p->rinv[k * 3 + j];
            }
            p->r_kinv[i * 3 + j] = (float)s;
            p->k_rinv[i * 3 + j] = (float)t;
        }
}

// {Spherical,Cylindrical,Plane,Mercator,Fisheye,Stereographic}Projector::mapForward (warpers_inl.hpp); the same float operations on
// the host and on the device.  Returns z_ > 0 (the plane's corners must lie in front of the panorama plane).
// LAST_KIND: the largest kind the caller can pass (the border walk never sees a kind whose roi is a full scan of its own kernel:
// its instantiation leaves the polar branch out).
// Fisheye / stereographic: no NaN guard and no special case at the singular points, as there: the stereographic quotient is 0 / 0 =
// NaN on the ray (0, -1, 0) (v_ = 0) and huge next to it.
// {CompressedRectilinear,Panini}Projector(a, b)::mapForward (`kind` is the family's A2B1 kind or the kind itself): nothing special
// at cosf(u_) = 0 (v infinite: the roi is refused), past tanf's pole (a = 1.5: u_ / a reaches 120 degrees) or at u_ beyond 90 degrees.
template <int LAST_KIND = MIS_WARP_PANINI_A15B1>
MIS_HD bool map_forward(int kind, const float* m, float scale, float x, float y, float* u, float* v, float a = 0.f, float b = 0.f,
                        const float* t = nullptr) {     // t: PlaneProjector::t, read by the affine kind only
    float x_ = (m[0] * x + m[1] * y) + m[2];
    float y_ = (m[3] * x + m[4] * y) + m[5];
    float z_ = (m[6] * x + m[7] * y) + m[8];
    if (LAST_KIND >= MIS_WARP_COMPRESSED_PLANE_A2B1 && kind >= MIS_WARP_COMPRESSED_PLANE_A2B1 && kind <= MIS_WARP_PANINI_A15B1) {
        float u_ = mis_atan2f(x_, z_);
        float v_ = mis_asinf(y_ / sqrtf((x_ * x_ + y_ * y_) + z_ * z_));
        if (kind <= MIS_WARP_COMPRESSED_PLANE_A15B1) {
            *u = scale * a * mis_tanf(u_ / a);
            *v = scale * b * mis_tanf(v_) / mis_cosf(u_);
        } else {
            float tg = a * mis_tanf(u_ / a);
            *u = scale * tg;
            float sinu = mis_sinf(u_);
            if (fabsf(sinu) < 1e-7f) *v = scale * b * mis_tanf(v_);
            else *v = scale * b * tg * mis_tanf(v_) / sinu;
        }
    } else if (LAST_KIND >= MIS_WARP_FISHEYE && (kind == MIS_WARP_FISHEYE || kind == MIS_WARP_STEREOGRAPHIC)) {
        float u_ = mis_atan2f(x_, z_);
        float v_ = MIS_PI_F - mis_acosf(y_ / sqrtf((x_ * x_ + y_ * y_) + z_ * z_));
        float su, cu;
        mis_sincosf(u_, &su, &cu);
        if (kind == MIS_WARP_FISHEYE) {
            *u = scale * v_ * cu;
            *v = scale * v_ * su;
        } else {
            float sv, cv;
            mis_sincosf(v_, &sv, &cv);
            float r = sv / (1.f - cv);
            *u = scale * r * cu;
            *v = scale * r * su;
        }
    } else if (kind == MIS_WARP_PLANE) {
        *u = scale * (x_ / z_ * 1.f);
        *v = scale * (y_ / z_ * 1.f);
    } else if (kind == MIS_WARP_AFFINE) {
        *u = scale * (t[0] + x_ / z_ * (1.f - t[2]));
        *v = scale * (t[1] + y_ / z_ * (1.f - t[2]));
    } else if (kind == MIS_WARP_CYLINDRICAL) {
        *u = scale * mis_atan2f(x_, z_);
        *v = scale * y_ / sqrtf(x_ * x_ + z_ * z_);
    } else if (kind == MIS_WARP_MERCATOR) {
        *u = scale * mis_atan2f(x_, z_);
        float v_ = mis_asinf(y_ / sqrtf((x_ * x_ + y_ * y_) + z_ * z_));
        *v = scale * mis_logf(mis_tanf((float)(3.14159265358979323846 / 4) + v_ / 2));
    } else {
        *u = scale * mis_atan2f(x_, z_);
        float w = y_ / sqrtf((x_ * x_ + y_ * y_) + z_ * z_);
        *v = scale * (MIS_PI_F - mis_acosf(w == w ? w : 0));
    }
    return z_ > 0.f;
}

// {Spherical,RotationWarperBase}::detectResultRoi, second half: the float extremes of the border projection -> integer roi, with
// the pole tests for the spherical kind.  The other kinds refuse extremes that static_cast<int> cannot take (infinite or NaN:
// OpenCV would return a meaningless rectangle) -> MIS_E_INVALID.
int roi_from_extremes(const Projector* p, int sw, int sh, float tl_uf, float tl_vf, float br_uf, float br_vf, int* tlx, int* tly, int* brx, int* bry) {
    if (p->kind != MIS_WARP_SPHERICAL) {
        auto fits = [](float f) { return f > -2147483520.f && f < 2147483520.f; };      // false for NaN and +-inf
        if (!(fits(tl_uf) && fits(tl_vf) && fits(br_uf) && fits(br_vf))) return MIS_E_INVALID;
        *tlx = (int)tl_uf; *tly = (int)tl_vf; *brx = (int)br_uf; *bry = (int)br_vf;
        return MIS_OK;
    }
    tl_uf = (float)(int)tl_uf; tl_vf = (float)(int)tl_vf; br_uf = (float)(int)br_uf; br_vf = (float)(int)br_vf;
    for (int pass = 0; pass < 2; pass++) {
        float x = p->rinv[1], y = pass == 0 ? p->rinv[4] : -p->rinv[4], z = p->rinv[7];
        if (y > 0.f) {
            float x_ = (p->k[0] * x + p->k[1] * y) / z + p->k[2];
            float y_ = p->k[4] * y / z + p->k[5];
            if (x_ > 0.f && x_ < (float)sw && y_ > 0.f && y_ < (float)sh) {
                float pv = pass == 0 ? (float)(3.14159265358979323846 * (double)p->scale) : 0.f;
                if (0.f < tl_uf) tl_uf = 0.f;
                if (pv < tl_vf) tl_vf = pv;
                if (0.f > br_uf) br_uf = 0.f;
                if (pv > br_vf) br_vf = pv;
            }
        }
    }
    *tlx = (int)tl_uf; *tly = (int)tl_vf; *brx = (int)br_uf; *bry = (int)br_vf;
    return MIS_OK;
}

// detectResultRoi on the host (single-call entry points; a job's frames go through mis_warper_roi_batch: one small kernel for all
// of them).  Nothing is cached: every call pays it.
//  * spherical (SphericalWarper::detectResultRoi) and cylindrical (detectResultRoiByBorder): the 2(W+H) border pixels;
//  * plane (PlaneWarper::detectResultRoi): the four corners (0,0), (0,h-1), (w-1,0), (w-1,h-1).  A corner with z_ <= 0 lies behind
//    the panorama plane and OpenCV's rectangle means nothing: MIS_E_INVALID.
//  * mercator, fisheye, stereographic, compressed-plane, Panini (RotationWarperBase::detectResultRoi: these warpers have no override):
//    every pixel, O(w h).
//    With a pole inside the frame the extreme lies at an interior pixel; a NaN (Mercator: the upper pole; stereographic: the ray
//    (0, -1, 0)) is skipped as std::min / std::max skip it.
int detect_result_roi(const Projector* p, int sw, int sh, int* tlx, int* tly, int* brx, int* bry) {
    float tl_uf = FLT_MAX, tl_vf = FLT_MAX, br_uf = -FLT_MAX, br_vf = -FLT_MAX, u, v;
    auto upd = [&]() {
        if (u < tl_uf) tl_uf = u;
        if (v < tl_vf) tl_vf = v;
        if (u > br_uf) br_uf = u;
        if (v > br_vf) br_vf = v;
    };
    const int kind = p->kind;
    if (kind_planar(kind)) {
        const float cx[4] = {0.f, 0.f, (float)(sw - 1), (float)(sw - 1)}, cy[4] = {0.f, (float)(sh - 1), 0.f, (float)(sh - 1)};
        bool front = true;
        for (int c = 0; c < 4; c++) { front &= map_forward(kind, p->r_kinv, p->scale, cx[c], cy[c], &u, &v, 0.f, 0.f, p->t); upd(); }
        if (!front) return MIS_E_INVALID;
    } else if (MIS_WARP_ROI_IS_FULL_SCAN(kind)) {
        for (int y = 0; y < sh; ++y)
            for (int x = 0; x < sw; ++x) { map_forward(kind, p->r_kinv, p->scale, (float)x, (float)y, &u, &v, p->a, p->b); upd(); }
    } else {
        for (int x = 0; x < sw; ++x) {
            map_forward(kind, p->r_kinv, p->scale, (float)x, 0, &u, &v); upd();
            map_forward(kind, p->r_kinv, p->scale, (float)x, (float)(sh - 1), &u, &v); upd();
        }
        for (int y = 0; y < sh; ++y) {
            map_forward(kind, p->r_kinv, p->scale, 0, (float)y, &u, &v); upd();
            map_forward(kind, p->r_kinv, p->scale, (float)(sw - 1), (float)y, &u, &v); upd();
        }
    }
    return roi_from_extremes(p, sw, sh, tl_uf, tl_vf, br_uf, br_vf, tlx, tly, brx, bry);
}

// the (x, y, width, height) rectangle of an inclusive roi; its size in 64 bits: a width or height past INT_MAX (extremes on either
// side of +-2^30, e.g. a plane corner just in front of the panorama plane) is refused rather than wrapped -> MIS_E_INVALID
int roi_rect(int tlx, int tly, int brx, int bry, MisRect* r) {
    const long long w = (long long)brx + 1 - tlx, h = (long long)bry + 1 - tly;
    if (w < 1 || h < 1 || w > INT_MAX || h > INT_MAX) return MIS_E_INVALID;
    r->x = tlx; r->y = tly; r->width = (int)w; r->height = (int)h;
    return MIS_OK;
}

int projector_and_roi(int kind, float scale, const float K[9], const float R[9], int w, int h, Projector* p, int* tlx, int* tly, int* brx, int* bry) {
    projector_set(p, kind, scale, K, R);
    return detect_result_roi(p, w, h, tlx, tly, brx, bry);
}

// frames (or views) per batched grid: the batch kernels take an array of WarpArgs of this length by value
constexpr int WB_MAX = 16;

struct WarpArgs {
    float m[9];  // k_rinv
    float scale;
    int tlx, tly, dw, dh, sw, sh, cn;
    int kind;        // MIS_WARP_* (read by the table fills and the u8 warps; the fused kernels take it as a template argument)
    float pa, pb;    // the (A, B) of a compressed-plane / Panini kind; the affine kind's (t0, t1) of Projector::t (its t2 is +-0: w = 1 -
                     // t2 = 1), read by the table fills.  No member of its own: the struct keeps its 128 bytes, and with them every
                     // kernel that takes it -- or an array of it -- its code
    const uint8_t* src;
    size_t sstride;
    void* dst;       // s16x3 (fused) or u8 x cn
    size_t dstride;  // bytes
    uint8_t* mask;
    size_t mstride;
};

// {Spherical,Cylindrical,Plane,Mercator}Projector::mapBackward with the separable terms pre-evaluated (table_terms); the plane divides
// by z whatever its sign
MIS_HD void map_backward(int kind, const float* m, float sinu, float cosu, float sinv, float cosv, float* x, float* y) {
    float x_ = sinv * sinu, y_ = cosv, z_ = sinv * cosu;
    float xx = (m[0] * x_ + m[1] * y_) + m[2] * z_;
    float yy = (m[3] * x_ + m[4] * y_) + m[5] * z_;
    float z = (m[6] * x_ + m[7] * y_) + m[8] * z_;
    if (kind_planar(kind) || z > 0) { *x = xx / z; *y = yy / z; }
    else { *x = -1.f; *y = -1.f; }
}

// the separable terms of output column `col` ({su, cu}) and row `row` ({s, c}) of a warp kind (u' = u / scale, v' = v / scale):
// spherical {sin u', cos u'} {sin(pi - v'), cos(pi - v')}; cylindrical {sin u', cos u'} {1, v'}; plane {u', 1} {1, v'};
// mercator {sin u', cos u'} {cos v_, sin v_}, v_ = atan(sinh v') (a unit ray like the spherical one; v' = +-inf gives v_ = +-pi/2);
// affine: the plane's with PlaneProjector::mapBackward's u' = u / scale - t0, v' = v / scale - t1 (its w = 1 - t2 is 1: t2 = +-0)
MIS_HD void col_terms(int kind, float scale, float col, float t0, float* su, float* cu) {
    const float u = col / scale;
    if (kind == MIS_WARP_PLANE) { *su = u; *cu = 1.f; }
    else if (kind == MIS_WARP_AFFINE) { *su = u - t0; *cu = 1.f; }
    else mis_sincosf(u, su, cu);
}
MIS_HD void row_terms(int kind, float scale, float row, float t1, float* s, float* c) {
    const float v = row / scale;
    if (kind == MIS_WARP_AFFINE) { *s = 1.f; *c = v - t1; }
    else if (kind == MIS_WARP_SPHERICAL) mis_sincosf(MIS_PI_F - v, s, c);
    else if (kind == MIS_WARP_MERCATOR) mis_sincosf(mis_atanf(mis_sinhf(v)), c, s);
    else { *s = 1.f; *c = v; }
}

// remap INTER_LINEAR, BORDER_REFLECT on u8: INTER_BITS = 5, Q15 weights, round at bit 14
template <int CN>
__device__ __forceinline__ void sample_linear(const uint8_t* src, size_t stride, int sw, int sh, float x, float y, int* out) {
    int sxq = mis_round_sat_f(x * 32.f), syq = mis_round_sat_f(y * 32.f);
    int fx = sxq & 31, fy = syq & 31;
    int sx = mis_sat_short(sxq >> 5), sy = mis_sat_short(syq >> 5);
    int x0, x1, y0, y1;
    if ((unsigned)sx < (unsigned)(sw - 1) && (unsigned)sy < (unsigned)(sh - 1)) { x0 = sx; x1 = sx + 1; y0 = sy; y1 = sy + 1; }
    else { x0 = mis_reflect(sx, sw); x1 = mis_reflect(sx + 1, sw); y0 = mis_reflect(sy, sh); y1 = mis_reflect(sy + 1, sh); }
    int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
    const uint8_t* r0 = src + (size_t)y0 * stride;
    const uint8_t* r1 = src + (size_t)y1 * stride;
#pragma unroll
    for (int c = 0; c < CN; c++) {
        int s = r0[x0 * CN + c] * w00 + r0[x1 * CN + c] * w01 + r1[x0 * CN + c] * w10 + r1[x1 * CN + c] * w11;
        out[c] = (s + (1 << 14)) >> 15;  // always within 0..255
    }
}

// remap INTER_NEAREST, BORDER_CONSTANT(0): is the nearest source pixel inside the image?
__device__ __forceinline__ bool nearest_inside(int sw, int sh, float x, float y, int* sx, int* sy) {
    *sx = mis_sat_short(mis_round_sat_f(x));
    *sy = mis_sat_short(mis_round_sat_f(y));
    return (unsigned)*sx < (unsigned)sw && (unsigned)*sy < (unsigned)sh;
}

// ---- the per-pixel map path: the kinds whose backward ray is not separable (fisheye, stereographic) ----
// {Fisheye,Stereographic}Projector::mapBackward (warpers_inl.hpp), the reference's operation sequence kept literally: the polar angle
// u_ = atan2(v', u') and the radius rho = |(u', v')| of the output pixel, the polar distance v_ = rho (fisheye) or 2 atan(1 / rho)
// (stereographic), then the spherical ray of (u_, pi - v_) through k_rinv with the z > 0 test (map_backward).  Nothing is special-
// cased at the centre pixel u' = v' = 0: atan2(0, 0) = 0; fisheye gets the ray (0, -1, 0); stereographic 1 / 0 = +inf,
// atan(+inf) = pi / 2, v_ = pi, the ray (0, +1, 0).
MIS_HD void map_backward_polar(int kind, const float* m, float scale, float u, float v, float* x, float* y) {
    const float up = u / scale, vp = v / scale;
    const float u_ = mis_atan2f(vp, up);
    float v_ = sqrtf(up * up + vp * vp);
    if (kind == MIS_WARP_STEREOGRAPHIC) v_ = 2.f * mis_atanf(1.f / v_);
    float sinv, cosv, sinu, cosu;
    mis_sincosf(MIS_PI_F - v_, &sinv, &cosv);
    mis_sincosf(u_, &sinu, &cosu);
    map_backward(kind, m, sinu, cosu, sinv, cosv, x, y);
}

// ---- the column-hoisted map path: the half-separable kinds (compressed-plane, Panini) ----
// {CompressedRectilinear,Panini}Projector(a, b)::mapBackward (warpers_inl.hpp), the reference's operation sequence kept literally:
//   u' = u / scale, v' = v / scale, lam = a atan(u' / a)
//   compressed:  v_ = atan(v' cos(lam) / b)
//   Panini:      v_ = |lam| > 1e-7 ? atan(v' sin(lam) / (b a tan(lam / a))) : atan(v' / b)
//   ray (sin(lam) cos(v_), sin(v_), cos(lam) cos(v_)) through k_rinv with the z > 0 test (map_backward).
// Nothing is special-cased where cos(lam) turns negative (|lam| > 90 degrees) or tan(lam / a) passes its pole (a = 1.5).
// The sequence is split where its terms stop depending on the row: col_hoist evaluates, from u alone, lam, sin(lam), cos(lam) and for
// Panini the divisor b a tan(lam / a) and the branch; col_pixel the rest.  Every float operation is the literal sequence's with the
// same operands in the same order, so the split changes no bit (map_backward_col, the unsplit form, is what the host evaluates for
// the test aid mis_debug_warper_map_f32).
struct ColTerms { float sl, cl, den; bool big; };     // sin(lam), cos(lam); Panini: b a tan(lam / a), |lam| > 1e-7
template <int FAM>
MIS_HD ColTerms col_hoist(float scale, float pa, float pb, float u) {
    ColTerms t;
    const float lam = pa * mis_atanf(u / scale / pa);
    mis_sincosf(lam, &t.sl, &t.cl);
    t.big = fabsf(lam) > 1e-7f;
    t.den = FAM == MIS_WARP_PANINI_A2B1 ? pb * pa * mis_tanf(lam / pa) : 0.f;
    return t;
}
template <int FAM>
MIS_HD void col_pixel(const ColTerms& t, float pb, float vp, float* sinv, float* cosv) {
    float q;
    if (FAM == MIS_WARP_PANINI_A2B1) q = t.big ? vp * t.sl / t.den : vp / pb;
    else q = vp * t.cl / pb;
    mis_sincosf(mis_atanf(q), sinv, cosv);
}
// the unsplit sequence for one pixel, every term evaluated where the reference evaluates it (host: the test aid's reference; the
// kernels use the split form)
MIS_HD void map_backward_col(int fam, const float* m, float scale, float pa, float pb, float u, float v, float* x, float* y) {
    u /= scale; v /= scale;
    const float lam = pa * mis_atanf(u / pa);
    float v_;
    if (fam == MIS_WARP_PANINI_A2B1) {
        if (fabsf(lam) > 1e-7f) v_ = mis_atanf(v * mis_sinf(lam) / (pb * pa * mis_tanf(lam / pa)));
        else v_ = mis_atanf(v / pb);
    } else v_ = mis_atanf(v * mis_cosf(lam) / pb);
    const float cosv = mis_cosf(v_);
    const float x_ = mis_sinf(lam) * cosv, y_ = mis_sinf(v_), z_ = mis_cosf(lam) * cosv;
    const float xx = (m[0] * x_ + m[1] * y_) + m[2] * z_;
    const float yy = (m[3] * x_ + m[4] * y_) + m[5] * z_;
    const float z = (m[6] * x_ + m[7] * y_) + m[8] * z_;
    if (z > 0) { *x = xx / z; *y = yy / z; }
    else { *x = -1.f; *y = -1.f; }
}

// Run-time value -> template instantiation, one helper per kernel family: `launch` is a generic lambda that takes the value as
// std::integral_constant(s) and names the kernel with them, so only the instantiations listed here exist.
template <int V> using int_c = std::integral_constant<int, V>;
template <class F> void with_polar_kind(int kind, F&& launch) {         // warp_polar_fused_kernel, warp_polar_fused_batch_kernel
    if (kind == MIS_WARP_FISHEYE) launch(int_c<MIS_WARP_FISHEYE>{});
    else launch(int_c<MIS_WARP_STEREOGRAPHIC>{});
}
template <class F> void with_col_kind(int kind, F&& launch) {           // warp_col_fused_kernel, warp_col_fused_batch_kernel, warp_col_u8_kernel: the family
    if (col_kind_of(kind).family == MIS_WARP_COMPRESSED_PLANE_A2B1) launch(int_c<MIS_WARP_COMPRESSED_PLANE_A2B1>{});
    else launch(int_c<MIS_WARP_PANINI_A2B1>{});
}
template <class F> void with_scan_kind(int kind, F&& launch) {          // warp_roi_scan_kernel (MIS_WARP_ROI_IS_FULL_SCAN kinds)
    if (kind == MIS_WARP_MERCATOR) launch(int_c<MIS_WARP_MERCATOR>{});
    else if (kind == MIS_WARP_FISHEYE) launch(int_c<MIS_WARP_FISHEYE>{});
    else if (kind == MIS_WARP_STEREOGRAPHIC) launch(int_c<MIS_WARP_STEREOGRAPHIC>{});
    else with_col_kind(kind, launch);
}
template <class F> void with_ztest(int kind, F&& launch) {              // warp_fused_kernel, warp_strip_batch_kernel: ZTEST = not plane / affine
    if (kind_planar(kind)) launch(std::false_type{});
    else launch(std::true_type{});
}
template <class F> void with_cn_linear(int cn, bool linear, F&& launch) {       // warp_u8_kernel, warp_polar_u8_kernel
    if (cn == 3) { if (linear) launch(int_c<3>{}, std::true_type{}); else launch(int_c<3>{}, std::false_type{}); }
    else { if (linear) launch(int_c<1>{}, std::true_type{}); else launch(int_c<1>{}, std::false_type{}); }
}

}  // namespace
