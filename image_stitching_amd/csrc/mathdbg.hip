// mathdbg.hip -- test aid: the functions of dev_math.h that mis_debug_math_f32 (warp.hip) does not reach, and the raw f32 sqrt /
// reciprocal / division that the header's premise names, on the host or in a one-thread-per-element kernel.  A translation unit of
// its own, built with the library's flags: no kernel of the product shares a module with it.
#include "common.h"
#include "dev_math.h"

namespace {

// One element of a (and b) in, one of out; the element types follow fn (MIS_MATHX_* in mistitch.h).  dev_math.h's inline functions
// themselves are called, host and device alike.
MIS_HD void debug_mathx_eval(int fn, const void* a, const void* b, void* out, int i) {
    const float* af = (const float*)a; const float* bf = (const float*)b;
    const int* ai = (const int*)a; const int* bi = (const int*)b;
    const double* ad = (const double*)a;
    float* of = (float*)out; int* oi = (int*)out; double* od = (double*)out;
    switch (fn) {
        case MIS_MATHX_SIN: of[i] = mis_sinf(af[i]); break;
        case MIS_MATHX_COS: of[i] = mis_cosf(af[i]); break;
        case MIS_MATHX_ACOS: of[i] = mis_acosf(af[i]); break;
        case MIS_MATHX_SQRT: of[i] = sqrtf(af[i]); break;
        case MIS_MATHX_RCP: of[i] = 1.0f / af[i]; break;
        case MIS_MATHX_ATAN2: of[i] = mis_atan2f(af[i], bf[i]); break;
        case MIS_MATHX_FAST_ATAN2: of[i] = mis_fast_atan2(af[i], bf[i]); break;
        case MIS_MATHX_DIV: of[i] = af[i] / bf[i]; break;
        case MIS_MATHX_ROUND_F: oi[i] = mis_round_f(af[i]); break;
        case MIS_MATHX_ROUND_SAT_F: oi[i] = mis_round_sat_f(af[i]); break;
        case MIS_MATHX_FLOOR_F: oi[i] = mis_floor_f(af[i]); break;
        case MIS_MATHX_SAT_SHORT: oi[i] = mis_sat_short(ai[i]); break;
        case MIS_MATHX_REFLECT101: oi[i] = mis_reflect101(ai[i], bi[i]); break;
        case MIS_MATHX_REFLECT: oi[i] = mis_reflect(ai[i], bi[i]); break;
        case MIS_MATHX_REFLECT1: oi[i] = mis_reflect1(ai[i], bi[i]); break;
        case MIS_MATHX_LOG_D: od[i] = mis_log_d(ad[i]); break;
        default: oi[i] = mis_round_d(ad[i]); break;
    }
}

__global__ __launch_bounds__(256) void debug_mathx_kernel(int fn, const void* a, const void* b, void* out, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) debug_mathx_eval(fn, a, b, out, i);
}

}  // namespace

extern "C" int mis_debug_math(MisContext* ctx, int fn, const void* a, const void* b, void* out, int n) {
    if (fn < MIS_MATHX_SIN || fn > MIS_MATHX_ROUND_D || !a || !out || n < 0) return MIS_E_INVALID;
    const bool two = (fn >= MIS_MATHX_ATAN2 && fn <= MIS_MATHX_DIV) || (fn >= MIS_MATHX_REFLECT101 && fn <= MIS_MATHX_REFLECT1);
    if (two && !b) return MIS_E_INVALID;
    if (!ctx) {
        for (int i = 0; i < n; i++) debug_mathx_eval(fn, a, b, out, i);
        return MIS_OK;
    }
    if (n == 0) return MIS_OK;
    MIS_CHECK(ctx, n <= (1 << 20), MIS_E_INVALID, "mis_debug_math: at most 2^20 elements per call with a context (%d)", n);
    const size_t in_sz = fn >= MIS_MATHX_LOG_D ? sizeof(double) : 4, out_sz = fn == MIS_MATHX_LOG_D ? sizeof(double) : 4;
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    char* d = nullptr;
    int rc;
    if ((rc = mis_dev_stage(ctx, 3 * sizeof(double) * (size_t)n, (void**)&d)) != MIS_OK) return rc;
    char *da = d, *db = d + sizeof(double) * (size_t)n, *dout = d + 2 * sizeof(double) * (size_t)n;     // (8-byte slots whatever the type)
    MIS_HIP(ctx, hipMemcpyAsync(da, a, in_sz * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    if (two) MIS_HIP(ctx, hipMemcpyAsync(db, b, in_sz * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(debug_mathx_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, fn, (const void*)da, (const void*)db, (void*)dout, n);
    MIS_HIP(ctx, hipGetLastError());
    MIS_HIP(ctx, hipMemcpyAsync(out, dout, out_sz * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MIS_OK;
}
