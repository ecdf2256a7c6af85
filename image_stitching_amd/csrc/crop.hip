// crop.hip -- the device cropper: crop(cv::Mat& source) of the reference (image_stitching/cropper.cpp:124-209, API in cropper.h)
// as kernels, rectangle for rectangle what host/cropper.cpp and image_stitching_amd/cropper.py give (tests/test_crop_device_gpu.py).
// The sequential parts of the host cropper are restated in parallel form ("the device cropper"):
//   which contours exist   a foreground component (8-connected) has an external contour exactly when the left neighbour of its
//                          raster-first pixel lies in the 4-connected background region of the frame
//   the contour            the cycle through its start state in the successor table of (pixel, direction) states; its length and
//                          its points with multiplicity come from pointer doubling, not from walking it
//   the fill               the complement of the frame's 4-connected region among the pixels that are not contour points
//   the sorted lists       cumulative histograms of the contour points' x and y
// Per call, in stream order (R = ceil(log2(8 * border pixels)) doubling rounds, data-dependent):
//   crop_mask_kernel                                  source -> padded foreground plane
//   crop_ccl_{init,merge,flatten}_kernel  x 3         labelling: foreground 8-connected, background 4-connected, the fill's free space
//   crop_slot_kernel                                  border pixels get slots of the state tables; the count goes to the host (4 bytes)
//   crop_succ_kernel, crop_start_kernel               successor table, start states of every external contour
//   crop_double_kernel  x R                           marks and jumps
//   crop_count_kernel, crop_winner_kernel             contour lengths, the ordered reduction
//   crop_wall_kernel                                  the winner's points: walls, x / y histograms
//   crop_rowz_kernel, crop_colz_kernel                prefix counts of the filled mask's zeros along rows and columns
//   crop_shrink_kernel                                one workgroup: cumulative histograms, the shrink loop, rectangle + status
//   crop_copy_kernel                                  (mis_crop only) the dense copy, sized by the rectangle on the device
// 19 + R launches for mis_crop_rect (1 + 9 + 1 + 2 + R + 3 + 2 + 1), four memsets and two small downloads; mis_crop_stats reports a call's counts.
// The per-element steps live in crop_core.h, which tools/micro/crop_emul.cpp runs on the host in the same order.
// No kernel waits for another workgroup and every loop is bounded by the image: a bug gives a wrong rectangle, not a hang.
#include "common.h"
#include "crop_core.h"
#include <algorithm>

namespace {

constexpr int CROP_TB = 256;

__global__ __launch_bounds__(CROP_TB) void crop_mask_kernel(CropGrid g, const uint8_t* __restrict__ src, size_t stride, int channels, uint8_t* mask) {
    const int p = blockIdx.x * CROP_TB + threadIdx.x;
    if (p < g.pixels()) mask[p] = crop_mask_px(g, src, stride, channels, p);
}

// crop_ccl_init of crop_core.h with the run taken from a ballot: a wavefront holds one aligned chunk of CROP_CHUNK pixels, and a
// member's run starts behind the highest lane below it that holds no member
static_assert(CROP_CHUNK == 64 && CROP_TB % 64 == 0, "a chunk is one wavefront");
__global__ __launch_bounds__(CROP_TB) void crop_ccl_init_kernel(int n, int* L, const uint8_t* __restrict__ plane, uint8_t want) {
    const int p = blockIdx.x * CROP_TB + threadIdx.x, lane = threadIdx.x & 63;
    const bool in = p < n && plane[p] == want;
    const unsigned long long gaps = ~__ballot(in) & ((1ull << lane) - 1ull);
    const int start = gaps ? 64 - __clzll(gaps) : 0;
    if (p < n) L[p] = in ? p - lane + start : -1;
}

__global__ __launch_bounds__(CROP_TB) void crop_ccl_merge_kernel(CropGrid g, int* L, const uint8_t* __restrict__ plane, uint8_t want, bool conn8) {
    const int p = blockIdx.x * CROP_TB + threadIdx.x;
    if (p < g.pixels()) crop_ccl_merge(g, L, plane, want, conn8, p);
}

__global__ __launch_bounds__(CROP_TB) void crop_ccl_flatten_kernel(int n, int* L) {
    const int p = blockIdx.x * CROP_TB + threadIdx.x;
    if (p < n) crop_ccl_flatten(L, p);
}

__global__ __launch_bounds__(CROP_TB) void crop_slot_kernel(CropGrid g, const uint8_t* __restrict__ mask, int* slot, int* pix, int* nslots) {
    const int p = blockIdx.x * CROP_TB + threadIdx.x;
    if (p < g.pixels()) crop_slot_px(g, mask, slot, pix, nslots, p);
}

__global__ __launch_bounds__(CROP_TB) void crop_succ_kernel(CropGrid g, int nstates, const uint8_t* __restrict__ mask, const int* __restrict__ slot,
                                                            const int* __restrict__ pix, int* nxt) {
    const int idx = blockIdx.x * CROP_TB + threadIdx.x;
    if (idx < nstates) crop_succ_state(g, mask, slot, pix, nxt, idx);
}

__global__ __launch_bounds__(CROP_TB) void crop_start_kernel(CropGrid g, int nslots, const uint8_t* __restrict__ mask, const int* __restrict__ fg_label,
                                                             const int* __restrict__ bg_label, const int* __restrict__ pix, uint8_t* mark) {
    const int k = blockIdx.x * CROP_TB + threadIdx.x;
    if (k < nslots) crop_start_slot(g, mask, fg_label, bg_label, pix, mark, k);
}

__global__ __launch_bounds__(CROP_TB) void crop_double_kernel(int nstates, const int* __restrict__ jump, int* __restrict__ jump_next, uint8_t* mark) {
    const int idx = blockIdx.x * CROP_TB + threadIdx.x;
    if (idx < nstates) crop_double_state(jump, jump_next, mark, idx);
}

__global__ __launch_bounds__(CROP_TB) void crop_count_kernel(int nstates, const int* __restrict__ fg_label, const int* __restrict__ slot, const int* __restrict__ pix,
                                                             const uint8_t* __restrict__ mark, int* count) {
    const int idx = blockIdx.x * CROP_TB + threadIdx.x;
    if (idx < nstates) crop_count_state(fg_label, slot, pix, mark, count, idx);
}

__global__ __launch_bounds__(CROP_TB) void crop_winner_kernel(int nslots, const int* __restrict__ pix, const int* __restrict__ count, unsigned long long* key) {
    const int k = blockIdx.x * CROP_TB + threadIdx.x;
    if (k < nslots) crop_winner_slot(pix, count, key, k);
}

__global__ __launch_bounds__(CROP_TB) void crop_wall_kernel(CropGrid g, int nstates, const int* __restrict__ fg_label, const int* __restrict__ pix,
                                                            const uint8_t* __restrict__ mark, const unsigned long long* __restrict__ key, uint8_t* wall, int* xhist, int* yhist) {
    const int idx = blockIdx.x * CROP_TB + threadIdx.x;
    if (idx < nstates) crop_wall_state(g, fg_label, pix, mark, *key, wall, xhist, yhist, idx);
}

// cmask is zero where the fill's labelling reached the frame (label 0).  A wavefront a row: the zeros left of x are the carry of the
// 64-pixel chunks before it plus the ballot's bits below the lane.
__global__ __launch_bounds__(CROP_TB) void crop_rowz_kernel(CropGrid g, const int* __restrict__ fill_label, int* rowz) {
    const int y = blockIdx.x * (CROP_TB / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (y >= g.h) return;                       // wave-uniform
    const int* row = fill_label + (size_t)(y + 1) * g.pw + 1;
    int* out = rowz + (size_t)y * (g.w + 1);
    int carry = 0;
    for (int x0 = 0; x0 < g.w; x0 += 64) {
        const int x = x0 + lane;
        const bool z = x < g.w && row[x] == 0;
        const unsigned long long b = __ballot(z);
        if (x < g.w) out[x] = carry + __popcll(b & ((1ull << lane) - 1ull));
        carry += __popcll(b);
    }
    if (lane == 0) out[g.w] = carry;
}

// a thread a column, rows in sequence: the loads and stores of a wavefront are 64 neighbours of one row
__global__ __launch_bounds__(CROP_TB) void crop_colz_kernel(CropGrid g, const int* __restrict__ fill_label, int* colz) {
    const int x = blockIdx.x * CROP_TB + threadIdx.x;
    if (x >= g.w) return;
    int n = 0;
    for (int y = 0; y < g.h; y++) {
        colz[(size_t)y * g.w + x] = n;
        n += fill_label[(size_t)(y + 1) * g.pw + x + 1] == 0;
    }
    colz[(size_t)g.h * g.w + x] = n;
}

__device__ void crop_block_scan(const int* hist, int* cum, int n, int* buf, int* carry) {
    const int t = threadIdx.x;
    if (t == 0) *carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += CROP_TB) {
        const int i = base + t;
        buf[t] = i < n ? hist[i] : 0;
        __syncthreads();
        for (int off = 1; off < CROP_TB; off <<= 1) {
            const int a = t >= off ? buf[t - off] : 0;
            __syncthreads();
            buf[t] += a;
            __syncthreads();
        }
        if (i < n) cum[i] = *carry + buf[t];
        __syncthreads();
        if (t == CROP_TB - 1) *carry += buf[t];
        __syncthreads();
    }
}

// One workgroup: the sorted coordinate lists in counted form, then the shrink loop on one thread (every step is O(1) on the prefix
// counts).  Writes the result block.
__global__ __launch_bounds__(CROP_TB) void crop_shrink_kernel(CropGrid g, const unsigned long long* __restrict__ key, const int* xhist, const int* yhist, int* cumx, int* cumy,
                                                              const int* rowz, const int* colz, int rounds, int* result) {
    __shared__ int buf[CROP_TB];
    __shared__ int carry;
    crop_block_scan(xhist, cumx, g.w, buf, &carry);
    crop_block_scan(yhist, cumy, g.h, buf, &carry);
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x != 0) return;
    const unsigned long long k = *key;
    int rect[4] = {0, 0, 0, 0};
    int status = CROP_EMPTY, count = 0, first = -1;
    if (k != 0) {
        count = crop_key_count(k);
        const int p = crop_key_first(k), py = p / g.pw, px = p - py * g.pw;
        first = (py - 1) * g.w + (px - 1);
        status = crop_shrink(CropShrink{cumx, cumy, rowz, colz, g.w, g.h, count}, rect);
    }
    for (int i = 0; i < 4; i++) result[CROP_R_X + i] = rect[i];
    result[CROP_R_STATUS] = status; result[CROP_R_COUNT] = count; result[CROP_R_FIRST] = first; result[CROP_R_ROUNDS] = rounds;
}

// the dense copy: a thread a byte of the source's rows, those outside the rectangle (known on the device only) leave at once
__global__ __launch_bounds__(CROP_TB) void crop_copy_kernel(CropGrid g, const uint8_t* __restrict__ src, size_t stride, int channels, const int* __restrict__ result,
                                                            uint8_t* dst, size_t dst_stride) {
    if (result[CROP_R_STATUS] != CROP_OK) return;
    const int rw = result[CROP_R_W] * channels, rh = result[CROP_R_H];
    const long long i = (long long)blockIdx.x * CROP_TB + threadIdx.x;
    if (i >= (long long)rw * rh) return;
    const int y = (int)(i / rw), b = (int)(i - (long long)y * rw);
    dst[(size_t)y * dst_stride + b] = src[(size_t)(result[CROP_R_Y] + y) * stride + (size_t)result[CROP_R_X] * channels + b];
}

__global__ __launch_bounds__(CROP_TB) void crop_cmask_kernel(CropGrid g, const int* __restrict__ fill_label, uint8_t* cmask) {
    const int i = blockIdx.x * CROP_TB + threadIdx.x;
    if (i >= g.w * g.h) return;
    const int y = i / g.w, x = i - y * g.w;
    cmask[i] = fill_label[(size_t)(y + 1) * g.pw + x + 1] == 0 ? 0 : 255;
}

// events between the stages of one call, for the caller that asked for their times (mis_crop_rect_timed)
struct CropStages {
    hipStream_t stream; bool on;
    std::vector<hipEvent_t> ev;
    CropStages(hipStream_t s, bool enabled) : stream(s), on(enabled) {}
    CropStages(const CropStages&) = delete;
    ~CropStages() { for (hipEvent_t e : ev) hipEventDestroy(e); }
    void mark() {
        if (!on) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) == hipSuccess) { hipEventRecord(e, stream); ev.push_back(e); }
    }
};

struct CropDebug { int* count; int* first; int32_t* xhist; int32_t* yhist; uint8_t* cmask; };

inline unsigned crop_blocks(long long n) { return (unsigned)((n + CROP_TB - 1) / CROP_TB); }

#define CROP_LAUNCH(kernel, n, ...)                                                                   \
    do {                                                                                              \
        hipLaunchKernelGGL(kernel, dim3(crop_blocks(n)), dim3(CROP_TB), 0, ctx->stream, __VA_ARGS__); \
        launches++;                                                                                   \
    } while (0)

// the three labellings: init, merge, flatten over the padded image
int crop_label(MisContext* ctx, const CropGrid& g, int* L, const uint8_t* plane, uint8_t want, bool conn8, int& launches) {
    const int P = g.pixels();
    CROP_LAUNCH(crop_ccl_init_kernel, P, P, L, plane, want);
    CROP_LAUNCH(crop_ccl_merge_kernel, P, g, L, plane, want, conn8);
    CROP_LAUNCH(crop_ccl_flatten_kernel, P, P, L);
    MIS_HIP(ctx, hipGetLastError());
    return MIS_OK;
}

int crop_run(MisContext* ctx, const uint8_t* src, int width, int height, int channels, size_t row_stride, uint8_t* dst, size_t dst_stride, bool copy,
             int* rect_out, int* status_out, const CropDebug* dbg, float* stage_ms = nullptr) {
    MIS_CHECK(ctx, src && rect_out && status_out, MIS_E_INVALID, "crop: null argument");
    MIS_CHECK(ctx, width > 0 && height > 0, MIS_E_INVALID, "crop: a source of %dx%d", width, height);
    MIS_CHECK(ctx, channels == 1 || channels == 3, MIS_E_INVALID, "crop: 8UC3 or 8UC1 image expected, not %d channels", channels);
    MIS_CHECK(ctx, row_stride >= (size_t)width * channels, MIS_E_INVALID, "crop: stride %zu smaller than a row (%zu)", row_stride, (size_t)width * channels);
    if (copy) MIS_CHECK(ctx, dst && dst_stride >= (size_t)width * channels, MIS_E_INVALID, "crop: the output needs a buffer of the source's size (stride %zu, a row is %zu)", dst_stride, (size_t)width * channels);
    // eight states a padded pixel are indexed with 32 bits
    MIS_CHECK(ctx, ((long long)width + 2) * ((long long)height + 2) < (1ll << 28), MIS_E_INVALID, "crop: %dx%d is beyond the cropper's 32-bit state indices (2^28 pixels with the frame)", width, height);
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    const CropGrid g = crop_grid(width, height);
    const size_t P = (size_t)g.pixels();

    // the per-pixel block
    size_t total = 0;
    auto take = [&](size_t bytes) { const size_t off = total; total += mis_align_up(bytes, 256); return off; };
    const size_t o_mask = take(P), o_wall = take(P), o_fg = take(P * 4), o_bg = take(P * 4), o_slot = take(P * 4), o_pix = take(P * 4);
    const size_t o_rowz = take((size_t)height * (width + 1) * 4), o_colz = take((size_t)(height + 1) * width * 4);
    const size_t o_small = total;           // zeroed at the start: histograms, the winner's key, the slot count
    const size_t o_xhist = take((size_t)width * 4), o_yhist = take((size_t)height * 4), o_key = take(8), o_nslots = take(4);
    const size_t small_bytes = total - o_small;
    const size_t o_cumx = take((size_t)width * 4), o_cumy = take((size_t)height * 4), o_result = take(CROP_R_N * 4);
    const size_t o_cmask = dbg ? take((size_t)width * height) : 0;
    PoolBlock blk(ctx);
    if (int rc = blk.alloc(total)) return rc;
    uint8_t* d = (uint8_t*)blk.p;
    uint8_t *mask = d + o_mask, *wall = d + o_wall;
    int *fg = (int*)(d + o_fg), *bg = (int*)(d + o_bg), *slot = (int*)(d + o_slot), *pix = (int*)(d + o_pix);
    int *rowz = (int*)(d + o_rowz), *colz = (int*)(d + o_colz), *xhist = (int*)(d + o_xhist), *yhist = (int*)(d + o_yhist);
    int *cumx = (int*)(d + o_cumx), *cumy = (int*)(d + o_cumy), *result = (int*)(d + o_result), *nslots_d = (int*)(d + o_nslots);
    unsigned long long* key = (unsigned long long*)(d + o_key);
    int* pin = nullptr;
    { void* sp = nullptr; if (int rc = mis_host_stage(ctx, 256, &sp)) return rc; pin = (int*)sp; }

    int launches = 0, rounds = 0;
    CropStages stages(ctx->stream, stage_ms != nullptr);
    MIS_HIP(ctx, hipMemsetAsync(d + o_small, 0, small_bytes, ctx->stream));
    MIS_HIP(ctx, hipMemsetAsync(wall, 0, P, ctx->stream));
    stages.mark();
    CROP_LAUNCH(crop_mask_kernel, P, g, src, row_stride, channels, mask);
    stages.mark();
    if (int rc = crop_label(ctx, g, fg, mask, 1, true, launches)) return rc;
    stages.mark();
    if (int rc = crop_label(ctx, g, bg, mask, 0, false, launches)) return rc;
    stages.mark();
    CROP_LAUNCH(crop_slot_kernel, P, g, mask, slot, pix, nslots_d);
    MIS_HIP(ctx, hipGetLastError());
    // the one number the host needs in between: it sizes the state tables and bounds the doubling rounds
    MIS_HIP(ctx, hipMemcpyAsync(pin, nslots_d, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int nslots = pin[0];
    MIS_CHECK(ctx, nslots >= 0 && (size_t)nslots <= P, MIS_E_INTERNAL, "crop: %d border pixels of %zu pixels", nslots, P);
    const int nstates = nslots * 8;
    stages.mark();

    PoolBlock tab(ctx);
    if (nslots == 0) { stages.mark(); stages.mark(); stages.mark(); }
    if (nslots > 0) {
        size_t tt = 0;
        auto ttake = [&](size_t bytes) { const size_t off = tt; tt += mis_align_up(bytes, 256); return off; };
        const size_t t_ja = ttake((size_t)nstates * 4), t_jb = ttake((size_t)nstates * 4), t_zero = tt, t_mark = ttake((size_t)nstates), t_count = ttake((size_t)nslots * 4);
        if (int rc = tab.alloc(tt)) return rc;
        uint8_t* t = (uint8_t*)tab.p;
        int *ja = (int*)(t + t_ja), *jb = (int*)(t + t_jb), *count = (int*)(t + t_count);
        uint8_t* mark = t + t_mark;
        MIS_HIP(ctx, hipMemsetAsync(t + t_zero, 0, tt - t_zero, ctx->stream));
        CROP_LAUNCH(crop_succ_kernel, nstates, g, nstates, mask, slot, pix, ja);
        CROP_LAUNCH(crop_start_kernel, nslots, g, nslots, mask, fg, bg, pix, mark);
        stages.mark();
        // a cycle holds a state at most once: after ceil(log2(states)) rounds every mark has gone round its cycle
        while ((1ll << rounds) < (long long)nstates) rounds++;
        for (int r = 0; r < rounds; r++) {
            CROP_LAUNCH(crop_double_kernel, nstates, nstates, ja, jb, mark);
            std::swap(ja, jb);
        }
        stages.mark();
        CROP_LAUNCH(crop_count_kernel, nstates, nstates, fg, slot, pix, mark, count);
        CROP_LAUNCH(crop_winner_kernel, nslots, nslots, pix, count, key);
        CROP_LAUNCH(crop_wall_kernel, nstates, g, nstates, fg, pix, mark, key, wall, xhist, yhist);
        MIS_HIP(ctx, hipGetLastError());
        stages.mark();
    }
    // the fill: the background labelling's plane is free again
    int* fill = bg;
    if (int rc = crop_label(ctx, g, fill, wall, 0, false, launches)) return rc;
    stages.mark();
    hipLaunchKernelGGL(crop_rowz_kernel, dim3((height + CROP_TB / 64 - 1) / (CROP_TB / 64)), dim3(CROP_TB), 0, ctx->stream, g, fill, rowz);
    launches++;
    CROP_LAUNCH(crop_colz_kernel, width, g, fill, colz);
    stages.mark();
    hipLaunchKernelGGL(crop_shrink_kernel, dim3(1), dim3(CROP_TB), 0, ctx->stream, g, key, xhist, yhist, cumx, cumy, rowz, colz, rounds, result);
    launches++;
    stages.mark();
    if (copy) CROP_LAUNCH(crop_copy_kernel, (long long)width * channels * height, g, src, row_stride, channels, result, dst, dst_stride);
    if (dbg) CROP_LAUNCH(crop_cmask_kernel, (long long)width * height, g, fill, d + o_cmask);
    MIS_HIP(ctx, hipGetLastError());
    MIS_HIP(ctx, hipMemcpyAsync(pin, result, CROP_R_N * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 4; i++) rect_out[i] = pin[CROP_R_X + i];
    *status_out = pin[CROP_R_STATUS];
    ctx->crop_stats = {launches, rounds, nslots, pin[CROP_R_COUNT]};
    if (stage_ms) {
        MIS_CHECK(ctx, (int)stages.ev.size() == MIS_CROP_STAGES + 1, MIS_E_INTERNAL, "crop: %zu stage events", stages.ev.size());
        for (int k = 0; k < MIS_CROP_STAGES; k++) MIS_HIP(ctx, hipEventElapsedTime(&stage_ms[k], stages.ev[k], stages.ev[k + 1]));
    }
    if (dbg) {
        *dbg->count = pin[CROP_R_COUNT]; *dbg->first = pin[CROP_R_FIRST];
        MIS_HIP(ctx, hipMemcpy(dbg->xhist, xhist, (size_t)width * 4, hipMemcpyDeviceToHost));
        MIS_HIP(ctx, hipMemcpy(dbg->yhist, yhist, (size_t)height * 4, hipMemcpyDeviceToHost));
        MIS_HIP(ctx, hipMemcpy(dbg->cmask, d + o_cmask, (size_t)width * height, hipMemcpyDeviceToHost));
    }
    return MIS_OK;
}

}  // namespace

extern "C" int mis_crop_rect(MisContext* ctx, const void* src, int width, int height, int channels, size_t row_stride, int rect_out[4], int* status_out) {
    if (!ctx) return MIS_E_INVALID;
    return crop_run(ctx, (const uint8_t*)src, width, height, channels, row_stride, nullptr, 0, false, rect_out, status_out, nullptr);
}

extern "C" int mis_crop_rect_timed(MisContext* ctx, const void* src, int width, int height, int channels, size_t row_stride, int rect_out[4], int* status_out,
                                   float ms[MIS_CROP_STAGES]) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, ms, MIS_E_INVALID, "crop: null argument");
    return crop_run(ctx, (const uint8_t*)src, width, height, channels, row_stride, nullptr, 0, false, rect_out, status_out, nullptr, ms);
}

extern "C" int mis_crop(MisContext* ctx, const void* src, int width, int height, int channels, size_t row_stride, void* dst, size_t dst_stride, int rect_out[4],
                        int* status_out) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, dst, MIS_E_INVALID, "crop: null argument");
    return crop_run(ctx, (const uint8_t*)src, width, height, channels, row_stride, (uint8_t*)dst, dst_stride, true, rect_out, status_out, nullptr);
}

extern "C" int mis_crop_debug_contour(MisContext* ctx, const void* src, int width, int height, int channels, size_t row_stride, int* count_out, int* first_out,
                                      int32_t* xhist, int32_t* yhist, uint8_t* cmask_out) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, count_out && first_out && xhist && yhist && cmask_out, MIS_E_INVALID, "crop: null argument");
    int rect[4], status = 0;
    const CropDebug dbg{count_out, first_out, xhist, yhist, cmask_out};
    return crop_run(ctx, (const uint8_t*)src, width, height, channels, row_stride, nullptr, 0, false, rect, &status, &dbg);
}

extern "C" int mis_crop_stats(const MisContext* ctx, int* out, int capacity, int* count) {
    if (!ctx || !count || capacity < 0 || (capacity > 0 && !out)) return MIS_E_INVALID;
    *count = (int)ctx->crop_stats.size();
    for (int k = 0; k < capacity && k < *count; k++) out[k] = ctx->crop_stats[k];
    return MIS_OK;
}
