// akaze.hip -- AKAZE::create()->detectAndCompute on the GPU: the finder behind features_type == "akaze".
// Reference call sites: image_stitching/image_stitching.cpp:547-550 (`AKAZE::create()`), :613 (`computeImageFeatures`).  The
// definition is SURVEY Appendix A.19 (a recollection of upstream's defaults and AKAZEFeatures.cpp, with one defined departure: the
// suppression of step 6 is independent of order); the per-element arithmetic is akaze_core.h, shared with the host emulation.
//
// A detect is one chain of launches on the context's stream with one host read at its end (the counts):
//   level start (grey / copy / area average, fused with the Gaussian into Lsmooth) -> k-contrast (level 0: maximum, histogram, walk)
//   -> Scharr + flow -> one launch per FED step (Lt ping-pong, tile and ring in LDS) -> Lx, Ly -> Ldet (second derivatives from
//   Lx / Ly in registers, never stored) -> candidates per row of every level, counted, scanned and written in (level, y, x) order
//   -> suppression over the row lists -> refinement -> (max_points) -> ordered compaction -> orientation and MLDB, one wave each.
// Candidates are compacted in order (count, scan, write) instead of appended through an atomic counter and sorted afterwards: the
// order is (level, y, x) by construction, two runs give the same bytes, and the row offsets of the scan are the bins of the
// suppression (a candidate's rivals lie in a few rows of three levels).
#include "common.h"
#include "akaze_core.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int TW = 64, TH = 16;      // a stencil workgroup's tile: 256 threads, four rows a thread

struct Taps { int n; float k[AKZ_MAX_TAPS]; };

struct AkzDev {      // device view of the scale space of the current frame size
    AkzPlan plan;
    float* plane[AKZ_MAX_LEVELS][AKZ_PLANES];
    int row_base[AKZ_MAX_LEVELS + 1];      // level l's rows are row_base[l] .. row_base[l + 1] of the row table
    float radius[AKZ_MAX_LEVELS];          // esigma * derivative_factor
};

// ------------------------------------------------------------------ level start + Gaussian ------
// MODE 0: grey / 255 of the BGR frame; 1: copy of the previous Lt; 2: its area average.  The start values of the tile and its ring
// (replicated borders: clamped coordinates) are staged in LDS, filtered along rows into LDS and along columns into Lsmooth.
template <int MODE, int R>
__global__ __launch_bounds__(256) void akz_start_kernel(const void* __restrict__ src, size_t stride, int sw, int sh, float sx, float sy, float* __restrict__ start,
                                                        float* __restrict__ smooth, int w, int h, Taps t) {
    constexpr int SW = TW + 2 * R, SH = TH + 2 * R;
    __shared__ float st[SH * SW];
    __shared__ float rp[SH * TW];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, tid = threadIdx.x;
    for (int i = tid; i < SH * SW; i += 256) {
        const int gx = akz_clampi(x0 - R + i % SW, 0, w - 1), gy = akz_clampi(y0 - R + i / SW, 0, h - 1);
        float v;
        if (MODE == 0) v = akz_gray01((const uint8_t*)src + (size_t)gy * stride + 3 * (size_t)gx);
        else if (MODE == 1) v = ((const float*)src)[(size_t)gy * w + gx];
        else v = akz_area_px((const float*)src, sw, sh, sx, sy, gx, gy);
        st[i] = v;
    }
    __syncthreads();
    for (int i = tid; i < SH * TW; i += 256) {
        const float* p = st + (i / TW) * SW + i % TW;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * R + 1; k++) acc += t.k[k] * p[k];
        rp[i] = acc;
    }
    __syncthreads();
    const int cx = tid % TW, x = x0 + cx;
    if (x >= w) return;
    for (int ry = tid / TW; ry < TH; ry += 256 / TW) {
        const int y = y0 + ry;
        if (y >= h) break;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 2 * R + 1; k++) acc += t.k[k] * rp[(ry + k) * TW + cx];
        smooth[(size_t)y * w + x] = acc;
        start[(size_t)y * w + x] = MODE == 0 ? acc : st[(ry + R) * SW + cx + R];
    }
}

// ------------------------------------------------------------------ k-contrast ------------------
// stats: [0] hmax as float bits, [1] the k-contrast as float bits, [2 ..] the histogram
__global__ __launch_bounds__(256) void akz_hmax_kernel(const float* __restrict__ ls, int w, int h, unsigned* stats) {
    __shared__ float red[256];
    const int x = 1 + blockIdx.x * 256 + threadIdx.x, y = 1 + blockIdx.y;
    float m = 0.f;
    if (x < w - 1 && y < h - 1) {
        float lx, ly;
        akz_scharr(ls, w, h, x, y, &lx, &ly);
        m = sqrtf(lx * lx + ly * ly);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    // (non-negative floats order like their bit patterns)
    if (threadIdx.x == 0 && red[0] > 0.f) atomicMax(&stats[0], __float_as_uint(red[0]));
}
__global__ __launch_bounds__(256) void akz_hist_kernel(const float* __restrict__ ls, int w, int h, unsigned* stats) {
    __shared__ unsigned hist[AKZ_HIST_BINS];
    for (int i = threadIdx.x; i < AKZ_HIST_BINS; i += 256) hist[i] = 0;
    __syncthreads();
    const float hmax = __uint_as_float(stats[0]);
    const int x = 1 + blockIdx.x * 256 + threadIdx.x, y = 1 + blockIdx.y;
    if (x < w - 1 && y < h - 1 && hmax > 0.f) {
        float lx, ly;
        akz_scharr(ls, w, h, x, y, &lx, &ly);
        const float m = sqrtf(lx * lx + ly * ly);
        if (m != 0.f) atomicAdd(&hist[akz_hist_bin(m, hmax)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < AKZ_HIST_BINS; i += 256)
        if (hist[i]) atomicAdd(&stats[2 + i], hist[i]);
}
__global__ void akz_kcontrast_kernel(unsigned* stats) {
    if (threadIdx.x == 0 && blockIdx.x == 0) stats[1] = __float_as_uint(akz_kcontrast(stats + 2, __uint_as_float(stats[0])));
}

// ------------------------------------------------------------------ flow, diffusion -------------
__global__ __launch_bounds__(256) void akz_flow_kernel(const float* __restrict__ ls, float* __restrict__ flow, int w, int h, const unsigned* __restrict__ stats, int octave) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const float k = akz_level_k(__uint_as_float(stats[1]), octave);
    float lx, ly;
    akz_scharr(ls, w, h, x, y, &lx, &ly);
    flow[(size_t)y * w + x] = akz_flow_g2(lx, ly, k);
}
// one FED step: the tile of Lt and of the flow with their one-pixel ring in LDS, four rows a thread
__global__ __launch_bounds__(256) void akz_fed_kernel(const float* __restrict__ src, const float* __restrict__ g, float* __restrict__ dst, int w, int h, float tau) {
    constexpr int SW = TW + 2, SH = TH + 2;
    __shared__ float sl[SH * SW];
    __shared__ float sg[SH * SW];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, tid = threadIdx.x;
    for (int i = tid; i < SH * SW; i += 256) {
        const int gx = akz_clampi(x0 - 1 + i % SW, 0, w - 1), gy = akz_clampi(y0 - 1 + i / SW, 0, h - 1);
        sl[i] = src[(size_t)gy * w + gx];
        sg[i] = g[(size_t)gy * w + gx];
    }
    __syncthreads();
    const int cx = tid % TW, x = x0 + cx;
    if (x >= w) return;
    for (int ry = tid / TW; ry < TH; ry += 256 / TW) {
        const int y = y0 + ry;
        if (y >= h) break;
        const int o = (ry + 1) * SW + cx + 1;
        dst[(size_t)y * w + x] = akz_diffuse(sl[o], sg[o], sl[o - 1], sg[o - 1], x > 0, sl[o + 1], sg[o + 1], x < w - 1, sl[o - SW], sg[o - SW], y > 0, sl[o + SW],
                                             sg[o + SW], y < h - 1, tau);
    }
}

// ------------------------------------------------------------------ derivatives -----------------
__global__ __launch_bounds__(256) void akz_deriv1_kernel(const float* __restrict__ ls, float* __restrict__ lx, float* __restrict__ ly, int w, int h, int s) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const float norm = akz_deriv_norm(s);
    lx[(size_t)y * w + x] = akz_deriv_x(ls, w, h, x, y, s, norm);
    ly[(size_t)y * w + x] = akz_deriv_y(ls, w, h, x, y, s, norm);
}
__global__ __launch_bounds__(256) void akz_deriv2_kernel(const float* __restrict__ lx, const float* __restrict__ ly, float* __restrict__ ldet, int w, int h, int s) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const float norm = akz_deriv_norm(s);
    const float lxx = akz_deriv_x(lx, w, h, x, y, s, norm), lxy = akz_deriv_y(lx, w, h, x, y, s, norm), lyy = akz_deriv_y(ly, w, h, x, y, s, norm);
    ldet[(size_t)y * w + x] = akz_ldet(lxx, lyy, lxy, s);
}

// ------------------------------------------------------------------ candidates ------------------
__device__ __forceinline__ int akz_row_level(const AkzDev& D, int row) {
    int l = 0;
    while (l + 1 < D.plan.nlev && row >= D.row_base[l + 1]) l++;
    return l;
}
// One workgroup a row of a level.  WRITE = false: the row's candidate count into rows[row]; true: the candidates, in x order, at
// the row's offset (rows[] scanned in between), none beyond the list's capacity.
template <bool WRITE>
__global__ __launch_bounds__(256) void akz_cand_kernel(AkzDev D, float threshold, unsigned* rows, AkzCand* cand, unsigned cap) {
    __shared__ unsigned wsum[4];
    __shared__ unsigned running;
    const int row = blockIdx.x, l = akz_row_level(D, row), y = row - D.row_base[l];
    const AkzLevel& L = D.plan.lv[l];
    const bool live_row = y >= L.border && y < L.h - L.border && L.w > 2 * L.border;
    if (!live_row) { if (!WRITE && threadIdx.x == 0) rows[row] = 0; return; }
    if (WRITE && rows[row] == rows[row + 1]) return;
    const float* ldet = D.plane[l][AKZ_LDET];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) running = WRITE ? rows[row] : 0;
    __syncthreads();
    for (int xb = L.border; xb < L.w - L.border; xb += 256) {
        const int x = xb + threadIdx.x;
        const bool is = x < L.w - L.border && akz_is_candidate(ldet, L.w, L.h, x, y, L.border, threshold);
        const unsigned long long m = __ballot(is);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int k = 0; k < 4; k++) { if (k < wave) before += wsum[k]; total += wsum[k]; }
        const unsigned base = running;
        if (WRITE && is) {
            const unsigned pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < cap) cand[pos] = AkzCand{x, y, l, ldet[(size_t)y * L.w + x]};
        }
        __syncthreads();
        if (threadIdx.x == 0) running = base + total;
        __syncthreads();
    }
    if (!WRITE && threadIdx.x == 0) rows[row] = running;
}
// exclusive scan of the row counts in place, rows[nrows] = counters[0] = the total
__global__ __launch_bounds__(1024) void akz_scan_kernel(unsigned* rows, int nrows, unsigned* counters) {
    __shared__ unsigned part[1024];
    const int tid = threadIdx.x, per = (nrows + 1023) / 1024, b = tid * per, e = min(b + per, nrows);
    unsigned s = 0;
    for (int i = b; i < e; i++) s += rows[i];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    unsigned run = tid ? part[tid - 1] : 0;
    for (int i = b; i < e; i++) { const unsigned c = rows[i]; rows[i] = run; run += c; }
    if (tid == 1023) { rows[nrows] = part[1023]; counters[0] = part[1023]; }
}

__device__ __forceinline__ void akz_count(bool v, unsigned* counter) {      // one atomic a wave
    const unsigned long long m = __ballot(v);
    if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(counter, (unsigned)__popcll(m));
}
// step 6: candidate p is dropped iff a candidate of the levels l - 1 .. l + 1 inside its radius wins over it; the rivals are
// found through the row offsets (rows are the bins: a radius covers a few rows of each level)
__global__ __launch_bounds__(256) void akz_suppress_kernel(AkzDev D, const unsigned* __restrict__ rows, const AkzCand* __restrict__ cand, unsigned cap,
                                                           const unsigned* __restrict__ counters, uint8_t* keep, unsigned* n_kept) {
    const unsigned n = min(counters[0], cap);
    for (unsigned i0 = blockIdx.x * 256; i0 < n; i0 += gridDim.x * 256) {
        const unsigned i = i0 + threadIdx.x;
        bool kept = false;
        if (i < n) {
            const AkzCand p = cand[i];
            const float pr = D.plan.lv[p.level].ratio, rad = D.radius[p.level], py = (float)p.y * pr;
            kept = true;
            for (int l = max(p.level - 1, 0); kept && l <= min(p.level + 1, D.plan.nlev - 1); l++) {
                const AkzLevel& L = D.plan.lv[l];
                const int ya = max((int)floorf((py - rad) / L.ratio), 0), yb = min((int)ceilf((py + rad) / L.ratio), L.h - 1);
                for (int y = ya; kept && y <= yb; y++) {
                    const unsigned b = min(rows[D.row_base[l] + y], n), e = min(rows[D.row_base[l] + y + 1], n);
                    for (unsigned j = b; j < e; j++)
                        if (j != i && akz_suppresses(cand[j], L.ratio, p, pr, rad)) { kept = false; break; }
                }
            }
            keep[i] = kept;
        }
        akz_count(kept, n_kept);
    }
}
struct AkzKp { MisKeyPoint kp; int level; };
__global__ __launch_bounds__(256) void akz_refine_kernel(AkzDev D, const AkzCand* __restrict__ cand, unsigned cap, const unsigned* __restrict__ counters,
                                                         uint8_t* keep, AkzKp* kps, unsigned* n_kept) {
    const unsigned n = min(counters[0], cap);
    for (unsigned i0 = blockIdx.x * 256; i0 < n; i0 += gridDim.x * 256) {
        const unsigned i = i0 + threadIdx.x;
        bool ok = false;
        if (i < n && keep[i]) {
            const AkzCand p = cand[i];
            const AkzLevel& L = D.plan.lv[p.level];
            float dx, dy;
            ok = akz_refine(D.plane[p.level][AKZ_LDET], L.w, p.x, p.y, &dx, &dy);
            if (ok) {
                AkzKp k;
                k.kp.x = ((float)p.x + dx) * L.ratio + 0.5f * (L.ratio - 1.f);
                k.kp.y = ((float)p.y + dy) * L.ratio + 0.5f * (L.ratio - 1.f);
                k.kp.size = 2.f * D.radius[p.level];
                k.kp.angle = 0.f; k.kp.response = p.resp; k.kp.octave = L.octave;
                k.level = p.level;
                kps[i] = k;
            }
            keep[i] = ok;
        }
        akz_count(ok, n_kept);
    }
}
// max_points: a refined keypoint stays iff fewer than max_points others come before it by (response descending, order)
__global__ __launch_bounds__(256) void akz_topk_kernel(const AkzCand* __restrict__ cand, unsigned cap, const unsigned* __restrict__ counters,
                                                       const uint8_t* __restrict__ keep, uint8_t* keep2, int max_points) {
    const unsigned n = min(counters[0], cap);
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    bool ok = keep[i];
    if (ok) {
        const float r = cand[i].resp;
        int before = 0;
        for (unsigned j = 0; j < n && before < max_points; j++)
            if (keep[j] && (cand[j].resp > r || (cand[j].resp == r && j < i))) before++;
        ok = before < max_points;
    }
    keep2[i] = ok;
}
// ordered compaction by one workgroup: the kept keypoints, in candidate order, and their levels; counters[3] = their number
__global__ __launch_bounds__(1024) void akz_compact_kernel(const AkzKp* __restrict__ kps, unsigned cap, unsigned* counters, const uint8_t* __restrict__ keep,
                                                           MisKeyPoint* out, int* levels) {
    __shared__ unsigned wsum[16];
    __shared__ unsigned running;
    const unsigned n = min(counters[0], cap);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) running = 0;
    __syncthreads();
    for (unsigned i0 = 0; i0 < n; i0 += 1024) {
        const unsigned i = i0 + threadIdx.x;
        const bool is = i < n && keep[i];
        const unsigned long long m = __ballot(is);
        if (lane == 0) wsum[wave] = __popcll(m);
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int k = 0; k < 16; k++) { if (k < wave) before += wsum[k]; total += wsum[k]; }
        const unsigned base = running;
        if (is) {
            const unsigned pos = base + before + __popcll(m & ((1ull << lane) - 1ull));
            out[pos] = kps[i].kp;
            levels[pos] = kps[i].level;
        }
        __syncthreads();
        if (threadIdx.x == 0) running = base + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) counters[3] = running;
}

// ------------------------------------------------------------------ orientation, MLDB -----------
// one wave a keypoint: the 13 x 13 grid's samples into LDS, one window a lane, the best window by a wave reduction
__global__ __launch_bounds__(256) void akz_orient_kernel(AkzDev D, MisKeyPoint* kps, const int* __restrict__ levels, const unsigned* __restrict__ counters) {
    __shared__ float srx[4][AKZ_ORI_GRID], sry[4][AKZ_ORI_GRID], sang[4][AKZ_ORI_GRID];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned n = counters[3];
    for (unsigned i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
        const int l = levels[i];
        const AkzLevel& L = D.plan.lv[l];
        const MisKeyPoint kp = kps[i];
        const float xf = kp.x / L.ratio, yf = kp.y / L.ratio;
        const int s = akz_fround(0.5f * kp.size / L.ratio);
        for (int p = lane; p < AKZ_ORI_GRID; p += 64)
            akz_ori_sample(D.plane[l][AKZ_LX], D.plane[l][AKZ_LY], L.w, L.h, xf, yf, s, p, &srx[wave][p], &sry[wave][p], &sang[wave][p]);
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        float sx = 0.f, sy = 0.f, best = -1.f;
        int bk = lane;
        if (lane < AKZ_ORI_WINDOWS) best = akz_window(srx[wave], sry[wave], sang[wave], lane, &sx, &sy);
        for (int off = 32; off > 0; off >>= 1) {
            const float ob = __shfl_xor(best, off), ox = __shfl_xor(sx, off), oy = __shfl_xor(sy, off);
            const int ok = __shfl_xor(bk, off);
            if (ob > best || (ob == best && ok < bk)) { best = ob; sx = ox; sy = oy; bk = ok; }
        }
        // (upstream keeps a window only when its score is above zero: no gradient at all gives angle 0)
        if (lane == 0) kps[i].angle = best > 0.f ? akz_angle_degrees(sx, sy) : 0.f;
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}
// one wave a keypoint: a cell's samples over the lanes and a butterfly sum, the 29 cell triples in LDS, then 64 bits a ballot
__global__ __launch_bounds__(256) void akz_mldb_kernel(AkzDev D, const MisKeyPoint* __restrict__ kps, const int* __restrict__ levels,
                                                       const unsigned* __restrict__ counters, uint8_t* desc) {
    __shared__ float vals[4][3 * AKZ_CELLS + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned n = counters[3];
    for (unsigned i = blockIdx.x * 4 + wave; i < n; i += gridDim.x * 4) {
        const int l = levels[i];
        const AkzLevel& L = D.plan.lv[l];
        const MisKeyPoint kp = kps[i];
        const float xf = kp.x / L.ratio, yf = kp.y / L.ratio, a = kp.angle * (AKZ_PI_F / 180.f), co = cosf(a), si = sinf(a);
        const int s = akz_fround(0.5f * kp.size / L.ratio);
        for (int c = 0; c < AKZ_CELLS; c++) {
            float v[3];
            akz_cell_lane_sums(D.plane[l][AKZ_LT], D.plane[l][AKZ_LX], D.plane[l][AKZ_LY], L.w, L.h, xf, yf, s, co, si, c, lane, 64, v);
            for (int off = 32; off > 0; off >>= 1) {
                v[0] += __shfl_xor(v[0], off); v[1] += __shfl_xor(v[1], off); v[2] += __shfl_xor(v[2], off);
            }
            if (lane == 0) {
                int step, i0, j0;
                akz_cell(c, &step, &i0, &j0);
                const float nsamp = (float)(step * step);
                vals[wave][3 * c] = v[0] / nsamp; vals[wave][3 * c + 1] = v[1] / nsamp; vals[wave][3 * c + 2] = v[2] / nsamp;
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        uint8_t* row = desc + (size_t)i * AKZ_DESC_BYTES;
        for (int t = 0; t < 8; t++) {
            const int b = 64 * t + lane;
            const unsigned long long m = __ballot(b < AKZ_DESC_BITS && akz_bit(vals[wave], b));
            // lanes 0 .. 7 write the eight bytes of this ballot, as far as the row goes
            if (lane < 8 && 8 * t + lane < AKZ_DESC_BYTES) row[8 * t + lane] = (uint8_t)(m >> (8 * lane));
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

}  // namespace

struct MisAkaze {
    MisContext* ctx;
    MisAkazeParams p;
    int max_w, max_h;
    int cur_w = 0, cur_h = 0;
    AkzDev dev;
    uint8_t* mem = nullptr;
    size_t bytes = 0;
    float* scratch = nullptr;       // the other Lt buffer of the FED ping-pong
    unsigned* rows = nullptr;       // candidate count / offset of every row of every level (+ 1)
    unsigned* counters = nullptr;   // [0] candidates [1] after suppression [2] after refinement [3] keypoints; [8 ..] k-contrast stats
    AkzCand* cand = nullptr;
    AkzKp* kps = nullptr;
    uint8_t *keep = nullptr, *keep2 = nullptr;
    MisKeyPoint* okp = nullptr;
    int* olevel = nullptr;
    uint8_t* odesc = nullptr;
    unsigned cap = 0;
    int nrows = 0;
    Taps g0, g1;
    std::vector<float> fed[AKZ_MAX_LEVELS];      // the reordered steps into each level
    unsigned last_counts[4] = {0, 0, 0, 0};      // candidates, after suppression, after refinement, the k-contrast's float bits
    std::vector<int> last_levels;                // class_id of the last detect's keypoints
    bool detected = false;
};

// The keypoint capacity of a frame size: one candidate per 32 pixels of the frame, at least 16384.  A strict
// 3 x 3 maximum above the threshold is far rarer on any image that is not noise; a frame beyond it is refused with the count.
static unsigned akaze_capacity(int w, int h) { return (unsigned)std::max<size_t>(16384, (size_t)w * h / 32); }

static int akaze_plan(MisAkaze* s, int w, int h) {
    AkzDev& D = s->dev;
    if (!akz_plan(w, h, s->p.n_octaves, s->p.n_octave_layers, &D.plan)) return MIS_E_UNSUPPORTED;
    size_t off = 0;
    auto carve = [&](size_t b) { size_t o = off; off += mis_align_up(b, 256); return s->mem ? s->mem + o : (uint8_t*)nullptr; };
    int rows = 0;
    for (int l = 0; l < D.plan.nlev; l++) {
        AkzLevel& L = D.plan.lv[l];
        for (int k = 0; k < AKZ_PLANES; k++) D.plane[l][k] = (float*)carve(sizeof(float) * (size_t)L.w * L.h);
        D.row_base[l] = rows;
        rows += L.h;
        D.radius[l] = L.esigma * 1.5f;
        s->fed[l].clear();
        if (l > 0) {
            float tau[AKZ_MAX_FED];
            const int n = akz_fed_schedule(akz_etime(s->p.n_octave_layers, D.plan.lv[l - 1].octave, D.plan.lv[l - 1].sublevel),
                                           akz_etime(s->p.n_octave_layers, L.octave, L.sublevel), tau);
            if (n < 1 || n > AKZ_MAX_FED) return MIS_E_UNSUPPORTED;
            s->fed[l].assign(tau, tau + n);
            L.nsteps = n;
        }
    }
    D.row_base[D.plan.nlev] = rows;
    s->nrows = rows;
    s->cap = akaze_capacity(w, h);
    s->scratch = (float*)carve(sizeof(float) * (size_t)w * h);
    s->rows = (unsigned*)carve(sizeof(unsigned) * (size_t)(rows + 1));
    s->counters = (unsigned*)carve(sizeof(unsigned) * (8 + 2 + AKZ_HIST_BINS));
    s->cand = (AkzCand*)carve(sizeof(AkzCand) * s->cap);
    s->kps = (AkzKp*)carve(sizeof(AkzKp) * s->cap);
    s->keep = carve(s->cap);
    s->keep2 = carve(s->cap);
    s->okp = (MisKeyPoint*)carve(sizeof(MisKeyPoint) * s->cap);
    s->olevel = (int*)carve(sizeof(int) * s->cap);
    s->odesc = carve((size_t)AKZ_DESC_BYTES * s->cap);
    s->bytes = off;
    s->cur_w = w; s->cur_h = h;
    return MIS_OK;
}

extern "C" void mis_akaze_default_params(MisAkazeParams* p) {
    if (!p) return;
    p->threshold = 0.001f; p->n_octaves = 4; p->n_octave_layers = 4; p->max_points = -1;
    p->descriptor_type = MIS_AKAZE_DESCRIPTOR_MLDB; p->descriptor_size = 0; p->descriptor_channels = 3; p->diffusivity = MIS_AKAZE_DIFF_PM_G2;
}

extern "C" int mis_akaze_create(MisContext* ctx, const MisAkazeParams* params, int max_width, int max_height, MisAkaze** out) {
    if (!ctx || !out) return MIS_E_INVALID;
    *out = nullptr;
    MisAkazeParams p;
    mis_akaze_default_params(&p);
    if (params) p = *params;
    MIS_CHECK(ctx, p.descriptor_type == MIS_AKAZE_DESCRIPTOR_MLDB, MIS_E_UNSUPPORTED, "AKAZE: only the MLDB descriptor (rotation invariant) is built");
    MIS_CHECK(ctx, p.diffusivity == MIS_AKAZE_DIFF_PM_G2, MIS_E_UNSUPPORTED, "AKAZE: only the PM-G2 diffusivity is built");
    MIS_CHECK(ctx, p.descriptor_size == 0 && p.descriptor_channels == 3, MIS_E_UNSUPPORTED, "AKAZE: only the full 486-bit, 3-channel descriptor is built");
    MIS_CHECK(ctx, p.n_octaves >= 1 && p.n_octaves <= 6 && p.n_octave_layers >= 1 && p.n_octave_layers <= 8 && p.n_octaves * p.n_octave_layers <= AKZ_MAX_LEVELS &&
                       p.threshold >= 0.f && p.max_points != 0,
              MIS_E_INVALID, "AKAZE: bad parameters (1 .. 6 octaves, 1 .. 8 layers, at most %d levels, threshold >= 0, max_points -1 or > 0)", AKZ_MAX_LEVELS);
    MIS_CHECK(ctx, max_width >= 16 && max_height >= 16 && max_width <= 16384 && max_height <= 16384, MIS_E_INVALID, "AKAZE: image size out of range");
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    MisAkaze* s = new MisAkaze();
    s->ctx = ctx; s->p = p; s->max_w = max_width; s->max_h = max_height;
    s->g0.n = akz_gauss_taps(1.6, s->g0.k);
    s->g1.n = akz_gauss_taps(1.0, s->g1.k);
    int rc = akaze_plan(s, max_width, max_height);      // sizes only (mem == nullptr)
    if (rc != MIS_OK) { delete s; return mis_set_error(ctx, rc, "AKAZE: the parameters need a FED cycle of more than %d steps", AKZ_MAX_FED); }
    const size_t need = s->bytes;
    if (hipMalloc((void**)&s->mem, need) != hipSuccess) { delete s; return mis_set_error(ctx, MIS_E_HIP, "AKAZE: cannot allocate %zu bytes of scale space", need); }
    akaze_plan(s, max_width, max_height);
    *out = s;
    return MIS_OK;
}

extern "C" int mis_akaze_destroy(MisAkaze* s) {
    if (!s) return MIS_OK;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    if (s->mem) hipFree(s->mem);
    delete s;
    return MIS_OK;
}

template <int MODE>
static void launch_start(hipStream_t st, const void* src, size_t stride, int sw, int sh, float* start, float* smooth, int w, int h, const Taps& t) {
    const dim3 grid((w + TW - 1) / TW, (h + TH - 1) / TH), block(256);
    const float sx = (float)sw / (float)w, sy = (float)sh / (float)h;
    if (t.n == 9) hipLaunchKernelGGL((akz_start_kernel<MODE, 4>), grid, block, 0, st, src, stride, sw, sh, sx, sy, start, smooth, w, h, t);
    else hipLaunchKernelGGL((akz_start_kernel<MODE, 2>), grid, block, 0, st, src, stride, sw, sh, sx, sy, start, smooth, w, h, t);
}

extern "C" int mis_akaze_detect(MisAkaze* s, const MisImage* bgr, MisFeatures* out) {
    if (!s) return MIS_E_INVALID;
    MisContext* ctx = s->ctx;
    MIS_CHECK(ctx, bgr && out && bgr->data, MIS_E_INVALID, "null argument");
    MIS_CHECK(ctx, bgr->dtype == MIS_U8 && bgr->channels == 3, MIS_E_UNSUPPORTED, "AKAZE input must be 8UC3 (BGR)");
    MIS_CHECK(ctx, bgr->width >= 16 && bgr->height >= 16 && bgr->width <= s->max_w && bgr->height <= s->max_h, MIS_E_INVALID,
              "image %dx%d outside the detector's range (16x16 .. %dx%d)", bgr->width, bgr->height, s->max_w, s->max_h);
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevView din;
    int rc;
    if ((rc = din.read(ctx, bgr)) != MIS_OK) return rc;
    const int w = bgr->width, h = bgr->height;
    s->detected = false;
    if (w != s->cur_w || h != s->cur_h) {
        MIS_HIP(ctx, hipStreamSynchronize(st));
        rc = akaze_plan(s, w, h);
        MIS_CHECK(ctx, rc == MIS_OK, rc, "AKAZE: cannot plan a %dx%d frame", w, h);
    }
    const AkzDev& D = s->dev;
    const int nlev = D.plan.nlev;
    unsigned* stats = s->counters + 8;
    MIS_HIP(ctx, hipMemsetAsync(s->counters, 0, sizeof(unsigned) * (8 + 2 + AKZ_HIST_BINS), st));
    for (int l = 0; l < nlev; l++) {
        const AkzLevel& L = D.plan.lv[l];
        const dim3 rows((L.w + 255) / 256, L.h), block(256), tiles((L.w + TW - 1) / TW, (L.h + TH - 1) / TH);
        float* lt = D.plane[l][AKZ_LT];
        if (l == 0) {
            launch_start<0>(st, din.data, din.stride, w, h, lt, D.plane[0][AKZ_LSMOOTH], L.w, L.h, s->g0);
            if (L.w > 2 && L.h > 2) {
                const dim3 inner((L.w - 2 + 255) / 256, L.h - 2);
                hipLaunchKernelGGL(akz_hmax_kernel, inner, block, 0, st, (const float*)D.plane[0][AKZ_LSMOOTH], L.w, L.h, stats);
                hipLaunchKernelGGL(akz_hist_kernel, inner, block, 0, st, (const float*)D.plane[0][AKZ_LSMOOTH], L.w, L.h, stats);
            }
            hipLaunchKernelGGL(akz_kcontrast_kernel, dim3(1), dim3(64), 0, st, stats);
            // (level 0 is not diffused: its flow plane is there so that every level has one for mis_akaze_debug_level)
            hipLaunchKernelGGL(akz_flow_kernel, rows, block, 0, st, (const float*)D.plane[0][AKZ_LSMOOTH], D.plane[0][AKZ_FLOW], L.w, L.h, (const unsigned*)stats, 0);
        } else {
            const AkzLevel& Pv = D.plan.lv[l - 1];
            const std::vector<float>& tau = s->fed[l];
            // the start lands where an even number of steps away is Lt[l]
            float* a = (tau.size() & 1) ? s->scratch : lt;
            float* b = (tau.size() & 1) ? lt : s->scratch;
            if (Pv.octave != L.octave) launch_start<2>(st, D.plane[l - 1][AKZ_LT], 0, Pv.w, Pv.h, a, D.plane[l][AKZ_LSMOOTH], L.w, L.h, s->g1);
            else launch_start<1>(st, D.plane[l - 1][AKZ_LT], 0, Pv.w, Pv.h, a, D.plane[l][AKZ_LSMOOTH], L.w, L.h, s->g1);
            hipLaunchKernelGGL(akz_flow_kernel, rows, block, 0, st, (const float*)D.plane[l][AKZ_LSMOOTH], D.plane[l][AKZ_FLOW], L.w, L.h, (const unsigned*)stats, L.octave);
            for (size_t k = 0; k < tau.size(); k++) {
                hipLaunchKernelGGL(akz_fed_kernel, tiles, block, 0, st, (const float*)a, (const float*)D.plane[l][AKZ_FLOW], b, L.w, L.h, tau[k] / L.tau_div);
                std::swap(a, b);
            }
        }
        hipLaunchKernelGGL(akz_deriv1_kernel, rows, block, 0, st, (const float*)D.plane[l][AKZ_LSMOOTH], D.plane[l][AKZ_LX], D.plane[l][AKZ_LY], L.w, L.h, L.sigma_size);
        hipLaunchKernelGGL(akz_deriv2_kernel, rows, block, 0, st, (const float*)D.plane[l][AKZ_LX], (const float*)D.plane[l][AKZ_LY], D.plane[l][AKZ_LDET], L.w, L.h,
                           L.sigma_size);
    }
    const int grid = 8 * ctx->num_cu;
    hipLaunchKernelGGL(akz_cand_kernel<false>, dim3(s->nrows), dim3(256), 0, st, D, s->p.threshold, s->rows, s->cand, s->cap);
    hipLaunchKernelGGL(akz_scan_kernel, dim3(1), dim3(1024), 0, st, s->rows, s->nrows, s->counters);
    hipLaunchKernelGGL(akz_cand_kernel<true>, dim3(s->nrows), dim3(256), 0, st, D, s->p.threshold, s->rows, s->cand, s->cap);
    hipLaunchKernelGGL(akz_suppress_kernel, dim3(grid), dim3(256), 0, st, D, (const unsigned*)s->rows, (const AkzCand*)s->cand, s->cap, (const unsigned*)s->counters, s->keep,
                       s->counters + 1);
    hipLaunchKernelGGL(akz_refine_kernel, dim3(grid), dim3(256), 0, st, D, (const AkzCand*)s->cand, s->cap, (const unsigned*)s->counters, s->keep, s->kps, s->counters + 2);
    const uint8_t* keep = s->keep;
    if (s->p.max_points > 0) {
        hipLaunchKernelGGL(akz_topk_kernel, dim3((s->cap + 255) / 256), dim3(256), 0, st, (const AkzCand*)s->cand, s->cap, (const unsigned*)s->counters, (const uint8_t*)s->keep,
                           s->keep2, s->p.max_points);
        keep = s->keep2;
    }
    hipLaunchKernelGGL(akz_compact_kernel, dim3(1), dim3(1024), 0, st, (const AkzKp*)s->kps, s->cap, s->counters, keep, s->okp, s->olevel);
    hipLaunchKernelGGL(akz_orient_kernel, dim3(grid), dim3(256), 0, st, D, s->okp, (const int*)s->olevel, (const unsigned*)s->counters);
    hipLaunchKernelGGL(akz_mldb_kernel, dim3(grid), dim3(256), 0, st, D, (const MisKeyPoint*)s->okp, (const int*)s->olevel, (const unsigned*)s->counters, s->odesc);
    MIS_HIP(ctx, hipGetLastError());
    // the one host read of a detect: the counts (the keypoint count sizes the output block)
    unsigned counts[10] = {0};      // [0 .. 3] the counters, [9] the k-contrast
    MIS_HIP(ctx, hipMemcpyAsync(counts, s->counters, sizeof(counts), hipMemcpyDeviceToHost, st));
    MIS_HIP(ctx, hipStreamSynchronize(st));
    MIS_CHECK(ctx, counts[0] <= s->cap, MIS_E_OVERFLOW, "AKAZE: %u candidates exceed the capacity %u of a %dx%d frame", counts[0], s->cap, w, h);
    const int n = (int)counts[3];
    memset(out, 0, sizeof(*out));
    out->img_w = w; out->img_h = h; out->desc_cols = AKZ_DESC_BYTES; out->desc_dtype = MIS_U8;
    const size_t kb = mis_align_up(sizeof(MisKeyPoint) * (size_t)std::max(n, 1), 256), db = (size_t)AKZ_DESC_BYTES * std::max(n, 1);
    uint8_t* blk = nullptr;
    if ((rc = mis_feat_block_alloc(ctx, kb + db, (void**)&blk)) != MIS_OK) return rc;
    out->owner_ = blk; out->keypoints = (MisKeyPoint*)blk; out->descriptors = blk + kb; out->n = n;
    s->last_levels.assign((size_t)n, 0);
    if (n) {
        MIS_HIP(ctx, hipMemcpyAsync(out->keypoints, s->okp, sizeof(MisKeyPoint) * (size_t)n, hipMemcpyDeviceToDevice, st));
        MIS_HIP(ctx, hipMemcpyAsync(out->descriptors, s->odesc, (size_t)AKZ_DESC_BYTES * n, hipMemcpyDeviceToDevice, st));
        MIS_HIP(ctx, hipMemcpyAsync(s->last_levels.data(), s->olevel, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
        MIS_HIP(ctx, hipStreamSynchronize(st));      // (the finder's buffers are the next detect's)
    }
    s->last_counts[0] = counts[0]; s->last_counts[1] = counts[1]; s->last_counts[2] = counts[2]; s->last_counts[3] = counts[9];
    s->detected = true;
    return MIS_OK;
}

extern "C" int mis_akaze_detect_batch(MisAkaze* s, const MisImage* imgs, int n, MisFeatures* out) {
    if (!s) return MIS_E_INVALID;
    MIS_CHECK(s->ctx, imgs && out && n >= 1, MIS_E_INVALID, "null argument");
    for (int i = 0; i < n; i++) {
        const int rc = mis_akaze_detect(s, &imgs[i], &out[i]);
        if (rc != MIS_OK) {
            for (int k = 0; k < i; k++) mis_features_free(s->ctx, &out[k]);
            return rc;
        }
        out[i].img_idx = i;
    }
    return MIS_OK;
}

extern "C" int mis_akaze_debug_level(MisAkaze* s, int level, int which, float* host_out, int* width, int* height) {
    if (!s) return MIS_E_INVALID;
    MisContext* ctx = s->ctx;
    MIS_CHECK(ctx, width && height, MIS_E_INVALID, "null argument");
    MIS_CHECK(ctx, s->detected, MIS_E_STATE, "mis_akaze_debug_level: no detect before it");
    MIS_CHECK(ctx, level >= 0 && level < s->dev.plan.nlev && which >= 0 && which < AKZ_PLANES, MIS_E_INVALID, "bad level / plane");
    const AkzLevel& L = s->dev.plan.lv[level];
    *width = L.w; *height = L.h;
    if (host_out) {
        MIS_HIP(ctx, hipSetDevice(ctx->device));
        MIS_HIP(ctx, hipMemcpyAsync(host_out, s->dev.plane[level][which], sizeof(float) * (size_t)L.w * L.h, hipMemcpyDeviceToHost, ctx->stream));
        MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return MIS_OK;
}

extern "C" int mis_akaze_debug_counts(MisAkaze* s, unsigned* counts4) {
    if (!s) return MIS_E_INVALID;
    MIS_CHECK(s->ctx, counts4, MIS_E_INVALID, "null argument");
    MIS_CHECK(s->ctx, s->detected, MIS_E_STATE, "mis_akaze_debug_counts: no detect before it");
    memcpy(counts4, s->last_counts, sizeof(s->last_counts));
    return MIS_OK;
}

extern "C" int mis_akaze_debug_class_ids(MisAkaze* s, int* host_out, int capacity) {
    if (!s) return MIS_E_INVALID;
    MIS_CHECK(s->ctx, host_out && capacity >= (int)s->last_levels.size(), MIS_E_INVALID, "mis_akaze_debug_class_ids: room for %d ids, %zu keypoints", capacity,
              s->last_levels.size());
    if (!s->last_levels.empty()) memcpy(host_out, s->last_levels.data(), sizeof(int) * s->last_levels.size());
    return MIS_OK;
}

extern "C" int mis_akaze_debug_fed(MisAkaze* s, int level, float* taus, int* n) {
    if (!s) return MIS_E_INVALID;
    MIS_CHECK(s->ctx, n && level >= 0 && level < s->dev.plan.nlev, MIS_E_INVALID, "bad level");
    const std::vector<float>& t = s->fed[level];
    *n = (int)t.size();
    if (taus && !t.empty()) memcpy(taus, t.data(), sizeof(float) * t.size());
    return MIS_OK;
}
