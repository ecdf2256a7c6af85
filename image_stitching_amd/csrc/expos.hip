// expos.hip -- exposure compensation, in the step between warp and blend:
//   ExposureCompensator::createDefault(expos_comp_type) + setNrFeeds(expos_comp_nr_feeds) / setNrGainsFilteringIterations(2) /
//   setBlockSize(64, 64): GAIN, GAIN_BLOCKS (the reference's default, with one feed), CHANNELS, CHANNELS_BLOCKS,
//   feed(corners, images_warped, masks_warped)                    image_stitching/image_stitching.cpp:1002-1023
//   compensator->apply(img_idx, corners[img_idx], img_warped, mask_warped)                       image_stitching.cpp:1162
// The seam finders of the same step are seam_voronoi.hip, seam.hip and seam_gc.hip.
//
// Division of labour.  The overlap statistics (one wave per pair of overlapping 64x64 blocks: pixel count and the two
// sums of BGR norms, accumulated in the reference's row-major order so that the doubles agree bit for bit), the
// per-pixel gain application run on the device; the normal
// equations of the gains (a dense LU solve with partial pivoting over a few hundred blocks) and the 3-tap
// smoothing of the tiny gain maps are host work, as in the reference.
//
// The whole-frame members (GAIN, CHANNELS) cannot use that kernel: one wave would walk a 0.1 MP overlap serially.  Their
// statistics come from frame_stats_kernel, whose grid runs over (pair, strip of rows) with full waves and whose sums are
// integers, so they do not depend on the order of the additions: the intersect count, for CHANNELS the per-channel sums of both
// frames, and for GAIN the sum of norms of both frames EXACTLY (exact_sum.h: every correctly rounded double square root is an
// integer below 2^61 in units of 2^-52, added limb by limb into 64-bit counters and rounded once on the host).  That sum is the
// same in every run and for every memory form and equals the exactly rounded sum of the norms (Python's math.fsum) bit for bit;
// OpenCV's running double sum, which rounds once per pixel, differs from it by at most count * 2^-53 relative.  GAIN_BLOCKS keeps
// its ordered kernel; CHANNELS_BLOCKS (integer sums: any order is exact) uses the strip kernel over the block pairs.
// With nr_feeds > 1 the feeds after the first run on private device copies multiplied by the previous feed's gains
// (cv::multiply(8U image, double scalar) works in float32: saturate_cast<uchar>(cvRound((float)v * (float)g))); the copies stay on
// the device and only the counters come back, one copy and one wait per feed.  The caller's images are never altered by a feed.
#include "common.h"
#include "dev_math.h"
#include "exact_sum.h"
#include "seam_plan.h"      // seam_overlap: the rectangle two units share
#include <float.h>
#include <math.h>
#include <algorithm>
#include <vector>

namespace {

struct ImgDesc {
    const uint8_t* img; size_t istride;
    const uint8_t* msk; size_t mstride;
    int cx, cy, w, h;
};
struct PairDesc { int a, b, x0, y0, x1, y1; };   // images a, b and the pano rectangle the two blocks share
struct PairStat { double s1, s2; int cnt, pad; };

// GainCompensator::singleFeed inner loop: intersect = both masks 255; N = count; Isum += norm(BGR).
// One wave per pair.  The 64 lanes fetch 64 consecutive pixels of the row-major scan, take the (correctly rounded)
// double square roots in parallel and then the wave adds them in lane order, which is the order of the scalar loop
// (a pixel outside the intersection contributes +0.0, which leaves a non-negative sum unchanged).
__global__ __launch_bounds__(256) void overlap_stats_kernel(const ImgDesc* __restrict__ imgs, const PairDesc* __restrict__ pairs, int npairs,
                                                            PairStat* __restrict__ out) {
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (p >= npairs) return;
    const PairDesc pd = pairs[p];
    const ImgDesc A = imgs[pd.a], B = imgs[pd.b];
    const int rw = pd.x1 - pd.x0, total = rw * (pd.y1 - pd.y0);
    double s1 = 0, s2 = 0;
    int cnt = 0;
    for (int base = 0; base < total; base += 64) {
        const int q = base + lane;
        double v1 = 0, v2 = 0;
        bool ok = false;
        if (q < total) {
            const int y = pd.y0 + q / rw, x = pd.x0 + q % rw;
            const size_t ya = (size_t)(y - A.cy), xa = (size_t)(x - A.cx), yb = (size_t)(y - B.cy), xb = (size_t)(x - B.cx);
            ok = A.msk[ya * A.mstride + xa] == 255 && B.msk[yb * B.mstride + xb] == 255;
            if (ok) {
                const uint8_t* u = A.img + ya * A.istride + 3 * xa;
                const uint8_t* v = B.img + yb * B.istride + 3 * xb;
                v1 = sqrt((double)(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]));
                v2 = sqrt((double)(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
            }
        }
        cnt += __popcll(__ballot(ok));
        for (int l = 0; l < 64; l++) {
            s1 += __shfl(v1, l);
            s2 += __shfl(v2, l);
        }
    }
    if (lane == 0) { out[p].s1 = s1; out[p].s2 = s2; out[p].cnt = cnt; out[p].pad = 0; }
}

// Order-free statistics of the pairs, whole frames or blocks: grid (pair, strip of STRIP_ROWS rows of the shared rectangle), 256
// threads over the strip's pixels in row-major order.  out[pair * STAT_WORDS + k], zeroed by the caller:
//   k = 0 the intersect count;
//   NORMS:    1, 2 the low and high limb sums of image a's norms (exact_sum.h), 3, 4 those of image b;
//   CHANNELS: 1..3 the B, G, R sums of image a, 4..6 those of image b.
// Per lane in registers, then across the wave, then one integer atomicAdd per wave and counter: integers, so any order is exact.
constexpr int STRIP_ROWS = 8, STAT_WORDS = 8;
enum { STATS_NORMS = 0, STATS_CHANNELS = 1 };
template <int MODE>
__global__ __launch_bounds__(256) void frame_stats_kernel(const ImgDesc* __restrict__ imgs, const PairDesc* __restrict__ pairs, unsigned long long* __restrict__ out) {
    constexpr int NW = MODE == STATS_NORMS ? 5 : 7;
    const int p = blockIdx.x;
    const PairDesc pd = pairs[p];
    const int rw = pd.x1 - pd.x0, r0 = blockIdx.y * STRIP_ROWS;
    if (r0 >= pd.y1 - pd.y0) return;
    const int total = rw * (min(r0 + STRIP_ROWS, pd.y1 - pd.y0) - r0);
    const ImgDesc A = imgs[pd.a], B = imgs[pd.b];
    unsigned long long acc[NW];
#pragma unroll
    for (int k = 0; k < NW; k++) acc[k] = 0;
    for (int q = threadIdx.x; q < total; q += 256) {
        const int y = pd.y0 + r0 + q / rw, x = pd.x0 + q % rw;
        const size_t ya = (size_t)(y - A.cy), xa = (size_t)(x - A.cx), yb = (size_t)(y - B.cy), xb = (size_t)(x - B.cx);
        if (A.msk[ya * A.mstride + xa] != 255 || B.msk[yb * B.mstride + xb] != 255) continue;
        const uint8_t* u = A.img + ya * A.istride + 3 * xa;
        const uint8_t* v = B.img + yb * B.istride + 3 * xb;
        acc[0]++;
        if (MODE == STATS_NORMS) {
            // sqrt >= 1 or 0: times 2^52 it is an integer below 2^61, exactly
            const unsigned long long t1 = (unsigned long long)(sqrt((double)(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])) * MIS_EXACT_SCALE);
            const unsigned long long t2 = (unsigned long long)(sqrt((double)(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])) * MIS_EXACT_SCALE);
            acc[1] += t1 & 0xffffffffull; acc[2] += t1 >> 32;
            acc[3] += t2 & 0xffffffffull; acc[4] += t2 >> 32;
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) { acc[1 + k] += u[k]; acc[4 + k] += v[k]; }
        }
    }
#pragma unroll
    for (int k = 0; k < NW; k++) {
        unsigned long long a = acc[k];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
        if ((threadIdx.x & 63) == 0 && a) atomicAdd(out + (size_t)p * STAT_WORDS + k, a);
    }
}

// cv::multiply(image, scalar gain) per unit (a whole frame: uw = w, uh = h, or the blocks of the frame's grid), the gain or
// the three gains of a unit at g[unit * gc ..]: saturate_cast<uchar>(cvRound((float)v * (float)g)).  Runs on the private copies
// between feeds and on the caller's image in mis_compensator_apply for GAIN and CHANNELS.
template <typename T>
__global__ __launch_bounds__(256) void unit_gain_kernel(T* __restrict__ img, size_t stride_elems, int w, int h, const float* __restrict__ g, int gc, int uw, int uh, int mw) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const float* gu = g + (size_t)((y / uh) * mw + x / uw) * gc;
    T* p = img + (size_t)y * stride_elems + 3 * (size_t)x;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int v = mis_round_f((float)p[k] * gu[gc == 3 ? k : 0]);
        p[k] = (T)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

// BlocksCompensator::apply: gain map -> resize(INTER_LINEAR, float) -> multiply(image, gains, image): one thread per pixel;
// MC = 1: one map for the three channels (GAIN_BLOCKS), MC = 3: an interleaved map per channel (CHANNELS_BLOCKS)
template <typename T, int MC>
__global__ __launch_bounds__(256) void gain_apply_kernel(T* __restrict__ img, size_t stride_elems, int w, int h, const float* __restrict__ map, int mw, int mh,
                                                         double sx, double sy) {
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    float fy = (float)(((double)y + 0.5) * sy - 0.5);
    int iy = mis_floor_f(fy);
    fy -= (float)iy;
    if (iy < 0) { iy = 0; fy = 0.f; }
    if (iy >= mh - 1) { iy = mh - 1; fy = 0.f; }
    const int iy1 = iy + 1 < mh ? iy + 1 : iy;
    float fx = (float)(((double)x + 0.5) * sx - 0.5);
    int ix = mis_floor_f(fx);
    fx -= (float)ix;
    if (ix < 0) { ix = 0; fx = 0.f; }
    if (ix >= mw - 1) { ix = mw - 1; fx = 0.f; }
    const int ix1 = ix + 1 < mw ? ix + 1 : ix;
    float g[MC];
#pragma unroll
    for (int c = 0; c < MC; c++) {
        const float h0 = map[(iy * mw + ix) * MC + c] * (1.f - fx) + map[(iy * mw + ix1) * MC + c] * fx;
        const float h1 = map[(iy1 * mw + ix) * MC + c] * (1.f - fx) + map[(iy1 * mw + ix1) * MC + c] * fx;
        g[c] = h0 * (1.f - fy) + h1 * fy;
    }
    T* p = img + (size_t)y * stride_elems + 3 * (size_t)x;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int v = mis_round_f((float)p[k] * g[MC == 3 ? k : 0]);
        p[k] = (T)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

// core/src/lapack.cpp LUImpl<double> as cv::solve(A, b, x, DECOMP_LU) drives it: partial pivoting, eps = 100 * DBL_EPSILON
bool solve_lu(std::vector<double>& A, std::vector<double>& b, int m) {
    const double eps = DBL_EPSILON * 100;
    for (int i = 0; i < m; i++) {
        int k = i;
        for (int j = i + 1; j < m; j++) if (fabs(A[(size_t)j * m + i]) > fabs(A[(size_t)k * m + i])) k = j;
        if (fabs(A[(size_t)k * m + i]) < eps) return false;
        if (k != i) {
            for (int j = i; j < m; j++) std::swap(A[(size_t)i * m + j], A[(size_t)k * m + j]);
            std::swap(b[i], b[k]);
        }
        const double d = -1 / A[(size_t)i * m + i];
        const double* ri = &A[(size_t)i * m];
        for (int j = i + 1; j < m; j++) {
            double* rj = &A[(size_t)j * m];
            const double alpha = rj[i] * d;
            for (int c = i + 1; c < m; c++) rj[c] += alpha * ri[c];
            b[j] += alpha * b[i];
        }
    }
    for (int i = m - 1; i >= 0; i--) {
        double s = b[i];
        for (int k = i + 1; k < m; k++) s -= A[(size_t)i * m + k] * b[k];
        b[i] = s / A[(size_t)i * m + i];
    }
    return true;
}

inline int reflect101(int p, int len) {
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p;
    return p;
}

struct Block { int x, y, w, h, img; };

}  // namespace

struct MisCompensator {
    MisContext* ctx = nullptr;
    int type = MIS_EXPOS_GAIN_BLOCKS, nr_feeds = 1;
    int bw = 64, bh = 64, nfilt = 2;
    int n = 0;
    int mc = 1;                        // channels of a map / gains per unit: 3 for the channel types
    // block types: the smoothed maps (mc interleaved channels); GAIN / CHANNELS: one 1 x 1 three-channel "map" per image, the
    // float gains that apply() multiplies by
    std::vector<std::vector<float>> maps;
    std::vector<int> mw, mh;
    float* dev_maps = nullptr;         // all maps back to back
    size_t dev_maps_cap = 0;           // floats allocated
    std::vector<size_t> dev_ofs;
    std::vector<double> gains;         // GAIN / CHANNELS: n x 3 accumulated gains
    // GAIN / CHANNELS, the last feed: [channel][i * n + j]
    std::vector<int> dbg_N;
    std::vector<double> dbg_I;
};

namespace {

bool blocks_type(int type) { return type == MIS_EXPOS_GAIN_BLOCKS || type == MIS_EXPOS_CHANNELS_BLOCKS; }
bool channels_type(int type) { return type == MIS_EXPOS_CHANNELS || type == MIS_EXPOS_CHANNELS_BLOCKS; }

// GainCompensator::singleFeed after the pixel loops: N, I, then the normal equations over the units that meet another unit.
// cnt: raw intersect counts; s1, s2: the sums of unit i's and unit j's values over the intersection, per pair
void solve_gains(int nb, const std::vector<std::pair<int, int>>& pair_ij, const int* cnt_, const double* s1, const double* s2, std::vector<double>& gains,
                 std::vector<int>* N_out = nullptr, std::vector<double>* I_out = nullptr) {
    const int np = (int)pair_ij.size();
    std::vector<int> N((size_t)nb * nb, 0);
    std::vector<double> I((size_t)nb * nb, 0.0);
    std::vector<char> skip(nb, 1);
    for (int p = 0; p < np; p++) {
        const int i = pair_ij[p].first, j = pair_ij[p].second, cnt = std::max(1, cnt_[p]);
        N[(size_t)i * nb + j] = N[(size_t)j * nb + i] = cnt;
        if (i != j) skip[i] = skip[j] = 0;
        I[(size_t)i * nb + j] = s1[p] / cnt;
        I[(size_t)j * nb + i] = s2[p] / cnt;
    }
    gains.assign(nb, 1.0);
    int neq = 0;
    for (int i = 0; i < nb; i++) neq += !skip[i];
    if (neq > 0) {
        const double alpha = 0.01, beta = 100;
        std::vector<double> A((size_t)neq * neq, 0.0), b(neq, 0.0);
        for (int i = 0, ki = 0; i < nb; i++) {
            if (skip[i]) continue;
            for (int j = 0, kj = 0; j < nb; j++) {
                if (skip[j]) continue;
                const double nij = N[(size_t)i * nb + j], iij = I[(size_t)i * nb + j], iji = I[(size_t)j * nb + i];
                b[ki] += beta * nij;
                A[(size_t)ki * neq + ki] += beta * nij;
                if (j != i) {
                    A[(size_t)ki * neq + ki] += 2 * alpha * iij * iij * nij;
                    A[(size_t)ki * neq + kj] -= 2 * alpha * iij * iji * nij;
                }
                kj++;
            }
            ki++;
        }
        if (solve_lu(A, b, neq))
            for (int i = 0, j = 0; i < nb; i++) if (!skip[i]) gains[i] = b[j++];
    }
    if (N_out) *N_out = std::move(N);
    if (I_out) *I_out = std::move(I);
}

// nfilt passes of the separable [1 2 1] / 4 (BORDER_REFLECT_101) over a one-channel map
void smooth_map(std::vector<float>& m, int mw, int mh, int nfilt) {
    std::vector<float> t((size_t)mw * mh);
    for (int it = 0; it < nfilt; it++) {
        for (int y = 0; y < mh; y++)
            for (int x = 0; x < mw; x++) t[y * mw + x] = (m[y * mw + reflect101(x - 1, mw)] + m[y * mw + reflect101(x + 1, mw)]) * 0.25f + m[y * mw + x] * 0.5f;
        for (int y = 0; y < mh; y++)
            for (int x = 0; x < mw; x++) m[y * mw + x] = (t[reflect101(y - 1, mh) * mw + x] + t[reflect101(y + 1, mh) * mw + x]) * 0.25f + t[y * mw + x] * 0.5f;
    }
}

// c->maps -> the device: the device copy is grow-only (a free + malloc per feed synchronises the device twice) and filled by ONE
// copy from the context's pinned staging
int upload_maps(MisCompensator* c) {
    MisContext* ctx = c->ctx;
    size_t total = 0;
    c->dev_ofs.assign(c->n, 0);
    for (int i = 0; i < c->n; i++) { c->dev_ofs[i] = total; total += c->maps[i].size(); }
    if (c->dev_maps_cap < total) {
        if (c->dev_maps) { MIS_HIP(ctx, hipStreamSynchronize(ctx->stream)); MIS_HIP(ctx, hipFree(c->dev_maps)); c->dev_maps = nullptr; c->dev_maps_cap = 0; }
        MIS_HIP(ctx, hipMalloc(&c->dev_maps, (total + total / 2) * sizeof(float)));
        c->dev_maps_cap = total + total / 2;
    }
    void* hs = nullptr;
    int rcs = mis_host_stage(ctx, total * sizeof(float), &hs);
    if (rcs != MIS_OK) return rcs;
    for (int i = 0; i < c->n; i++) memcpy((float*)hs + c->dev_ofs[i], c->maps[i].data(), c->maps[i].size() * sizeof(float));
    MIS_HIP(ctx, hipMemcpyAsync(c->dev_maps, hs, total * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the staging buffer is reusable when this returns
    return MIS_OK;
}

// one gain per block (and channel) -> a small float map per image, every channel smoothed on its own
int maps_from_block_gains(MisCompensator* c, const std::vector<double>* gains /* [mc] */) {
    for (int i = 0, q = 0; i < c->n; i++) {
        const int mw = c->mw[i], mh = c->mh[i], nbk = mw * mh;
        std::vector<float> out((size_t)nbk * c->mc), m(nbk);
        for (int ch = 0; ch < c->mc; ch++) {
            for (int k = 0; k < nbk; k++) m[k] = (float)gains[ch][q + k];
            smooth_map(m, mw, mh, c->nfilt);
            for (int k = 0; k < nbk; k++) out[(size_t)k * c->mc + ch] = m[k];
        }
        q += nbk;
        c->maps[i] = std::move(out);
    }
    return upload_maps(c);
}

// the units of a feed: the blocks of every image (BlocksCompensator::feed) or the frames themselves, and the pairs i <= j whose
// rectangles intersect
void make_units(MisCompensator* c, const MisPoint* corners, const MisImage* images, int n, std::vector<Block>& B, std::vector<PairDesc>& pairs,
                std::vector<std::pair<int, int>>& pair_ij) {
    c->n = n; c->mw.assign(n, 1); c->mh.assign(n, 1); c->maps.assign(n, {});
    for (int i = 0; i < n; i++) {
        const int W = images[i].width, H = images[i].height;
        if (!blocks_type(c->type)) { B.push_back({corners[i].x, corners[i].y, W, H, i}); continue; }
        c->mw[i] = (W + c->bw - 1) / c->bw; c->mh[i] = (H + c->bh - 1) / c->bh;
        const int bw = (W + c->mw[i] - 1) / c->mw[i], bh = (H + c->mh[i] - 1) / c->mh[i];
        for (int by = 0; by < c->mh[i]; by++)
            for (int bx = 0; bx < c->mw[i]; bx++) {
                const int ox = bx * bw, oy = by * bh;
                B.push_back({corners[i].x + ox, corners[i].y + oy, std::min(ox + bw, W) - ox, std::min(oy + bh, H) - oy, i});
            }
    }
    const int nb = (int)B.size();
    for (int i = 0; i < nb; i++)
        for (int j = i; j < nb; j++) {
            SeamRect r;
            if (seam_overlap(SeamFrame{B[i].x, B[i].y, B[i].w, B[i].h}, SeamFrame{B[j].x, B[j].y, B[j].w, B[j].h}, &r)) { pairs.push_back({B[i].img, B[j].img, r.x0, r.y0, r.x1, r.y1}); pair_ij.emplace_back(i, j); }
        }
}

// GAIN_BLOCKS with one feed: the reference's configuration
int feed_blocks_once(MisCompensator* c, const MisPoint* corners, const MisImage* images, const MisImage* masks, int n) {
    MisContext* ctx = c->ctx;
    std::vector<Block> B;
    std::vector<PairDesc> pairs;
    std::vector<std::pair<int, int>> pair_ij;
    make_units(c, corners, images, n, B, pairs, pair_ij);
    const int nb = (int)B.size(), np = (int)pairs.size();

    std::vector<PairStat> stats(np);
    {   // the staged frames live until the statistics are on the host
        std::vector<DevView> di(n), dm(n);
        std::vector<ImgDesc> desc(n);
        int rc;
        for (int i = 0; i < n; i++) {
            if ((rc = di[i].read(ctx, &images[i])) != MIS_OK || (rc = dm[i].read(ctx, &masks[i])) != MIS_OK) return rc;
            desc[i] = {(const uint8_t*)di[i].data, di[i].stride, (const uint8_t*)dm[i].data, dm[i].stride, corners[i].x, corners[i].y, images[i].width, images[i].height};
        }
        const size_t b_desc = mis_align_up(sizeof(ImgDesc) * n, 256), b_pairs = mis_align_up(sizeof(PairDesc) * np, 256), b_stats = sizeof(PairStat) * np;
        void* buf = nullptr; size_t got = 0;
        if ((rc = mis_pool_alloc(ctx, b_desc + b_pairs + b_stats, &buf, &got)) != MIS_OK) return rc;
        char* p = (char*)buf;
        hipError_t e = hipMemcpyAsync(p, desc.data(), sizeof(ImgDesc) * n, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(p + b_desc, pairs.data(), sizeof(PairDesc) * np, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(overlap_stats_kernel, dim3((np + 3) / 4), dim3(256), 0, ctx->stream, (const ImgDesc*)p, (const PairDesc*)(p + b_desc), np,
                               (PairStat*)(p + b_desc + b_pairs));
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(stats.data(), p + b_desc + b_pairs, b_stats, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        mis_pool_free(ctx, buf, got);
        if (e != hipSuccess) return mis_set_error(ctx, MIS_E_HIP, "compensator feed: %s", hipGetErrorString(e));
    }
    std::vector<int> cnt(np);
    std::vector<double> s1(np), s2(np), gains;
    for (int p = 0; p < np; p++) { cnt[p] = stats[p].cnt; s1[p] = stats[p].s1; s2[p] = stats[p].s2; }
    solve_gains(nb, pair_ij, cnt.data(), s1.data(), s2.data(), gains);
    return maps_from_block_gains(c, &gains);
}

// Every other member of the family and every nr_feeds: statistics -> gains -> (not after the last feed) the copies multiplied by
// the gains, nr_feeds times; the result is the product of the feeds' gains.
int feed_family(MisCompensator* c, const MisPoint* corners, const MisImage* images, const MisImage* masks, int n) {
    MisContext* ctx = c->ctx;
    std::vector<Block> B;
    std::vector<PairDesc> pairs;
    std::vector<std::pair<int, int>> pair_ij;
    make_units(c, corners, images, n, B, pairs, pair_ij);
    const int nb = (int)B.size(), np = (int)pairs.size(), mc = c->mc;
    const bool ordered = c->type == MIS_EXPOS_GAIN_BLOCKS, frames = !blocks_type(c->type);
    int max_rows = 1;
    for (const PairDesc& pd : pairs) max_rows = std::max(max_rows, pd.y1 - pd.y0);

    std::vector<DevView> di(n), dm(n);
    std::vector<ImgDesc> desc(n);
    int rc;
    // device layout: descriptors | pairs | statistics | float gains of every unit | the private copies (dense rows), feeds > 1 only
    const size_t b_desc = mis_align_up(sizeof(ImgDesc) * n, 256), b_pairs = mis_align_up(sizeof(PairDesc) * np, 256);
    const size_t b_stats = mis_align_up(ordered ? sizeof(PairStat) * np : sizeof(unsigned long long) * STAT_WORDS * np, 256);
    const size_t b_gains = mis_align_up(sizeof(float) * nb * mc, 256);
    std::vector<size_t> copy_ofs(n, 0);
    size_t b_copies = 0;
    if (c->nr_feeds > 1)
        for (int i = 0; i < n; i++) { copy_ofs[i] = b_copies; b_copies += mis_align_up((size_t)images[i].width * 3 * images[i].height, 256); }
    for (int i = 0; i < n; i++)
        if ((rc = di[i].read(ctx, &images[i])) != MIS_OK || (rc = dm[i].read(ctx, &masks[i])) != MIS_OK) return rc;
    void* hs = nullptr;        // pinned: [statistics | gains]
    if ((rc = mis_host_stage(ctx, b_stats + b_gains, &hs)) != MIS_OK) return rc;
    void* buf = nullptr; size_t got = 0;
    if ((rc = mis_pool_alloc(ctx, b_desc + b_pairs + b_stats + b_gains + b_copies, &buf, &got)) != MIS_OK) return rc;
    char* p = (char*)buf;
    char* d_stats = p + b_desc + b_pairs;
    float* d_gains = (float*)(d_stats + b_stats);
    uint8_t* d_copies = (uint8_t*)d_gains + b_gains;
    hipError_t e = hipSuccess;
    for (int i = 0; i < n; i++) {
        const uint8_t* img = (const uint8_t*)di[i].data;
        size_t stride = di[i].stride;
        if (c->nr_feeds > 1) {
            const size_t row = (size_t)images[i].width * 3;
            if (e == hipSuccess) e = hipMemcpy2DAsync(d_copies + copy_ofs[i], row, di[i].data, di[i].stride, row, images[i].height, hipMemcpyDeviceToDevice, ctx->stream);
            img = d_copies + copy_ofs[i];
            stride = row;
        }
        desc[i] = {img, stride, (const uint8_t*)dm[i].data, dm[i].stride, corners[i].x, corners[i].y, images[i].width, images[i].height};
    }
    if (e == hipSuccess) e = hipMemcpyAsync(p, desc.data(), sizeof(ImgDesc) * n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p + b_desc, pairs.data(), sizeof(PairDesc) * np, hipMemcpyHostToDevice, ctx->stream);

    std::vector<double> acc[3], g[3], s1(np), s2(np);
    std::vector<int> cnt(np);
    for (int ch = 0; ch < mc; ch++) acc[ch].assign(nb, 1.0);
    if (frames) { c->dbg_N.assign((size_t)mc * n * n, 0); c->dbg_I.assign((size_t)mc * n * n, 0.0); }
    for (int feed = 0; feed < c->nr_feeds && e == hipSuccess; feed++) {
        if (ordered) {
            hipLaunchKernelGGL(overlap_stats_kernel, dim3((np + 3) / 4), dim3(256), 0, ctx->stream, (const ImgDesc*)p, (const PairDesc*)(p + b_desc), np, (PairStat*)d_stats);
        } else {
            e = hipMemsetAsync(d_stats, 0, b_stats, ctx->stream);
            if (e != hipSuccess) break;
            const dim3 grid(np, (max_rows + STRIP_ROWS - 1) / STRIP_ROWS);
            if (mc == 3)
                hipLaunchKernelGGL(frame_stats_kernel<STATS_CHANNELS>, grid, dim3(256), 0, ctx->stream, (const ImgDesc*)p, (const PairDesc*)(p + b_desc), (unsigned long long*)d_stats);
            else
                hipLaunchKernelGGL(frame_stats_kernel<STATS_NORMS>, grid, dim3(256), 0, ctx->stream, (const ImgDesc*)p, (const PairDesc*)(p + b_desc), (unsigned long long*)d_stats);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(hs, d_stats, b_stats, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);      // the one wait of this feed
        if (e != hipSuccess) break;
        for (int ch = 0; ch < mc; ch++) {
            for (int q = 0; q < np; q++) {
                if (ordered) {
                    const PairStat& st = ((const PairStat*)hs)[q];
                    cnt[q] = st.cnt; s1[q] = st.s1; s2[q] = st.s2;
                } else {
                    const unsigned long long* w = (const unsigned long long*)hs + (size_t)q * STAT_WORDS;
                    cnt[q] = (int)w[0];
                    if (mc == 3) { s1[q] = (double)w[1 + ch]; s2[q] = (double)w[4 + ch]; }      // below 2^53: exact
                    else { s1[q] = mis_limbs_to_double(w[1], w[2]); s2[q] = mis_limbs_to_double(w[3], w[4]); }
                }
            }
            std::vector<int> N;
            std::vector<double> I;
            solve_gains(nb, pair_ij, cnt.data(), s1.data(), s2.data(), g[ch], frames ? &N : nullptr, frames ? &I : nullptr);
            for (int u = 0; u < nb; u++) acc[ch][u] *= g[ch][u];
            if (frames) {
                std::copy(N.begin(), N.end(), c->dbg_N.begin() + (size_t)ch * n * n);
                std::copy(I.begin(), I.end(), c->dbg_I.begin() + (size_t)ch * n * n);
            }
        }
        if (feed + 1 == c->nr_feeds) break;
        // the next feed sees the copies multiplied by this feed's (unsmoothed, per-unit) gains, in float32
        float* hg = (float*)((char*)hs + b_stats);
        for (int u = 0; u < nb; u++)
            for (int ch = 0; ch < mc; ch++) hg[(size_t)u * mc + ch] = (float)g[ch][u];
        e = hipMemcpyAsync(d_gains, hg, sizeof(float) * nb * mc, hipMemcpyHostToDevice, ctx->stream);
        for (int i = 0, u0 = 0; i < n && e == hipSuccess; i++) {
            const int W = images[i].width, H = images[i].height, mw = c->mw[i], mh = c->mh[i];
            hipLaunchKernelGGL(unit_gain_kernel<uint8_t>, dim3((W + 255) / 256, H), dim3(256), 0, ctx->stream, d_copies + copy_ofs[i], (size_t)W * 3, W, H,
                               d_gains + (size_t)u0 * mc, mc, (W + mw - 1) / mw, (H + mh - 1) / mh, mw);
            e = hipGetLastError();
            u0 += mw * mh;
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    mis_pool_free(ctx, buf, got);
    if (e != hipSuccess) return mis_set_error(ctx, MIS_E_HIP, "compensator feed: %s", hipGetErrorString(e));

    if (!frames) return maps_from_block_gains(c, acc);
    c->gains.assign((size_t)n * 3, 1.0);
    for (int i = 0; i < n; i++) {
        c->maps[i].resize(3);
        for (int k = 0; k < 3; k++) {
            c->gains[(size_t)i * 3 + k] = acc[mc == 3 ? k : 0][i];
            c->maps[i][k] = (float)c->gains[(size_t)i * 3 + k];
        }
    }
    return upload_maps(c);
}

}  // namespace

extern "C" void mis_compensator_default_params(MisCompensatorParams* params) {
    if (!params) return;
    params->type = MIS_EXPOS_GAIN_BLOCKS;
    params->nr_feeds = 1;
    params->block_width = params->block_height = 64;
    params->nr_gain_filtering_iterations = 2;
}

extern "C" int mis_compensator_create_ex(MisContext* ctx, const MisCompensatorParams* params, MisCompensator** out) {
    if (!ctx || !out) return MIS_E_INVALID;
    MIS_CHECK(ctx, params, MIS_E_INVALID, "compensator: null parameters");
    MIS_CHECK(ctx, params->type >= MIS_EXPOS_GAIN && params->type <= MIS_EXPOS_CHANNELS_BLOCKS, MIS_E_INVALID,
              "compensator: type %d (GAIN 1, GAIN_BLOCKS 2, CHANNELS 3, CHANNELS_BLOCKS 4; NO needs no compensator)", params->type);
    MIS_CHECK(ctx, params->nr_feeds >= 1, MIS_E_INVALID, "compensator: %d feeds", params->nr_feeds);
    if (blocks_type(params->type))
        MIS_CHECK(ctx, params->block_width > 0 && params->block_height > 0 && params->nr_gain_filtering_iterations >= 0, MIS_E_INVALID,
                  "compensator: block %dx%d, %d filtering passes", params->block_width, params->block_height, params->nr_gain_filtering_iterations);
    MisCompensator* c = new MisCompensator();
    c->ctx = ctx; c->type = params->type; c->nr_feeds = params->nr_feeds;
    c->bw = params->block_width; c->bh = params->block_height; c->nfilt = params->nr_gain_filtering_iterations;
    c->mc = channels_type(c->type) ? 3 : 1;
    *out = c;
    return MIS_OK;
}

extern "C" int mis_compensator_create(MisContext* ctx, int block_w, int block_h, int nr_filtering, MisCompensator** out) {
    const MisCompensatorParams params = {MIS_EXPOS_GAIN_BLOCKS, 1, block_w, block_h, nr_filtering};
    return mis_compensator_create_ex(ctx, &params, out);
}

extern "C" int mis_compensator_destroy(MisCompensator* c) {
    if (!c) return MIS_OK;
    if (c->dev_maps) { hipSetDevice(c->ctx->device); hipStreamSynchronize(c->ctx->stream); hipFree(c->dev_maps); }
    delete c;
    return MIS_OK;
}

extern "C" int mis_compensator_feed(MisCompensator* c, const MisPoint* corners, const MisImage* images, const MisImage* masks, int n) {
    if (!c) return MIS_E_INVALID;
    MisContext* ctx = c->ctx;
    MIS_CHECK(ctx, corners && images && masks && n > 0, MIS_E_INVALID, "compensator feed: null argument or no images");
    for (int i = 0; i < n; i++) {
        MIS_CHECK(ctx, images[i].data && images[i].dtype == MIS_U8 && images[i].channels == 3, MIS_E_UNSUPPORTED, "compensator feed: image %d is not 8UC3", i);
        MIS_CHECK(ctx, masks[i].data && masks[i].dtype == MIS_U8 && masks[i].channels == 1 && masks[i].width == images[i].width && masks[i].height == images[i].height,
                  MIS_E_INVALID, "compensator feed: mask %d does not match its image", i);
    }
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    if (c->type == MIS_EXPOS_GAIN_BLOCKS && c->nr_feeds == 1) return feed_blocks_once(c, corners, images, masks, n);
    return feed_family(c, corners, images, masks, n);
}

extern "C" int mis_compensator_gains(const MisCompensator* c, int index, double gains[3]) {
    if (!c) return MIS_E_INVALID;
    MIS_CHECK(c->ctx, !blocks_type(c->type), MIS_E_UNSUPPORTED, "compensator: a block type has a gain map, not per-image gains");
    MIS_CHECK(c->ctx, gains && index >= 0 && index < c->n, MIS_E_INVALID, "compensator: image index %d out of range (fed %d)", index, c->n);
    for (int k = 0; k < 3; k++) gains[k] = c->gains[(size_t)index * 3 + k];
    return MIS_OK;
}

extern "C" int mis_compensator_gain_map_channels(const MisCompensator* c, int index, float* map_host, int capacity, int* blocks_x, int* blocks_y, int* channels) {
    if (!c) return MIS_E_INVALID;
    MIS_CHECK(c->ctx, blocks_type(c->type), MIS_E_UNSUPPORTED, "compensator: GAIN and CHANNELS have per-image gains, not a gain map");
    MIS_CHECK(c->ctx, index >= 0 && index < c->n, MIS_E_INVALID, "compensator: image index %d out of range (fed %d)", index, c->n);
    if (blocks_x) *blocks_x = c->mw[index];
    if (blocks_y) *blocks_y = c->mh[index];
    if (channels) *channels = c->mc;
    if (map_host) {
        MIS_CHECK(c->ctx, capacity >= (int)c->maps[index].size(), MIS_E_INVALID, "compensator: gain map needs %zu floats", c->maps[index].size());
        memcpy(map_host, c->maps[index].data(), c->maps[index].size() * sizeof(float));
    }
    return MIS_OK;
}

extern "C" int mis_compensator_gain_map(const MisCompensator* c, int index, float* map_host, int capacity, int* blocks_x, int* blocks_y) {
    if (!c) return MIS_E_INVALID;
    MIS_CHECK(c->ctx, c->type == MIS_EXPOS_GAIN_BLOCKS, MIS_E_UNSUPPORTED, "compensator: one-channel gain maps are GAIN_BLOCKS' (mis_compensator_gain_map_channels)");
    return mis_compensator_gain_map_channels(c, index, map_host, capacity, blocks_x, blocks_y, nullptr);
}

extern "C" int mis_compensator_debug_stats(const MisCompensator* c, int i, int j, int channel, int* N, double* I_ij, double* I_ji) {
    if (!c) return MIS_E_INVALID;
    MIS_CHECK(c->ctx, !blocks_type(c->type), MIS_E_UNSUPPORTED, "compensator: debug statistics are GAIN's and CHANNELS'");
    MIS_CHECK(c->ctx, i >= 0 && i < c->n && j >= 0 && j < c->n && channel >= 0 && channel < c->mc, MIS_E_INVALID,
              "compensator: pair (%d, %d) channel %d out of range (fed %d, %d channels)", i, j, channel, c->n, c->mc);
    const size_t base = (size_t)channel * c->n * c->n, n = c->n;
    if (N) *N = c->dbg_N[base + i * n + j];
    if (I_ij) *I_ij = c->dbg_I[base + i * n + j];
    if (I_ji) *I_ji = c->dbg_I[base + j * n + i];
    return MIS_OK;
}

extern "C" int mis_compensator_apply(MisCompensator* c, int index, MisImage* image) {
    if (!c) return MIS_E_INVALID;
    MisContext* ctx = c->ctx;
    MIS_CHECK(ctx, index >= 0 && index < c->n, MIS_E_INVALID, "compensator: image index %d out of range (fed %d)", index, c->n);
    MIS_CHECK(ctx, image && image->data && image->channels == 3 && (image->dtype == MIS_U8 || image->dtype == MIS_S16), MIS_E_UNSUPPORTED,
              "compensator apply: 8UC3 or 16SC3 (values 0..255) only");
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    DevView d;
    int rc;
    if ((rc = d.read_write(ctx, image)) != MIS_OK) return rc;
    const int w = image->width, h = image->height, mw = c->mw[index], mh = c->mh[index];
    const float* map = c->dev_maps + c->dev_ofs[index];
    // resize(): inv_scale = dsize / ssize, scale = 1 / inv_scale
    const double sx = 1.0 / ((double)w / (double)mw), sy = 1.0 / ((double)h / (double)mh);
    dim3 grid((w + 255) / 256, h), block(256);
    const bool u8 = image->dtype == MIS_U8;
    if (!blocks_type(c->type)) {        // GAIN / CHANNELS: the image's three float gains
        if (u8) hipLaunchKernelGGL(unit_gain_kernel<uint8_t>, grid, block, 0, ctx->stream, (uint8_t*)d.data, d.stride, w, h, map, 3, w, h, 1);
        else hipLaunchKernelGGL(unit_gain_kernel<int16_t>, grid, block, 0, ctx->stream, (int16_t*)d.data, d.stride / 2, w, h, map, 3, w, h, 1);
    } else if (c->mc == 1) {
        if (u8) hipLaunchKernelGGL((gain_apply_kernel<uint8_t, 1>), grid, block, 0, ctx->stream, (uint8_t*)d.data, d.stride, w, h, map, mw, mh, sx, sy);
        else hipLaunchKernelGGL((gain_apply_kernel<int16_t, 1>), grid, block, 0, ctx->stream, (int16_t*)d.data, d.stride / 2, w, h, map, mw, mh, sx, sy);
    } else {
        if (u8) hipLaunchKernelGGL((gain_apply_kernel<uint8_t, 3>), grid, block, 0, ctx->stream, (uint8_t*)d.data, d.stride, w, h, map, mw, mh, sx, sy);
        else hipLaunchKernelGGL((gain_apply_kernel<int16_t, 3>), grid, block, 0, ctx->stream, (int16_t*)d.data, d.stride / 2, w, h, map, mw, mh, sx, sy);
    }
    MIS_HIP(ctx, hipGetLastError());
    return d.commit();
}
