// seam_gc.hip -- GraphCutSeamFinder(COST_COLOR), the seam finder of the reference's try_cuda branch and of OpenCV's own stitcher:
//   seam_finder = makePtr<detail::GraphCutSeamFinderGpu>(GraphCutSeamFinderBase::COST_COLOR)      image_stitching.cpp:1037-1054
//   seam_finder->find(images_warped_f, corners, masks_warped)                                     image_stitching.cpp:1065
// restated from the published algorithm ([OpenCV-upstream, recalled]): per overlapping pair, in
// PairwiseSeamFinder::run order, a 4-connected grid graph over the roi grown by 10 pixels with integer capacities, cut by a
// maximum flow; the pixels of the source side leave image 2's mask, the others image 1's.  The labels are the MINIMAL source side
// (the nodes the source reaches in the residual graph), which is the same set for every maximum flow: the result is a property of
// the input and is pinned bit for bit to the numpy / scipy reference tests/refimpl_seam_graphcut.py (tests/test_seam_graphcut_gpu.py).
//
// The whole finder runs on the device, on gathered copies of the images and masks (the packed block and the input contract of
// seam_stage.h, shared with seam.hip).  The pairs of one dependency level of the pair plan (seam_plan.h, in run order: pairs that
// share no image; a pair waits for every earlier pair that shares one with it) go into one set of launches
// with the pair on the grid's y; levels follow each other in stream order.  Per level:
//   gc_build_kernel          a thread a node: four capacities, the terminal, the start state
//   gc_relabel_init_kernel   | the global relabel: exact distances to a drain in the residual graph by relaxation sweeps, a tile
//   gc_relabel_sweep_kernel  | relaxed to its fixpoint in LDS per sweep, sweeps repeated until one changes nothing
//   gc_count_kernel          the nodes with excess that still reach a drain: none left -> the preflow is maximal
//   gc_round_kernel          a round set: GC_INNER synchronous push / relabel rounds of a 32 x 32 tile in LDS; pushes over the
//   gc_absorb_kernel         tile's border go to an outbox plane, which the absorb launch behind it empties
//   gc_writeback_kernel      the two mask rules over the roi
// Only the first phase of push-relabel runs, on the REVERSED problem (the grid edges are symmetric): excess starts at the sink
// terminals and drains at the source terminals; when no node with excess reaches a drain any more, the nodes that still reach
// one are the nodes the source reaches in the residual graph of a maximum flow.  Heights only steer the pushes: whatever they
// are, a push keeps the preflow a preflow, and the decision to stop is taken on the exact distances of a global relabel, so
// stale halo heights cost rounds, never correctness.
// No kernel waits for another workgroup, every device loop has a compile-time bound, and the host bounds the launches
// (GC_SET_CAP round sets a level, a sweep bound from the grid's size): a bug gives a wrong mask or MIS_E_INTERNAL, not a hang.
#include "common.h"
#include "seam_gc_core.h"
#include "seam_stage.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int GC_K = 8;                 // round sets between two global relabels (and two host reads of the counts)
constexpr int GC_SWEEP_BATCH = 16;      // relabel sweeps between two host reads of their change flags (a settled sweep leaves after one step)
// Hard cap on the round sets of a level: 16 x the worst count observed -- 128 on config 3's 54 pairs, 32 on the test scenes
// (profiles/seam_graphcut_v1.json).
constexpr int GC_SET_CAP = 2048;

// the counters of a level, in device memory, copied to the pinned job block before every host read
struct GcCounters {
    int* active;        // [pair] the gate of every launch but the build: 0 when the pair is finished (its count as of the last SETTLED relabel)
    int* count;         // [pair] nodes with excess and a height below hmax, as of the last sweep batch
    int* set_active;    // [GC_K][pair] active nodes (by the heights of the moment) at the end of each round set
    int* changed;       // [GC_SWEEP_BATCH] tiles that a sweep changed
};

__global__ __launch_bounds__(256) void gc_build_kernel(const GcPair* __restrict__ pairs, const GcPlanes G, int* active, float terminal_cost, float penalty) {
    const GcPair P = pairs[blockIdx.y];
    if (blockIdx.x == 0 && threadIdx.x == 0) active[blockIdx.y] = 1;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P.gw * P.gh) return;
    const int gy = k / P.gw;
    gc_build_node(P, G, terminal_cost, penalty, k - gy * P.gw, gy);
}

__global__ __launch_bounds__(256) void gc_relabel_init_kernel(const GcPair* __restrict__ pairs, const GcPlanes G, const int* __restrict__ active) {
    if (!active[blockIdx.y]) return;
    const GcPair P = pairs[blockIdx.y];
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= P.gw * P.gh) return;
    G.height[(size_t)P.base + k] = G.drain[(size_t)P.base + k] > 0 ? 1 : P.hmax;
}

// One sweep of the global relabel: the tile's heights (with the halo as the last sweep left it) are relaxed to their fixpoint in
// LDS -- at most GC_TN steps, the longest path inside a tile.
__global__ __launch_bounds__(GC_TN) void gc_relabel_sweep_kernel(const GcPair* __restrict__ pairs, const GcPlanes G, const int* __restrict__ active, int* changed) {
    if (!active[blockIdx.y]) return;
    const GcPair P = pairs[blockIdx.y];
    if ((int)blockIdx.x >= P.tiles_x * P.tiles_y) return;
    __shared__ int hs[GC_HS * GC_HS];
    const int ty = blockIdx.x / P.tiles_x, tx = blockIdx.x - ty * P.tiles_x;
    const int tx0 = tx * GC_T, ty0 = ty * GC_T;
    for (int i = threadIdx.x; i < GC_HS * GC_HS; i += GC_TN) gc_load_height(P, G, tx0, ty0, i, hs);
    const int lx = threadIdx.x % GC_T, ly = threadIdx.x / GC_T;
    const int gx = tx0 + lx, gy = ty0 + ly;
    const bool in = gx < P.gw && gy < P.gh;
    const size_t k = (size_t)P.base + (size_t)gy * P.gw + gx;
    int r[4] = {0, 0, 0, 0};
    if (in)
        for (int d = 0; d < 4; d++) r[d] = G.res[d][k];
    __syncthreads();
    const int c = gc_hs_at(lx, ly);
    const int h0 = hs[c];
    int h = h0;
    for (int it = 0; it < GC_TN; it++) {
        const int nh = in ? gc_relax(r, h, hs, lx, ly) : h;
        if (!__syncthreads_or(nh < h)) break;
        hs[c] = nh; h = nh;
        __syncthreads();
    }
    const bool moved = in && h != h0;
    if (moved) G.height[k] = h;
    if (__syncthreads_or(moved) && threadIdx.x == 0) atomicAdd(changed, 1);
}

// grid (1, pairs): the pair's nodes with excess whose height is below hmax
__global__ __launch_bounds__(GC_TN) void gc_count_kernel(const GcPair* __restrict__ pairs, const GcPlanes G, const int* __restrict__ active, int* count) {
    if (!active[blockIdx.y]) return;
    const GcPair P = pairs[blockIdx.y];
    __shared__ int total;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    int n = 0;
    const int V = P.gw * P.gh;
    for (int k = threadIdx.x; k < V; k += GC_TN) n += G.excess[(size_t)P.base + k] > 0 && G.height[(size_t)P.base + k] < P.hmax;
    if (n) atomicAdd(&total, n);
    __syncthreads();
    if (threadIdx.x == 0) count[blockIdx.y] = total;
}

// behind a settled global relabel: a pair without active nodes is finished, no later launch of the level touches it
__global__ __launch_bounds__(64) void gc_gate_kernel(int* active, const int* __restrict__ count, int np) {
    for (int q = threadIdx.x; q < np; q += 64) active[q] = count[q];
}

// A round set on one tile.  A tile without excess leaves at once; the rounds end early when no node of the tile can move.
__global__ __launch_bounds__(GC_TN) void gc_round_kernel(const GcPair* __restrict__ pairs, const GcPlanes G, const int* __restrict__ active) {
    if (!active[blockIdx.y]) return;
    const GcPair P = pairs[blockIdx.y];
    if ((int)blockIdx.x >= P.tiles_x * P.tiles_y) return;
    __shared__ int hs[GC_HS * GC_HS];
    __shared__ int ps[4 * GC_TN];
    const int ty = blockIdx.x / P.tiles_x, tx = blockIdx.x - ty * P.tiles_x;
    const int tx0 = tx * GC_T, ty0 = ty * GC_T;
    const int lx = threadIdx.x % GC_T, ly = threadIdx.x / GC_T;
    GcNode s;
    gc_node_load(P, G, tx0 + lx, ty0 + ly, s);
    if (!__syncthreads_or(s.in && s.e > 0)) return;
    for (int i = threadIdx.x; i < GC_HS * GC_HS; i += GC_TN) gc_load_height(P, G, tx0, ty0, i, hs);
    __syncthreads();
    const int c = gc_hs_at(lx, ly);
    for (int r = 0; r < GC_INNER; r++) {
        gc_push(s, hs, ps, lx, ly, P.hmax);
        __syncthreads();
        gc_absorb_relabel(s, hs, ps, lx, ly, P.hmax);
        __syncthreads();
        hs[c] = s.h;
        if (!__syncthreads_or(s.in && s.e > 0 && (s.h < P.hmax || s.drain > 0))) break;
    }
    gc_node_store(P, G, tx0 + lx, ty0 + ly, s);
}

__global__ __launch_bounds__(256) void gc_absorb_kernel(const GcPair* __restrict__ pairs, const GcPlanes G, const int* __restrict__ active, int* set_active) {
    if (!active[blockIdx.y]) return;
    const GcPair P = pairs[blockIdx.y];
    const int k = blockIdx.x * 256 + threadIdx.x;
    if ((int)(blockIdx.x * 256) >= P.gw * P.gh) return;
    bool act = false;
    if (k < P.gw * P.gh) { const int gy = k / P.gw; act = gc_border_absorb(P, G, k - gy * P.gw, gy); }
    const int n = __syncthreads_count(act);
    if (n && threadIdx.x == 0) atomicAdd(&set_active[blockIdx.y], n);
}

// over the roi (not the gap): in S and mask1 set -> mask2 cleared; not in S and mask2 set -> mask1 cleared
__global__ __launch_bounds__(256) void gc_writeback_kernel(const GcPair* __restrict__ pairs, const GcPlanes G) {
    const GcPair P = pairs[blockIdx.y];
    const int rw = P.gw - 2 * GC_GAP, rh = P.gh - 2 * GC_GAP;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= rw * rh) return;
    const int y = k / rw, x = k - y * rw;
    const int gx = x + GC_GAP, gy = y + GC_GAP;
    const bool in_s = G.height[(size_t)P.base + (size_t)gy * P.gw + gx] < P.hmax;
    // a roi pixel lies inside both images
    uint8_t* m1 = P.mask1 + (size_t)(gy + P.oy1) * P.w1 + (gx + P.ox1);
    uint8_t* m2 = P.mask2 + (size_t)(gy + P.oy2) * P.w2 + (gx + P.ox2);
    const bool s1 = *m1 != 0, s2 = *m2 != 0;
    if (in_s && s1) *m2 = 0;
    if (!in_s && s2) *m1 = 0;
}

struct GcDebug {        // mis_seam_graphcut_debug_pair: the one pair to run, and where its planes go
    int i, j;
    int32_t* cap_right; int32_t* cap_down; int32_t* terminals; uint8_t* labels;
    size_t capacity_elems;
    int* grid_w; int* grid_h;
};

struct HostPair { int i, j, level; GcPair p; };

int gc_find(MisContext* ctx, const MisPoint* corners, const MisImage* images, MisImage* masks, int n, float terminal_cost, float penalty, const GcDebug* dbg) {
    // everything is checked before anything is staged or written
    for (int i = 0; i < n; i++) {
        const MisImage& I = images[i];
        if (int rc = seam_check_input(ctx, I, masks[i], i)) return rc;
        MIS_CHECK(ctx, I.width <= 32000 && I.height <= 32000 && std::abs((long long)corners[i].x) < (1 << 28) && std::abs((long long)corners[i].y) < (1 << 28),
                  MIS_E_UNSUPPORTED, "image %d: %dx%d at (%d, %d) is beyond the graph-cut finder's 32-bit node indices", i, I.width, I.height, corners[i].x, corners[i].y);
    }
    if (dbg) MIS_CHECK(ctx, dbg->i >= 0 && dbg->j > dbg->i && dbg->j < n, MIS_E_INVALID, "debug pair (%d, %d) of %d images: need 0 <= i < j < n", dbg->i, dbg->j, n);
    if (n == 0) return MIS_OK;
    MIS_HIP(ctx, hipSetDevice(ctx->device));

    // the pair plan in PairwiseSeamFinder::run order; the debug entry plans its one pair alone
    std::vector<SeamFrame> frames = seam_frames(corners, images, n);
    if (dbg) frames = {frames[dbg->i], frames[dbg->j]};
    const SeamPlan plan = seam_plan(frames, SEAM_ORDER_RUN);
    const int nlevels = plan.nlevels;
    std::vector<HostPair> work;
    for (const SeamPair& sp : plan.pairs) {
        const int i = dbg ? dbg->i : sp.i, j = dbg ? dbg->j : sp.j;
        const SeamRect& r = sp.roi;
        HostPair hp{};
        hp.i = i; hp.j = j; hp.level = sp.level;
        GcPair& p = hp.p;
        p.w1 = images[i].width; p.h1 = images[i].height; p.w2 = images[j].width; p.h2 = images[j].height;
        p.ox1 = r.x0 - GC_GAP - corners[i].x; p.oy1 = r.y0 - GC_GAP - corners[i].y; p.ox2 = r.x0 - GC_GAP - corners[j].x; p.oy2 = r.y0 - GC_GAP - corners[j].y;
        p.gw = r.x1 - r.x0 + 2 * GC_GAP; p.gh = r.y1 - r.y0 + 2 * GC_GAP;
        p.tiles_x = (p.gw + GC_T - 1) / GC_T; p.tiles_y = (p.gh + GC_T - 1) / GC_T;
        MIS_CHECK(ctx, (long long)p.gw * p.gh < (1 << 29), MIS_E_UNSUPPORTED, "pair (%d, %d): a grid of %dx%d nodes is beyond 32-bit node indices", i, j, p.gw, p.gh);
        p.hmax = p.gw * p.gh + 2;
        work.push_back(hp);
    }
    if (dbg) {
        MIS_CHECK(ctx, !work.empty(), MIS_E_INVALID, "debug pair (%d, %d): the images do not overlap", dbg->i, dbg->j);
        *dbg->grid_w = work[0].p.gw; *dbg->grid_h = work[0].p.gh;
        if (dbg->capacity_elems == 0) return MIS_OK;       // a query of the grid's size
        MIS_CHECK(ctx, dbg->capacity_elems >= (size_t)work[0].p.gw * work[0].p.gh && dbg->cap_right && dbg->cap_down && dbg->terminals && dbg->labels, MIS_E_INVALID,
                  "debug pair (%d, %d): the grid is %dx%d, the planes hold %zu elements", dbg->i, dbg->j, work[0].p.gw, work[0].p.gh, dbg->capacity_elems);
    }
    std::stable_sort(work.begin(), work.end(), [](const HostPair& a, const HostPair& b) { return a.level < b.level; });
    // per level: its pairs, their node bases, the largest node and tile count of a pair (the launches' x extent)
    std::vector<int> lv_first((size_t)nlevels + 1, 0), lv_nodes((size_t)nlevels, 0), lv_maxv((size_t)nlevels, 0), lv_maxt((size_t)nlevels, 0), lv_maxroi((size_t)nlevels, 0);
    long long plane_elems = 1, total_nodes = 0;
    int max_pairs = 1;
    for (size_t k = 0; k < work.size(); k++) {
        const int l = work[k].level - 1;
        GcPair& p = work[k].p;
        MIS_CHECK(ctx, (long long)lv_nodes[l] + p.gw * p.gh < (1 << 30), MIS_E_UNSUPPORTED, "level %d holds more than 2^30 graph nodes", l + 1);
        p.base = lv_nodes[l];
        lv_nodes[l] += p.gw * p.gh;
        lv_maxv[l] = std::max(lv_maxv[l], p.gw * p.gh);
        lv_maxt[l] = std::max(lv_maxt[l], p.tiles_x * p.tiles_y);
        lv_maxroi[l] = std::max(lv_maxroi[l], (p.gw - 2 * GC_GAP) * (p.gh - 2 * GC_GAP));
        lv_first[l + 1] = (int)k + 1;
        plane_elems = std::max<long long>(plane_elems, lv_nodes[l]);
        total_nodes += p.gw * p.gh;
    }
    for (int l = 0; l < nlevels; l++) { if (lv_first[l + 1] < lv_first[l]) lv_first[l + 1] = lv_first[l]; max_pairs = std::max(max_pairs, lv_first[l + 1] - lv_first[l]); }

    // the device block: packed images and masks, the pair table, the counters, the 12 planes
    const SeamSlots slots(images, n);
    const std::vector<size_t>&ioff = slots.ioff, &moff = slots.moff;
    size_t total = slots.bytes;
    const size_t table_off = total; total += mis_align_up(std::max<size_t>(1, work.size()) * sizeof(GcPair), 256);
    const int n_ctr = max_pairs * (2 + GC_K) + GC_SWEEP_BATCH;
    const size_t ctr_off = total; total += mis_align_up((size_t)n_ctr * sizeof(int), 256);
    const size_t plane_bytes = mis_align_up((size_t)plane_elems * sizeof(int), 256);
    const size_t planes_off = total; total += 12 * plane_bytes;
    PoolBlock blk(ctx);
    if (int rc = blk.alloc(total)) return rc;
    uint8_t* d = (uint8_t*)blk.p;
    // the pinned job block: the pair table on its way up, the counters on their way down, the debug planes
    const size_t pin_ctr = mis_align_up(std::max<size_t>(1, work.size()) * sizeof(GcPair), 256);
    const size_t pin_dbg = pin_ctr + mis_align_up((size_t)n_ctr * sizeof(int), 256);
    const size_t dbg_plane = dbg ? mis_align_up((size_t)work[0].p.gw * work[0].p.gh * sizeof(int), 256) : 0;
    uint8_t* pin = nullptr;
    { void* sp = nullptr; if (int rc = mis_host_stage(ctx, pin_dbg + 4 * dbg_plane, &sp)) return rc; pin = (uint8_t*)sp; }
    GcPair* table = (GcPair*)pin;
    int* hctr = (int*)(pin + pin_ctr);

    for (int i = 0; i < n; i++) {
        MIS_HIP(ctx, seam_gather(d + ioff[i], images[i], ctx->stream));
        MIS_HIP(ctx, seam_gather(d + moff[i], masks[i], ctx->stream));
    }
    for (size_t k = 0; k < work.size(); k++) {
        GcPair& p = work[k].p;
        p.img1 = d + ioff[work[k].i]; p.img2 = d + ioff[work[k].j];
        p.mask1 = d + moff[work[k].i]; p.mask2 = d + moff[work[k].j];
        table[k] = p;
    }
    const GcPair* dtable = (const GcPair*)(d + table_off);
    if (!work.empty()) MIS_HIP(ctx, hipMemcpyAsync(d + table_off, table, work.size() * sizeof(GcPair), hipMemcpyHostToDevice, ctx->stream));
    GcPlanes G;
    {
        int* pl = (int*)(d + planes_off);
        const size_t pe = plane_bytes / sizeof(int);
        for (int k = 0; k < 4; k++) { G.res[k] = pl + (size_t)k * pe; G.outbox[k] = pl + (size_t)(8 + k) * pe; }
        G.excess = pl + 4 * pe; G.height = pl + 5 * pe; G.drain = pl + 6 * pe; G.term = pl + 7 * pe;
    }
    int* dctr = (int*)(d + ctr_off);
    GcCounters C{dctr, dctr + max_pairs, dctr + 2 * (size_t)max_pairs, dctr + (size_t)max_pairs * (2 + GC_K)};

    std::vector<int>& st = ctx->gc_stats;
    st.assign(6, 0);
    st[0] = (int)work.size(); st[1] = nlevels; st[2] = (int)std::min<long long>(total_nodes, INT32_MAX); st[3] = GC_SET_CAP;
    for (int l = 0; l < nlevels; l++) {
        const GcPair* lp = dtable + lv_first[l];
        const int np = lv_first[l + 1] - lv_first[l];
        const dim3 node_grid((lv_maxv[l] + 255) / 256, np), tile_grid(lv_maxt[l], np);
        MIS_HIP(ctx, hipMemsetAsync(dctr, 0, (size_t)n_ctr * sizeof(int), ctx->stream));
        hipLaunchKernelGGL(gc_build_kernel, node_grid, dim3(256), 0, ctx->stream, lp, G, C.active, terminal_cost, penalty);
        MIS_HIP(ctx, hipGetLastError());
        if (dbg) {
            const size_t bytes = (size_t)work[0].p.gw * work[0].p.gh * sizeof(int);
            MIS_HIP(ctx, hipMemcpyAsync(pin + pin_dbg, G.res[GC_R], bytes, hipMemcpyDeviceToHost, ctx->stream));
            MIS_HIP(ctx, hipMemcpyAsync(pin + pin_dbg + dbg_plane, G.res[GC_D], bytes, hipMemcpyDeviceToHost, ctx->stream));
            MIS_HIP(ctx, hipMemcpyAsync(pin + pin_dbg + 2 * dbg_plane, G.term, bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
        // a relaxation sweep settles at least the nodes whose shortest residual path crosses one more tile border: no more
        // sweeps than nodes
        const int sweep_cap = lv_maxv[l] + GC_SWEEP_BATCH;
        int sets = 0;
        for (;;) {
            hipLaunchKernelGGL(gc_relabel_init_kernel, node_grid, dim3(256), 0, ctx->stream, lp, G, C.active);
            bool settled = false;
            for (int sweeps = 0; !settled; sweeps += GC_SWEEP_BATCH) {
                MIS_CHECK(ctx, sweeps < sweep_cap, MIS_E_INTERNAL, "graph-cut seams: the global relabel of level %d did not settle in %d sweeps", l + 1, sweeps);
                MIS_HIP(ctx, hipMemsetAsync(C.changed, 0, GC_SWEEP_BATCH * sizeof(int), ctx->stream));
                for (int b = 0; b < GC_SWEEP_BATCH; b++) hipLaunchKernelGGL(gc_relabel_sweep_kernel, tile_grid, dim3(GC_TN), 0, ctx->stream, lp, G, C.active, C.changed + b);
                // (counted behind every batch, read only when the batch has settled: heights still on their way down count too few)
                hipLaunchKernelGGL(gc_count_kernel, dim3(1, np), dim3(GC_TN), 0, ctx->stream, lp, G, C.active, C.count);
                MIS_HIP(ctx, hipGetLastError());
                MIS_HIP(ctx, hipMemcpyAsync(hctr, dctr, (size_t)n_ctr * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
                MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
                st[5] += GC_SWEEP_BATCH;
                for (int b = 0; b < GC_SWEEP_BATCH; b++) settled |= hctr[(size_t)max_pairs * (2 + GC_K) + b] == 0;
            }
            st[4]++;
            int open_pair = -1;
            for (int q = 0; q < np; q++)
                if (hctr[max_pairs + q] != 0) { open_pair = q; break; }
            if (open_pair < 0) break;
            MIS_CHECK(ctx, sets < GC_SET_CAP, MIS_E_INTERNAL, "graph-cut seams: pair (%d, %d) still has %d active nodes after %d round sets (the cap)",
                      work[lv_first[l] + open_pair].i, work[lv_first[l] + open_pair].j, hctr[max_pairs + open_pair], sets);
            hipLaunchKernelGGL(gc_gate_kernel, dim3(1), dim3(64), 0, ctx->stream, C.active, C.count, np);
            MIS_HIP(ctx, hipMemsetAsync(C.set_active, 0, (size_t)max_pairs * GC_K * sizeof(int), ctx->stream));
            for (int s = 0; s < GC_K; s++) {
                hipLaunchKernelGGL(gc_round_kernel, tile_grid, dim3(GC_TN), 0, ctx->stream, lp, G, C.active);
                hipLaunchKernelGGL(gc_absorb_kernel, node_grid, dim3(256), 0, ctx->stream, lp, G, C.active, C.set_active + (size_t)s * max_pairs);
            }
            MIS_HIP(ctx, hipGetLastError());
            sets += GC_K;
        }
        st.push_back(sets);
        if (dbg) {
            MIS_HIP(ctx, hipMemcpyAsync(pin + pin_dbg + 3 * dbg_plane, G.height, (size_t)work[0].p.gw * work[0].p.gh * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
            MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
            const size_t V = (size_t)work[0].p.gw * work[0].p.gh;
            memcpy(dbg->cap_right, pin + pin_dbg, V * sizeof(int));
            memcpy(dbg->cap_down, pin + pin_dbg + dbg_plane, V * sizeof(int));
            memcpy(dbg->terminals, pin + pin_dbg + 2 * dbg_plane, V * sizeof(int));
            const int* h = (const int*)(pin + pin_dbg + 3 * dbg_plane);
            for (size_t k = 0; k < V; k++) dbg->labels[k] = h[k] < work[0].p.hmax;
            return MIS_OK;
        }
        hipLaunchKernelGGL(gc_writeback_kernel, dim3((lv_maxroi[l] + 255) / 256, np), dim3(256), 0, ctx->stream, lp, G);
        MIS_HIP(ctx, hipGetLastError());
    }
    if (dbg) return MIS_OK;
    // every level has finished: the masks go back to the caller, once
    for (int i = 0; i < n; i++) MIS_HIP(ctx, seam_scatter(masks[i], d + moff[i], ctx->stream));
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MIS_OK;
}

int gc_check_costs(MisContext* ctx, int cost_type, float terminal_cost, float penalty) {
    MIS_CHECK(ctx, cost_type != MIS_SEAM_GC_COST_COLOR_GRAD, MIS_E_UNSUPPORTED, "GraphCutSeamFinder: COST_COLOR_GRAD is not built (its gradient weights are undefined where the Sobel sums vanish; DESIGN.md section 8); COST_COLOR is");
    MIS_CHECK(ctx, cost_type == MIS_SEAM_GC_COST_COLOR, MIS_E_INVALID, "GraphCutSeamFinder: cost type %d", cost_type);
    MIS_CHECK(ctx, std::isfinite(terminal_cost) && terminal_cost >= 0.f && std::isfinite(penalty) && penalty >= 0.f, MIS_E_INVALID,
              "GraphCutSeamFinder: terminal_cost %g and bad_region_penalty %g must be finite and >= 0", (double)terminal_cost, (double)penalty);
    // a node's inflow: four edges of at most (2 * 195075 + 1 + penalty) * 255 and its terminal, below 2^31 (one more unit an edge for the rounding)
    const double inflow = 4.0 * ((2.0 * 195075.0 + 1.0 + (double)penalty) * 255.0 * (1.0 + 1.0 / 8388608.0) + 1.0) + (double)terminal_cost * 255.0 + 1.0;
    MIS_CHECK(ctx, inflow < 2147483648.0, MIS_E_INVALID, "GraphCutSeamFinder: terminal_cost %g and bad_region_penalty %g let a node's inflow reach 2^31", (double)terminal_cost, (double)penalty);
    return MIS_OK;
}

}  // namespace

extern "C" int mis_seam_graphcut(MisContext* ctx, const MisPoint* corners, const MisImage* images, MisImage* masks, int n, int cost_type, float terminal_cost,
                                 float bad_region_penalty) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, n >= 0 && (n == 0 || (corners && images && masks)), MIS_E_INVALID, "null argument");
    if (int rc = gc_check_costs(ctx, cost_type, terminal_cost, bad_region_penalty)) return rc;
    return gc_find(ctx, corners, images, masks, n, terminal_cost, bad_region_penalty, nullptr);
}

extern "C" int mis_seam_graphcut_debug_pair(MisContext* ctx, const MisPoint* corners, const MisImage* images, const MisImage* masks, int n, int i, int j, int32_t* cap_right,
                                            int32_t* cap_down, int32_t* terminals, uint8_t* labels, size_t capacity_elems, int* grid_w, int* grid_h) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, n > 0 && corners && images && masks && grid_w && grid_h, MIS_E_INVALID, "null argument");
    GcDebug dbg{i, j, cap_right, cap_down, terminals, labels, capacity_elems, grid_w, grid_h};
    return gc_find(ctx, corners, images, const_cast<MisImage*>(masks), n, 10000.f, 1000.f, &dbg);
}

extern "C" int mis_seam_graphcut_stats(const MisContext* ctx, int* out, int capacity, int* count) {
    if (!ctx || !count || capacity < 0 || (capacity > 0 && !out)) return MIS_E_INVALID;
    *count = (int)ctx->gc_stats.size();
    for (int k = 0; k < capacity && k < *count; k++) out[k] = ctx->gc_stats[k];
    return MIS_OK;
}
