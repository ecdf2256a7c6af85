// seam_plan.h -- the pair plan of the seam finders (seam.hip, seam_gc.hip, seam_voronoi.hip): which pairs of frames overlap, in
// what order they are processed, and which of them may run side by side.  Plain C++17 for the host: a CPU program includes it on
// its own (tools/micro/seam_plan_dump.cpp; pinned to the two references' pair lists by tests/test_seam_plan_cpu.py).
#pragma once
#include <algorithm>
#include <vector>

struct SeamFrame { int x, y, w, h; };       // a frame's corner in the panorama and its size
struct SeamRect { int x0, y0, x1, y1; };    // [x0, x1) x [y0, y1)

// detail::overlapRoi: the rectangle two frames share; false when it is empty (frames that only touch along an edge share none)
inline bool seam_overlap(const SeamFrame& a, const SeamFrame& b, SeamRect* r) {
    *r = SeamRect{std::max(a.x, b.x), std::max(a.y, b.y), std::min(a.x + a.w, b.x + b.w), std::min(a.y + a.h, b.y + b.h)};
    return r->x0 < r->x1 && r->y0 < r->y1;
}

enum SeamOrder {
    SEAM_ORDER_RUN,         // PairwiseSeamFinder::run: for i, for j > i
    SEAM_ORDER_DISTANCE     // DpSeamFinder::find: the most distant centres first
};

struct SeamPair { int i, j, level; SeamRect roi; long long dist; };     // i < j; level from 1; dist: squared centre distance
struct SeamPlan { std::vector<SeamPair> pairs; int nlevels = 0; };

// The overlapping pairs of n frames in processing order.  A pair reads its two images and reads / writes its two masks, nothing
// else: pairs without a common image commute.  A pair's level is 1 + the highest level among the earlier pairs that share an
// image with it, so the pairs of one level may run side by side and the levels in turn keep the order wherever it matters.
// Pairs whose frames do not overlap change nothing and are dropped first (a stable order of all pairs, filtered, is the stable
// order of the filtered pairs).
// SEAM_ORDER_DISTANCE, NOT PINNED: the reference orders the pairs with std::sort (unspecified for equal keys) + std::reverse; pairs
// at equal distance are ordered here as a stable sort + reverse leaves them (tie_order="reversed" of tests/refimpl_seam_dp.py, which
// states both readings).
inline SeamPlan seam_plan(const std::vector<SeamFrame>& f, SeamOrder order) {
    const int n = (int)f.size();
    SeamPlan plan;
    for (int i = 0; i + 1 < n; i++)
        for (int j = i + 1; j < n; j++) {
            const long long dx = ((long long)f[i].x + f[i].w / 2) - ((long long)f[j].x + f[j].w / 2), dy = ((long long)f[i].y + f[i].h / 2) - ((long long)f[j].y + f[j].h / 2);
            SeamPair p{i, j, 0, {}, dx * dx + dy * dy};
            if (seam_overlap(f[i], f[j], &p.roi)) plan.pairs.push_back(p);
        }
    if (order == SEAM_ORDER_DISTANCE) {
        std::stable_sort(plan.pairs.begin(), plan.pairs.end(), [](const SeamPair& a, const SeamPair& b) { return a.dist < b.dist; });
        std::reverse(plan.pairs.begin(), plan.pairs.end());
    }
    std::vector<int> last((size_t)n, 0);
    for (SeamPair& p : plan.pairs) {
        p.level = last[p.i] = last[p.j] = std::max(last[p.i], last[p.j]) + 1;
        plan.nlevels = std::max(plan.nlevels, p.level);
    }
    return plan;
}
