// seam_gc_core.h -- the per-node steps of the graph-cut seam finder's kernels (seam_gc.hip): the capacity build, one synchronous
// push / absorb / relabel round on a tile, one relaxation step of the global relabel, the border absorb.  Plain functions of a
// node's registers and the tile's two LDS arrays, with no barrier inside: the kernels call them with their barriers in between,
// and a host program can call them thread by thread in the same order (they compile as ordinary C++).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GC_HD __host__ __device__ __forceinline__
#define GC_UNROLL _Pragma("unroll")         // the four directions live in registers: every loop over them is unrolled
#else
#define GC_HD inline
#define GC_UNROLL
#endif

constexpr int GC_GAP = 10;                  // GraphCutSeamFinder: the roi grows by 10 pixels on every side
constexpr int GC_T = 32;                    // a workgroup's tile: 32 x 32 nodes, one thread a node
constexpr int GC_TN = GC_T * GC_T;
constexpr int GC_HS = GC_T + 2;             // the tile's heights in LDS carry a one-node halo
constexpr int GC_INNER = 32;                // push / relabel rounds of one round set (one launch)
enum { GC_L = 0, GC_R = 1, GC_U = 2, GC_D = 3 };     // a direction's opposite is dir ^ 1

// One pair of a level.  Images and masks are packed (w * 3 and w bytes a row); (ox, oy) is grid node (0, 0) in the image's own
// coordinates (roi.tl - gap - corner); the pair's nodes are [base, base + gw * gh) of every plane, row-major.
struct GcPair {
    const uint8_t* img1; const uint8_t* img2;
    uint8_t* mask1; uint8_t* mask2;
    int w1, h1, w2, h2;
    int ox1, oy1, ox2, oy2;
    int gw, gh, tiles_x, tiles_y;
    int base, hmax;                         // hmax = gw * gh + 2: the height of a node that reaches no drain
};

// Planar state: the residual capacity of a node's four edges, its excess, its height, what is left of its drain (the reversed
// problem's sink edge: a source terminal of the seam graph), its terminal as built, and what it pushed over its tile's border
// in the last round set (read once, by the neighbour on the other side).
struct GcPlanes {
    int* res[4];
    // excess: 32 bits suffice -- a node holds at most its own terminal plus what its four edges can carry in,
    // 4 * 99 743 505 + 2 550 000 < 2^31 with the default costs; mis_seam_graphcut refuses costs that break this bound
    int* excess;
    int* height;
    int* drain;
    int* term;
    int* outbox[4];
};

GC_HD int gc_round(float v) {               // cvRound: half to even
#if defined(__HIP_DEVICE_COMPILE__)
    return __float2int_rn(v);
#else
    return (int)lrintf(v);
#endif
}
GC_HD int gc_min(int a, int b) { return a < b ? a : b; }

struct GcPix { float n; bool m1, m2; };

GC_HD GcPix gc_pixel(const GcPair& P, int gx, int gy) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f;
    GcPix r; r.m1 = false; r.m2 = false;
    const int x1 = gx + P.ox1, y1 = gy + P.oy1, x2 = gx + P.ox2, y2 = gy + P.oy2;
    if (x1 >= 0 && x1 < P.w1 && y1 >= 0 && y1 < P.h1) {
        const size_t k = (size_t)y1 * P.w1 + x1;
        const uint8_t* p = P.img1 + k * 3;
        a0 = (float)p[0]; a1 = (float)p[1]; a2 = (float)p[2];
        r.m1 = P.mask1[k] != 0;
    }
    if (x2 >= 0 && x2 < P.w2 && y2 >= 0 && y2 < P.h2) {
        const size_t k = (size_t)y2 * P.w2 + x2;
        const uint8_t* p = P.img2 + k * 3;
        b0 = (float)p[0]; b1 = (float)p[1]; b2 = (float)p[2];
        r.m2 = P.mask2[k] != 0;
    }
    const float d0 = a0 - b0, d1 = a1 - b1, d2 = a2 - b2;
    r.n = (d0 * d0 + d1 * d1) + d2 * d2;
    return r;
}

GC_HD int gc_edge_cap(const GcPix& p, const GcPix& q, float penalty) {
    float w = (p.n + q.n) + 1.f;
    if (!(p.m1 && p.m2 && q.m1 && q.m2)) w = w + penalty;
    return gc_round(w * 255.f);
}

// One node of the capacity build: its four capacities (0 where the grid ends), its terminal, and the start of the reversed
// problem: excess at the sink terminals, drains at the source terminals.
GC_HD void gc_build_node(const GcPair& P, const GcPlanes& G, float terminal_cost, float penalty, int gx, int gy) {
    const GcPix c = gc_pixel(P, gx, gy);
    const size_t k = (size_t)P.base + (size_t)gy * P.gw + gx;
    G.res[GC_L][k] = gx > 0 ? gc_edge_cap(gc_pixel(P, gx - 1, gy), c, penalty) : 0;
    G.res[GC_R][k] = gx + 1 < P.gw ? gc_edge_cap(c, gc_pixel(P, gx + 1, gy), penalty) : 0;
    G.res[GC_U][k] = gy > 0 ? gc_edge_cap(gc_pixel(P, gx, gy - 1), c, penalty) : 0;
    G.res[GC_D][k] = gy + 1 < P.gh ? gc_edge_cap(c, gc_pixel(P, gx, gy + 1), penalty) : 0;
    const int t = gc_round(((c.m1 ? terminal_cost : 0.f) - (c.m2 ? terminal_cost : 0.f)) * 255.f);
    G.term[k] = t;
    G.excess[k] = t < 0 ? -t : 0;
    G.drain[k] = t > 0 ? t : 0;
    G.height[k] = 0;
    GC_UNROLL
    for (int d = 0; d < 4; d++) G.outbox[d][k] = 0;
}

// entry i of the tile's height array (halo included): the node's height, hmax outside the grid
GC_HD void gc_load_height(const GcPair& P, const GcPlanes& G, int tx0, int ty0, int i, int* hs) {
    const int ly = i / GC_HS, lx = i - ly * GC_HS;
    const int gx = tx0 - 1 + lx, gy = ty0 - 1 + ly;
    hs[i] = (gx >= 0 && gx < P.gw && gy >= 0 && gy < P.gh) ? G.height[(size_t)P.base + (size_t)gy * P.gw + gx] : P.hmax;
}
GC_HD int gc_hs_at(int lx, int ly) { return (ly + 1) * GC_HS + lx + 1; }
GC_HD int gc_hs_nbr(int lx, int ly, int d) {
    return d == GC_L ? gc_hs_at(lx - 1, ly) : d == GC_R ? gc_hs_at(lx + 1, ly) : d == GC_U ? gc_hs_at(lx, ly - 1) : gc_hs_at(lx, ly + 1);
}

struct GcNode {
    bool in;                // the thread has a node of the grid
    int e, drain, h;
    int r[4];
    int ob[4];              // pushed over the tile's border in this round set
};

GC_HD void gc_node_load(const GcPair& P, const GcPlanes& G, int gx, int gy, GcNode& s) {
    s.in = gx < P.gw && gy < P.gh;
    s.e = 0; s.drain = 0; s.h = P.hmax;
    GC_UNROLL
    for (int d = 0; d < 4; d++) { s.r[d] = 0; s.ob[d] = 0; }
    if (!s.in) return;
    const size_t k = (size_t)P.base + (size_t)gy * P.gw + gx;
    s.e = G.excess[k]; s.drain = G.drain[k]; s.h = G.height[k];
    GC_UNROLL
    for (int d = 0; d < 4; d++) s.r[d] = G.res[d][k];
}

// A round's push step: the node drains what it can, then pushes its excess to every lower neighbour with residual capacity
// (heights from LDS: the tile's own as of the last round, the halo's as of the launch).  What it pushes goes to ps[dir][thread];
// a push over the tile's border is also kept in ob[dir] for the neighbouring tile.
GC_HD void gc_push(GcNode& s, const int* hs, int* ps, int lx, int ly, int hmax) {
    int out[4] = {0, 0, 0, 0};
    if (s.in && s.e > 0) {
        if (s.drain > 0) { const int d = gc_min(s.e, s.drain); s.e -= d; s.drain -= d; }
        if (s.h < hmax)
            GC_UNROLL
            for (int d = 0; d < 4; d++)
                if (s.e > 0 && s.r[d] > 0 && hs[gc_hs_nbr(lx, ly, d)] < s.h) {
                    const int f = gc_min(s.e, s.r[d]);
                    out[d] = f; s.e -= f; s.r[d] -= f;
                }
    }
    const int t = ly * GC_T + lx;
    GC_UNROLL
    for (int d = 0; d < 4; d++) ps[d * GC_TN + t] = out[d];
    s.ob[GC_L] += lx == 0 ? out[GC_L] : 0;
    s.ob[GC_R] += lx == GC_T - 1 ? out[GC_R] : 0;
    s.ob[GC_U] += ly == 0 ? out[GC_U] : 0;
    s.ob[GC_D] += ly == GC_T - 1 ? out[GC_D] : 0;
}

// A round's second step (behind a barrier): the node takes what its neighbours in the tile pushed to it, and, if it still has
// excess and no lower neighbour to push to, rises to one above its lowest residual neighbour (hmax if it has none).
GC_HD void gc_absorb_relabel(GcNode& s, const int* hs, const int* ps, int lx, int ly, int hmax) {
    if (!s.in) return;
    const int t = ly * GC_T + lx;
    if (lx > 0) { const int f = ps[GC_R * GC_TN + t - 1]; s.e += f; s.r[GC_L] += f; }
    if (lx < GC_T - 1) { const int f = ps[GC_L * GC_TN + t + 1]; s.e += f; s.r[GC_R] += f; }
    if (ly > 0) { const int f = ps[GC_D * GC_TN + t - GC_T]; s.e += f; s.r[GC_U] += f; }
    if (ly < GC_T - 1) { const int f = ps[GC_U * GC_TN + t + GC_T]; s.e += f; s.r[GC_D] += f; }
    if (s.e > 0 && s.drain == 0 && s.h < hmax) {
        int lowest = hmax;
        GC_UNROLL
        for (int d = 0; d < 4; d++)
            if (s.r[d] > 0) lowest = gc_min(lowest, hs[gc_hs_nbr(lx, ly, d)]);
        if (lowest >= s.h) s.h = gc_min(lowest + 1, hmax);
    }
}

GC_HD void gc_node_store(const GcPair& P, const GcPlanes& G, int gx, int gy, const GcNode& s) {
    if (!s.in) return;
    const size_t k = (size_t)P.base + (size_t)gy * P.gw + gx;
    G.excess[k] = s.e; G.drain[k] = s.drain; G.height[k] = s.h;
    GC_UNROLL
    for (int d = 0; d < 4; d++) G.res[d][k] = s.r[d];
    GC_UNROLL
    for (int d = 0; d < 4; d++)
        if (s.ob[d]) G.outbox[d][k] = s.ob[d];      // (zero before: the build zeroes the outboxes, the absorb launch what it took)
}

// The absorb launch behind a round set: a node on a tile's border takes what the node across the border left in its outbox
// and zeroes it (every outbox entry has one reader).  -> whether the node is active: excess, and a height below hmax.
GC_HD bool gc_border_absorb(const GcPair& P, const GcPlanes& G, int gx, int gy) {
    const size_t k = (size_t)P.base + (size_t)gy * P.gw + gx;
    int e = G.excess[k];
    if (gx > 0 && gx % GC_T == 0) { const int f = G.outbox[GC_R][k - 1]; if (f) { e += f; G.res[GC_L][k] += f; G.outbox[GC_R][k - 1] = 0; } }
    if (gx + 1 < P.gw && (gx + 1) % GC_T == 0) { const int f = G.outbox[GC_L][k + 1]; if (f) { e += f; G.res[GC_R][k] += f; G.outbox[GC_L][k + 1] = 0; } }
    if (gy > 0 && gy % GC_T == 0) { const int f = G.outbox[GC_D][k - P.gw]; if (f) { e += f; G.res[GC_U][k] += f; G.outbox[GC_D][k - P.gw] = 0; } }
    if (gy + 1 < P.gh && (gy + 1) % GC_T == 0) { const int f = G.outbox[GC_U][k + P.gw]; if (f) { e += f; G.res[GC_D][k] += f; G.outbox[GC_U][k + P.gw] = 0; } }
    G.excess[k] = e;
    return e > 0 && G.height[k] < P.hmax;
}

// Global relabel, one relaxation step of a node: one above its lowest neighbour that it has residual capacity to, if that is lower
GC_HD int gc_relax(const int r[4], int h, const int* hs, int lx, int ly) {
    GC_UNROLL
    for (int d = 0; d < 4; d++)
        if (r[d] > 0) h = gc_min(h, hs[gc_hs_nbr(lx, ly, d)] + 1);
    return h;
}
