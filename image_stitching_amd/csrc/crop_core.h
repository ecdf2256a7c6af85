// crop_core.h -- the per-element steps of the device cropper's kernels (crop.hip; the reference's cropper.cpp:124-209 with the
// OpenCV pieces host/cropper.cpp restates).  Plain functions of one pixel, one contour state or -- the shrink loop -- one thread,
// with no barrier inside: the kernels call them one element a thread, and a host program can call them element by element in the
// same launch order (they compile as ordinary C++; the atomics become plain reads and writes there).
//
// Everything is indexed in the PADDED image: (w + 2) x (h + 2), one ring of background round the source, pixel (x, y) of the
// source at p = (y + 1) * pw + (x + 1).  No neighbour of a source pixel lies outside the padded image, the ring is one 4-connected
// background region that holds index 0, and raster order is the source's.
#pragma once
#include <limits.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CROP_HD __host__ __device__ __forceinline__
#else
#define CROP_HD inline
#endif

enum { CROP_OK = 0, CROP_EMPTY = 1, CROP_NO_RECT = 2 };      // the status word: cropper.cpp's two failures are results here
// the slots of the result block the last kernel writes: the rectangle, the status, the chosen contour's point count and first pixel
// (y * w + x of the source), the doubling rounds taken
enum { CROP_R_X = 0, CROP_R_Y, CROP_R_W, CROP_R_H, CROP_R_STATUS, CROP_R_COUNT, CROP_R_FIRST, CROP_R_ROUNDS, CROP_R_N };

struct CropGrid {
    int w, h, pw, ph;       // source and padded size
    CROP_HD int pixels() const { return pw * ph; }
};
CROP_HD CropGrid crop_grid(int w, int h) { return CropGrid{w, h, w + 2, h + 2}; }

// direction codes of contours.cpp: 0 = E, 1 = NE, 2 = N, 3 = NW, 4 = W, 5 = SW, 6 = S, 7 = SE (y grows downwards)
CROP_HD int crop_delta(const CropGrid& g, int s) {
    const int dx = (s == 0 || s == 1 || s == 7) ? 1 : ((s >= 3 && s <= 5) ? -1 : 0);
    const int dy = (s >= 1 && s <= 3) ? -1 : ((s >= 5) ? 1 : 0);
    return dy * g.pw + dx;
}

CROP_HD int crop_atomic_min(int* a, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicMin(a, v);
#else
    const int o = *a; if (v < o) *a = v; return o;
#endif
}
CROP_HD int crop_atomic_add(int* a, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(a, v);
#else
    const int o = *a; *a = o + v; return o;
#endif
}
CROP_HD void crop_atomic_max64(unsigned long long* a, unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(a, v);
#else
    if (v > *a) *a = v;
#endif
}

// ---- the mask: cvtColor(RGB2GRAY) > 0 with the 15-bit weights on channels 0, 1, 2 (cropper.cpp:128-131); one channel: > 0 ----
CROP_HD uint8_t crop_mask_px(const CropGrid& g, const uint8_t* src, size_t stride, int channels, int p) {
    const int py = p / g.pw, px = p - py * g.pw;
    if (px < 1 || py < 1 || px > g.w || py > g.h) return 0;
    const uint8_t* s = src + (size_t)(py - 1) * stride + (size_t)(px - 1) * channels;
    const int gray = channels == 3 ? (s[0] * 9798 + s[1] * 19235 + s[2] * 3735 + (1 << 14)) >> 15 : s[0];
    return gray > 0;
}

// ---- connected components: union-find with minimum-index roots over the pixels whose plane value is `want` ----
// A label is a parent link towards a smaller index of the same component, -1 outside the set; after init, merge (every pixel, in
// any order, also concurrently) and flatten, a member's label is its component's smallest index.
// init: a member starts linked to the first pixel of its run of members inside its aligned chunk of CROP_CHUNK consecutive indices
// (one wavefront's pixels; crop.hip takes the run from a ballot, which gives the same link).  A chunk may wrap from the end of a
// row into the next: only ring pixels meet there, which are one component anyway and never members of the foreground.
constexpr int CROP_CHUNK = 64;
CROP_HD void crop_ccl_init(int* L, const uint8_t* plane, uint8_t want, int p) {
    int q = -1;
    if (plane[p] == want)
        for (q = p; q > (p & ~(CROP_CHUNK - 1)) && plane[q - 1] == want;) q--;
    L[p] = q;
}

CROP_HD int crop_find(const int* L, int a) {
    for (int up = L[a]; up != a; up = L[a]) a = up;      // a stale link read elsewhere is still a link into the same component
    return a;
}

// links the components of a and b: the larger root goes under the smaller; where a turns out not to be a root any more, its old
// parent is carried on, so no link is ever lost
CROP_HD void crop_union(int* L, int a, int b) {
    a = crop_find(L, a); b = crop_find(L, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = crop_atomic_min(&L[a], b);
        if (old == a) break;
        a = old;
    }
}

// merge: the links to the neighbours before p in raster order (W, N; with conn8 also NW, NE) that no other pixel makes.  W is in
// p's run unless p opens a chunk.  The members among NW, N, NE are one run of the row above when N is one of them, and p's left
// neighbour, when a member, touches that run too and links to it (or leaves it to its own left neighbour): a row of a big
// component costs one union a chunk and one a run, not four a pixel.
CROP_HD void crop_ccl_merge(const CropGrid& g, int* L, const uint8_t* plane, uint8_t want, bool conn8, int p) {
    if (plane[p] != want) return;
    const int py = p / g.pw, px = p - py * g.pw;
    const bool W = px > 0 && plane[p - 1] == want;
    if (W && (p & (CROP_CHUNK - 1)) == 0) crop_union(L, p, p - 1);
    if (py == 0) return;
    const bool N = plane[p - g.pw] == want, NW = px > 0 && plane[p - g.pw - 1] == want;
    if (conn8) {
        const bool NE = px < g.pw - 1 && plane[p - g.pw + 1] == want;
        if (N) { if (!W) crop_union(L, p, p - g.pw); }
        else {
            if (NW && !W) crop_union(L, p, p - g.pw - 1);      // (W set: NW is W's upper neighbour)
            if (NE) crop_union(L, p, p - g.pw + 1);
        }
    } else if (N && !(W && NW)) {
        crop_union(L, p, p - g.pw);                            // (W and NW set: W links to NW, which is N's run)
    }
}

CROP_HD void crop_ccl_flatten(int* L, int p) { if (L[p] >= 0) L[p] = crop_find(L, L[p]); }

// ---- border pixels: a foreground pixel with a background pixel among its eight neighbours gets a slot of the state tables ----
CROP_HD void crop_slot_px(const CropGrid& g, const uint8_t* mask, int* slot, int* pix, int* nslots, int p) {
    int s = -1;
    if (mask[p]) {      // never on the ring: all eight neighbours exist
        bool border = false;
        for (int d = 0; d < 8; d++) border |= mask[p + crop_delta(g, d)] == 0;
        if (border) { s = crop_atomic_add(nslots, 1); pix[s] = p; }
    }
    slot[p] = s;
}

// ---- the successor of contour state (pixel of slot k, direction s_in towards its predecessor), icvFetchContour's inner loop:
// scan s_in + 1, s_in + 2, ... for the first foreground neighbour t, move there with s_in' = (t + 4) & 7.  A pixel without a
// foreground neighbour stays where it is (a contour of one point) ----
CROP_HD void crop_succ_state(const CropGrid& g, const uint8_t* mask, const int* slot, const int* pix, int* nxt, int idx) {
    const int p = pix[idx >> 3], s_in = idx & 7;
    int to = idx;
    for (int k = 1; k <= 8; k++) {
        const int t = (s_in + k) & 7;
        const int q = p + crop_delta(g, t);
        if (mask[q]) {
            // a traced pixel always touches the background; a neighbour without a slot ends the walk (never on a contour)
            if (slot[q] >= 0) to = slot[q] * 8 + ((t + 4) & 7);
            break;
        }
    }
    nxt[idx] = to;
}

// ---- the start state of every external contour.  A component has one exactly when its raster-first pixel (its label) has its left
// neighbour in the background region of the frame (label 0).  The start direction is the clockwise search of icvFetchContour
// from s = 4 downwards; an isolated pixel starts (and stays) in state 0 ----
CROP_HD void crop_start_slot(const CropGrid& g, const uint8_t* mask, const int* fg_label, const int* bg_label, const int* pix, uint8_t* mark, int k) {
    const int p = pix[k];
    if (fg_label[p] != p || bg_label[p - 1] != 0) return;
    int s = 4, s0 = 0;
    for (int i = 0; i < 8; i++) {
        s = (s - 1) & 7;
        if (mask[p + crop_delta(g, s)]) { s0 = s; break; }
    }
    mark[k * 8 + s0] = 1;
}

// ---- one round of pointer doubling: what is marked marks the state 2^round steps on, then every jump doubles ----
CROP_HD void crop_double_state(const int* jump, int* jump_next, uint8_t* mark, int idx) {
    const int j = jump[idx];
    if (mark[idx]) mark[j] = 1;      // (a state marked in this very round may mark on: still a state of the same cycle)
    jump_next[idx] = jump[j];
}

// ---- a marked state is one contour point: count it for its component (at the slot of the component's first pixel) ----
CROP_HD void crop_count_state(const int* fg_label, const int* slot, const int* pix, const uint8_t* mark, int* count, int idx) {
    if (mark[idx]) crop_atomic_add(&count[slot[fg_label[pix[idx >> 3]]]], 1);
}

// ---- the winner: maximal count, ties to the smallest first pixel, as one ordered key ----
CROP_HD void crop_winner_slot(const int* pix, const int* count, unsigned long long* key, int k) {
    if (count[k] > 0) crop_atomic_max64(key, ((unsigned long long)(unsigned)count[k] << 32) | (unsigned)(INT_MAX - pix[k]));
}
CROP_HD int crop_key_count(unsigned long long key) { return (int)(key >> 32); }
CROP_HD int crop_key_first(unsigned long long key) { return INT_MAX - (int)(key & 0xffffffffu); }      // padded index

// ---- the winner's points: walls of the fill and the x / y histograms (the sorted lists in counted form) ----
CROP_HD void crop_wall_state(const CropGrid& g, const int* fg_label, const int* pix, const uint8_t* mark, unsigned long long key, uint8_t* wall,
                             int* xhist, int* yhist, int idx) {
    if (!mark[idx] || key == 0) return;
    const int p = pix[idx >> 3];
    if (fg_label[p] != crop_key_first(key)) return;
    const int py = p / g.pw, px = p - py * g.pw;
    crop_atomic_add(&xhist[px - 1], 1);       // once per state: a pixel the contour passes k times counts k times
    crop_atomic_add(&yhist[py - 1], 1);
    wall[p] = 1;
}

// ---- the shrink loop of cropper.cpp:160-200, one thread.  cumx[x] = contour points with an x of at most x (xs[k] is the smallest x
// with cumx[x] > k), cumy alike; rowz[y * (w + 1) + x] = zeros of cmask in row y left of x, colz[y * w + x] = zeros of column x
// above y.  An unchanged rectangle gives unchanged out-codes, so a run of equal coordinates is stepped over in one go ----
struct CropShrink { const int* cumx; const int* cumy; const int* rowz; const int* colz; int w, h, count; };

CROP_HD int crop_shrink(const CropShrink& S, int rect[4]) {
    const int w = S.w, n = S.count;
    int minx = 0, maxx = n - 1, miny = 0, maxy = n - 1;
    int xl = 0, xr = S.w - 1, yt = 0, yb = S.h - 1;
    int rx = 0, ry = 0, rw = 0, rh = 0;
    while (minx < maxx && miny < maxy) {
        while (xl < S.w - 1 && S.cumx[xl] <= minx) xl++;
        while (xr > 0 && S.cumx[xr - 1] > maxx) xr--;
        while (yt < S.h - 1 && S.cumy[yt] <= miny) yt++;
        while (yb > 0 && S.cumy[yb - 1] > maxy) yb--;
        rx = xl; ry = yt; rw = xr - xl; rh = yb - yt;
        if (rw <= 0 || rh <= 0) break;
        const int top = S.rowz[(size_t)ry * (w + 1) + rx + rw] - S.rowz[(size_t)ry * (w + 1) + rx];
        const int bottom = S.rowz[(size_t)(ry + rh - 1) * (w + 1) + rx + rw] - S.rowz[(size_t)(ry + rh - 1) * (w + 1) + rx];
        const int left = S.colz[(size_t)(ry + rh) * w + rx] - S.colz[(size_t)ry * w + rx];
        const int right = S.colz[(size_t)(ry + rh) * w + rx + rw - 1] - S.colz[(size_t)ry * w + rx + rw - 1];
        if (top + bottom + left + right == 0) break;
        // checkInteriorExterior's tie rules (cropper.cpp:64-109)
        int ct = 0, cb = 0, cl = 0, cr = 0;
        if (top > bottom) { if (top > left && top > right) ct = 1; }
        else if (bottom > left) { if (bottom > right) cb = 1; }
        if (left >= right) { if (left >= bottom && left >= top) cl = 1; }
        else if (right >= top) { if (right >= bottom) cr = 1; }
        if (!(ct | cb | cl | cr)) break;
        // iterations until one of the moving list positions leaves its run of equal coordinates
        int d = INT_MAX;
        if (cl) { const int r = S.cumx[xl] - minx; d = r < d ? r : d; }
        if (cr) { const int r = maxx - (xr > 0 ? S.cumx[xr - 1] : 0) + 1; d = r < d ? r : d; }
        if (ct) { const int r = S.cumy[yt] - miny; d = r < d ? r : d; }
        if (cb) { const int r = maxy - (yb > 0 ? S.cumy[yb - 1] : 0) + 1; d = r < d ? r : d; }
        // the d iterations share this rectangle; the lists crossing before the last of them ends the loop on it
        const long long e = d - 1;
        if (!(minx + e * cl < maxx - e * cr && miny + e * ct < maxy - e * cb)) break;
        minx += d * cl; maxx -= d * cr; miny += d * ct; maxy -= d * cb;
    }
    rect[0] = rx; rect[1] = ry; rect[2] = rw; rect[3] = rh;
    return (rw <= 0 || rh <= 0) ? CROP_NO_RECT : CROP_OK;
}
