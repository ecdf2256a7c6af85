"""Plain numpy / scipy reference of cv::detail::DpSeamFinder(DpSeamFinder::COLOR), the reference pipeline's default seam finder
(DESIGN.md section 8), written from the published algorithm (OpenCV 4.x stitching/src/seam_finders.cpp, core's
cv::partition, imgproc's floodFill).

Nothing here calls the oracle (oracle/mo_seam.c) or the product library (csrc/seam.hip): both are checked against `find`, so a
misreading that the two share shows up as a disagreement with this module.  Where they walk pixels (stack flood fills, a touch
table filled per contour point, union-find, a scalar dynamic programme in float), this module uses whole-array operations:
scipy.ndimage.label per class, comparisons of shifted label arrays, connected components of a boolean distance matrix, one
vectorised DP step per line over exact integers.  Clauses that are sequential BY DEFINITION are restated as loops and say so.

Semantics restated:
  * find: the pairs (i, j), i < j, are generated in (i, j) order and sorted ascending by the squared distance between the image
    centres corner + (w / 2, h / 2) (integer halves), then reversed: the most distant pair first.  Every pair is processed on the
    masks as the earlier pairs left them; the images are the 8-bit BGR values as floats (convertTo(CV_32F)).
    NOT PINNED -- pairs at equal distance.  OpenCV sorts with std::sort, whose order of equal keys is unspecified: it depends on
    the C++ standard library OpenCV was built with and on the number of pairs (libstdc++'s introsort is a plain -- stable --
    insertion sort up to 16 elements and a quicksort above), none of which follows from the algorithm or can be observed
    offline.  tie_order="reversed" (the default: what the product and the oracle do) leaves equal keys as a stable sort plus the
    reverse does, i.e. in reverse generation order; tie_order="forward" keeps equal keys in generation order.
    test_refimpl_seam_dp_cpu.py prints on which scenes, and by how many mask pixels, the two differ.
  * process: a pair whose frame rectangles do not intersect is left alone.  Otherwise both masks are placed on the union
    rectangle (a mask byte is set when it is non-zero: 1 and 128 count like 255) and each mask's contour is the set pixels with
    a 4-neighbour that is unset or outside the union.
  * findComponents: every pixel is in one of three classes -- both masks (INTERS), first only (FIRST), second only (SECOND).
    The components are the 4-connected regions of each class, numbered over all classes by the raster position of their first
    pixel.  A component's box is its bounding box, its contour the pixels with a 4-neighbour of another label or outside the
    union, in RASTER ORDER (sequential by definition: the contour is produced by the raster scan, and later clauses depend on
    its order).
  * findEdges: two components are joined, in both directions, when a pixel of one is 4-adjacent to a pixel of the other.
  * resolveConflicts (sequential by definition): repeatedly take the FIRST edge (c1, c2), in the order of (c1, c2) pairs, with
    c1 an intersection component whose owner so far (state without the INTERS bit) differs from c2's state.
      - c1 has exactly one edge (c1, *) left: the whole of c1 takes c2's label;
      - otherwise getSeamTips, estimateSeam and updateLabelsUsingSeam, each only if the one before succeeded.
    Either way c1 now belongs to the image c2 does not belong to, c1's box and contour are recomputed from its remaining pixels,
    and the edge is erased.
    Settled: "the resolved edge leaves the graph in both directions" needs no switch.  Only edges (c, *) with c an intersection
    component are ever read (the conflict test requires INTERS on the first member, hasOnlyOneNeighbor counts the edges that
    start at c1), and two intersection components are never adjacent (they would be one component), so the direction (c2, c1)
    is never read again whether it is erased or not.  Keeping (c1, c2) instead would find the same conflict for ever.
    Settled likewise: OpenCV rescans c2's box and contour inside c2's OLD box, which misses what c2 just gained; c2 is never an
    intersection component and only an intersection component's box and contour are read after findEdges.
  * getSeamTips: the special points are c1's contour points, in contour order, that lie within 2 pixels (a 5 x 5 square clipped
    to the union) of the first mask's contour AND of the second's, and have a 4-neighbour labelled c2.  Fewer than two: failure.
    cv::partition(ClosePoints(10)): the classes of the transitive closure of "squared distance < 100" (strict), numbered by
    first member.  Fewer than two classes: failure.  A class centre is (cvRound(sum x / size), cvRound(sum y / size)), half to
    even.  The two classes i < j with the largest squared centre distance, the first pair encountered on ties (sequential by
    definition), and in each the member closest to its centre, the first on ties: p1 from class i, p2 from class j.
  * computeCosts (COLOR): between horizontally adjacent pixels (x - 1, x) of row y, both in c1,
        costV(y, x) = (|I1(y, x - 1) - I2(y, x)|^2 + |I1(y, x) - I2(y, x - 1)|^2) / 2
    and between vertically adjacent pixels (y - 1, y) of column x likewise costH(y, x); anywhere else the bad-region cost
    3 * 255^2 = 195075.  Pixel differences are squared Euclidean norms of BGR triples: integers below 2^18, exact in float32; a
    cost is an integer or a half-integer.
    Settled: "labels read one past the component's box count as not this component" needs no switch.  OpenCV fills costV for
    box columns 0 .. w and costH for box rows 0 .. h, reading labels one past the box, but estimateSeam only ever reads costV
    columns 0 .. w - 1 and costH rows 0 .. h - 1 (every step ends on a pixel of the box and reads the cost at that pixel or at
    its lower-indexed neighbour), so the extra line never reaches a result.  It is not computed here.
  * estimateSeam: src = p1, dst = p2 relative to the box.  The seam is horizontal when |dst.x - src.x| > |dst.y - src.y|
    (strict: equal differences give a vertical seam); src and dst are swapped when src lies after dst on that axis.  Vertical:
    for each row y after src's, every pixel (y, x) of c1 takes the best of
        1: cost(y - 1, x)     + costV(y - 1, x)
        2: (cost(y - 1, x - 1) + costV(y - 1, x - 1)) + costH(y, x - 1)
        3: (cost(y - 1, x + 1) + costV(y - 1, x + 1)) + costH(y, x)
    over the predecessors that are reachable and inside the box (only src is reachable in its own row), by (cost, step code)
    lexicographically -- std::min_element over pairs.  The horizontal case is the same with the axes and costV / costH
    exchanged.  dst unreachable: failure.  Otherwise the seam is traced back from dst and reported from p1 to p2.
    cost is CV_32F, so FLOAT32 IS THE SEMANTICS (dp="float32", additions associated as written); dp="int" runs the same step
    over doubled costs in int64, where every value is an exact integer.  While every float32 sum stays below 2^23 all its
    values are exact half-integers, no rounding takes part and the two agree: `find` records the largest sum per seam and
    check_exact=True asserts the bound and that both programmes choose the same seam.
  * updateLabelsUsingSeam: on c1's box, c1's contour and the seam are marked 255; the remaining pixels of c1 fall into
    4-connected sub-components numbered from 1 in raster order of their first pixel.  Then (sequential by definition: a point
    reads marks that earlier points wrote) every contour point, in contour order, takes the value of the LAST of its 8
    neighbours, in the order W E N S NW NE SW SE, that lies in the box and holds a value other than 0 and 255, or 0 if none
    does; every seam point, in seam order, takes the value of the pixel below it (horizontal seam: the seam follows the upper
    side of pixels) or to its right (vertical: the left side) if that is in the box and neither 0 nor 255, else 0.  For every
    value k, connect2[k] counts the contour points of value k with a 4-neighbour labelled c2 and connectOther[k] those with a
    4-neighbour inside the union labelled neither c1 nor c2 (unlabelled pixels included).  With len = the contour's length,
    value k goes over to c2 when connect2[k] / len > 0.05 and connectOther[k] / len < 0.1 (float64 divisions, both strict); all
    pixels of the box holding an accepted non-zero value take c2's label.
  * the masks: a pixel whose final component belongs to the first image (state FIRST or INTERS|FIRST) leaves the second mask,
    one whose component belongs to the second leaves the first; an intersection component without any neighbour stays in both.

`find` records the events it passes through in `trace` (a collections.Counter); SCENES as a whole must show every one of EVENTS.
"""
import collections

import numpy as np
from scipy import ndimage
from scipy.sparse import csgraph, csr_matrix

F32 = np.float32
FIRST, SECOND, INTERS = 1, 2, 4
BAD2 = 2 * 3 * 255 * 255            # the doubled bad-region cost
EXACT_BOUND = float(2 ** 23)        # below it every float32 half-integer is exact
_CROSS = ndimage.generate_binary_structure(2, 1)
_INF = np.int64(1) << 60

EVENTS = (
    "pair_rects_disjoint", "pair_masks_disjoint", "one_neighbour_relabel", "tips_too_few_points", "tips_one_cluster",
    "seam_vertical_unswapped", "seam_vertical_swapped", "seam_horizontal_unswapped", "seam_horizontal_swapped",
    "axis_tie_takes_vertical", "dst_unreachable", "dp_tie_by_step_code", "inters_with_hole", "several_inters_components",
    "sub_accepted", "sub_without_contact", "sub_rejected_5pct", "sub_rejected_10pct", "mask_byte_not_255", "equal_distance_pairs",
    "independent_pairs", "inters_without_neighbour", "inters_resolved_again", "pair_resolved",
)


# ------------------------------------------------------------------------------------------------ whole-array helpers
def _neighbours(a, fill):
    """The W, E, N, S neighbours of every element of a, `fill` outside."""
    p = np.pad(a, 1, constant_values=fill)
    return p[1:-1, :-2], p[1:-1, 2:], p[:-2, 1:-1], p[2:, 1:-1]


def _mask_contour(m):
    w, e, n, s = _neighbours(m, False)
    return m & ~(w & e & n & s)


def _label_contour(lab, l):
    """The pixels labelled l with a 4-neighbour of another label or outside the union, as (ys, xs) in raster order."""
    w, e, n, s = _neighbours(lab, -1)
    return np.nonzero((lab == l) & ((w != l) | (e != l) | (n != l) | (s != l)))


def _touches(lab, l):
    """Boolean map: a 4-neighbour inside the union is labelled l."""
    w, e, n, s = _neighbours(lab, -1)
    return (w == l) | (e == l) | (n == l) | (s == l)


def partition_close(pts, dist=10):
    """cv::partition(pts, ClosePoints(dist)): class of every point, classes numbered by first member."""
    p = np.asarray(pts, np.int64)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    _, cc = csgraph.connected_components(csr_matrix(d2 < dist * dist), directed=False)
    _, first = np.unique(cc, return_index=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    return rank[cc]


# ------------------------------------------------------------------------------------------------ one pair
class _Pair:
    def __init__(self, im1, im2, tl1, tl2, m1, m2, dp, check_exact, trace, seams, tag):
        self.dp, self.check_exact, self.trace, self.seams, self.tag = dp, check_exact, trace, seams, tag
        (h1, w1), (h2, w2) = m1.shape, m2.shape
        self.tl = (min(tl1[0], tl2[0]), min(tl1[1], tl2[1]))
        br = (max(tl1[0] + w1, tl2[0] + w2), max(tl1[1] + h1, tl2[1] + h2))
        self.uw, self.uh = br[0] - self.tl[0], br[1] - self.tl[1]
        self.s1 = (slice(tl1[1] - self.tl[1], tl1[1] - self.tl[1] + h1), slice(tl1[0] - self.tl[0], tl1[0] - self.tl[0] + w1))
        self.s2 = (slice(tl2[1] - self.tl[1], tl2[1] - self.tl[1] + h2), slice(tl2[0] - self.tl[0], tl2[0] - self.tl[0] + w2))
        self.M1 = np.zeros((self.uh, self.uw), bool); self.M1[self.s1] = m1 != 0
        self.M2 = np.zeros((self.uh, self.uw), bool); self.M2[self.s2] = m2 != 0
        self.I1 = np.zeros((self.uh, self.uw, 3), np.int64); self.I1[self.s1] = im1
        self.I2 = np.zeros((self.uh, self.uw, 3), np.int64); self.I2[self.s2] = im2
        # closeToContour as a map: a 5 x 5 square around the pixel, clipped to the union, meets the contour
        sq = np.ones((5, 5), bool)
        self.near1 = ndimage.binary_dilation(_mask_contour(self.M1), sq)
        self.near2 = ndimage.binary_dilation(_mask_contour(self.M2), sq)

    # findComponents + findEdges
    def components(self):
        classes = ((self.M1 & self.M2, INTERS), (self.M1 & ~self.M2, FIRST), (~self.M1 & self.M2, SECOND))
        found = []                                   # (raster position of the first pixel, state, boolean map)
        for cm, state in classes:
            lab, n = ndimage.label(cm, _CROSS)
            _, first = np.unique(lab.ravel(), return_index=True)
            for k in range(1, n + 1):
                found.append((int(first[k if lab.flat[first[0]] == 0 else k - 1]), state, lab == k))
        found.sort(key=lambda f: f[0])
        self.lab = np.zeros((self.uh, self.uw), np.int64)
        self.states = []
        for c, (_, state, cm) in enumerate(found):
            self.lab[cm] = c + 1
            self.states.append(state)
        a = np.concatenate([self.lab[:, :-1].ravel(), self.lab[:-1, :].ravel()])
        b = np.concatenate([self.lab[:, 1:].ravel(), self.lab[1:, :].ravel()])
        k = (a != b) & (a > 0) & (b > 0)
        self.edges = set(zip((a[k] - 1).tolist(), (b[k] - 1).tolist())) | set(zip((b[k] - 1).tolist(), (a[k] - 1).tolist()))
        ninters = sum(1 for s in self.states if s == INTERS)
        if ninters == 0:
            self.trace["pair_masks_disjoint"] += 1
        if ninters > 1:
            self.trace["several_inters_components"] += 1
        for c, s in enumerate(self.states):
            if s == INTERS:
                if not np.array_equal(ndimage.binary_fill_holes(self.lab == c + 1, _CROSS), self.lab == c + 1):
                    self.trace["inters_with_hole"] += 1
                if not any(e[0] == c for e in self.edges):
                    self.trace["inters_without_neighbour"] += 1

    # getSeamTips
    def seam_tips(self, c1, c2):
        ys, xs = _label_contour(self.lab, c1 + 1)
        k = self.near1[ys, xs] & self.near2[ys, xs] & _touches(self.lab, c2 + 1)[ys, xs]
        pts = np.stack([xs[k], ys[k]], 1).astype(np.int64)
        if len(pts) < 2:
            self.trace["tips_too_few_points"] += 1
            return None
        cls = partition_close(pts)
        n = int(cls.max()) + 1
        if n < 2:
            self.trace["tips_one_cluster"] += 1
            return None
        size = np.bincount(cls, minlength=n).astype(np.float64)
        cen = np.stack([np.rint(np.bincount(cls, pts[:, 0], n) / size), np.rint(np.bincount(cls, pts[:, 1], n) / size)], 1)
        d = ((cen[:, None, :] - cen[None, :, :]) ** 2).sum(-1)
        iu = np.triu_indices(n, 1)                                     # (i, j), i < j, in the order of the double loop
        best = int(np.argmax(d[iu]))                                   # the first maximum
        tips = []
        for c in (int(iu[0][best]), int(iu[1][best])):
            mem = pts[cls == c]
            tips.append(tuple(int(v) for v in mem[int(np.argmin(((mem - cen[c]) ** 2).sum(1)))]))   # the first minimum
        return tips

    # computeCosts: doubled, exact integers, over c1's box
    def costs(self, L, box):
        y0, y1, x0, x1 = box
        def d2(a, b):
            return ((a - b) ** 2).sum(-1)
        I1, I2 = self.I1, self.I2
        cv = np.full((self.uh, self.uw), BAD2, np.int64)
        ok = L[:, 1:] & L[:, :-1]
        cv[:, 1:][ok] = (d2(I1[:, :-1], I2[:, 1:]) + d2(I1[:, 1:], I2[:, :-1]))[ok]
        ch = np.full((self.uh, self.uw), BAD2, np.int64)
        ok = L[1:, :] & L[:-1, :]
        ch[1:, :][ok] = (d2(I1[:-1, :], I2[1:, :]) + d2(I1[1:, :], I2[:-1, :]))[ok]
        return cv[y0:y1, x0:x1], ch[y0:y1, x0:x1]

    @staticmethod
    def _dp(A, B, L, src, dst, mode):
        """The programme along axis 0 ("a") of A, B, L from src = (a, c) to dst.  A[a, c] is the cost of stepping a -> a + 1 at c,
        B[a, c] of moving c -> c + 1 (or back) in line a.  mode "int": doubled int64 costs; "float32": float32 halves.
        Returns (path from src to dst as (a, c) or None, total cost in doubled units, largest sum formed, ties met)."""
        n = L.shape[1]
        if mode == "int":
            A, B, inf = A.astype(np.int64), B.astype(np.int64), _INF
            cost = np.full(n, inf, np.int64)
        else:
            A, B, inf = A.astype(F32) / F32(2), B.astype(F32) / F32(2), F32(np.inf)
            cost = np.full(n, inf, F32)
        cost[src[1]] = 0
        ctl = np.zeros(L.shape, np.int8)
        big, ties = 0.0, 0
        for a in range(src[0] + 1, dst[0] + 1):
            base = cost + A[a - 1]                                      # (cost + A) first, as written
            cand = np.full((3, n), inf, cost.dtype)
            cand[0] = base
            cand[1, 1:] = base[:-1] + B[a, :-1]
            cand[2, :-1] = base[1:] + B[a, :-1]
            if mode == "int":
                cand[cand >= inf] = inf
            cand[:, ~L[a]] = inf
            step = np.argmin(cand, 0)                                   # the first minimum: the smallest step code on ties
            cost = cand[step, np.arange(n)]
            got = cost < inf
            ctl[a][got] = step[got] + 1
            if got.any():
                big = max(big, float(cand[cand < inf].max()))            # every sum formed, chosen or not
                ties += int(((cand == cost[None, :]) & got[None, :]).sum(0).max() > 1)
        if not cost[dst[1]] < inf:
            return None, None, big, ties
        total = float(cost[dst[1]]) * (1 if mode == "int" else 2)
        path, (a, c) = [dst], dst
        while a != src[0]:
            c += {1: 0, 2: -1, 3: 1}[int(ctl[a, c])]
            a -= 1
            path.append((a, c))
        return path[::-1], total, big, ties

    # estimateSeam
    def estimate_seam(self, c1, p1, p2):
        L = self.lab == c1 + 1
        ys, xs = np.nonzero(L)
        box = (int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1)
        cv, ch = self.costs(L, box)
        Lb = L[box[0]:box[1], box[2]:box[3]]
        src, dst = (p1[0] - box[2], p1[1] - box[0]), (p2[0] - box[2], p2[1] - box[0])          # (x, y)
        horizontal = abs(dst[0] - src[0]) > abs(dst[1] - src[1])
        if not horizontal and abs(dst[0] - src[0]) == abs(dst[1] - src[1]) != 0:
            self.trace["axis_tie_takes_vertical"] += 1
        if horizontal:                                                   # along x: transpose, exchange the two cost maps
            A, B, Lt, s, d = ch.T, cv.T, Lb.T, (src[0], src[1]), (dst[0], dst[1])
        else:
            A, B, Lt, s, d = cv, ch, Lb, (src[1], src[0]), (dst[1], dst[0])
        swapped = s[0] > d[0]
        if swapped:
            s, d = d, s
        path, total, big, ties = self._dp(A, B, Lt, s, d, self.dp)
        rec = dict(tag=self.tag, horizontal=horizontal, swapped=swapped, A=A, B=B, L=Lt, src=s, dst=d, total=total, big=big,
                   p1=p1, p2=p2, seam=None, other_dp_same=None)
        self.seams.append(rec)
        if self.check_exact or self.dp == "float32":
            other, ototal, obig, _ = self._dp(A, B, Lt, s, d, "int" if self.dp == "float32" else "float32")
            rec["other_dp_same"] = other == path
            fbig = big if self.dp == "float32" else obig
            rec["big"] = fbig
            if self.check_exact:
                assert fbig < EXACT_BOUND, "%s: a float32 sum of %g reaches 2^23: resize the scene" % (self.tag, fbig)
                assert other == path and ototal == total, "%s: the integer and the float32 programme choose different seams" % self.tag
        if path is None:
            self.trace["dst_unreachable"] += 1
            return None, horizontal
        if ties:
            self.trace["dp_tie_by_step_code"] += 1
        self.trace["seam_%s_%s" % ("horizontal" if horizontal else "vertical", "swapped" if swapped else "unswapped")] += 1
        if swapped:
            path = path[::-1]
        seam = [((a, c) if horizontal else (c, a)) for a, c in path]                         # back to (x, y) in the box
        seam = [(x + box[2], y + box[0]) for x, y in seam]
        assert seam[0] == tuple(p1) and seam[-1] == tuple(p2)                                # the CV_Assert pair
        rec["seam"] = seam
        return seam, horizontal

    # updateLabelsUsingSeam
    def update_labels(self, c1, c2, seam, horizontal):
        l1, l2 = c1 + 1, c2 + 1
        L = self.lab == l1
        cy, cx = _label_contour(self.lab, l1)
        y0, x0 = int(cy.min()), int(cx.min())                            # a component's box is its contour's box
        y1, x1 = int(cy.max()) + 1, int(cx.max()) + 1
        marked = np.zeros(L.shape, bool)
        marked[cy, cx] = True
        for x, y in seam:
            marked[y, x] = True
        sub, nc = ndimage.label((L & ~marked)[y0:y1, x0:x1], _CROSS)     # numbered in raster order of the first pixel
        M = sub.astype(np.int64)
        M[marked[y0:y1, x0:x1]] = 255
        h, w = M.shape
        for y, x in zip((cy - y0).tolist(), (cx - x0).tolist()):         # sequential by definition
            v = 0
            for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1)):
                c, r = x + dx, y + dy
                if 0 <= c < w and 0 <= r < h and M[r, c] not in (0, 255):
                    v = M[r, c]
            M[y, x] = v
        for x, y in seam:                                                # sequential by definition
            x, y = x - x0, y - y0
            r, c = (y + 1, x) if horizontal else (y, x + 1)
            M[y, x] = M[r, c] if r < h and c < w and M[r, c] not in (0, 255) else 0
        vals = M[cy - y0, cx - x0]
        nk = max(nc, 255) + 1
        con2 = np.bincount(vals[_touches(self.lab, l2)[cy, cx]], minlength=nk)
        w_, e_, n_, s_ = _neighbours(self.lab, l1)                       # outside the union never counts
        other = ((w_ != l1) & (w_ != l2)) | ((e_ != l1) & (e_ != l2)) | ((n_ != l1) & (n_ != l2)) | ((s_ != l1) & (s_ != l2))
        cono = np.bincount(vals[other[cy, cx]], minlength=nk)
        length = float(len(cy))
        accept = np.zeros(nk, bool)
        for k in range(nk):
            a5, a10 = con2[k] / length > 0.05, cono[k] / length < 0.1
            accept[k] = a5 and a10
            if 1 <= k <= nc:
                self.trace["sub_accepted" if accept[k] else "sub_rejected_10pct" if a5 else "sub_rejected_5pct" if con2[k] else "sub_without_contact"] += 1
        accept[0] = False
        self.lab[y0:y1, x0:x1][accept[M]] = l2

    # resolveConflicts
    def resolve(self):
        while True:
            conflict = [(a, b) for a, b in sorted(self.edges) if self.states[a] & INTERS and self.states[a] & ~INTERS != self.states[b]]
            if not conflict:
                break
            c1, c2 = conflict[0]
            if self.states[c1] != INTERS:
                self.trace["inters_resolved_again"] += 1
            if sum(1 for e in self.edges if e[0] == c1) == 1:
                self.trace["one_neighbour_relabel"] += 1
                self.lab[self.lab == c1 + 1] = c2 + 1
            else:
                tips = self.seam_tips(c1, c2)                           # (an emptied component has no contour: too few points)
                if tips:
                    seam, horizontal = self.estimate_seam(c1, tips[0], tips[1])
                    if seam:
                        self.update_labels(c1, c2, seam, horizontal)
            self.states[c1] = INTERS | (SECOND if self.states[c2] == FIRST else FIRST)
            self.edges.discard((c1, c2))
            self.edges.discard((c2, c1))
            self.trace["pair_resolved"] += 1

    def run(self, m1, m2):
        self.components()
        self.resolve()
        st = np.array([0] + self.states, np.int64)[self.lab]
        m2[((st & FIRST) != 0)[self.s2] & self.M1[self.s2]] = 0
        m1[((st & SECOND) != 0)[self.s1] & self.M2[self.s1]] = 0


# ------------------------------------------------------------------------------------------------ find
def pair_order(corners, sizes, tie_order="reversed"):
    """DpSeamFinder::find's pairs in processing order, with their squared centre distances."""
    n = len(sizes)
    cen = [(corners[i][0] + sizes[i][0] // 2, corners[i][1] + sizes[i][1] // 2) for i in range(n)]
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    dist = {p: (cen[p[0]][0] - cen[p[1]][0]) ** 2 + (cen[p[0]][1] - cen[p[1]][1]) ** 2 for p in pairs}
    if tie_order == "reversed":
        pairs = sorted(pairs, key=dist.get)[::-1]                        # sorted() is stable
    elif tie_order == "forward":
        pairs = sorted(pairs, key=lambda p: -dist[p])
    else:
        raise ValueError(tie_order)
    return pairs, dist


def find(images, corners, masks, *, dp="float32", tie_order="reversed", check_exact=False, trace=None, seams=None, order=None):
    """DpSeamFinder(COLOR)::find.  images: 8UC3 arrays, corners: (x, y), masks: 8U arrays; returns the new masks (copies).
    trace: a Counter that collects EVENTS; seams: a list that collects one record per estimateSeam call; order: an explicit
    list of pairs in place of find's own (for tests of order dependence)."""
    trace = collections.Counter() if trace is None else trace
    seams = [] if seams is None else seams
    out = [np.array(m, np.uint8) for m in masks]
    n = len(out)
    if n == 0:
        return out
    if any(((m != 0) & (m != 255)).any() for m in out):
        trace["mask_byte_not_255"] += 1
    sizes = [(m.shape[1], m.shape[0]) for m in out]
    pairs, dist = pair_order(corners, sizes, tie_order)
    if len(set(dist.values())) < len(dist):
        trace["equal_distance_pairs"] += 1
    work = []
    for i, j in (pairs if order is None else order):
        (x1, y1), (x2, y2), (w1, h1), (w2, h2) = corners[i], corners[j], sizes[i], sizes[j]
        if max(x1, x2) >= min(x1 + w1, x2 + w2) or max(y1, y2) >= min(y1 + h1, y2 + h2):
            trace["pair_rects_disjoint"] += 1
            continue
        work.append((i, j))
        _Pair(np.asarray(images[i], np.int64), np.asarray(images[j], np.int64), corners[i], corners[j], out[i], out[j], dp,
              check_exact, trace, seams, "pair (%d, %d)" % (i, j)).run(out[i], out[j])
    if any(not set(p) & set(q) for p in work for q in work):
        trace["independent_pairs"] += 1
    return out


def seam_shortest_path(rec):
    """The cost (doubled units) of the cheapest monotone path of a seam record, by Dijkstra over the same step graph.  Every
    path takes exactly dst.a - src.a steps, so every edge weighs one more than its cost (scipy drops zero-weight edges)."""
    A, B, L, (sa, sc), (da, dc) = rec["A"], rec["B"], rec["L"], rec["src"], rec["dst"]
    n = L.shape[1]
    rows, cols, wts = [], [], []
    for a in range(sa + 1, da + 1):
        for c in np.nonzero(L[a])[0].tolist():
            for pc, extra in ((c, 0), (c - 1, int(B[a, c - 1]) if c > 0 else 0), (c + 1, int(B[a, c]) if c < n - 1 else 0)):
                if 0 <= pc < n and (a - 1 > sa or pc == sc):
                    rows.append((a - 1) * n + pc); cols.append(a * n + c); wts.append(int(A[a - 1, pc]) + extra + 1)
    g = csr_matrix((wts, (rows, cols)), shape=(L.size, L.size), dtype=np.float64)
    d = csgraph.dijkstra(g, directed=True, indices=sa * n + sc)[da * n + dc]
    return None if np.isinf(d) else float(d) - (da - sa)


# ------------------------------------------------------------------------------------------------ scenes
def _world(x, y, seed, flat):
    """8UC3 content at pano position (x, y): a smooth ramp, a few hard edges, low-amplitude noise drawn per frame."""
    rng = np.random.default_rng(seed)
    if flat:
        return np.broadcast_to(np.array([90, 120, 60], np.uint8), x.shape + (3,)).copy()
    v = np.stack([70 + 1.5 * x + 0.5 * y, 150 - x + 0.8 * y, 110 + 0.3 * x - 1.2 * y], -1)
    v += 50 * ((x + 2 * y) % 23 < 7)[..., None] + 35 * ((3 * x - y) % 31 < 9)[..., None] * np.array([1, -1, 1])
    v += rng.integers(-3, 4, v.shape)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _full(x, y, w, h):
    return np.full(x.shape, 255, np.uint8)


def _where(cond, value=255):
    return lambda x, y, w, h: np.where(cond(x, y, w, h), value, 0).astype(np.uint8)


# name -> (frames [(corner x, corner y, w, h, mask formula over frame-local x, y)], flat content)
_F = _full
SCENES = {
    # pair geometry
    "side_by_side": ([(-7, -5, 40, 32, _F), (17, -5, 40, 32, _F)], False),
    "stacked": ([(3, -9, 44, 30, _F), (3, 9, 44, 30, _F)], False),
    "stacked_slant": ([(0, 0, 48, 30, _F), (0, 14, 48, 34, _where(lambda x, y, w, h: 4 * y >= 48 - x))], False),
    "corner_wide": ([(0, 0, 48, 36, _F), (20, 22, 48, 36, _F)], False),
    "corner_square": ([(-10, -10, 40, 40, _F), (10, 10, 40, 40, _F)], False),
    "corner_square_2": ([(10, -10, 40, 40, _F), (-10, 10, 40, 40, _F)], False),
    "near_edges": ([(-3, -2, 16, 44, _F), (-1, 2, 30, 44, _F)], False),
    "contained": ([(0, 0, 40, 30, _F), (10, 8, 16, 12, _F)], False),
    "apart": ([(0, 0, 20, 16, _F), (25, 3, 20, 16, _F)], False),
    "masks_apart": ([(0, 0, 30, 20, _where(lambda x, y, w, h: x < 12)), (10, 2, 30, 20, _where(lambda x, y, w, h: x > 8))], False),
    "identical": ([(2, 3, 24, 18, _F), (2, 3, 24, 18, _F)], False),
    # seam search
    "one_pixel": ([(0, 0, 20, 16, _F), (19, 15, 20, 16, _F)], False),
    "one_cluster": ([(0, 0, 20, 16, _F), (15, 11, 20, 16, _F)], False),
    "cluster_at_10": ([(0, 0, 20, 16, _F), (11, 5, 20, 16, _F)], False),
    "u_shape": ([(0, 0, 40, 30, _F), (0, 12, 40, 30, _where(lambda x, y, w, h: ~((x >= 6) & (x < 34) & (y < 12))))], False),
    "flat": ([(-7, -5, 40, 32, _F), (17, -5, 40, 32, _F)], True),
    "flat_stacked": ([(3, -9, 44, 30, _F), (3, 9, 44, 30, _F)], True),
    # components and relabelling
    "hole": ([(0, 0, 44, 36, _where(lambda x, y, w, h: (x - 34) ** 2 + (y - 18) ** 2 > 16)), (24, 0, 44, 36, _F)], False),
    "gap": ([(0, 0, 44, 36, _F), (24, 0, 44, 36, _where(lambda x, y, w, h: (y < 15) | (y > 19)))], False),
    "two_firsts": ([(0, 0, 44, 30, _where(lambda x, y, w, h: ~((x >= 20) & (x < 24) & (y < 18)))), (0, 16, 44, 30, _F)], False),
    "open_top": ([(0, 0, 50, 24, _where(lambda x, y, w, h: y >= 10)), (18, 0, 50, 24, _where(lambda x, y, w, h: y >= 10))], False),
    # mask values
    "bytes": ([(-7, -5, 40, 32, _where(lambda x, y, w, h: x + y > 6, 1)), (17, -5, 40, 32, lambda x, y, w, h: np.where((x + y) % 2 == 0, 128, 255).astype(np.uint8))], False),
    # several images
    "six": ([(0, 0, 40, 30, _F), (28, 0, 40, 30, _F), (56, 0, 40, 30, _F), (0, 20, 40, 30, _F), (28, 20, 40, 30, _F), (56, 20, 40, 30, _F)], False),
    "tie_three": ([(0, 0, 40, 30, _F), (22, 4, 40, 30, _F), (4, 22, 40, 30, _F)], False),
    "five": ([(-20, -12, 36, 28, _F), (4, -14, 36, 28, _where(lambda x, y, w, h: (x - 18) ** 2 + (y - 14) ** 2 < 400, 128)), (-18, 6, 36, 28, _F),
              (6, 8, 36, 28, _F), (70, 0, 30, 20, _F)], False),
}


def scene(name):
    """(images, corners, masks) of a named scene, deterministic."""
    frames, flat = SCENES[name]
    seed0 = sum(ord(ch) for ch in name)
    images, corners, masks = [], [], []
    for k, (cx, cy, w, h, fn) in enumerate(frames):
        y, x = np.mgrid[0:h, 0:w]
        images.append(_world(x + cx, y + cy, seed0 * 16 + k, flat))
        corners.append((cx, cy))
        masks.append(np.ascontiguousarray(fn(x, y, w, h), np.uint8))
    return images, corners, masks


def seam_scale_scene():
    """Two 422 x 237 frames (the seam scale of SURVEY F7) with curved mask edges and full-contrast content: float32 sums pass
    2^23 here, so the float32 programme alone is the reference."""
    w, h = 422, 237
    rng = np.random.default_rng(422237)
    images, masks, corners = [], [], [(-31, 12), (167, -9)]
    for cx, cy in corners:
        y, x = np.mgrid[0:h, 0:w]
        gx, gy = x + cx, y + cy
        chk = (((gx // 9) + (gy // 7)) % 2 * 255)[..., None] * np.array([1, 1, 1])
        v = np.where(((gx * 5 + gy * 3) % 41 < 20)[..., None], chk, 255 - chk) + rng.integers(-40, 41, (h, w, 3))
        images.append(np.clip(v, 0, 255).astype(np.uint8))
        u, t = (x - w / 2) / (w / 2), (y - h / 2) / (h / 2)
        masks.append(np.where(np.abs(u) ** 2.6 + np.abs(t) ** 3.2 + 0.05 * np.sin(9 * t) * u < 0.97, 255, 0).astype(np.uint8))
    return images, corners, masks
