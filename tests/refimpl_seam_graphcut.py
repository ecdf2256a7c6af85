"""Plain numpy / scipy reference of cv::detail::GraphCutSeamFinder(COST_COLOR, terminal_cost, bad_region_penalty) as SURVEY.md
appendix A.13 states it; nothing here calls the product library.

Pairs: PairwiseSeamFinder::run order -- for i, for j > i, every pair whose rectangles overlap (overlapRoi: the intersection,
non-empty in both dimensions).  Masks are edited in place, a later pair sees what the earlier ones left.

Graph of a pair (i, j, roi): gap = 10, the grid is (roi.h + 20) x (roi.w + 20); a grid pixel outside an image has colour (0, 0, 0)
and mask 0 for that image; a mask pixel is set when it is non-zero.  All weights are float32 and exact:
    n(p)      = sum_c (img1_c(p) - img2_c(p))^2                                     an integer <= 195075
    w(p, q)   = n(p) + n(q) + 1, + bad_region_penalty if any of mask1(p), mask1(q), mask2(p), mask2(q) is clear
    cap(p, q) = cap(q, p) = cvRound(w * 255.f)                                      one float32 multiply, round half to even
    term(p)   = cvRound((src - snk) * 255.f),  src = terminal_cost if mask1(p) else 0,  snk = terminal_cost if mask2(p) else 0
term > 0 is a source edge, term < 0 a sink edge.  S is the set of grid nodes reachable from the source in the residual graph of a
maximum flow -- the minimal source side, the same for every maximum flow.  For every roi pixel (not the gap): in S and mask1 set
-> mask2 cleared; not in S and mask2 set -> mask1 cleared.

The flow is scipy.sparse.csgraph.maximum_flow (Dinic, int32) with a super source and sink; its value is summed here in int64 from
the flow matrix."""
import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import breadth_first_order, maximum_flow

F32 = np.float32
GAP = 10
MAX_N = 3 * 255 * 255                          # n(p) <= 195075
INFLOW_BOUND = 2 ** 31                         # 4 edge capacities + one terminal stay below it (32-bit excesses)


def max_edge_capacity(bad_region_penalty=1000.0):
    return int(np.rint(((F32(MAX_N) + F32(MAX_N) + F32(1)) + F32(bad_region_penalty)) * F32(255)))


def max_terminal_capacity(terminal_cost=10000.0):
    return int(np.rint(F32(terminal_cost) * F32(255)))


def overlap_roi(tl1, size1, tl2, size2):
    """detail::overlapRoi -> (x, y, w, h) or None; sizes are (w, h)."""
    x0, y0 = max(tl1[0], tl2[0]), max(tl1[1], tl2[1])
    x1, y1 = min(tl1[0] + size1[0], tl2[0] + size2[0]), min(tl1[1] + size1[1], tl2[1] + size2[1])
    if x1 > x0 and y1 > y0:
        return x0, y0, x1 - x0, y1 - y0
    return None


def pair_list(corners, sizes):
    """PairwiseSeamFinder::run: (i, j, roi) in processing order."""
    out = []
    for i in range(len(sizes)):
        for j in range(i + 1, len(sizes)):
            roi = overlap_roi(corners[i], sizes[i], corners[j], sizes[j])
            if roi is not None:
                out.append((i, j, roi))
    return out


def _on_grid(a, tl, roi, fill_shape):
    """The grid's view of an image or mask: zero outside it."""
    x, y, w, h = roi
    gh, gw = h + 2 * GAP, w + 2 * GAP
    out = np.zeros((gh, gw) + fill_shape, a.dtype)
    ih, iw = a.shape[:2]
    ox, oy = x - GAP - tl[0], y - GAP - tl[1]                      # image coordinates of grid node (0, 0)
    gx0, gy0, gx1, gy1 = max(0, -ox), max(0, -oy), min(gw, iw - ox), min(gh, ih - oy)
    if gx1 > gx0 and gy1 > gy0:
        out[gy0:gy1, gx0:gx1] = a[gy0 + oy:gy1 + oy, gx0 + ox:gx1 + ox]
    return out


def capacities(img1, img2, mask1, mask2, tl1, tl2, roi, terminal_cost=10000.0, bad_region_penalty=1000.0):
    """-> (cap_right, cap_down, terminals), int64 planes of the grid's shape; cap_right's last column and cap_down's last row
    are 0 (no edge)."""
    a = _on_grid(np.asarray(img1), tl1, roi, (3,)).astype(F32)
    b = _on_grid(np.asarray(img2), tl2, roi, (3,)).astype(F32)
    m1 = _on_grid(np.asarray(mask1), tl1, roi, ()) != 0
    m2 = _on_grid(np.asarray(mask2), tl2, roi, ()) != 0
    d = a - b
    n = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    good = m1 & m2
    pen, one, s255 = F32(bad_region_penalty), F32(1), F32(255)

    def edge(np_, nq, ok):
        w = (np_ + nq) + one
        w = np.where(ok, w, w + pen)
        assert w.dtype == F32
        return np.rint(w * s255).astype(np.int64)
    cr = np.zeros(n.shape, np.int64)
    cd = np.zeros(n.shape, np.int64)
    cr[:, :-1] = edge(n[:, :-1], n[:, 1:], good[:, :-1] & good[:, 1:])
    cd[:-1, :] = edge(n[:-1, :], n[1:, :], good[:-1, :] & good[1:, :])
    tc = F32(terminal_cost)
    src = np.where(m1, tc, F32(0))
    snk = np.where(m2, tc, F32(0))
    term = np.rint((src - snk) * s255).astype(np.int64)
    return cr, cd, term


def _graph(cr, cd, term):
    gh, gw = term.shape
    V = gh * gw
    s, t = V, V + 1
    idx = np.arange(V).reshape(gh, gw)
    rows, cols, caps = [], [], []

    def both(u, v, c):
        keep = c > 0
        u, v, c = u[keep], v[keep], c[keep]
        rows.extend([u, v]); cols.extend([v, u]); caps.extend([c, c])
    both(idx[:, :-1].ravel(), idx[:, 1:].ravel(), cr[:, :-1].ravel())
    both(idx[:-1, :].ravel(), idx[1:, :].ravel(), cd[:-1, :].ravel())
    tf = term.ravel()
    pos, neg = np.flatnonzero(tf > 0), np.flatnonzero(tf < 0)
    rows.extend([np.full(len(pos), s), neg]); cols.extend([pos, np.full(len(neg), t)]); caps.extend([tf[pos], -tf[neg]])
    rows, cols, caps = np.concatenate(rows), np.concatenate(cols), np.concatenate(caps)
    assert caps.max(initial=0) < 2 ** 31
    return sp.csr_array((caps.astype(np.int32), (rows.astype(np.int32), cols.astype(np.int32))), shape=(V + 2, V + 2)), s, t


def _reach(res, start, transpose=False):
    g = sp.csr_array(res.T if transpose else res)
    order = breadth_first_order(g, start, directed=True, return_predecessors=False)
    out = np.zeros(res.shape[0], bool)
    out[order] = True
    return out


def min_cut(cr, cd, term):
    """-> (flow value (int), S, T_reach): S = the nodes reachable from the source in the residual graph (the minimal source side),
    T_reach = the nodes that reach the sink there (the complement of the maximal source side); bool planes of the grid's shape."""
    gh, gw = term.shape
    V = gh * gw
    if not (term > 0).any() or not (term < 0).any():
        # no source or no sink edge: the zero flow is maximal, the residual graph is the graph
        g, s, t = _graph(cr, cd, term)
        res = (g > 0).astype(np.int8)
        return 0, _reach(res, s)[:V].reshape(gh, gw), _reach(res, t, True)[:V].reshape(gh, gw)
    g, s, t = _graph(cr, cd, term)
    f = maximum_flow(g, s, t).flow
    value = int(f[[s], :].toarray().astype(np.int64).sum())
    res = (g.astype(np.int64) - f.astype(np.int64))
    res = sp.csr_array(res)
    res.data = (res.data > 0).astype(np.int8)
    res.eliminate_zeros()
    return value, _reach(res, s)[:V].reshape(gh, gw), _reach(res, t, True)[:V].reshape(gh, gw)


def find_in_pair(img1, img2, mask1, mask2, tl1, tl2, roi, terminal_cost=10000.0, bad_region_penalty=1000.0):
    """One pair: edits mask1 / mask2 in place -> (cap_right, cap_down, terminals, S, flow value)."""
    cr, cd, term = capacities(img1, img2, mask1, mask2, tl1, tl2, roi, terminal_cost, bad_region_penalty)
    value, S, _ = min_cut(cr, cd, term)
    x, y, w, h = roi
    Sr = S[GAP:GAP + h, GAP:GAP + w]
    v1 = mask1[y - tl1[1]:y - tl1[1] + h, x - tl1[0]:x - tl1[0] + w]
    v2 = mask2[y - tl2[1]:y - tl2[1] + h, x - tl2[0]:x - tl2[0] + w]
    set1, set2 = v1 != 0, v2 != 0
    v2[Sr & set1] = 0
    v1[~Sr & set2] = 0
    return cr, cd, term, S, value


def find(images, corners, masks, terminal_cost=10000.0, bad_region_penalty=1000.0, order=None, record=None):
    """GraphCutSeamFinder(COST_COLOR)::find -> the new masks (copies).  order: an explicit list of (i, j) in place of
    PairwiseSeamFinder::run's (for tests of order dependence); record: a dict that collects, per (i, j), what find_in_pair returns."""
    out = [np.array(m, np.uint8) for m in masks]
    sizes = [(m.shape[1], m.shape[0]) for m in out]
    pairs = pair_list(corners, sizes)
    if order is not None:
        by = {(i, j): r for i, j, r in pairs}
        pairs = [(i, j, by[(i, j)]) for i, j in order]
    for i, j, roi in pairs:
        r = find_in_pair(images[i], images[j], out[i], out[j], corners[i], corners[j], roi, terminal_cost, bad_region_penalty)
        if record is not None:
            record[(i, j)] = r
    return out
