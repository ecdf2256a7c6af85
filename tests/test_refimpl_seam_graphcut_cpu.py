"""The numpy / scipy reference of GraphCutSeamFinder(COST_COLOR) (tests/refimpl_seam_graphcut.py) against networkx's minimum cut
and by construction, the scenes that tests/test_seam_graphcut_gpu.py runs on the device -- with the regimes they are meant to
reach asserted here (a unique cut on the textured scenes, a real tie regime on the constant one, an empty source side, no
terminals) --, the capacity bounds, and the plumbing that needs no GPU: the class's names and refusals, the configuration names
that stay refused, the C ABI's new entries."""
import functools

import numpy as np
import pytest

import refimpl_seam_graphcut as gc

NAMES = ["texture", "constant", "col1", "row1", "tiny", "big", "holes", "inside", "empty", "serpentine", "three", "four"]
# Random texture with the frames offset along one axis only: the minimum cut is unique.  (Frames offset along both axes leave two
# 9 x 9 corners of the grid that lie in neither image behind uniform penalty edges: 162 tied nodes, asserted below for "tiny".)
RANDOM = ["texture", "holes", "serpentine"]


def _textured(seed, sizes, corners, noise=5):
    """Frames cut out of one random world, each with small noise of its own: overlapping pixels nearly agree."""
    rng = np.random.default_rng(seed)
    x0, y0 = min(c[0] for c in corners), min(c[1] for c in corners)
    X = max(c[0] + s[0] for c, s in zip(corners, sizes)) - x0
    Y = max(c[1] + s[1] for c, s in zip(corners, sizes)) - y0
    world = rng.integers(30, 226, (Y, X, 3)).astype(np.int64)
    out = []
    for (cx, cy), (w, h) in zip(corners, sizes):
        v = world[cy - y0:cy - y0 + h, cx - x0:cx - x0 + w] + rng.integers(-noise, noise + 1, (h, w, 3))
        out.append(np.clip(v, 0, 255).astype(np.uint8))
    return out


def _full(sizes):
    return [np.full((h, w), 255, np.uint8) for w, h in sizes]


def _serpentine(w, h, width=3, pitch=8):
    """A corridor `width` pixels wide folded over the frame: horizontal runs every `pitch` rows, joined at alternating ends."""
    m = np.zeros((h, w), np.uint8)
    rows = list(range(2, h - width - 1, pitch))
    for k, y in enumerate(rows):
        m[y:y + width, 2:w - 2] = 255
        if k + 1 < len(rows):
            x = w - 2 - width if k % 2 == 0 else 2
            m[y:rows[k + 1] + width, x:x + width] = 255
    return m, rows


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name in ("texture", "constant", "holes", "empty"):
        sizes, corners = [(48, 40), (48, 40)], [(0, 0), (28, 0)]                  # overlap: 20 columns
        images = _textured(11, sizes, corners)
        masks = _full(sizes)
        if name == "constant":
            images = [np.full((40, 48, 3), 120, np.uint8), np.full((40, 48, 3), 120, np.uint8)]
        if name == "holes":
            masks[0][10:16, 34:40] = 0          # a hole of image 1 inside the overlap
            masks[1][25:31, 6:11] = 0           # a hole of image 2 inside the overlap
            masks[1][5:8, 9:12] = 1             # set means non-zero, not 255
            masks[0][20, :] = 0                 # a cleared row of image 1
            masks[1][33, :] = 0
            masks[0][30:34, 40:44] = 0          # both clear: nodes with no terminal behind penalty edges
            masks[1][30:34, 12:16] = 0
        if name == "empty":
            masks = [np.zeros_like(m) for m in masks]
    elif name == "col1":
        sizes, corners = [(48, 40), (48, 40)], [(0, 0), (47, 3)]
        images, masks = _textured(12, sizes, corners), _full(sizes)
    elif name == "row1":
        sizes, corners = [(48, 40), (44, 38)], [(0, 0), (5, 39)]
        images, masks = _textured(13, sizes, corners), _full(sizes)
    elif name == "tiny":                        # roi 8 x 8, grid 28 x 28: smaller than one 32 x 32 tile
        sizes, corners = [(20, 16), (20, 16)], [(0, 0), (12, 8)]
        images, masks = _textured(14, sizes, corners), _full(sizes)
    elif name == "big":                         # roi 130 x 110, grid 150 x 130: 5 x 5 tiles, none of the last ones full
        sizes, corners = [(160, 110), (157, 113)], [(0, 0), (30, -2)]
        images, masks = _textured(15, sizes, corners, noise=12), _full(sizes)
    elif name == "inside":                      # image 1 wholly inside image 2: no source terminal
        sizes, corners = [(24, 20), (48, 40)], [(10, 8), (0, 0)]
        images, masks = _textured(16, sizes, corners), _full(sizes)
    elif name == "serpentine":
        sizes, corners = [(70, 52), (70, 52)], [(0, 0), (3, 1)]
        images = _textured(17, sizes, corners)
        s, rows = _serpentine(66, 50)           # the corridor in world coordinates, inside both frames
        w1, w2 = np.zeros((53, 73), np.uint8), np.zeros((53, 73), np.uint8)
        w1[2:52, 4:70] = s
        w2[2:52, 4:70] = s
        w2[2 + rows[0]:2 + rows[0] + 3, 4:12] = 0              # its first stretch is image 1's alone: the source terminals
        xe = 4 + 2 if (len(rows) - 1) % 2 else 4 + 66 - 2 - 6  # (the last run ends on the left when its index is odd)
        w1[2 + rows[-1]:2 + rows[-1] + 3, xe:xe + 6] = 0       # its last stretch is image 2's alone: the sink terminals
        masks = [np.ascontiguousarray(w1[0:52, 0:70]), np.ascontiguousarray(w2[1:53, 3:73])]
    elif name == "three":                       # every pair overlaps, all three share a region
        sizes, corners = [(48, 40), (44, 42), (50, 36)], [(0, 0), (22, 6), (10, 18)]
        images, masks = _textured(18, sizes, corners), _full(sizes)
    elif name == "four":
        sizes, corners = [(40, 36), (40, 36), (40, 36), (40, 36)], [(0, 0), (22, 2), (3, 19), (24, 20)]
        images, masks = _textured(19, sizes, corners), _full(sizes)
        images[3][...] = 90                     # a constant frame among the textured ones
    else:
        raise KeyError(name)
    for a in images + masks:
        a.setflags(write=False)
    return images, corners, masks


def scene(name):
    """-> (images, corners, masks); the arrays are shared and read-only."""
    return _scene(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (masks, record): the reference's masks and, per processed pair (i, j), (cap_right, cap_down, terminals, S, flow)."""
    images, corners, masks = scene(name)
    record = {}
    out = gc.find(images, corners, masks, record=record)
    for a in out:
        a.setflags(write=False)
    return out, record


def single_pair_graph(name, i=0, j=1):
    """The pair's graph on the scene's masks as given (what the library's debug entry builds)."""
    images, corners, masks = scene(name)
    sizes = [(m.shape[1], m.shape[0]) for m in masks]
    roi = gc.overlap_roi(corners[i], sizes[i], corners[j], sizes[j])
    cr, cd, term = gc.capacities(images[i], images[j], masks[i], masks[j], corners[i], corners[j], roi)
    return cr, cd, term


# ------------------------------------------------------------------------------------------------ the reference itself
def _networkx_cut(cr, cd, term, reverse=False):
    """networkx.minimum_cut -> (value, its source side as a plane).  networkx returns as the sink side the nodes that reach the sink
    in its residual graph, so its source side is the MAXIMAL one.  reverse: the same graph with every edge turned round, cut from
    the sink to the source (the grid edges are symmetric, so only the terminals swap)."""
    import networkx as nx
    gh, gw = term.shape
    g = nx.DiGraph()
    g.add_nodes_from(["s", "t"])
    for y in range(gh):
        for x in range(gw):
            if x + 1 < gw and cr[y, x] > 0:
                g.add_edge((y, x), (y, x + 1), capacity=int(cr[y, x])); g.add_edge((y, x + 1), (y, x), capacity=int(cr[y, x]))
            if y + 1 < gh and cd[y, x] > 0:
                g.add_edge((y, x), (y + 1, x), capacity=int(cd[y, x])); g.add_edge((y + 1, x), (y, x), capacity=int(cd[y, x]))
            t = -term[y, x] if reverse else term[y, x]
            if t > 0:
                g.add_edge("s", (y, x), capacity=int(t))
            elif t < 0:
                g.add_edge((y, x), "t", capacity=int(-t))
    value, (reach, _) = nx.minimum_cut(g, "s", "t")
    side = np.zeros((gh, gw), bool)
    for p in reach:
        if p != "s":
            side[p] = True
    return value, side


@pytest.mark.parametrize("name", ["tiny", "constant"])
def test_cut_value_and_both_extreme_cuts_equal_networkx(name):
    """Forward, networkx's source side is the complement of the reference's sink-reaching set; on the reversed graph its source
    side is the complement of the reference's S -- there the nodes that reach its sink are the nodes the source reaches here."""
    cr, cd, term = single_pair_graph(name)
    value, S, T = gc.min_cut(cr, cd, term)
    want_value, maximal = _networkx_cut(cr, cd, term)
    rev_value, not_minimal = _networkx_cut(cr, cd, term, reverse=True)
    assert value == want_value == rev_value and value > 0
    assert np.array_equal(~T, maximal)
    assert np.array_equal(S, ~not_minimal)
    assert not np.array_equal(S, ~T)                # both scenes have ties: the two checks are not one


@pytest.mark.parametrize("name", RANDOM)
def test_textured_scenes_have_a_unique_cut(name):
    for (i, j), (cr, cd, term, S, value) in reference(name)[1].items():
        _, S2, T = gc.min_cut(cr, cd, term)
        assert np.array_equal(S, S2)
        assert np.array_equal(S, ~T), "pair (%d, %d): %d nodes between the minimal and the maximal cut" % (i, j, (~S & ~T).sum())
        assert value > 0 and S.any() and not S.all()


def test_constant_scene_is_in_the_tie_regime():
    cr, cd, term, S, value = reference("constant")[1][(0, 1)]
    _, _, T = gc.min_cut(cr, cd, term)
    between = int((~S & ~T).sum())
    print("constant: %d of %d nodes between the minimal and the maximal cut" % (between, S.size))
    assert value > 0 and between >= 100 and not (S & T).any()
    cr, cd, term, S, value = reference("tiny")[1][(0, 1)]
    _, _, T = gc.min_cut(cr, cd, term)
    assert int((~S & ~T).sum()) == 2 * 9 * 9 and not term[~S & ~T].any()


def test_degenerate_scenes_reach_their_regimes():
    cr, cd, term, S, value = reference("inside")[1][(0, 1)]
    assert not (term > 0).any() and (term < 0).any() and value == 0 and not S.any()
    images, corners, masks = scene("inside")
    out = reference("inside")[0]
    assert not out[0].any() and np.array_equal(out[1], masks[1])          # image 1 loses everything, image 2 nothing
    cr, cd, term, S, value = reference("empty")[1][(0, 1)]
    assert not term.any() and value == 0 and not S.any()
    assert all(np.array_equal(a, b) for a, b in zip(reference("empty")[0], scene("empty")[2]))
    cr, cd, term, S, value = reference("holes")[1][(0, 1)]
    assert (cr >= 1000 * 255).any() and (cr[:, :-1] < 1000 * 255).any()    # penalty edges and plain ones
    for name, shape in (("col1", (57, 21)), ("row1", (21, 63)), ("tiny", (28, 28)), ("big", (130, 150))):
        assert reference(name)[1][(0, 1)][2].shape == shape


def test_every_scene_changes_masks_or_is_meant_not_to():
    for name in NAMES:
        out, masks = reference(name)[0], scene(name)[2]
        changed = sum(int((a != b).sum()) for a, b in zip(out, masks))
        assert (changed == 0) == (name == "empty"), name


def test_serpentine_source_and_sink_sit_at_the_corridor_ends():
    cr, cd, term, S, value = reference("serpentine")[1][(0, 1)]
    assert (term > 0).any() and (term < 0).any() and value > 0
    ys, xs = np.nonzero(term > 0)
    yt, xt = np.nonzero(term < 0)
    assert abs(int(ys.mean()) - int(yt.mean())) >= 30                      # the folds lie between them


def test_pair_order_matters_on_the_shared_overlaps():
    """Dependency levels may not reorder pairs that share an image: another order gives other masks."""
    for name in ("three", "four"):
        images, corners, masks = scene(name)
        pairs = [(i, j) for i, j, _ in gc.pair_list(corners, [(m.shape[1], m.shape[0]) for m in masks])]
        assert len(pairs) == (3 if name == "three" else 6)
        other = gc.find(images, corners, masks, order=pairs[::-1])
        assert any(not np.array_equal(a, b) for a, b in zip(other, reference(name)[0])), name


@pytest.mark.parametrize("name", NAMES)
def test_capacities_stay_below_the_bounds(name):
    edge, term_max = gc.max_edge_capacity(), gc.max_terminal_capacity()
    assert edge == 99743504 and term_max == 2550000 and 4 * 99743505 + term_max < gc.INFLOW_BOUND     # (390151 + 1000) * 255 = 99 743 505 rounds to float32
    for cr, cd, term, S, value in reference(name)[1].values():
        assert 0 <= cr.min() and cr.max() <= edge and 0 <= cd.min() and cd.max() <= edge and np.abs(term).max() <= term_max
        assert not cr[:, -1].any() and not cd[-1, :].any()


# ------------------------------------------------------------------------------------------------ plumbing
def test_finder_names_and_refusals():
    import image_stitching_amd as isa
    f = isa.GraphCutSeamFinder(None)
    assert (f.cost_type, f.terminal_cost, f.bad_region_penalty) == ("COST_COLOR", 10000.0, 1000.0)
    assert isa.GraphCutSeamFinder(None, "COST_COLOR", 5.0, 7.0).bad_region_penalty == 7.0
    with pytest.raises(NotImplementedError, match="COST_COLOR_GRAD"):
        isa.GraphCutSeamFinder(None, "COST_COLOR_GRAD")
    for bad in ("COLOR", "cost_color", "gc_color", 0):
        with pytest.raises(ValueError):
            isa.GraphCutSeamFinder(None, bad)
    assert "GraphCutSeamFinder" in isa.__all__
    assert callable(isa.Stitcher.set_seam_finder)


def test_configuration_names_stay_refused():
    from image_stitching_amd.stitching import SEAM_FIND_TYPES, StitchConfig, check_seam_config
    assert SEAM_FIND_TYPES == ("no", "voronoi", "dp_color", "dp_colorgrad")
    for name in ("gc_color", "gc_colorgrad"):
        with pytest.raises(NotImplementedError, match=name) as e:
            check_seam_config(StitchConfig(seam_find_type=name))
        assert "outside this library" not in str(e.value) and "GraphCutSeamFinder" in str(e.value)


def test_header_and_bindings_name_the_new_entries():
    from image_stitching_amd import _capi
    for name in ("mis_seam_graphcut", "mis_seam_graphcut_debug_pair", "mis_seam_graphcut_stats"):
        assert name in _capi.PROTOTYPES and name in _capi.header_functions()
    assert len(_capi.PROTOTYPES["mis_seam_graphcut"][1]) == 8
