"""GPU: isa.GraphCutSeamFinder (mis_seam_graphcut; the device push-relabel of csrc/seam_gc.hip) against the numpy / scipy reference
tests/refimpl_seam_graphcut.py -- masks bit for bit on every scene of test_refimpl_seam_graphcut_cpu.py (which asserts the regime
each one reaches: a unique cut, ties, a 1-pixel overlap, a grid below one 32 x 32 tile and one of 5 x 5 tiles, penalty edges and
nodes without terminals, no source, no terminals, a folded corridor, three and four frames with shared overlaps), and through
mis_seam_graphcut_debug_pair the integer capacities, the terminals and the label plane, gap included.  No tolerance anywhere: with
integer capacities the minimal source side is the same set for every maximum flow.

No test forces the round-set cap: the serpentine scene must converge under it."""
import numpy as np
import pytest

import refimpl_seam_graphcut as gc
from test_refimpl_seam_dp_gpu import _dev, _np, _pitched
from test_refimpl_seam_graphcut_cpu import NAMES, reference, scene

pytestmark = pytest.mark.gpu

MIS_E_INVALID, MIS_E_UNSUPPORTED = -1, -6


def _check_masks(got, want, name, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g = _np(g)
        assert g.shape == w.shape and g.dtype == np.uint8
        assert np.array_equal(g, w), "%s, %s: mask %d differs in %d pixels, first at %s" % (name, what, k, (g != w).sum(), np.argwhere(g != w)[0])


@pytest.mark.parametrize("name", NAMES)
def test_masks_equal_reference_device_and_host(ctx, name):
    """Every scene, once with device tensors and once with host arrays; the images are read only."""
    import image_stitching_amd as isa
    im, c, m = scene(name)
    want = reference(name)[0]
    di, dm = [_dev(i) for i in im], [_dev(k) for k in m]
    finder = isa.GraphCutSeamFinder(ctx)
    assert finder.find(di, c, dm) is dm
    _check_masks(dm, want, name, "device tensors")
    st = finder.stats()
    print("%s: %r" % (name, st))
    assert st["pairs"] == len(reference(name)[1]) and len(st["round_sets"]) == st["levels"]
    assert all(s < st["round_set_cap"] for s in st["round_sets"])
    hm = [k.copy() for k in m]
    isa.GraphCutSeamFinder(ctx, "COST_COLOR", 10000.0, 1000.0).find([i.copy() for i in im], c, hm)
    _check_masks(hm, want, name, "host arrays")
    for a, b in zip(di, im):
        assert np.array_equal(_np(a), b)


@pytest.mark.parametrize("name", NAMES)
def test_capacities_terminals_and_labels_equal_reference(ctx, name):
    """The debug entry builds and cuts one pair on the masks as given: the first pair of a scene sees them so in the reference's
    run too, so its record is the expectation for the capacity build and for the solver's label plane separately."""
    import image_stitching_amd as isa
    im, c, m = scene(name)
    (i, j), (cr, cd, term, S, value) = next(iter(reference(name)[1].items()))
    dm = [_dev(k) for k in m]
    gcr, gcd, gterm, lab = isa.GraphCutSeamFinder(ctx).debug_pair([_dev(x) for x in im], c, dm, i, j)
    assert gcr.shape == cr.shape and gcr.dtype == np.int32 and lab.dtype == np.uint8
    assert np.array_equal(gcr, cr), "cap_right differs in %d nodes" % (gcr != cr).sum()
    assert np.array_equal(gcd, cd), "cap_down differs in %d nodes" % (gcd != cd).sum()
    assert np.array_equal(gterm, term), "terminals differ in %d nodes" % (gterm != term).sum()
    assert set(np.unique(lab)) <= {0, 1}
    assert np.array_equal(lab.astype(bool), S), "labels differ in %d of %d nodes" % ((lab.astype(bool) != S).sum(), S.size)
    for g, w in zip(dm, m):
        assert np.array_equal(_np(g), w)                      # the debug entry edits nothing


@pytest.mark.parametrize("name", ["three", "four"])
def test_later_pairs_of_shared_overlaps_through_the_debug_entry(ctx, name):
    """A later pair's graph on the masks its predecessors left (the reference's masks just before the pair)."""
    import image_stitching_amd as isa
    im, c, m = scene(name)
    sizes = [(k.shape[1], k.shape[0]) for k in m]
    cur = [np.array(k) for k in m]
    finder = isa.GraphCutSeamFinder(ctx)
    for i, j, roi in gc.pair_list(c, sizes):
        cr, cd, term, S, value = reference(name)[1][(i, j)]
        gcr, gcd, gterm, lab = finder.debug_pair(im, c, cur, i, j)          # host arrays here
        assert np.array_equal(gcr, cr) and np.array_equal(gcd, cd) and np.array_equal(gterm, term), (i, j)
        assert np.array_equal(lab.astype(bool), S), (i, j)
        gc.find_in_pair(im[i], im[j], cur[i], cur[j], c[i], c[j], roi)
    _check_masks(cur, reference(name)[0], name, "pair by pair")


def test_serpentine_stays_under_the_cap(ctx):
    import image_stitching_amd as isa
    im, c, m = scene("serpentine")
    dm = [_dev(k) for k in m]
    finder = isa.GraphCutSeamFinder(ctx)
    finder.find([_dev(i) for i in im], c, dm)
    _check_masks(dm, reference("serpentine")[0], "serpentine", "device tensors")
    st = finder.stats()
    print("serpentine: %r" % (st,))
    assert st["levels"] == 1 and 0 < st["round_sets"][0] < st["round_set_cap"]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_pitched_views_at_odd_addresses(ctx, device):
    import image_stitching_amd as isa
    for name in ("holes", "three"):
        im, c, m = scene(name)
        pi = [_pitched(i, device) for i in im]
        pm = [_pitched(k, device) for k in m]
        isa.GraphCutSeamFinder(ctx).find([p[1] for p in pi], c, [p[1] for p in pm])
        _check_masks([p[1] for p in pm], reference(name)[0], name, "pitched views")
        for (holder, _, filled), k in zip(pi + pm, list(im) + list(m)):
            got, want = _np(holder).copy(), filled.copy()
            got[1:1 + k.shape[0], 1:1 + k.shape[1]] = 0
            want[1:1 + k.shape[0], 1:1 + k.shape[1]] = 0
            assert np.array_equal(got, want)                   # nothing outside a view is written
        for holder, _, filled in pi:
            assert np.array_equal(_np(holder), filled)


def test_mixed_host_and_device_buffers(ctx):
    import image_stitching_amd as isa
    im, c, m = scene("four")
    images = [_dev(i) if k % 2 else i.copy() for k, i in enumerate(im)]
    masks = [k_.copy() if k % 3 else _dev(k_) for k, k_ in enumerate(m)]
    isa.GraphCutSeamFinder(ctx).find(images, c, masks)
    _check_masks(masks, reference("four")[0], "four", "mixed buffers")


def test_repeat_gives_identical_bits_and_scenes_do_not_leak(ctx):
    """The same scene twice in one process with another one in between (the planes and counters are reused blocks)."""
    import image_stitching_amd as isa
    finder = isa.GraphCutSeamFinder(ctx)
    outs = []
    for name in ("big", "constant", "big"):
        im, c, m = scene(name)
        dm = [_dev(k) for k in m]
        finder.find([_dev(i) for i in im], c, dm)
        _check_masks(dm, reference(name)[0], name, "in the sequence")
        outs.append([_np(k) for k in dm])
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[2]))


def test_other_costs_reach_the_graph(ctx):
    """terminal_cost and bad_region_penalty are the call's, not constants of the kernels."""
    import image_stitching_amd as isa
    im, c, m = scene("holes")
    want = gc.find(im, c, m, terminal_cost=300.0, bad_region_penalty=7.5)
    assert any(not np.array_equal(a, b) for a, b in zip(want, reference("holes")[0]))
    dm = [_dev(k) for k in m]
    isa.GraphCutSeamFinder(ctx, "COST_COLOR", 300.0, 7.5).find([_dev(i) for i in im], c, dm)
    _check_masks(dm, want, "holes", "terminal_cost 300, penalty 7.5")


def _c_call(ctx, images, corners, masks, n, cost_type=0, terminal_cost=10000.0, penalty=1000.0):
    from image_stitching_amd import _capi as capi
    from image_stitching_amd.stitching import as_image
    k = max(1, len(masks))
    cs = (capi.MisPoint * k)(*[capi.MisPoint(int(c[0]), int(c[1])) for c in corners])
    im = (capi.MisImage * k)(*[as_image(i) for i in images])
    mk = (capi.MisImage * k)(*[as_image(m) for m in masks])
    return ctx.lib.mis_seam_graphcut(ctx.h, cs, im, mk, n, cost_type, terminal_cost, penalty)


def test_refusals_leave_the_masks_and_the_context_serves_on(ctx):
    import image_stitching_amd as isa
    im, c, m = scene("texture")
    di, dm = [_dev(i) for i in im], [_dev(k) for k in m]
    assert _c_call(ctx, di, c, dm, 0) == 0                                              # n == 0
    assert _c_call(ctx, di, c, [dm[0], dm[1][:-1]], 2) == MIS_E_INVALID                 # a mask one row short
    assert _c_call(ctx, [di[0][:, :-1], di[1]], c, dm, 2) == MIS_E_INVALID              # an image one column short
    assert _c_call(ctx, [di[0], di[1][:, :, 0].contiguous()], c, dm, 2) == MIS_E_INVALID   # a one-channel image
    assert _c_call(ctx, [di[0], di[1].float()], c, dm, 2) == MIS_E_INVALID              # a float image
    assert _c_call(ctx, di, c, dm, 2, cost_type=1) == MIS_E_UNSUPPORTED                 # COST_COLOR_GRAD, by name
    assert b"COST_COLOR_GRAD" in ctx.lib.mis_last_error(ctx.h)
    assert _c_call(ctx, di, c, dm, 2, cost_type=2) == MIS_E_INVALID
    for tc, pen in ((-1.0, 1000.0), (10000.0, -0.5), (float("nan"), 1000.0), (10000.0, float("inf")), (10000.0, 2.0e6), (1.0e7, 1000.0)):
        assert _c_call(ctx, di, c, dm, 2, 0, tc, pen) == MIS_E_INVALID, (tc, pen)       # not finite, negative, or past the 2^31 inflow bound
    assert ctx.lib.mis_seam_graphcut(None, None, None, None, 0, 0, 10000.0, 1000.0) != 0   # no context
    for g, w in zip(dm, m):
        assert np.array_equal(_np(g), w)
    isa.GraphCutSeamFinder(ctx).find(di, c, dm)
    _check_masks(dm, reference("texture")[0], "texture", "after the refusals")
    # a DP call and a graph-cut call share the context's staging: neither leaves anything for the other
    dm2 = [_dev(k) for k in m]
    isa.DpSeamFinder(ctx).find(di, c, dm2)
    dm3 = [_dev(k) for k in m]
    isa.GraphCutSeamFinder(ctx).find(di, c, dm3)
    _check_masks(dm3, reference("texture")[0], "texture", "after a DP call")
