"""The homography-based estimator (mis_focals_from_homography, mis_estimate_focal, mis_estimate_homography_cameras; SURVEY Appendix
A.16) against the float64 reference of tests/refimpl_estimator.py, without a GPU: exact tables built from known focals and
rotations, the oracle's match tables of two rendered scenes, every branch, the refusals and the Python surface.  The criteria and
their derivations are in the reference module's docstring."""
import ctypes as C
import functools

import numpy as np
import pytest

import ba_affine_twin as twin
import refimpl_estimator as re_
import refimpl_motion as rm

MIS_E_INVALID = -1      # include/mistitch.h


def _bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


def _lib():
    from image_stitching_amd import _capi as capi
    return capi, capi.load()


def _sizes(capi, sizes):
    arr = (capi.MisSize * len(sizes))()
    for k, (w, h) in enumerate(sizes):
        arr[k].width, arr[k].height = w, h
    return arr


def lib_focals(H):
    capi, lib = _lib()
    h = (C.c_double * 9)(*np.asarray(H, np.float64).reshape(9))
    f0, f1, ok0, ok1 = C.c_double(), C.c_double(), C.c_int(-1), C.c_int(-1)
    assert lib.mis_focals_from_homography(h, C.byref(f0), C.byref(f1), C.byref(ok0), C.byref(ok1)) == capi.MIS_OK
    assert ok0.value in (0, 1) and ok1.value in (0, 1)
    return f0.value, f1.value, bool(ok0.value), bool(ok1.value)


def lib_estimate(n, tab, sizes):
    """-> (focals, cameras) of the library on the table of dicts."""
    capi, lib = _lib()
    mis, keep = twin.marshal_table(n, tab)
    focals = (C.c_double * n)()
    assert lib.mis_estimate_focal(mis, n, _sizes(capi, sizes), focals) == capi.MIS_OK
    cams = (capi.MisCameraParams * n)()
    assert lib.mis_estimate_homography_cameras(mis, n, _sizes(capi, sizes), cams) == capi.MIS_OK
    return list(focals), twin._cams_out(cams, n)


def lib_candidates(n, tab):
    """The library's sqrt(f0 f1) candidates in table order.  The C ABI returns no candidate list, but one candidate is observable:
    mis_estimate_focal on a two-camera table that holds only one entry has at most one candidate, one is >= n - 1 = 1, so the focal
    that comes back is that candidate itself; where the entry's focals are not both ok it is the naive focal instead."""
    capi, lib = _lib()
    empty = dict(matches=np.zeros(0, rm.DMATCH_DTYPE), inliers_mask=np.zeros(0, np.uint8), src_img_idx=-1, dst_img_idx=-1, num_inliers=0, has_H=0, H=None, confidence=0.0)
    sizes, out = _sizes(capi, [(641, 361), (643, 363)]), []
    for k in range(n * n):
        if not tab[k]["has_H"]:
            continue
        two = [dict(empty) for _ in range(4)]
        two[1] = dict(empty, src_img_idx=0, dst_img_idx=1, num_inliers=int(tab[k]["num_inliers"]), has_H=1, H=tab[k]["H"], confidence=1.0)
        mis, keep = twin.marshal_table(2, two)
        focals = (C.c_double * 2)()
        assert lib.mis_estimate_focal(mis, 2, sizes, focals) == capi.MIS_OK and focals[0] == focals[1]
        f0, f1, ok0, ok1 = lib_focals(tab[k]["H"])
        if ok0 and ok1:
            out.append(focals[0])
        else:
            assert focals[0] == (641 + 361 + 643 + 363) / 2
    return out


def check_against_reference(n, tab, sizes):
    """The library on a table against the reference on it, by the module's criteria -> (reference result, library cameras)."""
    for k in range(n * n):
        if tab[k]["has_H"]:
            want, got = re_.focals_from_homography(tab[k]["H"]), lib_focals(tab[k]["H"])
            assert got[2:] == want[2:] and np.array_equal(_bits(got[:2]), _bits(want[:2])), ("focals of pair", divmod(k, n), got, want)
    ref = re_.estimate_cameras(n, tab, sizes)
    cand = lib_candidates(n, tab)
    assert len(cand) == len(ref["candidates"]) and np.array_equal(_bits(cand), _bits(ref["candidates"])), ("candidates", cand, ref["candidates"])
    focals, cams = lib_estimate(n, tab, sizes)
    assert np.array_equal(_bits(focals), _bits([ref["focal"]] * n))
    worst = re_.check_cameras(ref, cams, sizes)
    return ref, cams, worst


# ------------------------------------------------------------------------------------------------ the reference's own tree
def _poses(n):
    return [re_.rot(15.0 * i - 20.0, 3.0 * ((i % 3) - 1), 2.0 * ((i % 2) - 0.5)) for i in range(n)]


def _exact(focals, weights=None):
    n = len(focals)
    edges = [(i, i + 1) for i in range(n - 1)] + [(i, i + 2) for i in range(n - 2)]
    Rs = _poses(n)
    tab, herr = re_.exact_table(focals, Rs, edges, weights)
    return n, Rs, edges, tab, herr


def test_reference_tree_equals_scipy_where_weights_are_distinct():
    for focals in ([500.0] * 4, [500.0] * 7):
        n, Rs, edges, tab, _ = _exact(focals)
        assert len({tab[i * n + j]["num_inliers"] for i, j in edges}) == len(edges)
        centres, adj, tree = re_.spanning_tree(n, tab)
        centre, forest = rm.tree_centre(n, tab)
        mine = np.zeros((n, n), bool)
        for i, j in tree:
            mine[i, j] = mine[j, i] = True
        assert np.array_equal(mine, forest) and centre == centres[0] == re_.walk(n, tab)[0]
        assert len(tree) == n - 1


# ------------------------------------------------------------------------------------------------ exact tables
@pytest.mark.parametrize("focals", [[500.0] * 4, [480.0, 650.0, 480.0, 650.0, 480.0]], ids=["equal", "two-focals"])
def test_exact_tables_give_the_true_focals_and_rotations(focals):
    n, Rs, edges, tab, herr = _exact(focals)
    sizes = [(640, 360)] * n
    true_cand, cand_bound = [], 0.0
    for (a, b), He in herr.items():
        f0, f1, ok0, ok1 = lib_focals(tab[a * n + b]["H"])
        b0, b1 = re_.exact_focal_bound(tab[a * n + b]["H"], He)
        print("pair (%d, %d): f0 %.9f (bound %.2e) f1 %.9f (bound %.2e)" % (a, b, f0, b0, f1, b1))
        assert ok0 and ok1
        assert abs(f0 - focals[a]) <= b0 and abs(f1 - focals[b]) <= b1, (a, b, f0 - focals[a], b0, f1 - focals[b], b1)
        true_cand.append(float(np.sqrt(focals[a] * focals[b])))
        cand_bound = max(cand_bound, (re_.Err(f0, b0) * re_.Err(f1, b1)).sqrt().e)
    # the median moves by at most the largest move of a candidate
    got, cams = lib_estimate(n, tab, sizes)
    want = float(np.median(true_cand))
    assert len(set(got)) == 1 and abs(got[0] - want) <= cand_bound + 2 * re_.U * want, (got[0], want, cand_bound)
    ref, _, worst = check_against_reference(n, tab, sizes)
    assert len(ref["candidates"]) == 2 * len(edges)
    if len(set(focals)) == 1:
        # K is the true K up to the focal's bound: the chained rotations are R_c^T R_i.  Only the equal-focal table can be held to
        # the truth here: the estimator gives every camera the one median focal, which cannot reproduce K_from and K_to of two
        # different focals, so R_rel is not R_from^T R_to there; that table's rotations are held to the reference above instead
        ref = re_.estimate_cameras(n, tab, sizes, h_err=herr, f_err=cand_bound + 2 * re_.U * want)
        c = ref["centre"]
        for i in range(n):
            truth = re_._mul(re_._T(re_._mat(Rs[c], re_.E_R)), re_._mat(Rs[i], re_.E_R))
            G = cams[i]["R"]
            bound = 2 * ref["e"][i] + re_._errs(truth) + np.spacing(np.abs(G).astype(np.float32)).astype(np.float64)
            assert (np.abs(G - re_._vals(truth)) <= bound).all(), (i, np.abs(G - re_._vals(truth)).max(), bound.min())
        assert np.array_equal(cams[c]["R"], np.eye(3))


# ------------------------------------------------------------------------------------------------ real tables
@functools.lru_cache(maxsize=None)
def oracle_table(name):
    import oracle
    oracle.lib()
    w, h, cams, frames = re_.scene(name)
    orb = oracle.Orb(w, h)
    feats = []
    for f in frames:
        k, d = orb.run(f)
        feats.append(dict(img_w=w, img_h=h, kps=k, xy=np.stack([k["x"], k["y"]], 1), desc=d))
    pm = oracle.match_all_pairs(feats, oracle.match_default_params(match_conf=0.32))
    return [dict(m, has_H=1 if m.get("has_H", m["H"] is not None) else 0) for m in pm]


@pytest.mark.parametrize("name", ["A", "B"])
def test_library_equals_reference_on_the_oracles_tables(name):
    w, h, cams, _ = re_.scene(name)
    n = len(cams)
    tab = oracle_table(name)
    ref, got, worst = check_against_reference(n, tab, [(w, h)] * n)
    ratio, errs = re_.scene_conditions(ref, cams[0]["f"], [c["R"] for c in cams])
    print("\n    scene %s: %d candidates, median focal %.2f (true %.2f, ratio %.3f), tree edges off by %s degrees, rotations / bound %.3f"
          % (name, len(ref["candidates"]), ref["focal"], cams[0]["f"], ratio, ", ".join("%.2f" % e for e in errs), worst))
    assert len(ref["candidates"]) >= n - 1 and len(ref["edges"]) == n - 1
    if name == "B":
        assert len(ref["candidates"]) % 2 == 0 and max(len(a) for a in re_.spanning_tree(n, tab)[1]) == 2      # an even count, a tree with an inner node


# ------------------------------------------------------------------------------------------------ branches
def test_identity_and_pure_roll_give_no_focal():
    """0 / 0 and x / 0 are IEEE quotients, not traps: the calls return, both focals not ok."""
    for H in (np.eye(3), re_.rot(0, 0, 25.0), np.diag([2.0, 2.0, 1.0]) @ re_.rot(0, 0, -70.0)):
        got, want = lib_focals(H), re_.focals_from_homography(H)
        assert got == want == (0.0, 0.0, False, False), (H, got, want)


def _drop(tab, n, pairs):
    out = [dict(m) for m in tab]
    for i, j in pairs:
        for a, b in ((i, j), (j, i)):
            out[a * n + b] = dict(out[a * n + b], has_H=0, H=None, num_inliers=0)
    return out


def test_median_parities_naive_focal_and_unreached_cameras():
    n, Rs, edges, tab, _ = _exact([500.0, 520.0, 540.0, 560.0])
    sizes = [(640, 360), (640, 360), (480, 270), (640, 360)]
    # all ordered pairs with H: 10 candidates, even; one direction of one pair without its H: 9, odd
    ref, _, _ = check_against_reference(n, tab, sizes)
    assert len(ref["candidates"]) == 10
    odd = [dict(m) for m in tab]
    odd[0 * n + 1] = dict(odd[0 * n + 1], has_H=0, H=None)
    ref, _, _ = check_against_reference(n, odd, sizes)
    assert len(ref["candidates"]) == 9 and ref["focal"] == sorted(ref["candidates"])[4]
    # H = I on the only pairs left: no candidate, fewer than n - 1 -> the naive focal
    few = _drop(tab, n, [(0, 2), (1, 3), (1, 2), (2, 3)])
    for a, b in ((0, 1), (1, 0)):
        few[a * n + b] = dict(few[a * n + b], H=np.eye(3))
    ref, cams, _ = check_against_reference(n, few, sizes)
    assert ref["candidates"] == [] and ref["focal"] == (3 * (640 + 360) + 480 + 270) / 4 == cams[0]["focal"]
    assert [c["ppx"] for c in cams] == [320.0, 320.0, 240.0, 320.0] and [c["ppy"] for c in cams] == [180.0, 180.0, 135.0, 180.0]
    # two candidates of one pair among four cameras: still fewer than n - 1 = 3
    two = _drop(tab, n, [(0, 2), (1, 3), (1, 2), (2, 3)])
    ref, cams, _ = check_against_reference(n, two, sizes)
    assert len(ref["candidates"]) == 2 and cams[0]["focal"] == (3 * (640 + 360) + 480 + 270) / 4
    # cameras 2 and 3 have no edge: their distance to every leaf counts as 0, so they are the tree's centres, the walk from
    # camera 2 reaches nothing and every camera keeps R = I (max_spanning_tree_centers, as the adjusters have it)
    assert ref["centre"] == 2 and all(np.array_equal(c["R"], np.eye(3)) for c in cams)
    # no has_H at all: every R = I, the naive focal
    none = _drop(tab, n, edges)
    ref, cams, _ = check_against_reference(n, none, sizes)
    assert all(np.array_equal(c["R"], np.eye(3)) for c in cams) and cams[3]["focal"] == (3 * (640 + 360) + 480 + 270) / 4


def test_one_camera():
    tab, _ = re_.exact_table([500.0], [np.eye(3)], [])
    ref, cams, _ = check_against_reference(1, tab, [(640, 360)])
    assert cams[0]["focal"] == 1000.0 and np.array_equal(cams[0]["R"], np.eye(3)) and (cams[0]["ppx"], cams[0]["ppy"]) == (320.0, 180.0)


def test_refusals():
    capi, lib = _lib()
    n, Rs, edges, tab, _ = _exact([500.0] * 3)
    mis, keep = twin.marshal_table(n, tab)
    sizes, focals, cams = _sizes(capi, [(640, 360)] * n), (C.c_double * n)(), (capi.MisCameraParams * n)()
    h = (C.c_double * 9)(*np.eye(3).reshape(9))
    d, i = C.c_double(), C.c_int()
    assert lib.mis_focals_from_homography(None, C.byref(d), C.byref(d), C.byref(i), C.byref(i)) == MIS_E_INVALID
    assert lib.mis_focals_from_homography(h, None, C.byref(d), C.byref(i), C.byref(i)) == MIS_E_INVALID
    assert lib.mis_focals_from_homography(h, C.byref(d), C.byref(d), C.byref(i), None) == MIS_E_INVALID
    for bad_n in (0, -1):
        assert lib.mis_estimate_focal(mis, bad_n, sizes, focals) == MIS_E_INVALID
        assert lib.mis_estimate_homography_cameras(mis, bad_n, sizes, cams) == MIS_E_INVALID
    for args in ((None, n, sizes, focals), (mis, n, None, focals), (mis, n, sizes, None)):
        assert lib.mis_estimate_focal(*args) == MIS_E_INVALID
    for args in ((None, n, sizes, cams), (mis, n, None, cams), (mis, n, sizes, None)):
        assert lib.mis_estimate_homography_cameras(*args) == MIS_E_INVALID
    for bad in ([(640, 360), (0, 360), (640, 360)], [(640, 360), (640, 360), (640, -1)]):
        assert lib.mis_estimate_focal(mis, n, _sizes(capi, bad), focals) == MIS_E_INVALID
        assert lib.mis_estimate_homography_cameras(mis, n, _sizes(capi, bad), cams) == MIS_E_INVALID
    assert lib.mis_estimate_homography_cameras(mis, n, sizes, cams) == capi.MIS_OK


# ------------------------------------------------------------------------------------------------ the Python surface
def test_python_functions_equal_the_entries():
    import image_stitching_amd as isa
    n, Rs, edges, tab, _ = _exact([500.0, 520.0, 540.0])
    entries = [(i, j, tab[i * n + j]["matches"], tab[i * n + j]["inliers_mask"], tab[i * n + j]["num_inliers"], 1, tab[i * n + j]["H"], 2.0) for i, j in edges]
    pm = isa.stitching.PairwiseMatches.from_entries(None, n, entries)
    tab2 = re_.table_of(pm)
    focals, cams = lib_estimate(n, tab2, [(640, 360)] * n)
    assert isa.estimate_focal(pm, (640, 360)) == focals == isa.estimate_focal(pm, [(640, 360)] * n)
    got = isa.estimate_homography_cameras(pm, (640, 360))
    for g, c in zip(got, cams):
        assert g["focal"] == c["focal"] and (g["ppx"], g["ppy"]) == (320.0, 180.0) and np.array_equal(g["R"], c["R"])
    assert isa.focals_from_homography(tab2[1]["H"]) == lib_focals(tab2[1]["H"])
    with pytest.raises(TypeError):
        isa.estimate_homography_cameras([], (640, 360))
    with pytest.raises(ValueError):
        isa.estimate_focal(pm, [(640, 360)] * 2)
    with pytest.raises(isa.MisError):
        isa.estimate_focal(pm, (0, 360))


def test_create_panorama_configuration(monkeypatch):
    """create_panorama's stated configuration, on a Stitcher whose finder and matcher are not built (no device here)."""
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as s
    monkeypatch.setattr(s, "OrbFeatureFinder", lambda ctx, size: ("finder", size))
    monkeypatch.setattr(s, "make_matcher", lambda ctx, cfg: ("matcher", cfg.matcher_type))
    st = isa.Stitcher.create_panorama(None, (640, 360))
    hot = isa.StitchConfig.hot_path(matcher_type="homography", wave_correct="horiz")
    assert st.cfg == hot and st.cfg.warp_type == "spherical" and st.kind == isa.WARP_SPHERICAL and st.matcher == ("matcher", "homography")
    assert st.bundle_adjuster is isa.bundle_adjust_ray
    assert st.estimator.func is isa.estimate_homography_cameras and st.estimator.keywords == dict(img_sizes=(640, 360))
    st = isa.Stitcher.create_panorama(None, (640, 360), work_megapix=0.1, warp_type="cylindrical", wave_correct="no", seam_find_type="dp_color")
    assert st.work_scale < 1.0 and st.estimator.keywords == dict(img_sizes=st.work_size) and st.work_size == st.finder[1] != (640, 360)
    assert st.kind == isa.WARP_CYLINDRICAL and st.cfg.wave_correct == "no" and st.cfg.seam_find_type == "dp_color"
    st.set_estimator(None)
    assert st.estimator is None
    assert isa.Stitcher(None, (640, 360), isa.StitchConfig.hot_path()).estimator is None
    with pytest.raises(ValueError, match="estimate_transform has not run"):
        st.compose_panorama([])
