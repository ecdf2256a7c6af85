"""CPU: the host side of the timelapse output -- cv::detail::resultRoiIntersection against a numpy restatement, the new entries in
the built library and its bindings, the configuration name and the driver's refusal of --timelapse with --view."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOST = os.path.join(ROOT, "host")
E_INVALID = -1

NEW_ENTRIES = ["mis_result_roi_intersection", "mis_timelapser_create", "mis_timelapser_destroy", "mis_timelapser_initialize", "mis_timelapser_dst_roi",
               "mis_timelapser_process", "mis_timelapse_warp_batch", "mis_timelapse_warp_batch_timed"]


def _rectangle_sets():
    """200 seeded sets of 1 .. 6 rectangles: overlapping ones, disjoint ones, and sets whose intersection is exactly one pixel
    wide, high or both."""
    rng = np.random.default_rng(79)
    sets = []
    for k in range(200):
        n = int(rng.integers(1, 7))
        mode = k % 4
        if mode == 0:        # anything: mostly disjoint or barely overlapping
            xy = rng.integers(-300, 300, (n, 2))
            wh = rng.integers(1, 250, (n, 2))
        elif mode == 1:      # all contain a common block
            cx, cy = rng.integers(-100, 100, 2)
            xy = np.stack([cx - rng.integers(0, 90, n), cy - rng.integers(0, 90, n)], 1)
            wh = np.stack([cx - xy[:, 0] + rng.integers(1, 90, n), cy - xy[:, 1] + rng.integers(1, 90, n)], 1)
        elif mode == 2:      # a single-pixel intersection: one rectangle ends where another one's first pixel lies
            px, py = rng.integers(-50, 50, 2)
            xy = np.stack([px - rng.integers(0, 40, n), py - rng.integers(0, 40, n)], 1)
            wh = np.stack([px - xy[:, 0] + rng.integers(1, 40, n), py - xy[:, 1] + rng.integers(1, 40, n)], 1)
            xy[0] = (px, py)
            wh[0] = rng.integers(1, 40, 2)
            if n > 1:
                wh[1] = (px - xy[1, 0] + 1, py - xy[1, 1] + 1)      # ends at (px, py)
            else:
                wh[0] = (1, 1)
        else:                # touching but disjoint: the far edge of one is the near edge of another (width 0)
            xy = rng.integers(-60, 60, (max(n, 2), 2))
            wh = rng.integers(5, 80, (max(n, 2), 2))
            xy[1, 0] = xy[0, 0] + wh[0, 0]
        sets.append((xy.astype(int), wh.astype(int)))
    return sets


def _intersection_np(xy, wh):
    tl = xy.max(0)
    br = (xy + wh).min(0)
    return int(tl[0]), int(tl[1]), int(br[0] - tl[0]), int(br[1] - tl[1])


def test_result_roi_intersection_equals_numpy_restatement():
    import image_stitching_amd as isa
    from image_stitching_amd import _capi as capi
    lib = capi.load()
    refused = single = 0
    for xy, wh in _rectangle_sets():
        x, y, w, h = _intersection_np(xy, wh)
        corners, sizes = [tuple(p) for p in xy], [tuple(s) for s in wh]
        if w <= 0 or h <= 0:
            refused += 1
            with pytest.raises(ValueError, match=r"Rect\(tl = \(%d, %d\), br = \(%d, %d\)\) is empty" % (x, y, x + w, y + h)):
                isa.result_roi_intersection(corners, sizes)
            n = len(corners)
            r = capi.MisRect(7, 7, 7, 7)
            pts = (capi.MisPoint * n)(*[capi.MisPoint(*p) for p in corners])
            szs = (capi.MisSize * n)(*[capi.MisSize(*s) for s in sizes])
            assert lib.mis_result_roi_intersection(pts, szs, n, C.byref(r)) == E_INVALID and (r.x, r.y, r.width, r.height) == (7, 7, 7, 7)
        else:
            single += w == 1 or h == 1
            assert isa.result_roi_intersection(corners, sizes) == (x, y, w, h), (corners, sizes)
    assert refused >= 50 and single >= 20, (refused, single)
    # one rectangle is its own intersection; null pointers and n < 1 are refused
    assert isa.result_roi_intersection([(-3, 4)], [(5, 6)]) == (-3, 4, 5, 6)
    r, p, s = capi.MisRect(), (capi.MisPoint * 1)(capi.MisPoint(0, 0)), (capi.MisSize * 1)(capi.MisSize(2, 2))
    assert lib.mis_result_roi_intersection(None, s, 1, C.byref(r)) == E_INVALID and lib.mis_result_roi_intersection(p, None, 1, C.byref(r)) == E_INVALID
    assert lib.mis_result_roi_intersection(p, s, 0, C.byref(r)) == E_INVALID and lib.mis_result_roi_intersection(p, s, 1, None) == E_INVALID
    # extremes do not wrap: the far corner is a 64-bit sum
    big = 2 ** 31 - 1
    assert isa.result_roi_intersection([(big - 10, 0), (big - 4, 0)], [(big, 5), (20, 5)]) == (big - 4, 0, 20, 5)


def test_new_entries_are_exported_declared_and_bound():
    import image_stitching_amd as isa
    from image_stitching_amd import _capi as capi
    lib = C.CDLL(capi.LIB_PATH)
    declared = capi.header_functions()
    for name in NEW_ENTRIES:
        assert hasattr(lib, name), name + " is not exported by libmistitch.so"
        assert name in declared and name in capi.PROTOTYPES, name
    assert (capi.TIMELAPSE_AS_IS, capi.TIMELAPSE_CROP) == (0, 1)
    for name in ("Timelapser", "result_roi_intersection", "timelapse_warp_batch"):
        assert getattr(isa, name) is getattr(isa.stitching, name) is getattr(isa.timelapse, name), name
    # every new declaration cites the reference line it replaces
    header = open(capi.HEADER_PATH).read()
    section = header[header.index("timelapse -----"):header.index("JPEG ingest -----")]
    for cite in (":79", ":82", ":1083", ":1196", ":1197", ":1203-1204", ":1214"):
        assert cite in section, cite


def test_timelapse_type_is_checked_by_name():
    import image_stitching_amd as isa
    assert isa.StitchConfig().timelapse_type == "crop" and isa.StitchConfig(timelapse_type="as_is").timelapse_type == "as_is"
    assert isa.StitchConfig.hot_path().timelapse_type == "crop" and isa.StitchConfig.reference().timelapse_type == "crop"
    for bad in ("nonsense", "CROP", "", None, 1):
        with pytest.raises(ValueError, match="timelapse_type %s" % ("'nonsense'" if bad == "nonsense" else "")):
            isa.StitchConfig(timelapse_type=bad)


def test_stitch_main_refuses_timelapse_with_view_by_name(tmp_path):
    subprocess.run(["make", "-C", HOST, "stitch_main"], check=True, capture_output=True)
    exe = os.path.join(HOST, "stitch_main")
    for args in (["--timelapse", "--view", "0,0,60,64,48"], ["--timelapse", "crop", "--view", "0,0,60,64,48"],
                 ["--warp", "plane", "--timelapse", "as_is", "--view", "10,0,60,64,48"]):
        r = subprocess.run([exe, str(tmp_path)] + args, capture_output=True, text=True)
        assert r.returncode != 0 and "--timelapse" in r.stdout and "--view" in r.stdout and "no panorama" in r.stdout, (args, r.stdout)
    r = subprocess.run([exe, str(tmp_path), "--timelapse", "sideways"], capture_output=True, text=True)
    assert r.returncode != 0 and "timelapse_type 'sideways'" in r.stdout, r.stdout
    # the flag alone is accepted: the driver gets as far as looking for frames
    r = subprocess.run([exe, str(tmp_path), "--timelapse", "as_is"], capture_output=True, text=True)
    assert r.returncode != 0 and "Need more images" in r.stdout, r.stdout
