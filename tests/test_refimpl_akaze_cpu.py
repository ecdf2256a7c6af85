"""tests/refimpl_akaze.py (the numpy reference of the AKAZE finder) against facts that need no library: the
FED cycles, the diffusion's conservation, what a constant image and a single blob give, the symmetry under a quarter turn, the
descriptor's layout, and -- with the reference's own float32 planes standing in for a run -- the caps on undecided keypoints, bits
and angles that tests/akaze_check.py holds the library and its host emulation to."""
import math

import numpy as np
import pytest

import akaze_check as ac
import refimpl_akaze as ra


def test_level_plans_of_the_test_shapes():
    for (w, h), n in (((97, 71), 4), ((160, 96), 8), ((159, 96), 4), ((333, 251), 12), ((640, 320), 16)):
        lv = ra.plan(w, h)
        assert len(lv) == n, (w, h, len(lv))
        assert [l["sigma_size"] for l in lv[:4]] == [2, 3, 3, 4] and [l["border"] for l in lv[:4]] == [28, 42, 42, 57]
    assert (ra.plan(160, 96)[4]["w"], ra.plan(160, 96)[4]["h"]) == (80, 48)
    assert len(ra.plan(333, 251, n_octave_layers=3)) == 9


def test_fed_cycles_of_a_640x320_plan():
    levels = ra.plan(640, 320)
    for i in range(1, len(levels)):
        T = levels[i]["etime"] - levels[i - 1]["etime"]
        n, taus, order = ra.level_schedule(levels, i)
        assert n == int(math.ceil(math.sqrt(3 * T / 0.25 + 0.25) - 0.5 - 1e-8) + 0.5) and len(taus) == n
        assert abs(taus.sum() - T) <= 1e-12 * T
        assert sorted(order) == list(range(n))
        assert np.all(taus > 0)
    assert ra.fed_schedule(levels[1]["etime"] - levels[0]["etime"])[0] == 3


def test_diffusion_keeps_the_mean():
    frame = ac.rendered(97, 71)
    start = ra.gauss_blur(ra.gray01(frame), 1.0)
    g = ra.flow(start, 0.4)
    out = ra.diffuse(start, g, ra.fed_schedule(2.0)[1], 0)
    assert abs(out.mean() - start.mean()) <= 1e-14
    assert np.abs(out - start).max() > 1e-4      # (it did diffuse)


def test_a_constant_image_has_no_candidate():
    frame = np.full((96, 160, 3), 90, np.uint8)
    levels, planes, k0, kps = ra.detect(frame)
    assert k0 == 0.03 and kps == []
    assert all(ra.level_candidates(P["Ldet"], lv, np.float32(0.001)) == [] for P, lv in zip(planes, levels))


def _blob(amplitude, n=201, c=100.0, sigma=4.0):
    y, x = np.mgrid[0:n, 0:n]
    g = np.rint(30 + amplitude * np.exp(-((x - c) ** 2 + (y - c) ** 2) / (2 * sigma * sigma))).astype(np.uint8)
    return np.repeat(g[:, :, None], 3, axis=2)


def test_one_blob_gives_one_keypoint_at_its_centre():
    """An isotropic Gaussian blob of sigma 4, 36 grey levels above its background: exactly one keypoint, at its centre.  The
    amplitude matters.  Ldet carries sigma_size^4 and sigma_size is an integer (2, 3, 3, 4 over an octave), so a blob's response is
    not unimodal over the levels: it peaks at the end of every run of equal sigma_size (here 0.0113, 0.0011 | 0.0011, 0.0016 at
    amplitude 40 over levels 0 .. 3).  The suppression of step 6 -- like upstream's -- looks one level up and down only, so a blob
    strong enough to pass the threshold on several runs keeps one keypoint a run (second test).  At this amplitude only the
    strongest run's peak, level 3, is above the threshold 0.001."""
    c = 100.0
    levels, planes, k0, kps = ra.detect(_blob(36))
    assert len(kps) == 1, [(k["level"], k["pt"], k["response"]) for k in kps]
    assert abs(kps[0]["pt"][0] - c) <= 0.5 and abs(kps[0]["pt"][1] - c) <= 0.5, kps[0]["pt"]
    assert kps[0]["class_id"] == 3 and kps[0]["octave"] == 0 and kps[0]["size"] == 2 * 1.5 * 1.6 * 2 ** 0.75


def test_a_strong_blob_keeps_one_keypoint_for_every_run_of_equal_sigma_size():
    kps = ra.detect(_blob(200))[3]
    assert [k["class_id"] for k in kps] == [1, 3, 5]
    assert all(abs(k["pt"][0] - 100) <= 1 and abs(k["pt"][1] - 100) <= 1 for k in kps)


def test_a_quarter_turn_moves_angles_by_90_degrees_and_keeps_the_decided_bits():
    """The scale space, the keypoints and the MLDB sampling turn with the scene exactly.  The orientation does so only up to its
    window grid: the windows start at multiples of 0.15 rad, which a quarter turn does not map onto themselves, so the turned scene's
    best window holds other samples at its two edges, and where two windows score alike another window wins.  A corner
    with two gradient directions of like weight can pick the other one (seen here: a keypoint whose angle stays at 118 degrees).  So
    three keypoints in four must turn by 90 degrees within one window step (8.6 degrees; 40 of 51 do on this scene, typically
    within 0.3).  The descriptor's symmetry is checked at exactly the turned angle, for every keypoint."""
    frame = ac.rendered(256, 256)
    turned = np.ascontiguousarray(np.rot90(frame))      # pixel (x, y) -> (y, 255 - x)
    la, pa, _, ka = ra.detect(frame, tie_band=ac.BAND_COORD)
    lb, pb, _, kb = ra.detect(turned, tie_band=ac.BAND_COORD)
    assert len(ka) == len(kb) > 50
    where = {(k["level"], round(k["pt"][0], 6), round(k["pt"][1], 6)): k for k in kb}
    compared = bits = turned_by_90 = 0
    for k in ka:
        q = where.get((k["level"], round(k["pt"][1], 6), round(255 - k["pt"][0], 6)))
        assert q is not None, k["pt"]
        if min(k["gap"], q["gap"]) > 1e-6 and min(k["edge"], q["edge"]) > 1e-9 and min(k["tie"], q["tie"]) > 1e-9:
            d = (k["angle"] - q["angle"]) % 360
            turned_by_90 += abs(d - 90) <= math.degrees(0.15)
            compared += 1
            P = pb[q["level"]]
            vals, lo, hi = ra.mldb_values(P["Lt"], P["Lx"], P["Ly"], lb[q["level"]], q["pt"], q["size"], (k["angle"] - 90) % 360, tie_band=ac.BAND_COORD)
            dec = ra.mldb_decided(k["lo"], k["hi"], 1e-9) & ra.mldb_decided(lo, hi, 1e-9)
            assert np.array_equal(ra.mldb_bits(k["vals"])[dec], ra.mldb_bits(vals)[dec])
            bits += int(dec.sum())
    assert compared >= 0.9 * len(ka) and turned_by_90 >= 0.75 * compared and bits >= 0.95 * 486 * compared, (len(ka), compared, turned_by_90, bits)


def test_descriptor_rows_are_61_bytes_with_clear_pad_bits():
    assert len(ra.bit_pairs()) == 486 and len(ra.cells()) == 29
    assert [c[0] for c in ra.cells()].count(7) == 9 and ra.cells()[12] == (7, 4, 4)      # the 7-step grid's last cell runs from 4 to 10
    row = ra.pack_bits(np.ones(486, bool))
    assert row.shape == (61,) and row.dtype == np.uint8 and row[60] == 0x3F and np.all(row[:60] == 0xFF)
    bits = np.random.default_rng(0).integers(0, 2, 486).astype(bool)
    assert np.array_equal(ra.unpack_bits(ra.pack_bits(bits)), bits)
    _, _, _, kps = ra.detect(ac.rendered(333, 251))
    assert len(kps) > 100 and all(k["desc"].shape == (61,) and not k["desc"][60] & 0xC0 for k in kps)


@pytest.fixture(scope="module")
def cases():
    return ac.cases()


@pytest.mark.parametrize("i", range(8))
def test_the_references_float32_planes_stay_inside_bands_and_caps(cases, i):
    """The reference in float32 with another summation order, judged as a run: every band holds and the undecided shares stay under
    their caps on every chosen frame (so the caps are conditions the frames meet, not measurements of the library)."""
    c = cases[i]
    rep = ac.check_run(c["tag"], c["frame"], c["kw"], ac.reference_run(c["frame"], c["kw"]))
    print(c["tag"], rep)
