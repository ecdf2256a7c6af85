"""The affine-partial path bit for bit against tests/golden/affine_bits.json, which tools/affine_golden.py recorded from the
library at the commit the file names: every family case of tests/refimpl_affine.py through estimate_affine_partial (as it stands
and with refine_iters 0 and 1) and one AffineBestOf2NearestMatcher call on the matcher batch.  The reference of refimpl_affine
holds the model to a tolerance; this holds the LM schedule, the pending-flag protocol of the tail launches and the entry's copies
to the recorded bits."""
import json
import os
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import affine_golden  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    with open(affine_golden.GOLDEN) as fh:
        return json.load(fh)


def test_estimate_affine_partial_bits(ctx, golden):
    got = affine_golden.estimate_records(ctx)
    want = golden["estimate"]
    key = lambda r: (r["family"], r["name"], r["refine_iters"])
    assert [key(r) for r in got] == [key(r) for r in want], "the families' cases are not the recorded ones: the generators drifted"
    for g, w in zip(got, want):
        assert g["input"] == w["input"], "%s: the inputs differ from the recorded ones: the generators drifted" % (key(g),)
    for g, w in zip(got, want):
        assert g == w, "%s: got %s, recorded %s" % (key(g), g, w)


def test_affine_matcher_bits(ctx, golden):
    got = affine_golden.matcher_record(ctx)
    want = golden["matcher"]
    assert got["input"] == want["input"], "matcher batch: the inputs differ from the recorded ones: the generators drifted"
    assert len(got["entries"]) == len(want["entries"])
    for k, (g, w) in enumerate(zip(got["entries"], want["entries"])):
        assert g == w, "matcher entry %d: got %s, recorded %s" % (k, g, w)
