"""Stitcher.set_seam_finder(GraphCutSeamFinder(ctx)) end to end on the 640 x 360 sweep of test_seam_dp_grad_job_gpu.py (its four
frames with a gain each): the seam masks the job used against the numpy / scipy reference run on the very seam-scale images,
corners and masks the finder was handed -- bit for bit --, the panorama against the dp_color one, which it must not equal, and
against a second run, which it must.  A set finder runs with seam_find_type "no" too and replaces a configured finder."""
import numpy as np
import pytest

import refimpl_seam_graphcut as gc
from test_refimpl_seam_dp_grad_cpu import H, W, sweep_cams, sweep_frames

pytestmark = pytest.mark.gpu


def _config(seam):
    import image_stitching_amd as isa
    return isa.StitchConfig.hot_path(compose_megapix=-1, expos_comp_type="gain_blocks", seam_find_type=seam)


class _Recording:
    """A finder object that notes what the seam step hands to the finder inside it, and what comes back."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []

    def find(self, images, corners, masks):
        before = ([i.cpu().numpy() for i in images], [tuple(c) for c in corners], [m.cpu().numpy() for m in masks])
        out = self.inner.find(images, corners, masks)
        self.calls.append(before + ([m.cpu().numpy() for m in out],))
        return out


@pytest.fixture(scope="module")
def sweep(ctx):
    import torch
    import image_stitching_amd as isa
    cams = sweep_cams()
    dev = [torch.from_numpy(f).cuda() for f in sweep_frames(cams)]
    rec = _Recording(isa.GraphCutSeamFinder(ctx))
    st = isa.Stitcher(ctx, (W, H), _config("no"))
    st.set_seam_finder(rec)
    pano, mask = st.compose(dev, cams)
    dp, _ = isa.Stitcher(ctx, (W, H), _config("dp_color")).compose(dev, cams)
    return dict(cams=cams, dev=dev, rec=rec, pano=pano, mask=mask, dp=dp)


def test_seam_masks_equal_reference(sweep):
    assert len(sweep["rec"].calls) == 1                       # seam_find_type "no" and a set finder: the seam step ran, once
    images, corners, masks, got = sweep["rec"].calls[0]
    want = gc.find(images, corners, masks)
    changed = sum(int((a != b).sum()) for a, b in zip(want, masks))
    assert changed > 1000
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), "seam mask %d differs in %d pixels" % (k, (g != w).sum())


def test_panorama_differs_from_dp_color(sweep):
    import torch
    assert sweep["pano"].shape == sweep["dp"].shape and not torch.equal(sweep["pano"], sweep["dp"])


def test_second_run_is_identical_and_the_set_finder_replaces_the_configured_one(ctx, sweep):
    import torch
    import image_stitching_amd as isa
    st = isa.Stitcher(ctx, (W, H), _config("dp_color"))
    st.set_seam_finder(isa.GraphCutSeamFinder(ctx))
    pano, mask = st.compose(sweep["dev"], sweep["cams"])
    assert torch.equal(pano, sweep["pano"]) and torch.equal(mask, sweep["mask"])
    st.set_seam_finder(None)                                  # back to the configured finder
    dp, _ = st.compose(sweep["dev"], sweep["cams"])
    assert torch.equal(dp, sweep["dp"])
    for not_a_finder in ("gc_color", ("gc_color",), 1):        # a finder is an object with find(images, corners, masks), not a name
        with pytest.raises(TypeError):
            st.set_seam_finder(not_a_finder)
