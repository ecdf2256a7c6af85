"""A view out of a finished job: host/stitch_main --view writes view.ppm = the exact reference's remap
(tests/refimpl_warp_backward.py, (LINEAR, CONSTANT)) of that run's result.ppm through the HOST forward map of the view's camera;
Stitcher.render_view gives the same bytes; result.ppm, result_mask.pgm and cams.data are what a run without the flag writes."""
import os
import subprocess

import numpy as np
import pytest

import refimpl as ri
import refimpl_warp_backward as rb
from test_host_cpp import HOST, _build, _read_ppm, _write_job

pytestmark = pytest.mark.gpu
VIEW = (20.0, -3.0, 50.0, 257, 131)     # yaw, pitch, hfov, width, height


@pytest.mark.parametrize("warp", ["spherical", "cylindrical"])
def test_stitch_main_view_and_render_view_equal_the_reference(tmp_path, ctx, oracle_mod, warp):
    import torch
    import image_stitching_amd as isa
    _build()
    d0, d1 = str(tmp_path / "plain"), str(tmp_path / "view")
    os.makedirs(d0), os.makedirs(d1)
    cams, frames = _write_job(d0, oracle_mod, n=3, w=480, h=270)
    _write_job(d1, oracle_mod, n=3, w=480, h=270)
    yaw, pitch, hfov, vw, vh = VIEW
    exe = os.path.join(HOST, "stitch_main")
    r0 = subprocess.run([exe, d0, "--warp", warp], capture_output=True, text=True, timeout=600)
    r1 = subprocess.run([exe, d1, "--warp", warp, "--view", "%g,%g,%g,%d,%d" % VIEW], capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0 and r1.returncode == 0, r0.stdout + r0.stderr + r1.stdout + r1.stderr
    for name in ("result.ppm", "result_mask.pgm", "cams.data"):      # unchanged by the flag
        assert open(os.path.join(d0, name), "rb").read() == open(os.path.join(d1, name), "rb").read(), name
    assert not os.path.exists(os.path.join(d0, "view.ppm"))
    pano = _read_ppm(os.path.join(d1, "result.ppm"))
    view = _read_ppm(os.path.join(d1, "view.ppm"))
    assert view.shape == (vh, vw, 3)
    # where the panorama lies in the warper's plane, from the Python stitcher's run of the same job (its panorama is result.ppm)
    size = (frames[0].shape[1], frames[0].shape[0])
    s = isa.Stitcher(ctx, size, isa.StitchConfig.hot_path(compose_megapix=-1, warp_type=warp))
    res, _ = s.compose([torch.from_numpy(f).cuda() for f in frames], cams)
    pano_u8 = np.clip(res.cpu().numpy(), 0, 255).astype(np.uint8)
    assert np.array_equal(pano_u8, pano)
    c = s.composition
    K, R, _ = ri.camera(vw, vh, hfov, yaw, pitch)
    uv = isa.RotationWarper(None, c["warp_scale"], c["kind"]).warp_points(rb.view_points(vw, vh), K, R)
    xm, ym = rb.back_maps_f32(uv, c["pano_tl"], (vh, vw))
    want = rb.remap_exact(pano, xm, ym, rb.INTER_LINEAR, rb.BORDER_CONSTANT)
    assert (rb.nearest_mask(pano.shape, xm, ym) == 255).mean() > 0.5        # the view looks into the panorama
    assert np.array_equal(view, want)
    got = s.render_view(torch.from_numpy(pano_u8).cuda(), K, R, (vw, vh))
    assert np.array_equal(got.cpu().numpy(), want)
    # a malformed --view is refused before anything runs
    r = subprocess.run([exe, d1, "--view", "20,0,50,257"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--view" in r.stdout
