"""work_megapix without a GPU: the scales and sizes of image_stitching.cpp:589-603 and :1113-1125 as the package computes them,
against hand-written values, and the refusal of an engine that cannot resize frames to work scale."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H, NFRAMES = 256, 144, 4


def _cams():
    import synth
    return [synth.make_camera(W, H, 60.0, 13.0 * i - 20.0, 0.4 * ((i % 3) - 1), 0.3 * ((i % 2) - 0.5)) for i in range(NFRAMES)]


def test_work_geometry_values():
    from image_stitching_amd.stitching import StitchConfig, work_geometry
    ws, size = work_geometry(StitchConfig.hot_path(work_megapix=0.6), (3840, 2160))
    assert ws == math.sqrt(0.6e6 / 8294400) and abs(ws - 0.2689571768199595) < 1e-15
    assert size == (1033, 581)
    ws, size = work_geometry(StitchConfig.hot_path(work_megapix=0.6), (1920, 1080))
    assert ws == math.sqrt(0.6e6 / 2073600) and abs(ws - 0.537914353639919) < 1e-15
    assert size == (1033, 581)
    assert work_geometry(StitchConfig.hot_path(work_megapix=-1), (3840, 2160)) == (1.0, (3840, 2160))
    assert work_geometry(StitchConfig.hot_path(), (1920, 1080)) == (1.0, (1920, 1080))          # the default is -1
    assert work_geometry(StitchConfig.hot_path(work_megapix=3.0), (1920, 1080)) == (1.0, (1920, 1080))     # the min(1.0, ...)


def test_work_sizes_are_what_resize_gives():
    """The sizes above are the ones INTER_LINEAR_EXACT produces for the factor (cvRound of size * factor)."""
    import oracle
    from image_stitching_amd.stitching import StitchConfig, work_geometry
    for (w, h, mp) in ((3840, 2160, 0.6), (1920, 1080, 0.6), (1237, 701, 0.08), (640, 360, 0.05)):
        ws, size = work_geometry(StitchConfig.hot_path(work_megapix=mp), (w, h))
        out = oracle.resize_exact(np.zeros((h, w), np.uint8), fx=ws, fy=ws)
        assert (out.shape[1], out.shape[0]) == size


def test_compose_geometry_with_a_work_scale():
    from image_stitching_amd.stitching import StitchConfig, compose_geometry
    ws = 0.2689571768199595
    # compose_megapix = -1: compose_scale 1, compose_work_aspect = 1 / work_scale, frames keep their size
    g = compose_geometry(StitchConfig.hot_path(work_megapix=0.6), (3840, 2160), 1000.0, ws)
    assert g.compose_scale == 1.0 and g.aspect == 1.0 / ws and abs(g.aspect - 3.71806401235912) < 1e-14
    assert g.warp_scale == 3718.06396484375          # float(1000) * float(aspect), a float product
    assert g.size == (3840, 2160)
    # compose_megapix = 0.4: compose_scale / work_scale = sqrt(0.4 / 0.6)
    g = compose_geometry(StitchConfig(work_megapix=0.6), (3840, 2160), 1000.0, ws)
    assert g.compose_scale == 0.21960261528947078 and g.aspect == 0.21960261528947078 / ws and abs(g.aspect - 0.816496580927726) < 1e-15
    assert g.warp_scale == 816.49658203125
    assert g.size == (843, 474)
    # the default work scale keeps what every caller had
    a, b = compose_geometry(StitchConfig(), (3840, 2160), 1000.0), compose_geometry(StitchConfig(), (3840, 2160), 1000.0, 1.0)
    assert a == b and a.aspect == 0.21960261528947078 and a.warp_scale == float(np.float32(1000.0) * np.float32(0.21960261528947078))


def test_scaled_camera_is_the_double_product():
    from image_stitching_amd.stitching import scaled_camera
    cam = _cams()[1]
    ws = 0.537914353639919
    c = scaled_camera(cam, ws)
    K = np.asarray(cam["K"], np.float64)
    assert c["K"][0, 0] == K[0, 0] * ws and c["K"][0, 2] == K[0, 2] * ws and c["K"][1, 2] == K[1, 2] * ws
    assert c["K"][1, 1] == (K[0, 0] * ws) * (K[1, 1] / K[0, 0])
    assert np.array_equal(c["R"], cam["R"]) and cam["K"][0, 0] == K[0, 0]          # the caller's camera is untouched


def test_engine_that_cannot_resize_is_refused():
    """An engine without a work scale (the CPU engine of these tests) would run a work_megapix job at full resolution: refused at
    construction, by name.  The option used to be accepted and ignored."""
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    from oracle_engine import OracleEngine
    cams = _cams()
    for mp in (0.6 * W * H / (3840 * 2160), 0.02, 0.0301):
        cfg = StitchConfig.hot_path(work_megapix=mp)
        with pytest.raises(NotImplementedError, match="work_megapix"):
            StitchJob(None, (W, H), cams, engine=OracleEngine((W, H), config=cfg), config=cfg)


def test_work_scale_one_runs_as_before():
    """work_megapix = -1 and a value whose scale comes out as 1 construct and give the job the same cameras and the same result."""
    import synth
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    from oracle_engine import OracleEngine
    cams = _cams()
    frames = {i: synth.render_frame(c) for i, c in enumerate(cams)}
    outs = []
    for mp in (-1, 3.0, W * H / 1e6):
        cfg = StitchConfig.hot_path(work_megapix=mp)
        job = StitchJob(None, (W, H), cams, engine=OracleEngine((W, H), config=cfg), config=cfg)
        assert job.work_scale == 1.0 and job.work_size == (W, H)
        assert job.cams is cams and job.cams0 is cams and job.work_cams0 is cams
        outs.append(job.run(frames))
    for o in outs[1:]:
        assert o["indices"] == outs[0]["indices"] and o["pano_size"] == outs[0]["pano_size"]
        assert np.array_equal(np.asarray(o["confidence"]), np.asarray(outs[0]["confidence"]))
        assert np.array_equal(o["pano"], outs[0]["pano"]) and np.array_equal(o["mask"], outs[0]["mask"])
