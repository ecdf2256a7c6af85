"""The numpy reference of DpSeamFinder(COLOR_GRAD) (tests/refimpl_seam_dp_grad.py) against float64 ground truth and by
construction, the scenes on which COLOR and COLOR_GRAD must differ (without them the GPU tests of test_seam_dp_grad_gpu.py and
test_seam_dp_grad_job_gpu.py would show nothing), and the plumbing that needs no GPU: the configuration names, the finder's
constructor, the refusal of an engine that cannot run the finder.

The rounding bound of test_float32_planes_within_the_rounding_bound, from the operation count (u = 2^-24, the unit roundoff of
float32; G = 255 (0.114f + 0.587f + 0.299f), the largest grey value; every bound carries a factor 1 + 2^-10 for the second-order
terms, which are below 10 u relative):
  g  = fl(fl(pB + pG) + pR), pX = fl(X wX): three products and two sums, each of magnitude <= G    |g  - g*|  <= EG = 5 u G
  d  = fl(g(x + 1) - g(x - 1)): |d| <= G                                                           |d  - d*|  <= ED = 2 EG + u G
  s  = fl(fl(g(x - 1) + 2 g(x)) + g(x + 1)): partial sum <= 3 G, sum <= 4 G (2 g is exact)         |s  - s*|  <= ES = 4 EG + 7 u G
  gx = fl(fl(d(y - 1) + 2 d(y)) + d(y + 1)): the same shape over d                                 |gx - gx*| <= 4 ED + 7 u G
  gy = fl(s(y + 1) - s(y - 1)): |gy| <= 4 G                                                        |gy - gy*| <= 2 ES + 4 u G
"""
import functools

import numpy as np
import pytest

import refimpl_seam_dp as rs
import refimpl_seam_dp_grad as rg

U = 2.0 ** -24
G = 255.0 * (float(rg.WB) + float(rg.WG) + float(rg.WR))
SLOP = 1.0 + 2.0 ** -10
EG = 5 * U * G
ED = 2 * EG + U * G
ES = 4 * EG + 7 * U * G
BOUND_GX = (4 * ED + 7 * U * G) * SLOP
BOUND_GY = (2 * ES + 4 * U * G) * SLOP

# the 640 x 360 sweep of tests/test_distributed_gpu.py::test_job_with_the_reference_default_seam_step_equals_the_stitcher
W, H = 640, 360
GAINS = [0.8, 1.0, 1.2, 0.9]


def sweep_cams():
    import synth
    return [synth.make_camera(W, H, 60.0, 13.0 * i - 20.0, 0.4 * ((i % 3) - 1), 0.3 * ((i % 2) - 0.5)) for i in range(4)]


def sweep_frames(cams):
    import synth
    return [np.clip(synth.render_frame(c).astype(np.float32) * g, 0, 255).astype(np.uint8) for c, g in zip(cams, GAINS)]


def test_constant_image_has_zero_gradients():
    for shape in ((9, 13), (1, 5), (5, 1), (2, 2)):
        img = np.empty(shape + (3,), np.uint8)
        img[...] = (37, 200, 91)
        gx, gy = rg.gradients(img)
        assert gx.shape == gy.shape == shape and not gx.any() and not gy.any()


def test_horizontal_ramp():
    """gradx = 8 step inside, 0 in columns 0 and w - 1, grady = 0: exactly in float32 (g = step x survives the rounding), and in
    float64 up to the weights' own sum."""
    step, w, h = 10, 12, 7
    img = np.zeros((h, w, 3), np.uint8)
    img[...] = (np.arange(w) * step)[None, :, None]
    gx, gy = rg.gradients(img)
    gx64, gy64 = rg.gradients64(img)
    wsum = float(rg.WB) + float(rg.WG) + float(rg.WR)             # the float32 weights sum to 1 + 7.5e-9, not to 1
    assert np.abs(gx64[:, 1:-1] - 8.0 * step * wsum).max() <= 1e-11 and not gx64[:, [0, -1]].any() and np.abs(gy64).max() <= 1e-11
    assert np.array_equal(gx[:, 1:-1], np.full((h, w - 2), 8 * step, np.float32))
    assert not gx[:, 0].any() and not gx[:, -1].any()          # REFLECT_101: g(-1) = g(1)
    assert not gy.any()
    gxt, gyt = rg.gradients(np.ascontiguousarray(img.transpose(1, 0, 2)))
    assert np.array_equal(gyt, gx.T) and not gxt.any()


def test_one_pixel_and_one_line_images():
    gx, gy = rg.gradients(np.array([[[9, 200, 31]]], np.uint8))
    assert gx.shape == gy.shape == (1, 1) and gx[0, 0] == 0 and gy[0, 0] == 0
    rng = np.random.default_rng(3)
    row = rng.integers(0, 256, (1, 7, 3), dtype=np.uint8)
    gx, gy = rg.gradients(row)
    gx64, _ = rg.gradients64(row)
    assert not gy.any() and np.abs(gx - gx64).max() <= BOUND_GX and gx.any()      # every row reflects to row 0: gx = 4 d
    gxc, gyc = rg.gradients(np.ascontiguousarray(row.transpose(1, 0, 2)))
    _, gyc64 = rg.gradients64(np.ascontiguousarray(row.transpose(1, 0, 2)))
    assert not gxc.any() and np.abs(gyc - gyc64).max() <= BOUND_GY and np.array_equal(gyc64, gx64.T)      # (float64 is exact here: integers times 24-bit weights)


def test_float32_planes_within_the_rounding_bound():
    rng = np.random.default_rng(20)
    worst = [0.0, 0.0]
    for shape in ((33, 47), (2, 2), (3, 3), (17, 65), (64, 16)):
        for mode in ("uniform", "extremes"):
            img = rng.integers(0, 256, shape + (3,), dtype=np.uint8) if mode == "uniform" else (rng.integers(0, 2, shape + (3,)) * 255).astype(np.uint8)
            gx, gy = rg.gradients(img)
            gx64, gy64 = rg.gradients64(img)
            ex, ey = np.abs(gx - gx64).max(), np.abs(gy - gy64).max()
            worst = [max(worst[0], ex), max(worst[1], ey)]
            assert ex <= BOUND_GX and ey <= BOUND_GY, (shape, mode, ex, ey)
            assert np.abs(gx64).max() <= 4 * G and np.abs(gy64).max() <= 4 * G
    print("largest |gx - gx64| %.3g (bound %.3g), |gy - gy64| %.3g (bound %.3g)" % (worst[0], BOUND_GX, worst[1], BOUND_GY))


@functools.lru_cache(maxsize=None)
def edge_reference():
    """-> (scene, COLOR masks, COLOR_GRAD masks) of refimpl_seam_dp_grad.edge_scene."""
    im, c, m = rg.edge_scene()
    for a in im + m:
        a.setflags(write=False)
    return (im, c, m), rs.find(im, c, m), rg.find(im, c, m)


@functools.lru_cache(maxsize=None)
def grad_reference(name):
    """COLOR_GRAD masks of a named scene of refimpl_seam_dp (or "seam_scale", "edge")."""
    if name == "edge":
        return edge_reference()[2]
    from test_refimpl_seam_dp_cpu import scene
    im, c, m = scene(name)
    return rg.find(im, c, m)


def test_edge_scene_cuts_differ():
    """The strong edge inside the overlap draws the COLOR_GRAD seam; the COLOR seam goes elsewhere.  Both still partition the
    overlap: every pixel of the union stays in at least one mask."""
    (im, c, m), color, grad = edge_reference()
    assert any(not np.array_equal(a, b) for a, b in zip(color, grad))
    assert sum(int((a != b).sum()) for a, b in zip(color, grad)) >= 20
    for masks in (color, grad):
        for k, o in enumerate(m):
            assert not (masks[k] & ~o).any()                     # masks only lose pixels
        ox, oy = c[1][0] - c[0][0], c[1][1] - c[0][1]
        a = masks[0][oy:, ox:]
        b = masks[1][:a.shape[0], :a.shape[1]]
        assert ((a != 0) | (b != 0)).all()


def test_named_scenes_run_and_some_differ():
    from test_refimpl_seam_dp_cpu import NAMES, reference
    differ = [n for n in NAMES + ["seam_scale"] if any(not np.array_equal(a, b) for a, b in zip(reference(n)[0], grad_reference(n)))]
    print("COLOR_GRAD differs from COLOR on:", differ)
    assert "seam_scale" in differ and len(differ) >= 5
    for n in ("flat", "flat_stacked"):                           # constant content: zero gradients, the costs are COLOR's
        assert n not in differ


def test_flat_content_gives_the_color_masks_exactly():
    """Zero gradients divide by 1: the COLOR_GRAD programme must then be the COLOR programme (ties by step code included)."""
    from test_refimpl_seam_dp_cpu import reference
    for n in ("flat", "flat_stacked"):
        for a, b in zip(reference(n)[0], grad_reference(n)):
            assert np.array_equal(a, b)


@functools.lru_cache(maxsize=None)
def sweep_seam_inputs():
    """The sweep's seam-scale images, corners and masks by the CPU oracle (the twins of stitching.seam_scale_warp)."""
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import StitchConfig
    from oracle_engine import OracleEngine
    cams = sweep_cams()
    frames = sweep_frames(cams)
    eng = OracleEngine((W, H), config=StitchConfig(compose_megapix=-1))
    items = eng.seam_local(frames, cams, isa.Stitcher.warped_image_scale(cams))
    return [it[0] for it in items], [it[1].numpy() for it in items], [it[2].numpy() for it in items]


def test_sweep_seams_differ_between_color_and_colorgrad(oracle_mod):
    """Precondition of test_seam_dp_grad_job_gpu.py: on the sweep the two finders cut different masks."""
    corners, images, masks = sweep_seam_inputs()
    color, grad = rs.find(images, corners, masks), rg.find(images, corners, masks)
    n = sum(int((a != b).sum()) for a, b in zip(color, grad))
    print("sweep: %d mask pixels differ" % n)
    assert n >= 100


# ------------------------------------------------------------------------------------------------ plumbing
def test_config_names():
    from image_stitching_amd.stitching import SEAM_FIND_TYPES, StitchConfig, check_seam_config
    assert "dp_colorgrad" in SEAM_FIND_TYPES
    for name in ("no", "voronoi", "dp_color", "dp_colorgrad"):
        check_seam_config(StitchConfig(seam_find_type=name))
    for name in ("gc_color", "gc_colorgrad", "dp_colourgrad", "COLOR_GRAD"):
        with pytest.raises(NotImplementedError, match=name):
            check_seam_config(StitchConfig(seam_find_type=name))


def test_finder_constructs_by_name():
    import image_stitching_amd as isa
    assert isa.DpSeamFinder.COLOR_GRAD == "COLOR_GRAD" and isa.DpSeamFinder.COLOR == 0
    assert isa.DpSeamFinder(None, "COLOR_GRAD").cost_func == isa.DpSeamFinder.COLOR_GRAD
    assert isa.DpSeamFinder(None, "COLOR").cost_func == isa.DpSeamFinder.COLOR
    assert isa.DpSeamFinder(None).cost_func == 0 and isa.DpSeamFinder(None, 1).cost_func == 1      # integers go through as they are
    with pytest.raises(ValueError, match="GRAD_COLOR"):
        isa.DpSeamFinder(None, "GRAD_COLOR")
    assert callable(isa.seam_gradients)


def test_header_and_bindings_name_the_new_entries():
    from image_stitching_amd import _capi
    for name in ("mis_seam_dp_colorgrad", "mis_seam_gradients"):
        assert name in _capi.PROTOTYPES and name in _capi.header_functions()


def test_cpu_engine_refuses_dp_colorgrad_by_name():
    """An engine that does not declare the finder is refused at construction: never run with dp_color in its place."""
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    from oracle_engine import OracleEngine
    cams = sweep_cams()
    cfg = StitchConfig.hot_path(seam_find_type="dp_colorgrad")
    with pytest.raises(NotImplementedError, match="dp_colorgrad"):
        StitchJob(None, (W, H), cams, engine=OracleEngine((W, H), config=cfg), config=cfg)
    StitchJob(None, (W, H), cams, engine=OracleEngine((W, H), config=StitchConfig.hot_path(seam_find_type="dp_color")),
              config=StitchConfig.hot_path(seam_find_type="dp_color"))
