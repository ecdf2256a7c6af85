"""GPU: the timelapse output through the pipelines.  Stitcher.timelapse equals the frame-by-frame route written here from entries
that are pinned elsewhere (warp_fused -> compensator.apply -> numpy placement -> clamp), with supplied cameras under three
exposure compensators and through create_panorama; stitch_main --timelapse writes exactly the JPEG files imencode makes of the
Python canvases and no panorama; mis::Stitcher::timelapse's canvases are the Python ones."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cpp import HOST, _read_ppm, _write_job
from test_timelapse_gpu import place

pytestmark = pytest.mark.gpu


def _rect(ttype, rois):
    """dst_roi in numpy: resultRoi (as_is) or resultRoiIntersection (crop) of the warp rois."""
    r = np.array(rois)
    if ttype == "as_is":
        tl, br = r[:, :2].min(0), (r[:, :2] + r[:, 2:]).max(0)
    else:
        tl, br = r[:, :2].max(0), (r[:, :2] + r[:, 2:]).min(0)
    return int(tl[0]), int(tl[1]), int(br[0] - tl[0]), int(br[1] - tl[1])


def frame_by_frame(ctx, st, frames):
    """The route the fused batch replaces, on the stitcher's kept registration: the compose geometry as compose() derives it, the
    compensator fed at seam scale, then per frame warp_fused -> apply -> placement -> saturate_cast<uchar> -> (canvases, dst_roi)."""
    from image_stitching_amd import stitching as S
    cfg, idx, cams = st.cfg, list(st.indices), st.cameras
    scale = st.warped_image_scale([cams[i] for i in idx])
    g = S.compose_geometry(cfg, st.frame_size, scale, st.work_scale)
    comp = S.make_compensator(ctx, cfg)
    if comp is not None:
        kind = st.kind if st.kind != S.check_warp_config(cfg) else None
        items = [S.seam_scale_warp(ctx, cfg, st.frame_size, frames[i], cams[i], scale, st.work_scale, kind) for i in idx]
        comp.feed([it[0] for it in items], [it[1] for it in items], [it[2] for it in items])
    if g.aspect != 1.0:
        cams = {i: S.scaled_camera(cams[i], g.aspect) for i in idx}
    if g.size != tuple(st.frame_size):
        frames = {i: S.resize(ctx, frames[i], fx=g.compose_scale, fy=g.compose_scale) for i in idx}
    rois = S.warp_rois(ctx, g.warp_scale, g.size, [cams[i] for i in idx], st.kind)
    dst_roi = _rect(cfg.timelapse_type, rois)
    warper = S.RotationWarper(ctx, g.warp_scale, st.kind)
    out = []
    for k, i in enumerate(idx):
        tl, img_s, mask = warper.warp_fused(frames[i], cams[i]["K"], cams[i]["R"], rois[k])
        if comp is not None:
            comp.apply(k, tl, img_s, mask)
        out.append(np.clip(place(img_s.cpu().numpy(), tl, dst_roi), 0, 255).astype(np.uint8))
    return out, dst_roi, rois


@pytest.fixture(scope="module")
def job(tmp_path_factory, oracle_mod):
    """Three 320 x 180 frames with their cameras, also written as <k>.ppm / <k>.txt for the C++ drivers.  The middle frame is
    darkened to 85 %, so that the exposure compensators have gains to find that change pixels."""
    import torch
    d = str(tmp_path_factory.mktemp("timelapse_job"))
    cams, frames = _write_job(d, oracle_mod)
    frames[1] = np.rint(frames[1] * 0.85).astype(np.uint8)
    with open(os.path.join(d, "2.ppm"), "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (frames[1].shape[1], frames[1].shape[0]))
        fh.write(frames[1][:, :, ::-1].tobytes())
    return d, cams, [torch.from_numpy(f).cuda() for f in frames]


@pytest.mark.parametrize("expos,ttype,compose_megapix", [("no", "crop", -1), ("gain", "as_is", 0.03), ("gain", "crop", -1), ("gain_blocks", "crop", -1),
                                                         ("gain_blocks", "as_is", 0.03)])
def test_timelapse_with_supplied_cameras_equals_frame_by_frame(ctx, job, expos, ttype, compose_megapix):
    import image_stitching_amd as isa
    _, cams, frames = job
    cfg = isa.StitchConfig.hot_path(expos_comp_type=expos, timelapse_type=ttype, compose_megapix=compose_megapix, seam_find_type="dp_color")
    st = isa.Stitcher(ctx, (320, 180), cfg)
    canvases, dst_roi = st.timelapse(frames, cams)
    assert st.indices == [0, 1, 2] and len(canvases) == 3
    want, want_roi, rois = frame_by_frame(ctx, st, frames)
    assert tuple(dst_roi) == want_roi
    if ttype == "crop":
        assert all(dst_roi[2] * dst_roi[3] < r[2] * r[3] for r in rois) and dst_roi[2] >= 32 and dst_roi[3] >= 32
    for k, (c, e) in enumerate(zip(canvases, want)):
        c = c.cpu().numpy()
        assert c.dtype == np.uint8 and c.shape == e.shape and np.array_equal(c, e), (expos, ttype, k)
        assert e.any()
    if expos == "gain":      # the gains do something here: the test is not the "no" case again
        plain = isa.Stitcher(ctx, (320, 180), isa.StitchConfig.hot_path(timelapse_type=ttype, compose_megapix=compose_megapix))
        plain.estimate_transform(frames, cams)
        assert any(not np.array_equal(a.cpu().numpy(), b) for a, b in zip(plain.compose_timelapse(frames)[0], want))
    # the 16SC3 form holds the same values
    for c16, e in zip(st.compose_timelapse(frames, as_u8=False)[0], want):
        c16 = c16.cpu().numpy()
        assert c16.dtype == np.int16 and np.array_equal(c16, e.astype(np.int16))


def test_compose_timelapse_needs_a_registration(ctx):
    import image_stitching_amd as isa
    with pytest.raises(ValueError, match="estimate_transform has not run"):
        isa.Stitcher(ctx, (320, 180), isa.StitchConfig.hot_path()).compose_timelapse([])


@pytest.mark.parametrize("ttype", ["crop", "as_is"])
def test_timelapse_through_create_panorama_equals_frame_by_frame(ctx, ttype):
    import torch
    import image_stitching_amd as isa
    import refimpl_estimator as re_
    w, h, _, host = re_.scene("B")
    frames = [torch.from_numpy(f).cuda() for f in host]
    st = isa.Stitcher.create_panorama(ctx, (w, h), timelapse_type=ttype)
    canvases, dst_roi = st.timelapse(frames)
    assert len(canvases) == len(st.indices) == len(frames)
    want, want_roi, _ = frame_by_frame(ctx, st, frames)
    assert tuple(dst_roi) == want_roi
    for c, e in zip(canvases, want):
        assert np.array_equal(c.cpu().numpy(), e) and e.any()


def test_timelapse_through_create_scans_runs_the_affine_kind(ctx):
    """The scans mode: the affine kind goes through the fused batch, as its warp entries allow.  The five frames of
    test_scans_job_gpu.py overlap pairwise only: "as_is" gives five canvases of the union, "crop" has no canvas and says so."""
    import torch
    import image_stitching_amd as isa
    from test_scans_job_gpu import H as SH, W as SW, _frames
    frames = [torch.from_numpy(f).cuda() for f in _frames()[0]]
    st = isa.Stitcher.create_scans(ctx, (SW, SH), timelapse_type="as_is")
    canvases, dst_roi = st.timelapse(frames)
    assert st.kind == isa.WARP_AFFINE and len(canvases) == len(frames) == len(st.indices)
    want, want_roi, _ = frame_by_frame(ctx, st, frames)
    assert tuple(dst_roi) == want_roi and all(np.array_equal(c.cpu().numpy(), e) and e.any() for c, e in zip(canvases, want))
    st.cfg.timelapse_type = "crop"
    with pytest.raises(ValueError, match=r"intersection Rect\(tl = .* is empty"):
        st.compose_timelapse(frames)


def test_stitch_main_timelapse_writes_the_python_canvases_as_jpeg(ctx, job):
    import image_stitching_amd as isa
    d, cams, frames = job
    subprocess.run(["make", "-C", HOST, "stitch_main"], check=True, capture_output=True)
    for name in ("result.ppm", "result_mask.pgm"):
        assert not os.path.exists(os.path.join(d, name))
    r = subprocess.run([os.path.join(HOST, "stitch_main"), d, "--timelapse", "crop"], capture_output=True, text=True)
    assert r.returncode == 0 and "timelapse " in r.stdout and "kept 3 of 3" in r.stdout, r.stdout + r.stderr
    assert not os.path.exists(os.path.join(d, "result.ppm")) and not os.path.exists(os.path.join(d, "result_mask.pgm"))
    st = isa.Stitcher(ctx, (320, 180), isa.StitchConfig.hot_path(compose_megapix=-1, timelapse_type="crop"))
    canvases, dst_roi = st.timelapse(frames, cams)
    files = sorted(f for f in os.listdir(d) if f.startswith("fixed_"))
    assert files == ["fixed_1.jpg", "fixed_2.jpg", "fixed_3.jpg"]
    for k, c in enumerate(canvases):
        got = open(os.path.join(d, "fixed_%d.jpg" % (k + 1)), "rb").read()
        assert got == bytes(isa.imencode(ctx, c)), k
    assert "%dx%d" % (dst_roi[2], dst_roi[3]) in r.stdout


@pytest.mark.parametrize("expos,ttype", [("gain", "crop"), ("gain_blocks", "as_is")])
def test_cpp_stitcher_timelapse_equals_python(ctx, job, tmp_path, expos, ttype):
    import image_stitching_amd as isa
    d, cams, frames = job
    subprocess.run(["make", "-C", HOST, "timelapse_tool"], check=True, capture_output=True)
    prefix = str(tmp_path / "canvas_")
    r = subprocess.run([os.path.join(HOST, "timelapse_tool"), d, "3", ttype, expos, prefix], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    st = isa.Stitcher(ctx, (320, 180), isa.StitchConfig.hot_path(compose_megapix=-1, expos_comp_type=expos, timelapse_type=ttype))
    canvases, dst_roi = st.timelapse(frames, cams)
    assert "dst_roi %d %d %d %d" % tuple(dst_roi) in r.stdout and "kept 1 2 3" in r.stdout, r.stdout
    for k, c in enumerate(canvases):
        assert np.array_equal(_read_ppm(prefix + "%d.ppm" % (k + 1)), c.cpu().numpy()), (expos, ttype, k)
