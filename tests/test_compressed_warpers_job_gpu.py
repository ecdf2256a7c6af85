"""The jobs under warp_type = compressedPlaneA2B1 and paniniA1.5B1 on a three-frame narrow sweep (every roi finite: checked on the
reference alone by tests/test_refimpl_compressed_warpers_cpu.py): the Python StitchJob against the composition assembled from the
single-frame warper calls and the existing blender, and the C++ pipeline (host/stitch_main --warp paniniA2B1, the one kind without a
Python warp_type name) against the Python composition built with PaniniWarper(ctx, scale, 2, 1)."""
import os
import subprocess

import numpy as np
import pytest

import refimpl_compressed_warpers as rc
from test_host_cpp import HOST, _build, _read_ppm, _write_job

pytestmark = pytest.mark.gpu

W, H = 480, 270
CHILD_TIMEOUT = 300     # seconds, the child process
WARPS = ["compressedPlaneA2B1", "paniniA1.5B1"]


def _cams():
    import synth
    return [synth.make_camera(W, H, 60.0, 14.0 * i - 14.0, 0.4 * (i - 1), 0.3 * i) for i in range(3)]


def _composition(ctx, warper, frames, cams, size):
    """warpRoi, one fused warp per frame, a blender fed frame by frame -> (rois, pano, mask, bands)."""
    import image_stitching_amd as isa
    rois, warped = [], []
    for f, c in zip(frames, cams):
        K, R = np.asarray(c["K"], np.float32), np.asarray(c["R"], np.float32)
        roi = warper.warp_roi(size, K, R)
        rois.append(roi)
        warped.append(warper.warp_fused(f, K, R, roi))
    corners, sizes = [r[:2] for r in rois], [r[2:] for r in rois]
    x, y, pw, ph = isa.result_roi(corners, sizes)
    btype, bands, sharp = isa.blend_config(2, 5.0, (pw, ph))
    assert btype == isa.BLEND_MULTI_BAND
    bl = isa.MultiBandBlender(ctx, bands)
    bl.prepare(corners, sizes)
    for tl, img_s, msk in warped:
        bl.feed(img_s, msk, tl)
    pano, mask = bl.blend()
    ctx.synchronize()
    return rois, pano, mask, bands


@pytest.mark.parametrize("warp", WARPS)
def test_python_job_equals_per_frame_library_calls(ctx, warp):
    """The job's corners, sizes, panorama and mask equal, byte for byte, the composition assembled from per-frame calls.  Every roi
    lies in the reference sets; the panorama is not the spherical one."""
    import synth
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd.distributed import StitchJob
    from image_stitching_amd.stitching import StitchConfig
    kind = rc.KINDS[warp]
    cams = _cams()
    frames = {i: synth.render_frame_gpu(c) for i, c in enumerate(cams)}
    job = StitchJob(ctx, (W, H), cams, config=StitchConfig.hot_path(warp_type=warp))
    assert job.kind == kind and job.speculation_roi_ok()
    out = job.run(frames)
    idx = out["indices"]
    assert idx == [0, 1, 2]
    scale = isa.Stitcher.warped_image_scale([cams[i] for i in idx])
    cls = isa.PaniniWarper if rc.is_panini(kind) else isa.CompressedRectilinearWarper
    warper = cls(ctx, scale, *rc.AB[kind])
    assert warper.kind == kind
    rois, pano, mask, bands = _composition(ctx, warper, [frames[i] for i in idx], [cams[i] for i in idx], (W, H))
    assert [tuple(job._compose_rois[i]) for i in idx] == rois and bands == out["num_bands"]
    for i, roi in zip(idx, rois):
        assert rc.roi_matches(roi, rc.warp_roi_f64(kind, scale, W, H, cams[i]["K"], cams[i]["R"])), (i, roi)
    assert torch.equal(pano, out["pano"]) and torch.equal(mask, out["mask"])
    sph = StitchJob(ctx, (W, H), cams).run(frames)
    assert sph["pano"].shape != out["pano"].shape or not torch.equal(sph["pano"], out["pano"])


def test_stitch_main_panini_a2b1_equals_python_composition(tmp_path, ctx, oracle_mod):
    """host/stitch_main <dir> --warp paniniA2B1 (the hot path: no seam-scale step) against the composition built in Python with
    PaniniWarper(ctx, scale, 2, 1), byte for byte."""
    import torch
    import image_stitching_amd as isa
    _build()
    cams, frames = _write_job(str(tmp_path), oracle_mod, n=3, w=W, h=H)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    r = subprocess.run([os.path.join(HOST, "stitch_main"), str(tmp_path), "--warp", "paniniA2B1"], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _read_ppm(os.path.join(str(tmp_path), "result.ppm"))
    scale = isa.Stitcher.warped_image_scale(cams)
    warper = isa.PaniniWarper(ctx, scale, 2, 1)
    assert warper.kind == isa.WARP_PANINI_A2B1
    rois, pano, mask, _ = _composition(ctx, warper, dev, cams, (W, H))
    for c, roi in zip(cams, rois):
        assert rc.roi_matches(roi, rc.warp_roi_f64(rc.PANINI_A2B1, scale, W, H, c["K"], c["R"])), roi
    assert np.array_equal(np.clip(pano.cpu().numpy(), 0, 255).astype(np.uint8), got)
