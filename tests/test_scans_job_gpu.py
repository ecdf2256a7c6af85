"""The scans mode (cv::Stitcher::create(SCANS)) end to end: five 640 x 360 frames cut from a planar master under known similarities
(scale 1 -- the AffineWarper's forward and backward maps differ by s^2 otherwise, SURVEY Appendix C --, rotations within +-6
degrees, about 40 % overlap) through Stitcher.create_scans(...).stitch(frames) without cameras; the same composition assembled
from the single calls; the same at work_megapix = 0.1; the C++ driver's --mode scans."""
import functools
import os
import subprocess

import numpy as np
import pytest

import refimpl_affine_family as ra
import refimpl_motion as rm

pytestmark = pytest.mark.gpu

W, H, N = 640, 360, 5
RANSAC_THRESH = 3.0      # the matcher's ransac_thresh (mis_match_affine_default_params), px


@functools.lru_cache(maxsize=None)
def _frames():
    """-> (frames as (H, W, 3) uint8 BGR arrays, S: frame pixel -> master pixel, 3 x 3 each)."""
    import synth
    from scipy.ndimage import map_coordinates
    master = synth.render_frame(synth.make_camera(2400, 800, 130.0, 0.0))
    rots = (2.0, -4.5, 5.5, -1.5, 3.5)
    S = [ra.mat_of(ra.params_of(ra.similarity(rots[i], 1.0, 150.0 + 384.0 * i, 190.0 + 25.0 * ((i % 3) - 1)))) for i in range(N)]
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frames = []
    for Si in S:
        mx = Si[0, 0] * xx + Si[0, 1] * yy + Si[0, 2]
        my = Si[1, 0] * xx + Si[1, 1] * yy + Si[1, 2]
        assert mx.min() >= 0 and my.min() >= 0 and mx.max() <= master.shape[1] - 1 and my.max() <= master.shape[0] - 1
        f = np.stack([map_coordinates(master[..., c].astype(np.float64), [my, mx], order=1) for c in range(3)], -1)
        frames.append(np.clip(np.rint(f), 0, 255).astype(np.uint8))
    return frames, S


def _table(pm):
    return [dict(src_img_idx=m.src_img_idx, dst_img_idx=m.dst_img_idx, matches=m.matches, inliers_mask=m.inliers_mask, num_inliers=m.num_inliers,
                 has_H=1 if m.H is not None else 0, H=m.H, confidence=m.confidence) for m in pm]


def _assemble(ctx, st, frames, feats, pm):
    """The composition from the single calls: estimate_affine_cameras, bundle_adjust_affine_partial, AffineWarper.warp_fused and
    the configured blender, at the Stitcher's scales -> (pano, mask, estimated cameras, adjusted cameras)."""
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as s
    cfg = st.cfg
    est = isa.estimate_affine_cameras(pm)
    adj = isa.bundle_adjust_affine_partial(ctx, feats, pm, est, cfg.conf_thresh)
    cams = [dict(K=np.array([[c["focal"], 0, c["ppx"]], [0, c["focal"] * c["aspect"], c["ppy"]], [0, 0, 1]], np.float64), R=np.asarray(c["R"], np.float32))
            for c in adj]
    scale = isa.Stitcher.warped_image_scale(cams)
    g = s.compose_geometry(cfg, (W, H), scale, st.work_scale)
    if g.aspect != 1.0:
        cams = [s.scaled_camera(c, g.aspect) for c in cams]
    assert g.size == (W, H)         # compose_megapix -1: frames at full resolution
    warper = isa.AffineWarper(ctx, g.warp_scale)
    rois = [warper.warp_roi((W, H), c["K"], c["R"]) for c in cams]
    corners, sizes = [(r[0], r[1]) for r in rois], [(r[2], r[3]) for r in rois]
    x, y, pw, ph = isa.result_roi(corners, sizes)
    btype, bands, sharp = isa.blend_config(cfg.blend_type, cfg.blend_strength, (pw, ph))
    assert btype == isa.BLEND_MULTI_BAND
    blender = isa.MultiBandBlender(ctx, bands)
    blender.prepare(corners, sizes)
    for f, c, roi in zip(frames, cams, rois):
        tl, img_s, mask = warper.warp_fused(f, c["K"], c["R"], roi)
        blender.feed(img_s, mask, tl)
    pano, mask = blender.blend()
    return pano, mask, est, adj


def _run(ctx, **overrides):
    import torch
    import image_stitching_amd as isa
    host, S = _frames()
    frames = [torch.from_numpy(f).cuda() for f in host]
    st = isa.Stitcher.create_scans(ctx, (W, H), **overrides)
    pano, mask, feats, pm, idx = st.stitch(frames)
    return st, frames, pano, mask, feats, pm, idx


def test_scans_mode_stitches_without_cameras(ctx):
    import torch
    import image_stitching_amd as isa
    host, S = _frames()
    st, frames, pano, mask, feats, pm, idx = _run(ctx)
    assert st.cfg.matcher_type == "affine" and st.cfg.wave_correct == "no" and st.cfg.expos_comp_type == "no" and st.kind == isa.WARP_AFFINE
    assert type(st.matcher).__name__ == "AffineBestOf2NearestMatcher"
    # it keeps all frames
    assert [int(i) for i in idx] == list(range(N))
    # every estimated pairwise transform moves the frame corners to within the matcher's RANSAC threshold of the true one
    corners = np.array([[0, 0, 1], [W - 1, 0, 1], [0, H - 1, 1], [W - 1, H - 1, 1]], np.float64).T
    tab = _table(pm)
    edges = 0
    for i in range(N):
        for j in range(i + 1, N):
            m = tab[i * N + j]
            if not m["confidence"] > float(np.float32(st.cfg.conf_thresh)):
                continue
            edges += 1
            true = np.linalg.inv(S[j]) @ S[i]          # frame i pixels -> frame j pixels
            d = np.asarray(m["H"], np.float64).reshape(3, 3) @ corners - true @ corners
            err = float(np.hypot(d[0], d[1]).max())
            print("pair (%d, %d): %d inliers, corners off by %.3f px" % (i, j, m["num_inliers"], err))
            assert err <= RANSAC_THRESH, (i, j, err)
    assert edges >= N - 1
    # the panorama and the mask are the composition assembled from the single calls, byte for byte
    apano, amask, est, adj = _assemble(ctx, st, frames, feats, pm)
    ctx.synchronize()
    assert torch.equal(pano, apano) and torch.equal(mask, amask)
    assert all(np.array_equal(st.cameras[i]["R"], np.asarray(adj[i]["R"], np.float32)) for i in range(N))
    # the adjuster does not raise S
    xy = [np.stack([k["x"], k["y"]], 1).astype(np.float32) for k, _ in (f.download() for f in feats)]
    obs = [o for o in rm._observations(N, xy, tab, st.cfg.conf_thresh) if len(o[2])]
    s_est = ra.ba_cost(np.array([ra.params_of(c["R"]) for c in est]), obs)
    s_adj = ra.ba_cost(np.array([ra.params_of(c["R"]) for c in adj]), obs)
    print("S: estimated %.3f adjusted %.3f over %d observations" % (s_est, s_adj, sum(len(o[2]) for o in obs)))
    assert s_adj <= s_est
    # the panorama covers the strip of the five frames and shows the master: its mask is mostly set
    assert pano.shape[1] > 4 * 384 and float((mask > 0).float().mean()) > 0.6
    # cameras are refused where the estimator provides them
    with pytest.raises(ValueError):
        st.stitch(frames, [None] * N)
    with pytest.raises(ValueError):
        isa.Stitcher(ctx, (W, H), isa.StitchConfig.hot_path()).stitch(frames)


def test_scans_mode_at_work_scale(ctx):
    """work_megapix = 0.1: features, matches and cameras in work units, the composition at full resolution through
    compose_work_aspect -- the same assembly at that scale."""
    import torch
    st, frames, pano, mask, feats, pm, idx = _run(ctx, work_megapix=0.1)
    assert st.work_scale < 1.0 and [int(i) for i in idx] == list(range(N))
    apano, amask, est, adj = _assemble(ctx, st, frames, feats, pm)
    ctx.synchronize()
    assert torch.equal(pano, apano) and torch.equal(mask, amask)
    full = _run(ctx)[2]
    assert abs(pano.shape[0] - full.shape[0]) <= 8 and abs(pano.shape[1] - full.shape[1]) <= 8


def test_stitch_main_scans_mode(ctx, tmp_path):
    """stitch_main <dir> --mode scans reads no camera files and writes the Python mode's panorama byte for byte and its cameras
    in cams.data; --ba affine keeps failing as before."""
    import image_stitching_amd as isa
    from image_stitching_amd import serializer as ser
    from test_host_cpp import HOST, _build
    _build()
    host, S = _frames()
    tmp = str(tmp_path)
    for i, f in enumerate(host):
        with open(os.path.join(tmp, "%d.ppm" % (i + 1)), "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (W, H))
            fh.write(f[:, :, ::-1].tobytes())
    r = subprocess.run([os.path.join(HOST, "stitch_main"), tmp, "--mode", "scans"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    st, frames, pano, mask, feats, pm, idx = _run(ctx)
    assert ser.deserializeIndices(os.path.join(tmp, "indices.data")) == list(range(N))
    ser.serializeCameraParams([dict(st.cameras[i]["params"], R=np.asarray(st.cameras[i]["R"], np.float32)) for i in range(N)], os.path.join(tmp, "cams_py.data"))
    assert open(os.path.join(tmp, "cams.data")).read() == open(os.path.join(tmp, "cams_py.data")).read()
    with open(os.path.join(tmp, "result.ppm"), "rb") as fh:
        assert fh.readline() == b"P6\n"
        pw, ph = [int(v) for v in fh.readline().split()]
        assert fh.readline() == b"255\n"
        got = np.frombuffer(fh.read(), np.uint8).reshape(ph, pw, 3)
    want = np.clip(pano.cpu().numpy(), 0, 255).astype(np.uint8)[:, :, ::-1]
    assert got.shape == want.shape and np.array_equal(got, want)
    r = subprocess.run([os.path.join(HOST, "stitch_main"), tmp, "--mode", "scan"], capture_output=True, text=True)
    assert r.returncode != 0 and "'panorama' or 'scans'" in r.stdout
    r = subprocess.run([os.path.join(HOST, "stitch_main"), tmp, "--mode", "scans", "--ba", "affine"], capture_output=True, text=True)
    assert r.returncode == 1 and "'no', 'reproj' and 'ray'" in r.stdout
