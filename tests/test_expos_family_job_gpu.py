"""expos_comp_type gain / channels_blocks and expos_comp_nr_feeds end to end: Stitcher.compose against the stage calls composed by
hand, host/stitch_main --expos_comp ... --expos_comp_nr_feeds against them, and the two-rank sharded job against the single
process, byte for byte.  "channels" is no configuration name of the Python package (stitching.EXPOS_COMP_TYPES): its panorama is
composed by hand from ChannelsCompensator, and host/stitch_main --expos_comp channels must give those bytes.  The frames carry a
colour cast per frame, so the channel types have something to correct that the gain types cannot."""
import os
import subprocess

import numpy as np
import pytest

from test_host_cpp import HOST, _build, _read_ppm, _write_job
from test_range_matcher_job_gpu import H, N, W, _cams

pytestmark = pytest.mark.gpu

KINDS = ["gain", "channels", "channels_blocks"]
CONFIG_KINDS = ["gain", "channels_blocks"]               # the names the Python configuration takes
FEEDS = 2
CASTS = [(0.80, 0.95, 1.10), (1.15, 1.00, 0.85), (0.95, 1.10, 1.00), (1.05, 0.90, 1.15), (0.90, 1.00, 1.10), (1.10, 1.05, 0.90)]      # B, G, R per frame


def _cast(frame, k):
    return np.clip(np.rint(frame.astype(np.float32) * np.array(CASTS[k % len(CASTS)], np.float32)), 0, 255).astype(np.uint8)


def _config(kind, **kw):
    import image_stitching_amd as isa
    return isa.StitchConfig.hot_path(expos_comp_type=kind, expos_comp_nr_feeds=FEEDS, seam_find_type="voronoi", **kw)


def _compensator(ctx, kind):
    import image_stitching_amd as isa
    if kind == "gain":
        return isa.GainCompensator(ctx, FEEDS)
    if kind == "channels":
        return isa.ChannelsCompensator(ctx, FEEDS)
    return isa.BlocksChannelsCompensator(ctx, 64, 64, 2, FEEDS)


@pytest.fixture(scope="module")
def sweep(tmp_path_factory, oracle_mod):
    import torch
    tmp = str(tmp_path_factory.mktemp("expos_family"))
    cams, frames = _write_job(tmp, oracle_mod, n=3, w=480, h=270)
    frames = [_cast(f, k) for k, f in enumerate(frames)]
    for k, f in enumerate(frames):                                # the files stitch_main reads: the cast frames
        with open(os.path.join(tmp, "%d.ppm" % (k + 1)), "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (f.shape[1], f.shape[0]))
            fh.write(f[:, :, ::-1].tobytes())
    return dict(dir=tmp, cams=cams, frames=frames, dev=[torch.from_numpy(f).cuda() for f in frames], size=(480, 270))


@pytest.fixture(scope="module")
def composed(ctx, sweep):
    import image_stitching_amd as isa
    out = {}
    for kind in CONFIG_KINDS + ["no"]:
        res, mask = isa.Stitcher(ctx, sweep["size"], _config(kind)).compose(sweep["dev"], sweep["cams"])
        out[kind] = (np.clip(res.cpu().numpy(), 0, 255).astype(np.uint8), mask.cpu().numpy())
    return out


def _by_hand(ctx, sweep, kind):
    """The seam-scale pass and the compositing loop as single stage calls -> (panorama as bytes, mask)."""
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as S
    cfg, cams, dev, size = _config("gain"), sweep["cams"], sweep["dev"], sweep["size"]      # the scales and the blender: the same for every type
    scale = isa.Stitcher.warped_image_scale(cams)
    items = [S.seam_scale_warp(ctx, cfg, size, dev[i], cams[i], scale) for i in range(3)]
    corners, images, masks = [it[0] for it in items], [it[1] for it in items], [it[2] for it in items]
    comp = _compensator(ctx, kind)
    comp.feed(corners, images, masks)
    isa.VoronoiSeamFinder(ctx).find(images, corners, masks)
    warper = isa.SphericalWarper(ctx, scale)
    rois = S.warp_rois(ctx, scale, size, cams, isa.WARP_SPHERICAL)
    tl_sizes = [(r[0], r[1]) for r in rois], [(r[2], r[3]) for r in rois]
    x, y, pw, ph = isa.result_roi(*tl_sizes)
    btype, bands, sharp = isa.blend_config(cfg.blend_type, cfg.blend_strength, (pw, ph))
    assert btype == isa.BLEND_MULTI_BAND
    blender = isa.MultiBandBlender(ctx, bands)
    blender.prepare(*tl_sizes)
    for k in range(3):
        tl, img_s, mask = warper.warp_fused(dev[k], cams[k]["K"], cams[k]["R"], rois[k])
        comp.apply(k, tl, img_s, mask)
        S.seam_mask_apply(ctx, masks[k], mask)
        blender.feed(img_s, mask, tl)
    res, mask = blender.blend()
    return np.clip(res.cpu().numpy(), 0, 255).astype(np.uint8), mask.cpu().numpy()


@pytest.fixture(scope="module")
def by_hand(ctx, sweep):
    return {kind: _by_hand(ctx, sweep, kind) for kind in KINDS}


@pytest.mark.parametrize("kind", CONFIG_KINDS)
def test_compose_equals_the_stage_calls_by_hand(ctx, sweep, composed, by_hand, kind):
    import image_stitching_amd as isa
    want, wmask = composed[kind]
    assert np.array_equal(by_hand[kind][0], want) and np.array_equal(by_hand[kind][1], wmask)
    # the option reached the compensator: other types and no compensation give other panoramas
    for other in composed:
        if other != kind:
            assert not np.array_equal(composed[other][0], want), (kind, other)
    assert not np.array_equal(by_hand["channels"][0], want)
    one, _ = isa.Stitcher(ctx, sweep["size"], isa.StitchConfig.hot_path(expos_comp_type=kind, seam_find_type="voronoi")).compose(sweep["dev"], sweep["cams"])
    assert not np.array_equal(np.clip(one.cpu().numpy(), 0, 255).astype(np.uint8), want), "expos_comp_nr_feeds changed nothing"


@pytest.mark.parametrize("kind", KINDS)
def test_stitch_main_expos_comp_equals_python(sweep, composed, by_hand, kind):
    """host/stitch_main against the Python Stitcher with the same configuration; for "channels" against the stage calls by hand."""
    _build()
    r = subprocess.run([os.path.join(HOST, "stitch_main"), sweep["dir"], "--expos_comp", kind, "--expos_comp_nr_feeds", str(FEEDS), "--seam", "voronoi"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _read_ppm(os.path.join(sweep["dir"], "result.ppm"))
    want = composed[kind][0] if kind in CONFIG_KINDS else by_hand[kind][0]
    assert got.shape == want.shape and np.array_equal(got, want)


def test_stitch_main_refuses_bad_values_by_name(sweep):
    _build()
    for args, word in ((["--expos_comp", "gain_channels"], "gain_channels"), (["--expos_comp", "gain", "--expos_comp_nr_feeds", "0"], "expos_comp_nr_feeds")):
        r = subprocess.run([os.path.join(HOST, "stitch_main"), sweep["dir"]] + args, capture_output=True, text=True, timeout=600)
        assert r.returncode != 0 and word in r.stdout + r.stderr, args
        assert "Features in image" not in r.stdout


def _cast_gpu(frame, k):
    import torch
    g = torch.tensor(CASTS[k % len(CASTS)], dtype=torch.float32, device=frame.device)
    return torch.clamp(torch.round(frame.to(torch.float32) * g), 0, 255).to(torch.uint8)


def _py_rank_expos(rank, world, port, out_path, kind):
    """One rank of the Python sharded job with an exposure compensator, on the one GPU (gloo rendezvous)."""
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import synth
        import image_stitching_amd as isa
        from image_stitching_amd.distributed import StitchJob
        cams = _cams()
        job = StitchJob(isa.Context(0), (W, H), cams, rank=rank, world_size=world, group=dist.group.WORLD, config=_config(kind))
        frames = {i: _cast_gpu(synth.render_frame_gpu(cams[i]), i) for i in job.my_frames}
        out = job.run(frames)
        if rank == 0:
            np.savez(out_path, pano=out["pano"].cpu().numpy(), mask=out["mask"].cpu().numpy(), indices=np.array(out["indices"]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", CONFIG_KINDS)
def test_two_rank_job_equals_single_process(tmp_path, ctx, kind):
    import socket
    import torch.multiprocessing as mp
    import synth
    from image_stitching_amd.distributed import StitchJob
    cams = _cams()
    frames = {i: _cast_gpu(synth.render_frame_gpu(c), i) for i, c in enumerate(cams)}
    one = StitchJob(ctx, (W, H), cams, config=_config(kind)).run(frames)
    assert one["indices"] == list(range(N))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    npz = str(tmp_path / "py.npz")
    mp.start_processes(_py_rank_expos, args=(2, port, npz, kind), nprocs=2, join=True, start_method="spawn")
    py = np.load(npz)
    assert list(py["indices"]) == one["indices"]
    assert np.array_equal(py["mask"], one["mask"].cpu().numpy()) and np.array_equal(py["pano"], one["pano"].cpu().numpy())
    plain = StitchJob(ctx, (W, H), cams, config=_config("no")).run(frames)
    assert not np.array_equal(plain["pano"].cpu().numpy(), py["pano"])
