"""seam_find_type = "dp_colorgrad" end to end on 640 x 360 sweeps: Stitcher.compose against a composition whose seam masks come from
the numpy reference (tests/refimpl_seam_dp_grad.py), host/stitch_main --seam dp_colorgrad against its Python twin, the Python
StitchJob on one rank and on two against Stitcher.compose -- byte for byte --, and the panorama against the dp_color one, which it
must not equal (test_refimpl_seam_dp_grad_cpu.py::test_sweep_seams_differ_between_color_and_colorgrad holds the precondition)."""
import os
import subprocess

import numpy as np
import pytest

import refimpl_seam_dp_grad as rg
from test_host_cpp import HOST, _build, _read_ppm, _write_job
from test_refimpl_seam_dp_grad_cpu import H, W, sweep_cams, sweep_frames

pytestmark = pytest.mark.gpu


def _config(seam="dp_colorgrad"):
    import image_stitching_amd as isa
    return isa.StitchConfig.hot_path(compose_megapix=-1, expos_comp_type="gain_blocks", seam_find_type=seam)


@pytest.fixture(scope="module")
def sweep(ctx):
    """The four-frame sweep with a gain per frame, and its panoramas under dp_colorgrad and dp_color, composed once."""
    import torch
    import image_stitching_amd as isa
    cams = sweep_cams()
    dev = [torch.from_numpy(f).cuda() for f in sweep_frames(cams)]
    out = {seam: isa.Stitcher(ctx, (W, H), _config(seam)).compose(dev, cams) for seam in ("dp_colorgrad", "dp_color")}
    return dict(cams=cams, dev=dev, out=out)


def test_compose_equals_composition_with_reference_masks(ctx, sweep):
    """The same compositing loop with the seam step replaced: the library's seam-scale warps and compensator feed, the masks of
    the numpy COLOR_GRAD reference."""
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd import stitching as S
    cfg = _config()
    st = isa.Stitcher(ctx, (W, H), cfg)
    seen = {}

    def seam_step(frames, cameras, indices, warped_image_scale, work_scale=None):
        items = [S.seam_scale_warp(ctx, cfg, (W, H), frames[i], cameras[i], warped_image_scale, st.work_scale) for i in indices]
        corners, images, masks = [it[0] for it in items], [it[1] for it in items], [it[2] for it in items]
        comp = S.make_compensator(ctx, cfg)
        comp.feed(corners, images, masks)
        ref = rg.find([i.cpu().numpy() for i in images], corners, [m.cpu().numpy() for m in masks])
        seen["changed"] = sum(int((r != m.cpu().numpy()).sum()) for r, m in zip(ref, masks))
        return comp, [torch.from_numpy(r).cuda() for r in ref]
    st.seam_step = seam_step
    want, wmask = st.compose(sweep["dev"], sweep["cams"])
    assert seen["changed"] > 0
    got, gmask = sweep["out"]["dp_colorgrad"]
    assert torch.equal(gmask, wmask) and torch.equal(got, want)


def test_panorama_differs_from_dp_color(sweep):
    import torch
    a, b = sweep["out"]["dp_colorgrad"][0], sweep["out"]["dp_color"][0]
    assert a.shape == b.shape and not torch.equal(a, b)


def test_stitch_main_seam_dp_colorgrad_equals_python(tmp_path, ctx, oracle_mod):
    import torch
    import image_stitching_amd as isa
    _build()
    cams, frames = _write_job(str(tmp_path), oracle_mod, n=3, w=W, h=H)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    exe = os.path.join(HOST, "stitch_main")
    r = subprocess.run([exe, str(tmp_path), "--expos_comp", "gain_blocks", "--seam", "dp_colorgrad"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = _read_ppm(os.path.join(str(tmp_path), "result.ppm"))
    res, _ = isa.Stitcher(ctx, (W, H), _config()).compose(dev, cams)
    assert np.array_equal(np.clip(res.cpu().numpy(), 0, 255).astype(np.uint8), got)
    col, _ = isa.Stitcher(ctx, (W, H), _config("dp_color")).compose(dev, cams)
    assert not np.array_equal(np.clip(col.cpu().numpy(), 0, 255).astype(np.uint8), got)
    # the graph-cut finders stay refused by name, before any work
    for name in ("gc_color", "gc_colorgrad"):
        r = subprocess.run([exe, str(tmp_path), "--seam", name], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "not implemented" in r.stdout and name in r.stdout and "Features in image" not in r.stdout
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert "dp_colorgrad" in r.stdout + r.stderr                       # the usage string


@pytest.mark.parametrize("forced", [False, True])
def test_one_rank_job_equals_the_stitcher(ctx, sweep, forced):
    """(also with the all-gather of the seam-scale images forced on, as tests/test_distributed_gpu.py does for dp_color)"""
    import torch
    from image_stitching_amd.distributed import StitchJob
    want, wmask = sweep["out"]["dp_colorgrad"]
    out = StitchJob(ctx, (W, H), sweep["cams"], config=_config(), force_collectives=forced).run({i: f for i, f in enumerate(sweep["dev"])})
    assert out["indices"] == [0, 1, 2, 3]
    assert torch.equal(out["mask"], wmask) and torch.equal(out["pano"], want)


def _gpu_rank(rank, world, port, out_path):
    """One rank of the two-process job on the one GPU (gloo rendezvous), as _gpu_rank of tests/test_distributed_gpu.py."""
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import image_stitching_amd as isa
        from image_stitching_amd.distributed import StitchJob
        cams = sweep_cams()
        host = sweep_frames(cams)
        job = StitchJob(isa.Context(0), (W, H), cams, rank=rank, world_size=world, group=dist.group.WORLD, config=_config())
        out = job.run({i: torch.from_numpy(host[i]).cuda() for i in job.my_frames})
        if rank == 0:
            np.savez(out_path, pano=out["pano"].cpu().numpy(), mask=out["mask"].cpu().numpy(), indices=np.array(out["indices"]))
        else:
            assert out["pano"] is None
    finally:
        dist.destroy_process_group()


def test_two_rank_job_equals_the_stitcher(ctx, sweep, tmp_path):
    import socket
    import torch.multiprocessing as mp
    want, wmask = sweep["out"]["dp_colorgrad"]
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out_path = str(tmp_path / "rank0.npz")
    mp.start_processes(_gpu_rank, args=(2, port, out_path), nprocs=2, join=True, start_method="spawn")
    got = np.load(out_path)
    assert list(got["indices"]) == [0, 1, 2, 3]
    assert np.array_equal(got["mask"], wmask.cpu().numpy()) and np.array_equal(got["pano"], want.cpu().numpy())
