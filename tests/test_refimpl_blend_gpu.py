"""GPU: the multi-band, feather and plain blenders (blend.hip) against the numpy reference of tests/refimpl_blend.py -- every
accumulator level (Laplacian sums exactly, weight sums as float32 bits), the blended image and mask, the feed tile of every frame --
over the regimes of test_refimpl_blend_cpu.py, then the other entry points: strided / unaligned views, feed_batch across gather
groups, compose_frames, blend_columns strips and prepare() on a used blender.  Every frame is fed once, so no comparison depends on
the float32 order of a rect exchange's weight sums."""
import ctypes as C

import numpy as np
import pytest

import refimpl_blend as rb
from test_refimpl_blend_cpu import (FE, MB, NO, REGIME_IDS, REGIMES, bytes_mask, compare_levels, compare_result, full_mask, imgfull,
                                    img8, reference, scene, strip, tiny_frames_scene)

pytestmark = pytest.mark.gpu

E_UNSUPPORTED = -6


def _blender(ctx, btype, bands=0, sharp=0.0):
    import image_stitching_amd as isa
    if btype == MB:
        return isa.MultiBandBlender(ctx, bands)
    if btype == FE:
        return isa.FeatherBlender(ctx, sharp)
    return isa.Blender(ctx)


def _cs(frames):
    return [f[2] for f in frames], [(f[1].shape[1], f[1].shape[0]) for f in frames]


def _dev(frames):
    import torch
    return [(torch.from_numpy(np.ascontiguousarray(i)).cuda(), torch.from_numpy(np.ascontiguousarray(m)).cuda(), tl) for i, m, tl in frames]


def _prepared(ctx, sc, frames=None):
    gb = _blender(ctx, sc["btype"], sc["bands"], sc["sharp"])
    gb.prepare(*_cs(frames if frames is not None else sc["frames"]))
    return gb


def feed_rect(ctx, gb, size, tl):
    from image_stitching_amd import _capi as capi
    r = capi.MisRect()
    ctx.check(ctx.lib.mis_blender_feed_rect(gb.h, int(size[0]), int(size[1]), capi.MisPoint(int(tl[0]), int(tl[1])), C.byref(r)))
    return r.x, r.y, r.width, r.height


def lib_levels(ctx, gb, btype):
    nb = ctx.lib.mis_blender_num_bands(gb.h)
    out = [gb.level(l) for l in range(nb + 1)]
    return [(lap, None if btype == NO else wgt) for lap, wgt in out]


def check(ctx, tag, gb, ref, btype):
    compare_levels(tag, ref, lib_levels(ctx, gb, btype))
    img, mask = gb.blend()
    ctx.synchronize()
    compare_result(tag, img.cpu().numpy(), mask.cpu().numpy(), *ref.blend())


def blend_columns(ctx, gb, x0, x1):
    import torch
    from image_stitching_amd import stitching as st
    w, h = gb._size
    n = min(x1, w) - x0
    dst, msk = st._empty_image(ctx, h, n, 3, torch.int16), st._empty_image(ctx, h, n, 1, torch.uint8)
    d, m = st.as_image(dst), st.as_image(msk)
    ctx.check(ctx.lib.mis_blender_blend_columns(gb.h, int(x0), int(x1), C.byref(d), C.byref(m)))
    ctx.synchronize()
    return dst.cpu().numpy(), msk.cpu().numpy()


@pytest.mark.parametrize("tag,make", REGIMES, ids=REGIME_IDS)
def test_kernels_match_reference(ctx, tag, make):
    """Device tensors through feed(); the feed tile of every frame through mis_blender_feed_rect."""
    sc = make()
    ref = reference(sc)
    gb = _prepared(ctx, sc)
    for (img, mask, tl), f in zip(_dev(sc["frames"]), sc["frames"]):
        size = (f[1].shape[1], f[1].shape[0])
        want = ref.tile(tl, size)[:4] if sc["btype"] == MB else (tl[0], tl[1], size[0], size[1])
        assert feed_rect(ctx, gb, size, tl) == want, (tag, "feed tile", tl, size)
        gb.feed(img, mask, tl)
    check(ctx, tag, gb, ref, sc["btype"])


def _views(frames, c0):
    """Each frame as a column-slice view starting at column c0 of a wider device image / mask whose rows are 8 k + 1 pixels apart
    (odd in shorts, not a multiple of 16 bytes): three 2-byte loads per pixel, no DMA row staging, byte loads of the feather mask."""
    import torch
    out = []
    for img, mask, tl in frames:
        h, w = mask.shape
        pitch = w + c0 + (1 - (w + c0)) % 8 + 8
        bi = torch.zeros((h, pitch, 3), dtype=torch.int16, device="cuda")
        bm = torch.zeros((h, pitch), dtype=torch.uint8, device="cuda")
        vi, vm = bi[:, c0:c0 + w], bm[:, c0:c0 + w]
        vi.copy_(torch.from_numpy(img).cuda())
        vm.copy_(torch.from_numpy(mask).cuda())
        assert vi.data_ptr() % 4 != 0 and vm.data_ptr() % 4 != 0 and (vi.stride(0) * 2) % 16 != 0 and vm.stride(0) % 16 != 0
        out.append((vi, vm, tl))
    return out


@pytest.mark.parametrize("c0", [1, 3])
@pytest.mark.parametrize("btype", [MB, FE, NO])
def test_unaligned_strided_views(ctx, btype, c0):
    rng = np.random.default_rng(60 + c0 + btype)
    frames = strip(rng, 3, 150, 100, 90)
    frames.append((imgfull(rng, 40, 30), bytes_mask(rng, 40, 30), (20, 50)))
    frames.append((img8(rng, 3, 2), full_mask(rng, 3, 2), (0, 0)))
    sc = scene(btype, frames, 4, 0.04)
    gb = _prepared(ctx, sc)
    for img, mask, tl in _views(frames, c0):
        gb.feed(img, mask, tl)
    check(ctx, "views c0=%d type %d" % (c0, btype), gb, reference(sc), btype)
    sc = tiny_frames_scene()
    gb = _prepared(ctx, sc)
    for img, mask, tl in _views(sc["frames"], c0):
        gb.feed(img, mask, tl)
    check(ctx, "tiny-frame views c0=%d" % c0, gb, reference(sc), MB)


def _batch_frames(n, seed):
    """n + 3 overlapping frames (a single feed, a batch of n, a batch of 2), one with an all-zero mask inside the batch."""
    rng = np.random.default_rng(seed)
    fr = strip(rng, n + 3, 70, 60, 13)
    fr[2] = (imgfull(rng, fr[2][1].shape[1], fr[2][1].shape[0]), fr[2][1], fr[2][2])
    fr[min(n, 5)] = (fr[min(n, 5)][0], np.zeros_like(fr[min(n, 5)][1]), fr[min(n, 5)][2])
    fr[-1] = (fr[-1][0], bytes_mask(rng, fr[-1][1].shape[1], fr[-1][1].shape[0]), fr[-1][2])
    return fr


@pytest.mark.parametrize("n", [1, 16, 17, 19])
def test_feed_batch(ctx, n):
    """feed_batch of n frames (one or two gather groups): first on fresh accumulators, then behind a single feed (read-modify-write
    mode), each followed by a second batch -- against the reference fed the same frames one by one."""
    fr = _batch_frames(n, 70 + n)
    dev = _dev(fr)
    sc = scene(MB, fr, 3)
    ref = reference(sc)
    # fresh: batch(0 .. n), then batch(n + 1 .. n + 2)
    gb = _prepared(ctx, sc)
    for grp in (list(range(n + 1)), list(range(n + 1, n + 3))):
        gb.feed_batch([dev[k][0] for k in grp], [dev[k][1] for k in grp], [dev[k][2] for k in grp])
    check(ctx, "batch of %d, fresh" % (n + 1), gb, ref, MB)
    # single feed, then batch(1 .. n) with the zero mask inside, then batch(n + 1 .. n + 2)
    gb = _prepared(ctx, sc)
    gb.feed(*dev[0])
    for grp in (list(range(1, n + 1)), list(range(n + 1, n + 3))):
        gb.feed_batch([dev[k][0] for k in grp], [dev[k][1] for k in grp], [dev[k][2] for k in grp])
    check(ctx, "single feed + batch of %d" % n, gb, ref, MB)


def test_compose_frames_small_sweep(ctx):
    """mis_compose_frames (fused warp + batched feed) on a five-frame sweep; the reference is fed the warp_fused outputs of the same
    cameras (the warp itself is pinned by test_refimpl_warp_gpu.py)."""
    import torch
    import synth
    import image_stitching_amd as isa
    w, h = 320, 180
    cams = [synth.make_camera(w, h, 60.0, 11.0 * i - 22.0, 0.5 * (i - 2), 0.3 * i) for i in range(5)]
    frames = [torch.from_numpy(synth.render_frame(c)).cuda() for c in cams]
    scale = isa.Stitcher.warped_image_scale(cams)
    rois = isa.stitching.warp_rois(ctx, scale, (w, h), cams)
    corners, sizes = [(r[0], r[1]) for r in rois], [(r[2], r[3]) for r in rois]
    x, y, pw, ph = rb.result_roi(corners, sizes)
    for btype in (MB, FE):
        t, bands, sharp = isa.stitching.blend_config(btype, 5.0, (pw, ph))
        rt, rbands, rsharp = rb.blend_config(btype, 5.0, pw, ph)
        assert (t, bands, np.float32(sharp)) == (rt, rbands, np.float32(rsharp))
        warper = isa.SphericalWarper(ctx, scale)
        ref = rb.Blender(btype, bands, sharp).prepare(corners, sizes)
        for cam, f, roi in zip(cams, frames, rois):
            tl, img_s, msk = warper.warp_fused(f, cam["K"].astype(np.float32), cam["R"].astype(np.float32))
            assert tuple(tl) == tuple(roi[:2]) and tuple(msk.shape) == (roi[3], roi[2])
            ref.feed(img_s.cpu().numpy(), msk.cpu().numpy(), tl)
        gb = _blender(ctx, btype, bands, sharp)
        gb.prepare(corners, sizes)
        gb.compose_frames(frames, scale, cams, rois)
        check(ctx, "compose_frames type %d" % btype, gb, ref, btype)


STRIPS = [(37, 90), (50, 51), (260, 400), (256, 320), (33, 38), (0, 1), (1, 2), (0, 283)]


@pytest.mark.parametrize("btype", [MB, FE, NO])
def test_blend_columns_strips(ctx, btype):
    """mis_blender_blend_columns on strips the sharded job does not produce: odd x0, one column, x1 past the width, the last partial
    strip of 64, a strip inside one 16-pixel block of level 4, the first columns -- each against the reference's full blend."""
    rng = np.random.default_rng(80 + btype)
    frames = strip(rng, 4, 90, 70, 64, make_img=imgfull if btype == MB else img8)
    frames[0] = (frames[0][0], np.full_like(frames[0][1], 255), (0, frames[0][2][1]))
    frames[-1] = (frames[-1][0], frames[-1][1], (283 - frames[-1][1].shape[1], frames[-1][2][1]))
    sc = scene(btype, frames, 4, 0.05)
    ref = reference(sc)
    full = ref.blend()
    assert full[0].shape[1] == 283
    dev = _dev(frames)
    for x0, x1 in STRIPS:
        gb = _prepared(ctx, sc)
        for img, mask, tl in dev:
            gb.feed(img, mask, tl)
        img, mask = blend_columns(ctx, gb, x0, x1)
        compare_result("strip %d..%d" % (x0, x1), img, mask, *ref.blend_columns(x0, x1, full))


@pytest.mark.parametrize("btype", [MB, FE, NO])
def test_prepare_again_smaller_then_larger(ctx, btype):
    """One blender through prepare -> feed -> blend three times: a medium, a smaller and a larger panorama (the accumulators are
    grow-only and must come back zeroed)."""
    gb = _blender(ctx, btype, 5, 0.03)
    for k, (n, w, h) in enumerate([(3, 120, 90), (2, 50, 40), (4, 200, 130)]):
        rng = np.random.default_rng(90 + k)
        frames = strip(rng, n, w, h, int(w * 0.7), make_img=imgfull)
        sc = scene(btype, frames, 5, 0.03)
        gb.prepare(*_cs(frames))
        for img, mask, tl in _dev(frames):
            gb.feed(img, mask, tl)
        check(ctx, "prepare #%d" % k, gb, reference(sc), btype)


def test_feather_refuses_rows_wider_than_65536(ctx):
    import torch
    import image_stitching_amd as isa
    gb = isa.FeatherBlender(ctx, 0.01)
    gb.prepare([(0, 0)], [(65537, 2)])
    with pytest.raises(isa.MisError) as e:
        gb.feed(torch.zeros((2, 65537, 3), dtype=torch.int16, device="cuda"), torch.full((2, 65537), 255, dtype=torch.uint8, device="cuda"), (0, 0))
    assert e.value.code == E_UNSUPPORTED


@pytest.mark.parametrize("w,h", [(40, 40), (1280, 1280), (640, 2560), (1279, 1280), (9000, 2500)])
def test_blend_config_matches_reference(w, h):
    """The library's sizing: logf(blend_width), so a blend width of exactly 2^k gives k bands."""
    import image_stitching_amd as isa
    for btype in (MB, FE, NO):
        t, nb, sh = isa.stitching.blend_config(btype, 5.0, (w, h))
        rt, rnb, rsh = rb.blend_config(btype, 5.0, w, h)
        assert (t, nb, np.float32(sh)) == (rt, rnb, np.float32(rsh)), (btype, w, h)


@pytest.mark.parametrize("btype", [MB, FE])
def test_config3_4k_pair(ctx, btype):
    """Two adjacent BASELINE config-3 frames at 3840 x 2160 through the fused warp and one batched feed, blended with the band
    count (8) / sharpness blend_config gives for the 16-frame panorama, as the job does."""
    import torch
    import synth
    import image_stitching_amd as isa
    cams_all = synth.workload("config3")
    scale = isa.Stitcher.warped_image_scale(cams_all)
    rois = isa.stitching.warp_rois(ctx, scale, (3840, 2160), cams_all)
    _, _, pw, ph = rb.result_roi([r[:2] for r in rois], [r[2:] for r in rois])
    t, bands, sharp = isa.stitching.blend_config(btype, 5.0, (pw, ph))
    rt, rbands, rsharp = rb.blend_config(btype, 5.0, pw, ph)
    assert (t, bands, np.float32(sharp)) == (rt, rbands, np.float32(rsharp)) == (btype, 8 if btype == MB else 0, np.float32(rsharp))
    warper = isa.SphericalWarper(ctx, scale)
    items = []
    for cam in cams_all[7:9]:
        f = torch.from_numpy(synth.render_frame(cam)).cuda()
        items.append(warper.warp_fused(f, cam["K"].astype(np.float32), cam["R"].astype(np.float32)))
    corners, sizes = [i[0] for i in items], [(i[2].shape[1], i[2].shape[0]) for i in items]
    ref = rb.Blender(btype, bands, sharp).prepare(corners, sizes)
    for tl, img_s, msk in items:
        ref.feed(img_s.cpu().numpy(), msk.cpu().numpy(), tl)
    gb = _blender(ctx, btype, bands, sharp)
    gb.prepare(corners, sizes)
    gb.feed_batch([i[1] for i in items], [i[2] for i in items], [i[0] for i in items])
    check(ctx, "config-3 pair type %d" % btype, gb, ref, btype)
