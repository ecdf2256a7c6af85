"""GPU: the fused warp's entry points as entries -- what the other warp suites do not reach.  The timed entries (the benchmark's
measurement aid) write what the untimed ones write and refuse what they must; a batch of more than 16 frames (two grids) equals the
one-frame calls for the plane, cylindrical, fisheye and stereographic kinds; a bad frame in the middle of a batch fails the whole
call with the documented code and text, writes nothing, and leaves the context usable."""
import ctypes as C
import math

import numpy as np
import pytest

import refimpl as ri

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED = -1, -6
IMG_FILL, MASK_FILL = -7, 9      # values no warp writes: 16SC3 pixels are 0..255, mask bytes 0 or 255


def _capi():
    from image_stitching_amd import _capi as capi
    return capi


def _last_error(ctx):
    return ctx.lib.mis_last_error(ctx.h).decode()


def _mats(cams):
    fp = C.POINTER(C.c_float)
    Ks = np.ascontiguousarray(np.stack([np.asarray(c["K"], np.float32).reshape(9) for c in cams]))
    Rs = np.ascontiguousarray(np.stack([np.asarray(c["R"], np.float32).reshape(9) for c in cams]))
    return Ks, Rs, Ks.ctypes.data_as(fp), Rs.ctypes.data_as(fp)


def _prefilled(warper, rois):
    outs = [warper.alloc_fused(r) for r in rois]
    for d, m in outs:
        d.fill_(IMG_FILL); m.fill_(MASK_FILL)
    return outs


def _untouched(outs):
    return all(bool((d == IMG_FILL).all()) and bool((m == MASK_FILL).all()) for d, m in outs)


def _batch(ctx, kind, scale, srcs, cams, rois, dsts, masks, timed=None):
    """mis_warper_warp_fused_batch, or with timed = (repeats, want_avg) mis_warp_spherical_fused_batch_timed, into the caller's
    buffers -> (rc, [tl], avg_us)."""
    from image_stitching_amd.stitching import as_image
    capi = _capi()
    n = len(srcs)
    im = (capi.MisImage * n)(*[as_image(s) for s in srcs])
    ds = (capi.MisImage * n)(*[as_image(d) for d in dsts])
    ms = (capi.MisImage * n)(*[as_image(m) for m in masks])
    Ks, Rs, kp, rp = _mats(cams)
    rr = (capi.MisRect * n)(*[capi.MisRect(*[int(v) for v in r]) for r in rois])
    tls = (capi.MisPoint * n)()
    us = C.c_float(float("nan"))
    if timed is None:
        rc = ctx.lib.mis_warper_warp_fused_batch(ctx.h, int(kind), im, n, float(scale), kp, rp, rr, ds, ms, tls)
    else:
        assert kind == capi.WARP_SPHERICAL
        rc = ctx.lib.mis_warp_spherical_fused_batch_timed(ctx.h, im, n, float(scale), kp, rp, rr, ds, ms, tls, int(timed[0]),
                                                          C.byref(us) if timed[1] else None)
    return rc, [(t.x, t.y) for t in tls], us.value


def _timed_one(ctx, scale, src, cam, dst, msk, repeats, want_avg=True):
    """mis_warp_spherical_fused_timed into the caller's buffers -> (rc, tl, avg_us)."""
    from image_stitching_amd.stitching import _mat9, as_image
    capi = _capi()
    simg, dimg, mimg = as_image(src), as_image(dst), as_image(msk)
    (ka, kp), (ra, rp) = _mat9(cam["K"]), _mat9(cam["R"])
    tl, us = capi.MisPoint(), C.c_float(float("nan"))
    rc = ctx.lib.mis_warp_spherical_fused_timed(ctx.h, C.byref(simg), float(scale), kp, rp, C.byref(dimg), C.byref(mimg), C.byref(tl),
                                                int(repeats), C.byref(us) if want_avg else None)
    return rc, (tl.x, tl.y), us.value


def _ragged_scene(ctx, kind, n=3):
    """n frames of the 333 x 217 source at scale multiplier 0.37 (test_warpers_gpu.py), different yaws -> (scale, cams, srcs, rois);
    every roi spans at least two 64-column strips and two 16-row tiles and is ragged in both directions."""
    import torch
    import image_stitching_amd as isa
    w, h = 333, 217
    cams, scale = [], None
    for i in range(n):
        K, R, scale = ri.camera(w, h, 60.0, (-20.0, 0.0, 25.0, 11.0)[i % 4], 2.5 * (i - 1), 1.5 * i, 0.37, seam=True)
        cams.append({"K": K, "R": R})
    srcs = [torch.from_numpy(ri.content("rand", (h, w, 3), seed=40 + i)).cuda() for i in range(n)]
    rois = isa.stitching.warp_rois(ctx, scale, (w, h), cams, kind)
    for r in rois:
        assert r[2] > 64 and r[3] > 16 and r[2] % 64 != 0 and r[3] % 16 != 0, r
    return scale, cams, srcs, rois


@pytest.fixture(scope="module")
def spherical_scene(ctx):
    """The ragged three-frame spherical scene with the results of the untimed one-frame calls: computed once, read only."""
    import image_stitching_amd as isa
    capi = _capi()
    scale, cams, srcs, rois = _ragged_scene(ctx, capi.WARP_SPHERICAL)
    warper = isa.SphericalWarper(ctx, scale)
    want = [warper.warp_fused(s, c["K"], c["R"], r) for s, c, r in zip(srcs, cams, rois)]
    ctx.synchronize()
    return scale, cams, srcs, rois, warper, want


@pytest.mark.parametrize("repeats", [1, 3])
def test_timed_one_frame_equals_untimed(ctx, spherical_scene, repeats):
    """mis_warp_spherical_fused_timed: image, mask and tl of warp_fused(..., roi) for every launch count; the time is a number."""
    import torch
    scale, cams, srcs, rois, warper, want = spherical_scene
    for k in range(len(srcs)):
        (dst, msk), = _prefilled(warper, [rois[k]])
        rc, tl, us = _timed_one(ctx, scale, srcs[k], cams[k], dst, msk, repeats)
        ctx.synchronize()
        assert rc == 0, _last_error(ctx)
        assert tl == tuple(want[k][0]) == (rois[k][0], rois[k][1])
        assert torch.equal(dst, want[k][1]) and torch.equal(msk, want[k][2])
        assert math.isfinite(us) and us > 0
    # the Python wrapper bench.py calls
    (dst, msk), = _prefilled(warper, [rois[0]])
    us = warper.warp_fused_timed(srcs[0], cams[0]["K"], cams[0]["R"], rois[0], dst, msk, repeats)
    ctx.synchronize()
    assert torch.equal(dst, want[0][1]) and torch.equal(msk, want[0][2]) and math.isfinite(us) and us > 0


@pytest.mark.parametrize("repeats", [1, 3])
def test_timed_batch_equals_untimed(ctx, spherical_scene, repeats):
    """mis_warp_spherical_fused_batch_timed over three frames: what mis_warper_warp_fused_batch and the one-frame calls write."""
    import torch
    capi = _capi()
    scale, cams, srcs, rois, warper, want = spherical_scene
    plain = warper.warp_fused_batch(srcs, cams, rois)
    outs = _prefilled(warper, rois)
    rc, tls, us = _batch(ctx, capi.WARP_SPHERICAL, scale, srcs, cams, rois, [o[0] for o in outs], [o[1] for o in outs], timed=(repeats, True))
    ctx.synchronize()
    assert rc == 0, _last_error(ctx)
    assert math.isfinite(us) and us > 0
    for k in range(len(srcs)):
        assert tls[k] == tuple(plain[k][0]) == tuple(want[k][0])
        assert torch.equal(outs[k][0], plain[k][1]) and torch.equal(outs[k][1], plain[k][2])
        assert torch.equal(outs[k][0], want[k][1]) and torch.equal(outs[k][1], want[k][2])
    outs = _prefilled(warper, rois)      # the Python wrapper bench.py calls
    us = warper.warp_fused_batch_timed(srcs, cams, rois, [o[0] for o in outs], [o[1] for o in outs], repeats)
    ctx.synchronize()
    assert math.isfinite(us) and us > 0
    for k in range(len(srcs)):
        assert torch.equal(outs[k][0], want[k][1]) and torch.equal(outs[k][1], want[k][2])


def test_timed_entries_refuse_bad_arguments_and_recover(ctx, spherical_scene):
    """repeats = 0 and a null avg_us: MIS_E_INVALID with the entry's text, nothing written; the next good call is good."""
    import torch
    capi = _capi()
    scale, cams, srcs, rois, warper, want = spherical_scene
    one_text = "repeats must be >= 1 and avg_us non-null"
    batch_text = "repeats must be >= 1, n >= 1 and avg_us non-null"
    for repeats, want_avg in ((0, True), (1, False)):
        (dst, msk), = _prefilled(warper, [rois[0]])
        rc, _, _ = _timed_one(ctx, scale, srcs[0], cams[0], dst, msk, repeats, want_avg)
        assert rc == E_INVALID and _last_error(ctx) == one_text
        ctx.synchronize()
        assert _untouched([(dst, msk)])
        rc, tl, us = _timed_one(ctx, scale, srcs[0], cams[0], dst, msk, 1)
        ctx.synchronize()
        assert rc == 0 and tl == tuple(want[0][0]) and torch.equal(dst, want[0][1]) and torch.equal(msk, want[0][2])

        outs = _prefilled(warper, rois)
        dsts, masks = [o[0] for o in outs], [o[1] for o in outs]
        rc, _, _ = _batch(ctx, capi.WARP_SPHERICAL, scale, srcs, cams, rois, dsts, masks, timed=(repeats, want_avg))
        assert rc == E_INVALID and _last_error(ctx) == batch_text
        ctx.synchronize()
        assert _untouched(outs)
        rc, tls, us = _batch(ctx, capi.WARP_SPHERICAL, scale, srcs, cams, rois, dsts, masks, timed=(1, True))
        ctx.synchronize()
        assert rc == 0 and math.isfinite(us) and us > 0
        for k in range(len(srcs)):
            assert tls[k] == tuple(want[k][0]) and torch.equal(dsts[k], want[k][1]) and torch.equal(masks[k], want[k][2])


@pytest.mark.parametrize("kind_name", ["plane", "cylindrical", "fisheye", "stereographic"])
def test_batch_of_17_frames_equals_single_launches(ctx, kind_name):
    """17 frames = two grids (16 + 1) of mis_warper_warp_fused_batch for the kinds that had no such case: the bytes of 17
    mis_warper_warp_fused_roi calls.  The yaw sweep of +-40 degrees keeps the plane's frames (hfov 60) in front of the panorama plane."""
    import torch
    import image_stitching_amd as isa
    kind = isa.stitching.WARP_KINDS[kind_name]
    w, h, n = 48, 32, 17
    cams, scale = [], None
    for i in range(n):
        K, R, scale = ri.camera(w, h, 60.0, -40.0 + 5.0 * i, 0.5 * ((i % 3) - 1), 0.4 * ((i % 2) - 0.5))
        cams.append({"K": K, "R": R})
    srcs = [torch.from_numpy(ri.content("rand", (h, w, 3), seed=90 + i)).cuda() for i in range(n)]
    rois = isa.stitching.warp_rois(ctx, scale, (w, h), cams, kind)
    warper = isa.RotationWarper(ctx, scale, kind)
    single = [warper.warp_fused(s, c["K"], c["R"], r) for s, c, r in zip(srcs, cams, rois)]
    outs = _prefilled(warper, rois)
    rc, tls, _ = _batch(ctx, kind, scale, srcs, cams, rois, [o[0] for o in outs], [o[1] for o in outs])
    ctx.synchronize()
    assert rc == 0, _last_error(ctx)
    for k in range(n):
        assert tls[k] == tuple(single[k][0]) == (rois[k][0], rois[k][1])
        assert torch.equal(outs[k][0], single[k][1]) and torch.equal(outs[k][1], single[k][2]), k


@pytest.mark.parametrize("kind_name", ["cylindrical", "fisheye"])       # one separable and one polar kind
def test_batch_refusals_keep_their_contract(ctx, kind_name):
    """A three-frame batch whose frame 1 is bad -- an empty roi, a one-channel source, a mask with an odd row pitch -- fails as a
    whole with the code and the text of the check that refuses it, writes nothing, and the same context then warps the good batch."""
    import torch
    import image_stitching_amd as isa
    kind = isa.stitching.WARP_KINDS[kind_name]
    scale, cams, srcs, rois = _ragged_scene(ctx, kind)
    warper = isa.RotationWarper(ctx, scale, kind)
    want = [warper.warp_fused(s, c["K"], c["R"], r) for s, c, r in zip(srcs, cams, rois)]
    ctx.synchronize()

    def good():
        outs = _prefilled(warper, rois)
        rc, tls, _ = _batch(ctx, kind, scale, srcs, cams, rois, [o[0] for o in outs], [o[1] for o in outs])
        ctx.synchronize()
        assert rc == 0, _last_error(ctx)
        for k in range(3):
            assert tls[k] == tuple(want[k][0]) and torch.equal(outs[k][0], want[k][1]) and torch.equal(outs[k][1], want[k][2])

    def refused(code, text, srcs_=srcs, rois_=rois, mask1=None):
        outs = _prefilled(warper, rois)
        masks = [o[1] for o in outs]
        if mask1 is not None:
            masks[1] = mask1
        rc, _, _ = _batch(ctx, kind, scale, srcs_, cams, rois_, [o[0] for o in outs], masks)
        assert rc == code and _last_error(ctx) == text, (rc, _last_error(ctx))
        ctx.synchronize()
        assert _untouched(outs) and (mask1 is None or bool((mask1 == MASK_FILL).all()))
        good()

    x, y, rw, rh = rois[1]
    refused(E_INVALID, "frame 1: empty roi", rois_=[rois[0], (x, y, 0, rh), rois[2]])
    refused(E_UNSUPPORTED, "fused warp needs an 8UC3 source", srcs_=[srcs[0], srcs[1][:, :, 0].contiguous(), srcs[2]])
    pitch = rw + 1 if rw % 2 == 0 else rw + 2        # odd, and a row fits
    odd = torch.full((rh, pitch), MASK_FILL, dtype=torch.uint8, device=srcs[0].device)[:, :rw]
    assert odd.stride(0) % 2 == 1
    refused(E_INVALID, "fused warp outputs need 4-byte (image) / 2-byte (mask) aligned rows", mask1=odd)
