"""mis_warper_warp_backward and its batch form: a pinhole view rendered out of an image that lies in the warper's plane.

The device bytes and mask equal the exact reference (tests/refimpl_warp_backward.py: the integer cv::remap of a float32 map) applied
to the HOST forward map -- warp_points with a NULL context, minus src_tl in float32.  No bands and no excluded pixels: every kind
except the affine one, all twelve refimpl.WARP_GEOMS, the three (interp, border) pairs, 1 and 3 channels, views 1x1 .. 257x33,
sources 2x2, 5x7 and 300x40 placed so that the view's taps cross every source edge (src_tl negative and positive), pitched and
unaligned src / dst / mask rows.  A batch of 17 views of mixed sizes equals the single calls.  On the geometries whose float64 forward
reference is decided everywhere (tests/test_refimpl_warp_points_cpu.py) the device bytes also pass the float64 candidate check,
with at most 2 % of the pixels undecided.

Printed, not asserted: the mean absolute error of warp followed by warpBackward on a textured frame."""
import ctypes as C

import numpy as np
import pytest
import torch

import refimpl as ri
import refimpl_warp_backward as rb
import image_stitching_amd as isa

pytestmark = pytest.mark.gpu
capi, st = isa._capi, isa.stitching
KINDS = {n: k for n, k in rb.KINDS.items() if k != rb.AFFINE}
VIEWS = [(1, 1), (1, 7), (7, 1), (63, 9), (64, 8), (65, 9), (129, 17), (257, 33)]
SOURCES = [(2, 2), (5, 7), (300, 40)]
DECIDED_GEOMS = ("front", "roll+30", "roll-30", "hfov30", "hfov90", "hfov150")


def source(w, h, cn, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3) if cn == 3 else (h, w), dtype=np.uint8)


def dev_pitched(arr, extra):
    """arr on the device with `extra` bytes between its rows (extra = 0: dense) -> (buffer, view)."""
    h, w = arr.shape[:2]
    cn = arr.shape[2] if arr.ndim == 3 else 1
    buf = torch.full((h, w * cn + extra), 9, dtype=torch.uint8, device="cuda")
    buf[:, : w * cn] = torch.from_numpy(np.ascontiguousarray(arr).reshape(h, w * cn)).cuda()
    view = buf.as_strided((h, w, cn), (w * cn + extra, cn, 1)) if cn == 3 else buf[:, :w]
    return buf, view


def host_forward(kind, scale, K, R, vw, vh):
    return isa.RotationWarper(None, scale, kind).warp_points(rb.view_points(vw, vh), K, R)


def place_source(uv, sw, sh, k):
    """src_tl that puts the sw x sh source around the middle of the view's footprint (its taps then cross the source's edges), shifted
    by a few pixels that change with k."""
    fin = np.isfinite(uv).all(1)
    c = np.median(uv[fin], 0) if fin.any() else np.zeros(2)
    return int(np.clip(round(float(c[0])), -1e6, 1e6)) - sw // 2 + (k % 3) - 1, int(np.clip(round(float(c[1])), -1e6, 1e6)) - sh // 2 + (k % 2)


def reference(src, uv, src_tl, vw, vh, interp, border):
    xm, ym = rb.back_maps_f32(uv, src_tl, (vh, vw))
    return rb.remap_exact(src, xm, ym, interp, border), rb.nearest_mask(src.shape, xm, ym)


@pytest.mark.parametrize("name", list(KINDS))
def test_device_views_equal_the_exact_reference_on_the_host_map(ctx, name):
    kind = KINDS[name]
    k = 0
    tls = []
    for gi, g in enumerate(ri.WARP_GEOMS):
        for j in range(2):      # two (view, source, channels) combinations per geometry; all of them over the geometries
            (vw, vh), (sw, sh) = VIEWS[(2 * gi + j) % len(VIEWS)], SOURCES[(gi + j) % len(SOURCES)]
            cn = 3 if (gi + j) % 2 == 0 else 1
            K, R, scale = ri.camera(vw, vh, *g[1:])
            uv = host_forward(kind, scale, K, R, vw, vh)
            tl = place_source(uv, sw, sh, k)
            tls.append(tl)
            src = source(sw, sh, cn, 10 * gi + j)
            w = isa.RotationWarper(ctx, scale, kind)
            _, dsrc = dev_pitched(src, (0, 5, 16)[k % 3])
            for interp, border in rb.PAIRS:
                k += 1
                want, want_mask = reference(src, uv, tl, vw, vh, interp, border)
                if k % 2:       # the library's buffers (256-byte pitch: dword stores)
                    got, mask = w.warp_backward(dsrc, tl, K, R, (vw, vh), interp, border, with_mask=True)
                else:           # the caller's, rows off the 4-byte grid (byte stores) with a sentinel between them
                    bd, dv = dev_pitched(np.zeros_like(want), 3)
                    bm, mv = dev_pitched(np.zeros((vh, vw), np.uint8), 1)
                    got, mask = w.warp_backward(dsrc, tl, K, R, (vw, vh), interp, border, with_mask=True, dst=dv, mask=mv)
                    assert (bd[:, vw * cn:] == 9).all() and (bm[:, vw:] == 9).all(), "wrote between the rows"
                got, mask = got.cpu().numpy().reshape(want.shape), mask.cpu().numpy().reshape(vh, vw)
                assert np.array_equal(got, want), (name, g[0], (vw, vh), (sw, sh), cn, interp, border, tl, int((got != want).sum()))
                assert np.array_equal(mask, want_mask), (name, g[0], (vw, vh), (sw, sh), interp, border, tl)
    # the placements put the source on either side of the plane's origin (the kinds centred on it have no corner with both signs positive)
    assert any(t[0] < 0 for t in tls) and any(t[1] < 0 for t in tls) and any(t[0] > 0 or t[1] > 0 for t in tls)


@pytest.mark.parametrize("name", list(KINDS))
def test_float64_candidate_check_on_the_decided_geometries(ctx, name):
    kind = KINDS[name]
    vw, vh, sw, sh = 129, 17, 300, 40
    for gi, g in enumerate(ri.WARP_GEOMS):
        if g[0] not in DECIDED_GEOMS:
            continue
        K, R, scale = ri.camera(vw, vh, *g[1:])
        pts = rb.view_points(vw, vh)
        u, v, bu, bv, ok = (a.reshape(vh, vw) for a in rb.forward_ref(kind, K, R, scale, pts[:, 0], pts[:, 1]))
        tl = (int(round(float(np.median(u[ok])))) - sw // 2, int(round(float(np.median(v[ok])))) - sh // 2)
        src = source(sw, sh, 3, gi)
        w = isa.RotationWarper(ctx, scale, kind)
        for interp, border in rb.PAIRS:
            cands, in_band, und = rb.back_candidates(src, u, v, bu, bv, ok, tl, interp, border)
            assert und.mean() <= rb.MAX_UNDECIDED_SHARE, (name, g[0], und.mean())       # the reference alone
            got = w.warp_backward(torch.from_numpy(src).cuda(), tl, K, R, (vw, vh), interp, border).cpu().numpy()
            bad, _, _ = ri.check_candidates(got, cands, in_band, und)
            assert not bad.any(), (name, g[0], interp, border, int(bad.sum()))


def test_a_batch_of_17_mixed_views_equals_the_single_calls(ctx):
    sw, sh = 300, 40
    src = source(sw, sh, 3, 1)
    dsrc = torch.from_numpy(src).cuda()
    for kind in (rb.SPHERICAL, rb.FISHEYE, rb.PANINI_A15B1):
        scale = 80.0
        w = isa.RotationWarper(ctx, scale, kind)
        cams, sizes = [], []
        for i in range(17):
            vw, vh = VIEWS[i % len(VIEWS)]
            K, R, _ = ri.camera(vw, vh, 50.0 + 3 * i, -40.0 + 5 * i, 2.0 * (i % 5) - 4.0, 3.0 * i)
            cams.append({"K": K, "R": R})
            sizes.append((vw, vh))
        tl = (-150, 100 if kind == rb.SPHERICAL else -20)
        for interp, border in rb.PAIRS:
            outs = w.warp_backward_batch(dsrc, tl, cams, sizes, interp, border, with_mask=True)
            assert len(outs) == 17
            for i, (img, msk) in enumerate(outs):
                one, onem = w.warp_backward(dsrc, tl, cams[i]["K"], cams[i]["R"], sizes[i], interp, border, with_mask=True)
                assert img.shape[:2] == (sizes[i][1], sizes[i][0])
                assert torch.equal(img, one) and torch.equal(msk, onem), (kind, i, interp, border)
        plain = w.warp_backward_batch(dsrc, tl, cams, sizes)
        assert all(torch.equal(a, b[0]) for a, b in zip(plain, w.warp_backward_batch(dsrc, tl, cams, sizes, with_mask=True)))
        assert w.warp_backward_batch(dsrc, tl, [], []) == []


def test_warpBackward_is_opencvs_call_with_its_size_assertion(ctx, capsys):
    wd, hd = 160, 90
    K, R, scale = ri.camera(wd, hd, 60.0, 15.0, -5.0, 4.0)
    yy, xx = np.mgrid[0:hd, 0:wd]
    frame = np.stack([(127 + 100 * np.sin(xx / 9.0) * np.cos(yy / 7.0)), (xx * 255.0 / wd), (yy * 255.0 / hd)], -1).astype(np.uint8)
    for name, kind in KINDS.items():
        w = isa.RotationWarper(ctx, scale, kind)
        tl, warped = w.warp(torch.from_numpy(frame).cuda(), K, R)
        back = w.warpBackward(warped, K, R, capi.INTER_LINEAR, capi.BORDER_REFLECT, (wd, hd))
        assert back.shape == (hd, wd, 3)
        roi = w.warp_roi((wd, hd), K, R)
        uv = host_forward(kind, scale, K, R, wd, hd)
        want, _ = reference(warped.cpu().numpy(), uv, roi[:2], wd, hd, capi.INTER_LINEAR, capi.BORDER_REFLECT)
        assert np.array_equal(back.cpu().numpy(), want), name
        mae = np.abs(back.cpu().numpy().astype(np.int32) - frame.astype(np.int32)).mean()
        with capsys.disabled():
            print("warp -> warpBackward, %-18s mean absolute error %.3f grey levels" % (name, mae))
        with pytest.raises(ValueError):
            w.warpBackward(warped[:-1], K, R, capi.INTER_LINEAR, capi.BORDER_REFLECT, (wd, hd))
        with pytest.raises(ValueError):
            w.warpBackward(warped, K, R, capi.INTER_LINEAR, capi.BORDER_REFLECT, (2 * wd, hd))


def test_refusals_leave_the_outputs_untouched(ctx):
    K, R, scale = ri.camera(16, 8, 60.0, 0.0)
    src = torch.from_numpy(source(20, 10, 3, 0)).cuda()
    dst = torch.full((8, 16, 3), 5, dtype=torch.uint8, device="cuda")
    msk = torch.full((8, 16), 5, dtype=torch.uint8, device="cuda")
    _, kp = st._mat9(K)
    _, rp = st._mat9(R)
    si, di, mi = st.as_image(src), st.as_image(dst), st.as_image(msk)
    wb = ctx.lib.mis_warper_warp_backward
    tl = capi.MisPoint(-3, 4)

    def call(kind=0, s=si, sc=scale, k=kp, r=rp, interp=1, border=0, w=16, h=8, d=di, m=mi):
        return wb(ctx.h, kind, C.byref(s) if s is not None else None, tl, sc, k, r, interp, border, w, h, C.byref(d) if d is not None else None,
                  C.byref(m) if m is not None else None)

    assert call() == capi.MIS_OK
    dst.fill_(5); msk.fill_(5)
    for kind in (-1, 6, 7, 12, 14):
        assert call(kind=kind) == capi.MIS_E_UNSUPPORTED
    assert call(kind=capi.WARP_AFFINE) == capi.MIS_E_UNSUPPORTED
    assert b"AffineWarper" in ctx.lib.mis_last_error(ctx.h)
    for interp, border in ((0, 2), (2, 0), (1, 1), (1, 4), (0, 1)):
        assert call(interp=interp, border=border) == capi.MIS_E_UNSUPPORTED, (interp, border)
    gray16 = st.as_image(torch.zeros((10, 20), dtype=torch.int16, device="cuda"))
    assert call(s=gray16) == capi.MIS_E_UNSUPPORTED
    for kw in (dict(s=None), dict(k=None), dict(r=None), dict(d=None), dict(sc=0.0), dict(sc=-2.0), dict(w=0), dict(h=-1), dict(w=17), dict(h=7)):
        assert call(**kw) == capi.MIS_E_INVALID, kw
    tiny = st.as_image(torch.zeros((1, 20, 3), dtype=torch.uint8, device="cuda"))
    assert call(s=tiny) == capi.MIS_E_INVALID
    ctx.synchronize()
    assert (dst == 5).all() and (msk == 5).all()
    # a batch: the refused view names itself, and the views in front of it stay untouched as well
    w = isa.RotationWarper(ctx, scale, capi.WARP_SPHERICAL)
    with pytest.raises(ValueError):
        w.warp_backward_batch(src, (-3, 4), [{"K": K, "R": R}] * 3, [(16, 8), (16, 8), (0, 8)])
    outs = st._images([dst, dst, dst])
    Ks = np.ascontiguousarray(np.stack([K.reshape(9)] * 3)); Rs = np.ascontiguousarray(np.stack([R.reshape(9)] * 3))
    for last in ((16, 9), (0, 8)):      # a buffer of another size; an empty view
        sizes = st._c_array(capi.MisSize, [capi.MisSize(16, 8), capi.MisSize(16, 8), capi.MisSize(*last)])
        rc = ctx.lib.mis_warper_warp_backward_batch(ctx.h, 0, C.byref(si), tl, scale, 3, Ks.ctypes.data_as(C.c_void_p), Rs.ctypes.data_as(C.c_void_p), sizes, 1, 0, outs, None)
        assert rc == capi.MIS_E_INVALID and b"view 2" in ctx.lib.mis_last_error(ctx.h), last
    sizes = st._c_array(capi.MisSize, [capi.MisSize(16, 8)] * 3)
    assert ctx.lib.mis_warper_warp_backward_batch(ctx.h, 0, C.byref(si), tl, scale, -1, Ks.ctypes.data_as(C.c_void_p), Rs.ctypes.data_as(C.c_void_p), sizes, 1, 0, outs, None) == capi.MIS_E_INVALID
    assert ctx.lib.mis_warper_warp_backward_batch(ctx.h, 0, C.byref(si), tl, scale, 0, None, None, None, 1, 0, None, None) == capi.MIS_OK
    ctx.synchronize()
    assert (dst == 5).all()
    with pytest.raises(st.MisError) as e:
        isa.AffineWarper(ctx, 1.0).warp_backward(src, (0, 0), np.eye(3), np.eye(3), (16, 8))
    assert e.value.code == capi.MIS_E_UNSUPPORTED


def test_stitcher_render_view_goes_back_from_the_panorama(ctx, small_pair):
    cams, frames = small_pair
    s = isa.Stitcher(ctx, (480, 270))
    pano, mask = s.compose({i: torch.from_numpy(f).cuda() for i, f in enumerate(frames)}, cams)
    c = s.composition
    assert c["kind"] == capi.WARP_SPHERICAL and c["warp_scale"] > 0
    pano_u8 = pano.clamp(0, 255).to(torch.uint8).contiguous()
    K, R = np.asarray(cams[0]["K"], np.float32), np.asarray(cams[0]["R"], np.float32)
    view, vmask = s.render_view(pano_u8, K, R, (480, 270), with_mask=True)
    uv = host_forward(c["kind"], c["warp_scale"], K, R, 480, 270)
    want, want_mask = reference(pano_u8.cpu().numpy(), uv, c["pano_tl"], 480, 270, capi.INTER_LINEAR, capi.BORDER_CONSTANT)
    assert np.array_equal(view.cpu().numpy(), want) and np.array_equal(vmask.cpu().numpy().reshape(270, 480), want_mask)
    assert (want_mask == 255).mean() > 0.9      # the first camera looks into the panorama it is part of
