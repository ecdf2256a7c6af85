"""GPU: the timelapse sink.  (a) Timelapser.process against a numpy placement of the same 16SC3 image; (b) the fused batch
mis_timelapse_warp_batch against the sequence of already pinned entries it replaces -- mis_warper_warp_fused_roi ->
mis_compensator_apply -> numpy placement -> clamp -- for every warper kind, both canvas types, both output formats, with and
without gains, bit for bit; (c) the error contract: a refusal writes nothing.

The scene: four 160 x 120 frames, focal 150, yaws -8, 0, +8 and one frame at yaw 3 pitched by 3 degrees (the affine kind: four
similarities of its own).  For every kind the rois overlap, have negative corners, differ in size and are no multiple of the
kernel's 128 x 32 tile; the CROP intersection is at least 32 x 32 and smaller than every roi, the AS_IS union larger than every one
(asserted per kind)."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E_INVALID, E_UNSUPPORTED, E_STATE = -1, -6, -5
W, H, FOCAL = 160, 120, 150.0
POSES = [(-8.0, 0.0), (0.0, 0.0), (8.0, 0.0), (3.0, 3.0)]                  # (yaw, pitch) in degrees
AFFINE_T = [(-21.0, 3.5), (0.0, 0.0), (23.0, -4.0), (7.5, 9.0)]            # the affine kind's translations; its angle is the pitch
BRIGHTNESS = [0.55, 0.75, 0.95, 0.7]
KINDS = [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 13]                                # every kind mis_warper_warp_fused_batch accepts
S16_SENTINEL, U8_SENTINEL = -7, 201


def _rot(axis, deg):
    a = math.radians(deg)
    c, s = math.cos(a), math.sin(a)
    return {"y": np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]), "x": np.array([[1, 0, 0], [0, c, -s], [0, s, c]])}[axis]


def scene_cameras(kind):
    """-> (scale, [{"K", "R"}]) of the module's scene for a warper kind."""
    if kind == 13:
        cams = []
        for (_, ang), t in zip(POSES, AFFINE_T):
            a = math.radians(ang)
            cams.append({"K": np.eye(3, dtype=np.float32),
                         "R": np.array([[math.cos(a), -math.sin(a), t[0]], [math.sin(a), math.cos(a), t[1]], [0, 0, 1]], np.float32)})
        return 1.0, cams
    K = np.array([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]], np.float32)
    return FOCAL, [{"K": K, "R": (_rot("y", yaw) @ _rot("x", pitch)).astype(np.float32)} for yaw, pitch in POSES]


def place(img, tl, dst_roi):
    """Timelapser::process in numpy: the canvas of dst_roi's size set to 0, then the part of img (top-left at tl) inside it."""
    x, y, w, h = dst_roi
    out = np.zeros((h, w, 3), img.dtype)
    ih, iw = img.shape[:2]
    x0, y0 = max(tl[0], x), max(tl[1], y)
    x1, y1 = min(tl[0] + iw, x + w), min(tl[1] + ih, y + h)
    if x1 > x0 and y1 > y0:
        out[y0 - y:y1 - y, x0 - x:x1 - x] = img[y0 - tl[1]:y1 - tl[1], x0 - tl[0]:x1 - tl[0]]
    return out


def sentinel_canvas(w, h, dtype, extra_elems):
    """A caller's canvas whose rows are `extra_elems` elements wider than the image, everything set to the sentinel
    -> (view (h, w, 3), backing (h, pitch))."""
    import torch
    pitch = 3 * w + extra_elems
    back = torch.full((h + 2, pitch), S16_SENTINEL if dtype == torch.int16 else U8_SENTINEL, dtype=dtype, device="cuda")
    return back[1:h + 1].as_strided((h, w, 3), (pitch, 3, 1), back[1:h + 1].storage_offset()), back


def padding_untouched(back, w, h):
    sent = S16_SENTINEL if back.element_size() == 2 else U8_SENTINEL
    return bool((back[0] == sent).all()) and bool((back[h + 1] == sent).all()) and bool((back[1:h + 1, 3 * w:] == sent).all())


@pytest.fixture(scope="module")
def scenes(ctx):
    """Per kind, computed once and read only: the scene, the rois (the context-free mis_warper_roi), both canvas rectangles and the
    reference -- the fused one-frame warps (mis_warper_warp_fused_roi) as numpy 16SC3, the gains of a fed GainCompensator and the
    warps after its mis_compensator_apply."""
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd.stitching import warp_roi
    out = {}
    for kind in KINDS:
        scale, cams = scene_cameras(kind)
        # noise of four different brightnesses: the compensator's gains are then far enough from 1 to change most pixels
        srcs = [torch.from_numpy((np.random.default_rng(100 + i).integers(0, 256, (H, W, 3)) * BRIGHTNESS[i]).astype(np.uint8)).cuda() for i in range(len(cams))]
        rois = [warp_roi(scale, (W, H), c["K"], c["R"], kind) for c in cams]
        corners, sizes = [(r[0], r[1]) for r in rois], [(r[2], r[3]) for r in rois]
        union, crop = isa.result_roi(corners, sizes), isa.result_roi_intersection(corners, sizes)
        assert crop[2] >= 32 and crop[3] >= 32 and all(crop[2] < r[2] or crop[3] < r[3] for r in rois), (kind, crop, rois)
        assert all(union[2] > r[2] or union[3] > r[3] for r in rois) and any(r[0] < 0 or r[1] < 0 for r in rois), (kind, union, rois)
        assert len(set(sizes)) > 1 and (union[2] % 128 or union[3] % 32) and (crop[2] % 128 or crop[3] % 32)
        warper = isa.RotationWarper(ctx, scale, kind)
        warped = [warper.warp_fused(s, c["K"], c["R"], r) for s, c, r in zip(srcs, cams, rois)]
        comp = isa.GainCompensator(ctx)
        comp.feed(corners, [w[1].clamp(0, 255).to(torch.uint8).contiguous() for w in warped], [w[2].contiguous() for w in warped])
        gains = np.stack([comp.gains(k) for k in range(len(cams))])
        assert np.abs(gains - 1).max() > 0.05, gains
        plain = [w[1].cpu().numpy() for w in warped]
        gained = [comp.apply(k, corners[k], warped[k][1].clone()).cpu().numpy() for k in range(len(cams))]
        out[kind] = dict(scale=scale, cams=cams, srcs=srcs, rois=rois, corners=corners, rect={"as_is": union, "crop": crop},
                         plain=plain, gained=gained, gains=gains)
    ctx.synchronize()
    return out


# ---------------------------------------------------------------- (a) Timelapser.process
PLACE_CORNERS, PLACE_SIZES = [(-10, -5), (20, 8)], [(100, 80), (90, 70)]      # union (-10, -5, 120, 83), intersection (20, 8, 70, 67)
PLACE_CASES = [("first frame", (100, 80), (-10, -5)), ("partly outside", (50, 41), (61, 50)), ("partly outside, top left", (37, 23), (-30, -20)),
               ("wholly outside", (40, 30), (500, 500)), ("wholly outside, left", (40, 30), (-60, 0)), ("covers the canvas", (201, 151), (-31, -22)),
               ("one pixel", (1, 1), (25, 9))]


@pytest.mark.parametrize("ttype", ["as_is", "crop"])
def test_process_equals_numpy_placement(ctx, ttype):
    import torch
    import image_stitching_amd as isa
    t = isa.Timelapser(ctx, ttype)
    t.initialize(PLACE_CORNERS, PLACE_SIZES)
    roi = t.dst_roi()
    assert roi == ((-10, -5, 120, 83) if ttype == "as_is" else (20, 8, 70, 67))
    rng = np.random.default_rng(5)
    for tag, (w, h), tl in PLACE_CASES:
        img = rng.integers(-32768, 32768, (h, w, 3), dtype=np.int16)        # process copies any 16S value
        want = place(img, tl, roi)
        if tag.startswith("wholly"):
            assert not want.any()
        dimg = torch.from_numpy(img).cuda()
        got = t.process(dimg, None, tl)                                   # a canvas of the library's pitch
        assert t.getDst() is got and np.array_equal(got.cpu().numpy(), want), (ttype, tag)
        for extra in (1, 2, 5):      # rows of 6 w + 2, 4, 10 bytes: 2-byte and 4-byte aligned pitches
            view, back = sentinel_canvas(roi[2], roi[3], torch.int16, extra)
            t.process(dimg, None, tl, dst=view)
            assert np.array_equal(view.cpu().numpy(), want) and padding_untouched(back, roi[2], roi[3]), (ttype, tag, extra)
        host = np.full((roi[3], roi[2], 3), S16_SENTINEL, np.int16)         # host image in, host canvas out
        t.process(img, None, tl, dst=host)
        assert np.array_equal(host, want), (ttype, tag)


# ---------------------------------------------------------------- (b) the fused batch
def _expected(sc, ttype, gains, as_u8, order):
    ref = sc["gained"] if gains else sc["plain"]
    exp = [np.clip(place(ref[k], sc["corners"][k], sc["rect"][ttype]), 0, 255) for k in order]
    return [e.astype(np.uint8) if as_u8 else e for e in exp]


def _run(ctx, sc, kind, ttype, gains, as_u8, order, dsts=None):
    import image_stitching_amd as isa
    return isa.timelapse_warp_batch(ctx, kind, [sc["srcs"][k] for k in order], [sc["cams"][k] for k in order], [sc["rois"][k] for k in order],
                                    sc["scale"], sc["rect"][ttype], sc["gains"][order] if gains else None, as_u8, dsts)


@pytest.mark.parametrize("ttype", ["as_is", "crop"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_batch_equals_warp_apply_place_clamp(ctx, scenes, kind, ttype):
    sc = scenes[kind]
    order = list(range(len(sc["srcs"])))
    for gains in (False, True):
        for as_u8 in (False, True):
            got = _run(ctx, sc, kind, ttype, gains, as_u8, order)
            for k, (g, e) in enumerate(zip(got, _expected(sc, ttype, gains, as_u8, order))):
                g = g.cpu().numpy()
                assert g.dtype == e.dtype and g.shape == e.shape, (kind, ttype, gains, as_u8, k)
                assert np.array_equal(g, e), (kind, ttype, gains, as_u8, k, int((g != e).sum()))


@pytest.mark.parametrize("kind", [0, 4, 10])      # one kind per kernel class with tables of its own, the polar class included
@pytest.mark.parametrize("n", [1, 17])            # 17: two grids of 16 + 1 frames
def test_fused_batch_of_1_and_17(ctx, scenes, kind, n):
    sc = scenes[kind]
    order = [(3 * i + 1) % len(sc["srcs"]) for i in range(n)]
    for ttype in ("as_is", "crop"):
        got = _run(ctx, sc, kind, ttype, True, True, order)
        assert len(got) == n
        for g, e in zip(got, _expected(sc, ttype, True, True, order)):
            assert np.array_equal(g.cpu().numpy(), e), (kind, ttype, n)


@pytest.mark.parametrize("as_u8", [False, True])
def test_fused_batch_into_caller_buffers_of_any_pitch(ctx, scenes, as_u8):
    """Rows that are not 4-byte aligned take the element stores, aligned ones the dwordx3 stores: the same canvases, and nothing
    is written past a row's end or outside the canvas."""
    import torch
    kind, order = 8, [0, 1, 2, 3]
    sc = scenes[kind]
    for ttype in ("as_is", "crop"):
        x, y, w, h = sc["rect"][ttype]
        exp = _expected(sc, ttype, True, as_u8, order)
        for extra in (0, 1, 2, 3, 4):
            bufs = [sentinel_canvas(w, h, torch.uint8 if as_u8 else torch.int16, extra) for _ in order]
            _run(ctx, sc, kind, ttype, True, as_u8, order, dsts=[b[0] for b in bufs])
            for (view, back), e in zip(bufs, exp):
                assert np.array_equal(view.cpu().numpy(), e) and padding_untouched(back, w, h), (ttype, as_u8, extra)
    host = [np.zeros((h, w, 3), np.uint8 if as_u8 else np.int16) for _ in order]      # host frames in, host canvases out
    import image_stitching_amd as isa
    isa.timelapse_warp_batch(ctx, kind, [s.cpu().numpy() for s in sc["srcs"]], sc["cams"], sc["rois"], sc["scale"], sc["rect"][ttype], sc["gains"], as_u8, host)
    assert all(np.array_equal(a, e) for a, e in zip(host, exp))


def test_timed_entry_writes_what_the_untimed_one_writes(ctx, scenes):
    from image_stitching_amd.timelapse import timelapse_warp_batch_timed
    sc, order = scenes[0], [0, 1, 2, 3]
    got = _run(ctx, sc, 0, "crop", False, True, order)
    dsts = [g.clone().fill_(U8_SENTINEL) for g in got]
    us = timelapse_warp_batch_timed(ctx, 0, sc["srcs"], sc["cams"], sc["rois"], sc["scale"], sc["rect"]["crop"], None, dsts, True, 3)
    assert us > 0 and all(np.array_equal(d.cpu().numpy(), g.cpu().numpy()) for d, g in zip(dsts, got))


# ---------------------------------------------------------------- (c) the error contract
def _raw_call(ctx, sc, kind=0, n=None, scale=None, srcs=None, rois=None, dst_roi=None, gains=None, dsts="fresh", fmt=None, nulls=(), timed=None):
    """mis_timelapse_warp_batch through ctypes with one argument replaced -> (rc, error text, dsts array, prefilled tensors)."""
    import torch
    from image_stitching_amd import _capi as capi
    from image_stitching_amd.stitching import as_image
    m = len(sc["srcs"])
    n = m if n is None else n
    x, y, w, h = sc["rect"]["crop"] if dst_roi is None else dst_roi
    fmt = capi.U8 if fmt is None else fmt
    im = (capi.MisImage * m)(*[as_image(s) for s in (sc["srcs"] if srcs is None else srcs)])
    cw, ch = sc["rect"]["crop"][2:]
    filled = [torch.full((ch, cw, 3), U8_SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(m)]
    if isinstance(dsts, str):
        ds = (capi.MisImage * m)(*([as_image(f) for f in filled] if dsts == "filled" else [capi.MisImage() for _ in range(m)]))
    else:
        ds = (capi.MisImage * m)(*[as_image(d) for d in dsts])
    fp = C.POINTER(C.c_float)
    Ks = np.ascontiguousarray(np.stack([np.asarray(c["K"], np.float32).reshape(9) for c in sc["cams"]]))
    Rs = np.ascontiguousarray(np.stack([np.asarray(c["R"], np.float32).reshape(9) for c in sc["cams"]]))
    rr = (capi.MisRect * m)(*[capi.MisRect(*[int(v) for v in r]) for r in (sc["rois"] if rois is None else rois)])
    dr = capi.MisRect(int(x), int(y), int(w), int(h))
    g = None if gains is None else np.ascontiguousarray(np.asarray(gains, np.float64))
    args = dict(srcs=im, Ks=Ks.ctypes.data_as(fp), Rs=Rs.ctypes.data_as(fp), rois=rr, dst_roi=C.byref(dr), dsts=ds)
    for name in nulls:
        args[name] = None
    head = (ctx.h, int(kind), args["srcs"], int(n), float(sc["scale"] if scale is None else scale), args["Ks"], args["Rs"], args["rois"], args["dst_roi"],
            None if g is None else g.ctypes.data_as(C.POINTER(C.c_double)), args["dsts"], int(fmt))
    if timed is None:
        rc = ctx.lib.mis_timelapse_warp_batch(*head)
    else:
        rc = ctx.lib.mis_timelapse_warp_batch_timed(*head, int(timed[0]), timed[1])
    ctx.synchronize()
    return rc, ctx.lib.mis_last_error(ctx.h).decode(), ds, filled


def test_fused_batch_refusals_write_nothing(ctx, scenes):
    import torch
    from image_stitching_amd import _capi as capi
    sc = scenes[0]
    cw, ch = sc["rect"]["crop"][2:]
    grey = [s if i != 2 else s[:, :, 0].contiguous() for i, s in enumerate(sc["srcs"])]
    empty_roi = [r if i != 1 else (r[0], r[1], 0, r[3]) for i, r in enumerate(sc["rois"])]
    wrong = [torch.full((ch, cw + (1 if i == 3 else 0), 3), U8_SENTINEL, dtype=torch.uint8, device="cuda") for i in range(4)]
    nan_gains = np.ones((4, 3))
    nan_gains[2, 1] = np.nan
    cases = [
        (dict(kind=7), E_UNSUPPORTED, "unknown warp kind 7"), (dict(kind=12), E_UNSUPPORTED, "unknown warp kind 12"), (dict(kind=-1), E_UNSUPPORTED, "unknown"),
        (dict(nulls=("srcs",)), E_INVALID, "null"), (dict(nulls=("Ks",)), E_INVALID, "null"), (dict(nulls=("Rs",)), E_INVALID, "null"),
        (dict(nulls=("rois",)), E_INVALID, "null"), (dict(nulls=("dst_roi",)), E_INVALID, "null"), (dict(nulls=("dsts",)), E_INVALID, "null"),
        (dict(n=0), E_INVALID, "0 frames"), (dict(n=-3), E_INVALID, "-3 frames"), (dict(scale=0.0), E_INVALID, "scale"),
        (dict(dst_roi=(5, 5, 0, 40)), E_INVALID, "empty dst_roi"), (dict(dst_roi=(5, 5, 40, -1)), E_INVALID, "empty dst_roi"),
        (dict(dst_roi=(0, 0, 65536, 32768)), E_INVALID, "too many pixels"), (dict(fmt=capi.F32), E_INVALID, "format"),
        (dict(srcs=grey), E_INVALID, "frame 2: "), (dict(rois=empty_roi), E_INVALID, "frame 1: empty roi"),
        (dict(dsts=wrong), E_INVALID, "frame 3: "), (dict(gains=nan_gains), E_INVALID, "frame 2: gain 1"),
        (dict(timed=(0, C.byref(C.c_float()))), E_INVALID, "repeats"), (dict(timed=(2, None)), E_INVALID, "avg_us"),
    ]
    for kw, code, text in cases:
        for mode in ("filled", "fresh"):
            if "dsts" in kw and mode == "fresh":
                continue
            rc, err, ds, filled = _raw_call(ctx, sc, **dict(dict(dsts=mode), **kw))
            assert rc == code and text in err, (kw, mode, rc, err)
            if mode == "filled" and "dsts" not in kw:
                assert all(bool((f == U8_SENTINEL).all()) for f in filled), (kw, "a refused call wrote to an output")
            if mode == "fresh":
                assert all(d.data is None for d in ds), (kw, "a refused call allocated an output")
        if "dsts" in kw:
            assert all(bool((d == U8_SENTINEL).all()) for d in kw["dsts"]), kw
    # the context is still usable, and a library-allocated canvas comes back with the canvas's geometry
    rc, err, ds, _ = _raw_call(ctx, sc)
    assert rc == 0 and all(d.data and (d.width, d.height, d.channels, d.dtype) == (cw, ch, 3, capi.U8) for d in ds)
    for d in ds:
        assert ctx.lib.mis_image_free(ctx.h, C.byref(d)) == 0


def test_timelapser_refusals(ctx):
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd import _capi as capi
    from image_stitching_amd.stitching import as_image
    h = C.c_void_p()
    for bad in (2, -1):
        assert ctx.lib.mis_timelapser_create(ctx.h, bad, C.byref(h)) == E_INVALID and "timelapser type" in ctx.lib.mis_last_error(ctx.h).decode()
    with pytest.raises(ValueError, match="nonsense"):
        isa.Timelapser(ctx, "nonsense")
    t = isa.Timelapser(ctx, "crop")
    img = torch.zeros((4, 4, 3), dtype=torch.int16, device="cuda")
    with pytest.raises(isa.MisError) as e:      # before initialize
        t.dst_roi()
    assert e.value.code == E_STATE
    i, d = as_image(img), capi.MisImage()
    assert ctx.lib.mis_timelapser_process(t.h, C.byref(i), capi.MisPoint(0, 0), C.byref(d)) == E_STATE and d.data is None
    with pytest.raises(ValueError, match=r"Rect\(tl = \(50, 0\), br = \(10, 10\)\) is empty"):     # disjoint frames
        t.initialize([(0, 0), (50, 0)], [(10, 10), (10, 10)])
    pts = (capi.MisPoint * 2)(capi.MisPoint(0, 0), capi.MisPoint(50, 0))
    szs = (capi.MisSize * 2)(capi.MisSize(10, 10), capi.MisSize(10, 10))
    assert ctx.lib.mis_timelapser_initialize(t.h, pts, szs, 2) == E_INVALID
    assert "tl = (50, 0), br = (10, 10)" in ctx.lib.mis_last_error(ctx.h).decode()
    t.initialize([(0, 0), (5, 5)], [(10, 10), (10, 10)])
    assert t.dst_roi() == (5, 5, 5, 5)
    # an output of another geometry, a source of another type: refused, nothing written
    wrong = torch.full((5, 6, 3), S16_SENTINEL, dtype=torch.int16, device="cuda")
    for src, dst in ((img, wrong), (img.to(torch.uint8), torch.full((5, 5, 3), S16_SENTINEL, dtype=torch.int16, device="cuda"))):
        i, d = as_image(src), as_image(dst)
        assert ctx.lib.mis_timelapser_process(t.h, C.byref(i), capi.MisPoint(0, 0), C.byref(d)) == E_INVALID
        ctx.synchronize()
        assert bool((dst == S16_SENTINEL).all())
