"""GPU: mis_resize_linear_exact, mis_resize_linear_exact_batch and mis_rotate (csrc/imgops.hip) against the numpy reference of
tests/refimpl_imgops.py, byte for byte, at the smallest shapes at which the kernels branch: the ragged four-pixel group and its
byte stores, a row pair with one row, the second x block of the single kernel, sources too narrow for a dword group, the row-end
guard of the dword loads (pitched views of a parent of random bytes), unaligned bases and strides (the byte path), more than 32
frames in a call, and the table cache's key.  Every destination is a view into a parent filled with a sentinel byte: whatever lies
outside the dw * channels columns and dh rows must be untouched afterwards."""
import ctypes as C
import functools

import numpy as np
import pytest

import refimpl_imgops as rio

pytestmark = pytest.mark.gpu

SENT = 0xA5
KINDS = ("rand", "ramp", "full")


def _mis_image(ptr, w, h, c, stride, device=True):
    from image_stitching_amd import _capi as capi
    im = capi.MisImage()
    im.data, im.width, im.height, im.channels, im.stride, im.dtype, im.mem = ptr, w, h, c, stride, capi.U8, capi.MEM_DEVICE if device else capi.MEM_HOST
    return im


class View:
    """An h x w x c image at byte offset `off` with row stride `stride` inside a parent buffer of its own (16 spare bytes either
    side), on the device or on the host.  fill: an image to hold (the rest of the parent is random bytes), or None: a destination,
    the whole parent the sentinel."""

    def __init__(self, h, w, c, off=0, stride=None, fill=None, device=True, seed=0):
        import torch
        self.h, self.w, self.c, self.off, self.device = h, w, c, 16 + off, device
        self.stride = stride if stride is not None else w * c
        assert self.stride >= w * c
        size = self.off + (h - 1) * self.stride + w * c + 16
        if fill is None:
            self.host = np.full(size, SENT, np.uint8)
        else:
            self.host = np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)
            self._rows(self.host)[:] = np.asarray(fill).reshape(h, w * c)
        # (the device parent is 4-byte aligned and `off` decides the alignment of the view: 16 + off)
        self.dev = torch.from_numpy(self.host).cuda() if device else None
        assert self.dev is None or self.dev.data_ptr() % 4 == 0

    def _rows(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.off:], (self.h, self.w * self.c), (self.stride, 1))

    def image(self):
        base = self.dev.data_ptr() if self.device else self.host.ctypes.data
        return _mis_image(base + self.off, self.w, self.h, self.c, self.stride, self.device)

    def result(self):
        """-> the image the view holds now; asserts that every byte of the parent outside it is the sentinel still"""
        flat = self.dev.cpu().numpy() if self.device else self.host
        img = self._rows(flat).copy()
        rest = flat.copy()
        self._rows(rest)[:] = SENT
        assert (rest == SENT).all(), "bytes outside the destination view were written: %s" % np.flatnonzero(rest != SENT)[:8]
        return img.reshape((self.h, self.w) if self.c == 1 else (self.h, self.w, self.c))


def _resize(ctx, srcs, dsts, dsize=None, fx=0.0, fy=0.0, batch=True):
    """srcs, dsts: lists of View; one batch call, or one single call per frame"""
    from image_stitching_amd import _capi as capi
    n = len(srcs)
    dw, dh = dsize if dsize else (0, 0)
    if batch:
        sa, da = (capi.MisImage * n)(*[s.image() for s in srcs]), (capi.MisImage * n)(*[d.image() for d in dsts])
        ctx.check(ctx.lib.mis_resize_linear_exact_batch(ctx.h, sa, n, dw, dh, float(fx), float(fy), da))
    else:
        for s, d in zip(srcs, dsts):
            si, di = s.image(), d.image()
            ctx.check(ctx.lib.mis_resize_linear_exact(ctx.h, C.byref(si), dw, dh, float(fx), float(fy), C.byref(di)))
    ctx.synchronize()


def _check(tag, srcs_np, dsts, dsize=None, fx=0.0, fy=0.0, wants=None):
    for k, (a, d) in enumerate(zip(srcs_np, dsts)):
        want = wants[k] if wants else rio.resize_linear_exact(a, dsize=dsize, fx=fx, fy=fy)
        got = d.result()
        assert got.shape == want.shape and np.array_equal(got, want), (tag, k, np.argwhere(got != want)[:4])


# ------------------------------------------------------------------------------------------------ the sweep
SRC_PITCH, SRC_ROWS, DST_PITCH, DST_ROWS = 256, 12, 1024, 18      # 64 * 3 <= 256, 9 + 1 <= 12; 257 * 3 <= 1024, 17 < 18


@functools.lru_cache(maxsize=None)
def _sweep_parents():
    """Three source parents of SRC_ROWS x SRC_PITCH bytes (random, ramp, 255): a sweep source is the top-left sw * c bytes of sh
    rows, starting at row 0 (frame 0) or row 1 (frame 1), so what lies beyond a view's row end is the parent's content."""
    return {"rand": rio.image(SRC_ROWS, SRC_PITCH, 1, "rand", seed=77), "ramp": rio.image(SRC_ROWS, SRC_PITCH, 1, "ramp"),
            "full": rio.image(SRC_ROWS, SRC_PITCH, 1, "full")}


def _sweep_source(kind, frame, sw, sh, c):
    a = _sweep_parents()[kind][frame:frame + sh, :sw * c]
    return a if c == 1 else a.reshape(sh, sw, c)


@functools.lru_cache(maxsize=None)
def _sweep_reference(c):
    """the reference of every sweep geometry, frames 0 and 1: computed once, shared by the single and the batched test"""
    return [[rio.resize_linear_exact(_sweep_source(KINDS[k % 3], f, sw, sh, c), dsize=(dw, dh)) for f in (0, 1)]
            for k, (sw, sh, dw, dh) in enumerate(rio.sweep())]


@pytest.mark.parametrize("entry", ["single", "batch"])
@pytest.mark.parametrize("c", [1, 3])
def test_resize_sweep_vs_reference(c, entry):
    """Every geometry of refimpl_imgops.sweep() by size.  Sources: dword-aligned pitched views (stride 256) whose rows end inside
    random bytes; destinations: pitched views (stride 1024) into sentinel parents.  The batched entry takes two frames per call and
    runs on a context of its own, closed at the end: its table cache is grow-only, one device block per geometry."""
    import torch
    import image_stitching_amd as isa
    from image_stitching_amd import _capi as capi
    ctx = isa.Context(0)
    try:
        nf = 2 if entry == "batch" else 1
        parents = {k: torch.from_numpy(v).cuda() for k, v in _sweep_parents().items()}
        out = torch.empty((nf, DST_ROWS, DST_PITCH), dtype=torch.uint8, device="cuda")
        refs = _sweep_reference(c)
        for k, (sw, sh, dw, dh) in enumerate(rio.sweep()):
            src = parents[KINDS[k % 3]]
            out.fill_(SENT)
            si = [_mis_image(src.data_ptr() + f * SRC_PITCH, sw, sh, c, SRC_PITCH) for f in range(nf)]
            di = [_mis_image(out.data_ptr() + f * DST_ROWS * DST_PITCH, dw, dh, c, DST_PITCH) for f in range(nf)]
            if entry == "batch":
                ctx.check(ctx.lib.mis_resize_linear_exact_batch(ctx.h, (capi.MisImage * nf)(*si), nf, dw, dh, 0.0, 0.0, (capi.MisImage * nf)(*di)))
            else:
                ctx.check(ctx.lib.mis_resize_linear_exact(ctx.h, C.byref(si[0]), dw, dh, 0.0, 0.0, C.byref(di[0])))
            ctx.synchronize()
            got = out.cpu().numpy()
            for f in range(nf):
                want = refs[k][f].reshape(dh, dw * c)
                assert np.array_equal(got[f, :dh, :dw * c], want), (sw, sh, dw, dh, f, np.argwhere(got[f, :dh, :dw * c] != want)[:4])
                assert (got[f, dh:] == SENT).all() and (got[f, :dh, dw * c:] == SENT).all(), (sw, sh, dw, dh, f)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ by factor, and the cache key
@pytest.mark.parametrize("c", [1, 3])
def test_resize_by_factor_then_by_size(ctx, c):
    """The by-factor cases through both entries, each followed straight away by a by-size call of the same four sizes (another
    scale, the same sw, sh, dw, dh: the batched entry's table cache must tell them apart) and by the by-factor call again."""
    for h, w, fx, fy in rio.BY_FACTOR:
        imgs = [rio.image(h, w, c, kind, seed=h * w + c) for kind in ("rand", "ramp")]
        dw, dh = rio.geometry(w, h, None, fx, fy)[:2]
        calls = [{"fx": fx, "fy": fy}, {"dsize": (dw, dh)}, {"fx": fx, "fy": fy}]
        wants = [[rio.resize_linear_exact(a, **kw) for a in imgs] for kw in calls[:2]]
        for batch in (True, False):
            for kw, want in zip(calls, wants + wants[:1]):
                srcs = [View(h, w, c, fill=a, seed=3) for a in imgs]
                dsts = [View(dh, dw, c, stride=(dw * c + 3) // 4 * 4) for _ in imgs]
                _resize(ctx, srcs, dsts, batch=batch, **kw)
                _check((h, w, fx, fy, batch, sorted(kw)), imgs, dsts, wants=want)


# ------------------------------------------------------------------------------------------------ pitched views
def _up4(n):
    return (n + 3) // 4 * 4


@pytest.mark.parametrize("c", [1, 3])
def test_resize_pitched_sources_and_destinations(ctx, c):
    """Source views: dword-aligned with a stride that is a multiple of 4 while width * channels is not (the parent's random bytes
    follow each row: the dword path's row-end guard decides which bytes count), at odd byte offsets, and with odd strides (the
    byte path).  Destination views the same four ways (dword stores and the ragged tail, or byte stores), into sentinel parents.
    Both entries, the batched one with two frames."""
    geoms = [(13, 3, 7, 2), (17, 9, 9, 7), (20, 2, 64, 8), (5, 3, 257, 2), (64, 9, 65, 17), (7, 1, 5, 1), (3, 2, 8, 3), (16, 4, 6, 9)]
    for g, (sw, sh, dw, dh) in enumerate(geoms):
        imgs = [rio.image(sh, sw, c, KINDS[(g + f) % 3], seed=10 * g + f) for f in (0, 1)]
        sv = [(0, _up4(sw * c) + 4), (1, _up4(sw * c) + 4), (0, sw * c | 1), (3, (sw * c | 1) + 2)]
        dv = [(0, _up4(dw * c) + 4), (1, _up4(dw * c) + 4), (0, dw * c | 1), (2, _up4(dw * c))]
        for soff, sstride in sv:
            for doff, dstride in dv:
                for batch in (True, False):
                    srcs = [View(sh, sw, c, soff, sstride, fill=a, seed=g) for a in imgs]
                    dsts = [View(dh, dw, c, doff, dstride) for _ in imgs]
                    _resize(ctx, srcs, dsts, dsize=(dw, dh), batch=batch)
                    _check((sw, sh, dw, dh, soff, sstride, doff, dstride, batch), imgs, dsts, dsize=(dw, dh))


@pytest.mark.parametrize("which", ["source", "destination"])
@pytest.mark.parametrize("c", [1, 3])
def test_batch_of_33_with_only_the_last_frame_unaligned(ctx, c, which):
    """Frames 0 .. 31 travel in the first launch and are dword aligned; frame 32, alone in the second launch, is a view at an odd
    offset.  One set of flags serves the call."""
    sw, sh, dw, dh = 20, 5, 13, 4
    imgs = [rio.image(sh, sw, c, "rand", seed=100 + k) for k in range(33)]
    srcs = [View(sh, sw, c, 1 if (which == "source" and k == 32) else 0, _up4(sw * c) + 4, fill=a, seed=k) for k, a in enumerate(imgs)]
    dsts = [View(dh, dw, c, 1 if (which == "destination" and k == 32) else 0, _up4(dw * c) + 4) for k in range(33)]
    _resize(ctx, srcs, dsts, dsize=(dw, dh))
    _check((c, which), imgs, dsts, dsize=(dw, dh))


# ------------------------------------------------------------------------------------------------ batch sizes, host buffers
@pytest.mark.parametrize("c", [1, 3])
def test_batch_sizes_and_host_buffers(ctx, c):
    """1, 31, 32, 33 and 65 distinct frames in one call (at most 32 per launch), on the device; 33 host frames through the batched
    entry and host frames through the single one (both stage host images)."""
    sw, sh, dw, dh = 17, 5, 9, 3
    imgs = [rio.image(sh, sw, c, "rand", seed=500 + k) for k in range(65)]
    for n in (1, 31, 32, 33, 65):
        srcs = [View(sh, sw, c, 0, _up4(sw * c), fill=a, seed=k) for k, a in enumerate(imgs[:n])]
        dsts = [View(dh, dw, c, 0, _up4(dw * c)) for _ in range(n)]
        _resize(ctx, srcs, dsts, fx=dw / sw + 1e-3, fy=dh / sh + 1e-3)
        _check((c, n), imgs[:n], dsts, fx=dw / sw + 1e-3, fy=dh / sh + 1e-3)
    for batch, n in ((True, 33), (False, 3)):
        srcs = [View(sh, sw, c, 1, sw * c + 5, fill=a, seed=k, device=False) for k, a in enumerate(imgs[:n])]
        dsts = [View(dh, dw, c, 3, dw * c + 2, device=False) for _ in range(n)]
        _resize(ctx, srcs, dsts, dsize=(dw, dh), batch=batch)
        _check((c, "host", batch), imgs[:n], dsts, dsize=(dw, dh))


# ------------------------------------------------------------------------------------------------ rotate
def _rotate(ctx, src, dst, code):
    si, di = src.image(), dst.image()
    ctx.check(ctx.lib.mis_rotate(ctx.h, C.byref(si), int(code), C.byref(di)))
    ctx.synchronize()
    return dst.result()


@pytest.mark.parametrize("code", [0, 1, 2])
@pytest.mark.parametrize("c", [1, 3])
def test_rotate_vs_reference(ctx, c, code):
    """Every size of refimpl_imgops.ROTATE_SIZES (one pixel, one row, one column, the 256-thread block boundary, the shape of the
    older test): tight and pitched / odd-offset sources, sentinel-guarded destinations, device and host buffers."""
    for h, w in rio.ROTATE_SIZES:
        a = rio.image(h, w, c, "ramp" if (h + w) % 2 else "rand", seed=h + w + code)
        want = rio.rotate(a, code)
        dh, dw = want.shape[:2]
        for device, soff, sstride, doff, dstride in ((True, 0, w * c, 0, dw * c), (True, 1, w * c + 7, 3, dw * c + 5), (True, 0, _up4(w * c) + 4, 0, _up4(dw * c) + 4),
                                                     (False, 1, w * c + 3, 0, dw * c + 1)):
            got = _rotate(ctx, View(h, w, c, soff, sstride, fill=a, seed=code, device=device), View(dh, dw, c, doff, dstride, device=device), code)
            assert got.shape == want.shape and np.array_equal(got, want), (h, w, c, code, device, soff, sstride)


@pytest.mark.parametrize("c", [1, 3])
def test_rotate_round_trips(ctx, c):
    """90 clockwise then 90 counter-clockwise, and 180 twice, give the input back."""
    for h, w in rio.ROTATE_SIZES:
        a = rio.image(h, w, c, "rand", seed=3 * h + w)
        for first, second in ((0, 2), (2, 0), (1, 1)):
            mid = _rotate(ctx, View(h, w, c, fill=a), View(*rio.rotate(a, first).shape[:2], c), first)
            back = _rotate(ctx, View(mid.shape[0], mid.shape[1], c, fill=mid), View(h, w, c), second)
            assert np.array_equal(back, a), (h, w, first, second)
