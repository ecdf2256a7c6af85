"""The blender oracle (oracle/mo_blend.c) against the numpy reference of tests/refimpl_blend.py over the regimes shared with
test_refimpl_blend_gpu.py: every accumulator level (the Laplacian sums exactly, the weight sums as float32 bits), then the blended
image and mask.  The GPU tests compare the kernels with the same reference; the self-checks here pin the reference's building blocks
to closed forms and brute force."""
import math

import numpy as np
import pytest

import refimpl_blend as rb

MB, FE, NO = rb.BLEND_MULTI_BAND, rb.BLEND_FEATHER, rb.BLEND_NO


# ------------------------------------------------------------------------------------------------ scenes (shared with the GPU file)
def ragged(rng, w, h):
    """0 / 255 mask with ragged borders (a warped frame's shape)."""
    yy, xx = np.mgrid[0:h, 0:w]
    m = (xx >= min(3, w - 1) - (yy // 7) % 4) & (xx < w - (yy // 5) % 3) & (yy >= (xx // 9) % 3) & (yy < h - (xx // 11) % 2)
    return m.astype(np.uint8) * 255


def img8(rng, w, h):
    return rng.integers(0, 256, (h, w, 3)).astype(np.int16)


def imgfull(rng, w, h):
    return rng.integers(-32768, 32768, (h, w, 3)).astype(np.int16)


def scene(btype, frames, bands=0, sharp=0.0):
    return dict(btype=btype, bands=bands, sharp=sharp, frames=frames)


def strip(rng, n, w, h, x_step, y0=0, make_img=img8, make_mask=ragged, jitter=5):
    """n frames of about w x h in a horizontal strip, x_step apart."""
    out = []
    for i in range(n):
        ww, hh = w + int(rng.integers(-jitter, jitter + 1)), h + int(rng.integers(-jitter, jitter + 1))
        out.append((make_img(rng, ww, hh), make_mask(rng, ww, hh), (i * x_step + int(rng.integers(-3, 4)), y0 + int(rng.integers(-4, 5)))))
    return out


def full_mask(rng, w, h):
    return np.full((h, w), 255, np.uint8)


def bytes_mask(rng, w, h):
    return rng.integers(1, 255, (h, w)).astype(np.uint8)


def isolated_mask(rng, w, h):
    m = np.zeros((h, w), np.uint8)
    m[rng.integers(0, h, max(1, w * h // 40)), rng.integers(0, w, max(1, w * h // 40))] = 255
    return m


def checker_mask(rng, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


def tail_scene(l, above):
    """A frame whose tile has exactly FEED_TAIL_PIXELS = 8192 pixels at level l (or one 2^bands column more), bands = l + 2: the
    frame sits 3 * 2^bands from the roi's corner and as far from its far corner (two 1 x 1 frames span the roi), so its tile is
    the frame plus the gap on every side."""
    nb = l + 2
    q = 2 ** nb
    W, H = 2 ** l * 128 + (q if above else 0), 2 ** l * 64
    w, h = W - 6 * q, H - 6 * q
    rng = np.random.default_rng(100 + 2 * l + above)
    frames = [(img8(rng, 1, 1), full_mask(rng, 1, 1), (0, 0)),
              (img8(rng, w, h), ragged(rng, w, h), (3 * q, 3 * q)),
              (img8(rng, 1, 1), full_mask(rng, 1, 1), (W - 1, H - 1))]
    tile = rb.feed_tile((0, 0, W, H), nb, (3 * q, 3 * q), (w, h))
    assert tile[:4] == (0, 0, W, H) and (W >> l) * (H >> l) == 8192 + (H >> l) * (q >> l) * above
    return scene(MB, frames, nb)


def tiny_frames_scene():
    """1 x 1, 1 x 7, 7 x 1 and 5 x 5 frames inside a 301 x 203 panorama at 5 bands: margins of up to 96 + 31 pixels reflect the
    frame many times over (reflect_near off its one-fold path)."""
    rng = np.random.default_rng(5)
    frames = [(img8(rng, 301, 203), ragged(rng, 301, 203), (0, 0))]
    for (w, h), tl in zip([(1, 1), (1, 7), (7, 1), (5, 5), (1, 1)], [(150, 100), (3, 190), (290, 5), (120, 61), (300, 202)]):
        frames.append((img8(rng, w, h), full_mask(rng, w, h), tl))
    return scene(MB, frames, 5)


def content_scene(kind):
    rng = np.random.default_rng({"wide": 7, "one256": 8, "minus1": 9, "const": 10}[kind])
    fr = strip(rng, 3, 120, 90, 70, make_mask=ragged)
    if kind == "wide":
        fr = [(imgfull(rng, f[0].shape[1], f[0].shape[0]), f[1], f[2]) for f in fr]
    elif kind == "one256":
        fr[1][0][40, 50, 1] = 256
    elif kind == "minus1":
        fr[0][0][30, 33, 2] = -1
    else:
        fr = [(np.full(f[0].shape, v, np.int16), full_mask(rng, f[0].shape[1], f[0].shape[0]), f[2]) for f, v in zip(fr, (32767, -32767, 32767))]
    return scene(MB, fr, 4)


def mask_scene(btype, make_mask, seed, bands=4, sharp=0.05):
    rng = np.random.default_rng(seed)
    return scene(btype, strip(rng, 3, 110, 80, 60, make_mask=make_mask), bands, sharp)


def zero_mask_scene(btype):
    rng = np.random.default_rng(12)
    fr = strip(rng, 3, 100, 80, 55)
    fr[1] = (fr[1][0], np.zeros_like(fr[1][1]), fr[1][2])
    return scene(btype, fr, 3, 0.05)


def deep_scene(btype):
    """19 frames over the same pixels: weight sums above 1, 16-bit sums that wrap, two gather groups of a batch."""
    rng = np.random.default_rng(19)
    fr = [(imgfull(rng, 90 + i % 3, 70), bytes_mask(rng, 90 + i % 3, 70) if i % 2 else full_mask(rng, 90 + i % 3, 70), (i % 4, i % 3))
          for i in range(19)]
    return scene(btype, fr, 3, 0.2)


def geometry_scene(kind):
    rng = np.random.default_rng(30 + len(kind))
    if kind == "clamp-every-side":
        fr = [(img8(rng, 61, 47), ragged(rng, 61, 47), (0, 0)), (img8(rng, 70, 45), ragged(rng, 70, 45), (37, 29)),
              (img8(rng, 9, 11), full_mask(rng, 9, 11), (98, 63))]
        return scene(MB, fr, 3)
    if kind == "negative-odd-corners":
        fr = [(img8(rng, 77, 53), ragged(rng, 77, 53), (-37, -13)), (img8(rng, 64, 59), ragged(rng, 64, 59), (5, 3)),
              (img8(rng, 50, 40), ragged(rng, 50, 40), (-11, 27))]
        return scene(MB, fr, 4)
    if kind == "frame-is-panorama":
        return scene(MB, [(img8(rng, 96, 64), ragged(rng, 96, 64), (-5, 7))], 4)
    if kind == "width-multiple":
        return scene(MB, [(img8(rng, 128, 40), ragged(rng, 128, 40), (0, 0)), (img8(rng, 128, 40), ragged(rng, 128, 40), (128, 24))], 3)
    if kind == "one-row":
        return scene(MB, [(img8(rng, 50, 1), full_mask(rng, 50, 1), (0, 0)), (img8(rng, 40, 1), full_mask(rng, 40, 1), (30, 0))], 3)
    if kind == "bands0":
        return scene(MB, strip(rng, 3, 60, 40, 35), 0)
    if kind == "bands1":
        return scene(MB, strip(rng, 3, 60, 40, 35), 1)
    if kind == "bands-cropped":
        return scene(MB, [(img8(rng, 90, 70), ragged(rng, 90, 70), (0, 0))], 9)
    if kind == "max-len-256":
        return scene(MB, [(img8(rng, 150, 40), ragged(rng, 150, 40), (0, 0)), (img8(rng, 150, 33), ragged(rng, 150, 33), (106, 5))], 12)
    if kind == "max-len-257":
        return scene(MB, [(img8(rng, 150, 40), ragged(rng, 150, 40), (0, 0)), (img8(rng, 150, 33), ragged(rng, 150, 33), (107, 5))], 12)
    raise KeyError(kind)


def feather_sharp_scene(sharp):
    rng = np.random.default_rng(40)
    fr = strip(rng, 3, 130, 90, 80)
    fr.append((img8(rng, 60, 50), full_mask(rng, 60, 50), (40, 20)))       # rows without any zero
    return scene(FE, fr, 0, sharp)


def feather_cap_scene():
    """9000 x 40, zeros only in column 0: distances up to 8999 pass the 8192 cap."""
    rng = np.random.default_rng(41)
    m = np.full((40, 9000), 255, np.uint8)
    m[:, 0] = 0
    return scene(FE, [(img8(rng, 9000, 40), m, (0, 0))], 0, 1e-5)


def feather_chunk_scene(w):
    """Zeros only in the last 4096-pixel chunk of a row (its last column on every third row, its first column on row 1); rows 2, 4
    and 5 have no zero at all."""
    rng = np.random.default_rng(w)
    h = 7
    m = np.full((h, w), 255, np.uint8)
    m[::3, w - 1] = 0
    m[1, (w - 1) // 4096 * 4096] = 0
    return scene(FE, [(img8(rng, w, h), m, (0, 0)), (img8(rng, 40, 3), ragged(rng, 40, 3), (w - 40, 4))], 0, 1e-4)


def feather_height_scene(h):
    """Columns whose nearest zero is segments of 32 rows away."""
    rng = np.random.default_rng(200 + h)
    w = 50
    m = np.full((h, w), 255, np.uint8)
    m[0, 7] = 0
    m[h - 1, 40] = 0
    if h > 3:
        m[h // 2, 20:23] = 0
    return scene(FE, [(img8(rng, w, h), m, (0, 0)), (img8(rng, 1, h), full_mask(rng, 1, h), (49, 0))], 0, 1.0 / 37.0)


def plain_scene(make_mask, seed):
    rng = np.random.default_rng(seed)
    return scene(NO, strip(rng, 4, 90, 70, 50, make_mask=make_mask))


# (id, scene builder) -- the regimes of both files
REGIMES = [
    ("geom-clamp-every-side", lambda: geometry_scene("clamp-every-side")),
    ("geom-negative-odd-corners", lambda: geometry_scene("negative-odd-corners")),
    ("geom-frame-is-panorama", lambda: geometry_scene("frame-is-panorama")),
    ("geom-tiny-frames-5bands", tiny_frames_scene),
    ("geom-width-multiple-of-2^bands", lambda: geometry_scene("width-multiple")),
    ("geom-one-row", lambda: geometry_scene("one-row")),
    ("geom-bands0", lambda: geometry_scene("bands0")),
    ("geom-bands1", lambda: geometry_scene("bands1")),
    ("geom-bands9-cropped", lambda: geometry_scene("bands-cropped")),
    ("geom-max-len-256", lambda: geometry_scene("max-len-256")),
    ("geom-max-len-257", lambda: geometry_scene("max-len-257")),
    ("tail-l1-exact", lambda: tail_scene(1, 0)),
    ("tail-l1-above", lambda: tail_scene(1, 1)),
    ("tail-l2-exact", lambda: tail_scene(2, 0)),
    ("tail-l2-above", lambda: tail_scene(2, 1)),
    ("tail-l3-exact", lambda: tail_scene(3, 0)),
    ("tail-l3-above", lambda: tail_scene(3, 1)),
    ("content-full-s16", lambda: content_scene("wide")),
    ("content-one-256", lambda: content_scene("one256")),
    ("content-one-minus1", lambda: content_scene("minus1")),
    ("content-const-32767", lambda: content_scene("const")),
    ("mask-ragged-mb", lambda: mask_scene(MB, ragged, 50)),
    ("mask-all255-mb", lambda: mask_scene(MB, full_mask, 51)),
    ("mask-bytes-mb", lambda: mask_scene(MB, bytes_mask, 52)),
    ("mask-isolated-mb", lambda: mask_scene(MB, isolated_mask, 53, bands=3)),
    ("mask-checker-mb", lambda: mask_scene(MB, checker_mask, 54, bands=2)),
    ("mask-zero-frame-mb", lambda: zero_mask_scene(MB)),
    ("mask-zero-frame-feather", lambda: zero_mask_scene(FE)),
    ("mask-bytes-feather", lambda: mask_scene(FE, bytes_mask, 55)),
    ("mask-isolated-feather", lambda: mask_scene(FE, isolated_mask, 56, sharp=0.3)),
    ("plain-ragged", lambda: plain_scene(ragged, 57)),
    ("plain-bytes", lambda: plain_scene(bytes_mask, 58)),
    ("plain-checker", lambda: plain_scene(checker_mask, 59)),
    ("deep19-mb", lambda: deep_scene(MB)),
    ("deep19-feather", lambda: deep_scene(FE)),
    ("deep19-plain", lambda: deep_scene(NO)),
    ("feather-sharp-1", lambda: feather_sharp_scene(1.0)),
    ("feather-sharp-1/37", lambda: feather_sharp_scene(1.0 / 37.0)),
    ("feather-sharp-4e-4", lambda: feather_sharp_scene(4e-4)),
    ("feather-sharp-1e-5", lambda: feather_sharp_scene(1e-5)),
    ("feather-cap-9000x40", feather_cap_scene),
    ("feather-w4095", lambda: feather_chunk_scene(4095)),
    ("feather-w4096", lambda: feather_chunk_scene(4096)),
    ("feather-w4097", lambda: feather_chunk_scene(4097)),
    ("feather-w8193", lambda: feather_chunk_scene(8193)),
    ("feather-h1", lambda: feather_height_scene(1)),
    ("feather-h31", lambda: feather_height_scene(31)),
    ("feather-h32", lambda: feather_height_scene(32)),
    ("feather-h33", lambda: feather_height_scene(33)),
    ("feather-h65", lambda: feather_height_scene(65)),
]
REGIME_IDS = [r[0] for r in REGIMES]


def reference(sc):
    return rb.blend_frames(sc["btype"], sc["frames"], sc["bands"], sc["sharp"])


def compare_levels(tag, ref, levels):
    """levels: [(lap, wgt)] of the blender under test (wgt None for the plain blender)."""
    assert len(levels) == ref.nb + 1, (tag, "bands", len(levels) - 1, ref.nb)
    for l, ((lap, wgt), (rlap, rwgt)) in enumerate(zip(levels, ref.levels())):
        assert lap.shape == rlap.shape, (tag, "level shape", l)
        bad = np.argwhere(lap != rlap)
        assert not bad.size, (tag, "laplacian level", l, bad[:5].tolist(), lap[tuple(bad[0])], rlap[tuple(bad[0])])
        if wgt is not None:
            bad = np.argwhere(wgt.view(np.uint32) != rwgt.view(np.uint32))
            assert not bad.size, (tag, "weight level", l, bad[:5].tolist(), wgt[tuple(bad[0])], rwgt[tuple(bad[0])])


def compare_result(tag, img, mask, rimg, rmask):
    assert img.shape == rimg.shape and mask.shape == rmask.shape, (tag, img.shape, rimg.shape)
    bad = np.argwhere(mask != rmask)
    assert not bad.size, (tag, "mask", bad[:5].tolist())
    bad = np.argwhere(img != rimg)
    assert not bad.size, (tag, "image", bad[:5].tolist(), img[tuple(bad[0])], rimg[tuple(bad[0])])


# ------------------------------------------------------------------------------------------------ the oracle against the reference
@pytest.mark.parametrize("tag,make", REGIMES, ids=REGIME_IDS)
def test_oracle_matches_reference(oracle_mod, tag, make):
    sc = make()
    ref = reference(sc)
    ob = oracle_mod.Blender(sc["btype"], sc["bands"], sc["sharp"])
    ob.prepare([f[2] for f in sc["frames"]], [(f[1].shape[1], f[1].shape[0]) for f in sc["frames"]])
    for img, mask, tl in sc["frames"]:
        ob.feed(img, mask, tl)
    assert ob.roi()[:4] == ref.roi
    levels = [ob.level(l) for l in range(ob.num_bands + 1)]
    compare_levels(tag, ref, [(lap.copy(), None if sc["btype"] == NO else wgt.copy()) for lap, wgt in levels])
    compare_result(tag, *ob.blend(), *ref.blend())


@pytest.mark.parametrize("w,h,strength", [(40, 40, 5.0), (1280, 1280, 5.0), (640, 2560, 5.0), (80, 80, 5.0), (1279, 1280, 5.0),
                                          (20, 20, 5.0), (19, 20, 5.0), (9000, 2500, 5.0), (7000, 3000, 1.0)])
def test_blend_config_matches_reference(oracle_mod, w, h, strength):
    """The reference program's sizing.  log(blend_width) of a float is logf: at a blend width of exactly 2^k (a 40 x 40, 1280 x
    1280 or 640 x 2560 panorama at strength 5) the band count is k, where a float64 log gives k - 1."""
    for btype in (MB, FE, NO):
        t, nb, sh = oracle_mod.blend_config(btype, strength, w, h)
        rt, rnb, rsh = rb.blend_config(btype, strength, w, h)
        assert (t, nb, np.float32(sh)) == (rt, rnb, np.float32(rsh)), (btype, w, h)
    bw = math.sqrt(w * h) * strength / 100
    if bw > 1 and bw == 2.0 ** round(math.log2(bw)):
        assert rb.blend_config(MB, strength, w, h)[1] == round(math.log2(bw))


# ------------------------------------------------------------------------------------------------ self-checks of the reference
def _closed_reflect(p, n):
    """BORDER_REFLECT index map, closed form (period 2 n)."""
    p = p % (2 * n)
    return p if p < n else 2 * n - 1 - p


def _closed_reflect101(p, n):
    if n == 1:
        return 0
    p = p % (2 * n - 2)
    return p if p < n else 2 * n - 2 - p


def test_padding_folds_like_opencv():
    for n in (1, 2, 3, 7):
        a = np.arange(n)
        for pad in (0, 1, n, 2 * n + 1, 5 * n + 3):
            assert np.pad(a, (pad, pad + 2), mode="symmetric").tolist() == [_closed_reflect(p, n) for p in range(-pad, n + pad + 2)]
        assert rb._pad101(a, 0, 2).tolist() == [_closed_reflect101(p, n) for p in range(-2, n + 2)]


def test_constant_images_survive_pyramids():
    for c in (-32768, -7, 0, 255, 32767):
        g = np.full((8, 6, 3), c, np.int16)
        assert np.all(rb.pyr_down_s16(g) == c) and np.all(rb.pyr_up_s16(g) == c)
        assert np.all(rb.pyr_up_s16(g[:1, :1]) == c)
    for v in (0.0, 1.0, 0.5, 2.0 ** -20):
        assert np.all(rb.pyr_down_f32(np.full((6, 10), v, np.float32)) == np.float32(v))


def test_impulse_responses():
    g = np.zeros((12, 12, 3), np.int16)
    g[6, 4] = 256
    d = rb.pyr_down_s16(g)[:, :, 0]
    assert d[3, 2] == 36 and d[3, 1] == 6 and d[2, 2] == 6 and d[2, 1] == 1 and d.sum() == 36 + 4 * 6 + 4 * 1
    w = np.zeros((12, 12), np.float32)
    w[6, 4] = 1
    assert rb.pyr_down_f32(w)[3, 2] == np.float32(36 / 256)
    c = np.zeros((5, 5, 3), np.int16)
    c[2, 2] = 64
    u = rb.pyr_up_s16(c)[:, :, 0]
    assert u[4, 4] == 36 and u[4, 5] == 24 and u[5, 4] == 24 and u[5, 5] == 16 and u[3, 4] == 24 and u[3, 3] == 16
    # the right / bottom neighbour of the last sample is itself, the left / top one is sample 1
    e = np.zeros((1, 3, 3), np.int16)
    e[0, 2] = 64
    assert rb.pyr_up_s16(e)[0, :, 0].tolist() == [0, 0, 8, 32, 56, 64]
    e = np.zeros((1, 3, 3), np.int16)
    e[0, 1] = 64
    assert rb.pyr_up_s16(e)[0, :, 0].tolist() == [16, 32, 48, 32, 8, 0]


def test_distance_transform_against_brute_force():
    rng = np.random.default_rng(3)
    for _ in range(30):
        h, w = int(rng.integers(1, 12)), int(rng.integers(1, 12))
        m = (rng.random((h, w)) < rng.random()).astype(np.uint8) * 255
        zy, zx = np.nonzero(m == 0)
        yy, xx = np.mgrid[0:h, 0:w]
        if zy.size:
            brute = np.min(np.abs(yy[:, :, None] - zy) + np.abs(xx[:, :, None] - zx), axis=2)
        else:
            brute = np.full((h, w), rb.DIST_CAP)
        assert np.array_equal(rb.l1_distance(m), brute)
        d = rb._l1_distance_separable(m != 0)
        d[d < 0] = rb.DIST_CAP
        assert np.array_equal(np.minimum(d, rb.DIST_CAP), brute)
    m = np.full((3, 9000), 255, np.uint8)
    m[:, 0] = 0
    assert rb.l1_distance(m)[1].tolist()[8190:8195] == [8190, 8191, 8192, 8192, 8192]


def test_feed_tile_invariants():
    for nb in range(9):
        q = 2 ** nb
        for rx, ry in ((0, 0), (-37, 5)):
            for rw0, rh0 in ((1, 1), (300, 7), (513, 260)):
                rw, rh = -(-rw0 // q) * q, -(-rh0 // q) * q
                for fx in sorted({0, min(1, rw0 - 1), rw0 // 3, rw0 - 1}):
                    for fy in sorted({0, rh0 // 2, rh0 - 1}):
                        for fw, fh in ((1, 1), (rw0 - fx, rh0 - fy), (max(1, (rw0 - fx) // 2), 1)):
                            x, y, W, H, (top, left, bottom, right) = rb.feed_tile((rx, ry, rw, rh), nb, (rx + fx, ry + fy), (fw, fh))
                            assert (x - rx) % q == 0 and (y - ry) % q == 0 and W % q == 0 and H % q == 0
                            assert rx <= x and ry <= y and x + W <= rx + rw and y + H <= ry + rh
                            assert min(top, left, bottom, right) >= 0
                            assert max(top, left, bottom, right) <= 3 * q + q
                            assert (top, left) == (ry + fy - y, rx + fx - x) and W == left + fw + right and H == top + fh + bottom
                            # the roi is padded to multiples of 2^bands, so the snapped, rounded-up tile never overshoots it: the
                            # shift-back of MultiBandBlender::feed is never taken inside a blender
                            assert (x, y) == (rx + (max(rx, rx + fx - 3 * q) - rx) // q * q, ry + (max(ry, ry + fy - 3 * q) - ry) // q * q)


def test_regimes_reach_their_edges():
    """The multi-band regimes clamp a tile at each side of the roi, start frames off the 2^bands grid, reflect frames smaller than
    their margins, and put level-l tiles of exactly 8192 pixels (FEED_TAIL_PIXELS) on both sides of l = 1, 2, 3."""
    seen, tails = set(), set()
    for tag, make in REGIMES:
        sc = make()
        if sc["btype"] != MB:
            continue
        b = reference(sc)
        q, (rx, ry, rw, rh) = 2 ** b.nb, b.roi
        for img, m, (fx, fy) in sc["frames"]:
            h, w = m.shape
            x, y, W, H, (top, left, bottom, right) = b.tile((fx, fy), (w, h))
            seen |= {k for k, v in [("left", fx - 3 * q < rx), ("top", fy - 3 * q < ry), ("right", fx + w + 3 * q > rx + rw),
                                    ("bottom", fy + h + 3 * q > ry + rh), ("off-grid", (fx - rx) % q and (fy - ry) % q),
                                    ("folds", min(left, right) > w and min(top, bottom) > h)] if v}
            tails |= {(l, (W >> l) * (H >> l) - 8192 > 0) for l in (1, 2, 3) if 0 <= (W >> l) * (H >> l) - 8192 <= (H >> l) * (q >> l)}
    assert seen == {"left", "top", "right", "bottom", "off-grid", "folds"}
    assert {(l, a) for l in (1, 2, 3) for a in (False, True)} <= tails


def test_fully_masked_frame_round_trips():
    """One frame that is the whole panorama, mask 255: every weight is exactly 1, each level's normalisation truncates by at most 1
    and pyrUp does not grow an error, so the result is within bands + 1 of the frame."""
    rng = np.random.default_rng(4)
    for nb in (0, 2, 4):
        img = imgfull(rng, 64, 48) // 2
        b = rb.blend_frames(MB, [(img, full_mask(rng, 64, 48), (3, -2))], nb)
        assert all(np.all(w == 1) for _, w in b.levels())
        out, m = b.blend()
        assert np.all(m == 255)
        assert np.abs(out.astype(int) - img).max() <= nb + 1
