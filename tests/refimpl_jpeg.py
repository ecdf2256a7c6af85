"""Independent numpy restatement of a baseline JPEG decode with libjpeg-turbo's defaults (JDCT_ISLOW, fancy upsampling), the
reference of mis_jpeg_decode.  Written from the arithmetic alone: marker parser, Huffman decode, int64 islow IDCT, triangle
upsampling, fixed-point YCbCr -> RGB.  It is slow (the Huffman decode is a Python loop) and is meant for the small fixtures
under tests/golden/jpeg.

    info(data)                -> dict(width, height, components, h, v, restart_interval)
    coefficients(data)        -> (info, [int16 (blocks_y, blocks_x, 64) per component, natural order], [uint16 (64,) tables])
    decode(data)              -> uint8 (H, W, 3) RGB, or (H, W) for a one-component file

Errors: Unsupported for what the library refuses by name (progressive, CMYK, ...), Invalid for a broken stream."""
import numpy as np


class Unsupported(Exception):
    pass


class Invalid(Exception):
    pass


ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])


def _fix(x, bits):
    return int(x * (1 << bits) + 0.5)


class _Huff:
    def __init__(self, counts, symbols):
        self.lookup = {}
        code = 0
        k = 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                self.lookup[(length, code)] = symbols[k]
                code += 1
                k += 1
            if code > (1 << length):
                raise Invalid("over-subscribed Huffman table")
            code <<= 1


class _Bits:
    """Bit reader over one entropy-coded segment (no markers inside): FF 00 is a stuffed FF."""

    def __init__(self, seg):
        out = bytearray()
        i = 0
        n = len(seg)
        while i < n:
            b = seg[i]
            if b == 0xFF:
                if i + 1 < n and seg[i + 1] == 0x00:
                    out.append(0xFF)
                    i += 2
                    continue
                break       # a marker or a lone FF: the segment's data ends here
            out.append(b)
            i += 1
        self.data = bytes(out)
        self.pos = 0        # in bits

    def bit(self):
        byte = self.pos >> 3
        if byte >= len(self.data):
            raise Invalid("entropy-coded data ends inside a symbol")
        v = (self.data[byte] >> (7 - (self.pos & 7))) & 1
        self.pos += 1
        return v

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.lookup.get((length, code))
            if s is not None:
                return s
        raise Invalid("Huffman code not in the table")


def _extend(v, s):
    return v if v >= (1 << (s - 1)) else v - (1 << s) + 1


def _parse(data):
    data = bytes(data)
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        raise Invalid("no SOI")
    pos = 2
    qt, hdc, hac = {}, {}, {}
    frame = None
    dri = 0
    while True:
        if pos >= n:
            raise Invalid("stream ends before SOS")
        if data[pos] != 0xFF:
            raise Invalid("marker expected")
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos >= n:
            raise Invalid("stream ends inside a marker")
        m = data[pos]
        pos += 1
        if m == 0xD8 or m == 0x01 or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9:
            raise Invalid("EOI before SOS")
        if pos + 2 > n:
            raise Invalid("truncated segment length")
        length = (data[pos] << 8) | data[pos + 1]
        if length < 2 or pos + length > n:
            raise Invalid("truncated segment")
        seg = data[pos + 2:pos + length]
        pos += length
        if m == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq != 0:
                    raise Unsupported("16-bit quantisation table")
                if tq > 3 or i + 65 > len(seg):
                    raise Invalid("bad DQT")
                t = np.zeros(64, np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[i + 1:i + 65], np.uint8)
                qt[tq] = t
                i += 65
        elif m == 0xC4:
            i = 0
            while i < len(seg):
                if i + 17 > len(seg):
                    raise Invalid("bad DHT")
                tc, th = seg[i] >> 4, seg[i] & 15
                counts = list(seg[i + 1:i + 17])
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or i + 17 + total > len(seg):
                    raise Invalid("bad DHT")
                (hdc if tc == 0 else hac)[th] = _Huff(counts, list(seg[i + 17:i + 17 + total]))
                i += 17 + total
        elif m == 0xC0 or m == 0xC1 or m == 0xC2 or (0xC3 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC)):
            if m == 0xC2:
                raise Unsupported("progressive (SOF2)")
            if m != 0xC0:
                raise Unsupported("SOF%d" % (m - 0xC0))
            if frame is not None:
                raise Invalid("two frame headers")
            if len(seg) < 6:
                raise Invalid("bad SOF")
            prec, h, w, nc = seg[0], (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if prec != 8:
                raise Unsupported("%d-bit precision" % prec)
            if nc == 4:
                raise Unsupported("4 components")
            if nc not in (1, 3):
                raise Unsupported("%d components" % nc)
            if len(seg) != 6 + 3 * nc:
                raise Invalid("bad SOF")
            if w == 0 or h == 0:
                raise Invalid("zero dimension")
            comps = [(seg[6 + 3 * c], seg[7 + 3 * c] >> 4, seg[7 + 3 * c] & 15, seg[8 + 3 * c]) for c in range(nc)]
            if nc == 3:
                lay = [(c[1], c[2]) for c in comps]
                if lay[1] != (1, 1) or lay[2] != (1, 1) or lay[0] not in ((1, 1), (2, 1), (2, 2)):
                    raise Unsupported("sampling layout")
            else:
                if not (1 <= comps[0][1] <= 4 and 1 <= comps[0][2] <= 4):
                    raise Invalid("bad sampling factor")
            frame = dict(width=w, height=h, comps=comps)
        elif m == 0xDD:
            if len(seg) != 2:
                raise Invalid("bad DRI")
            dri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            if frame is None:
                raise Invalid("SOS before SOF")
            nc = len(frame["comps"])
            if len(seg) < 1:
                raise Invalid("bad SOS")
            ns = seg[0]
            if ns != nc:
                raise Unsupported("multi-scan or non-interleaved file")
            if len(seg) != 4 + 2 * ns:
                raise Invalid("bad SOS")
            sel = []
            for c in range(ns):
                if seg[1 + 2 * c] != frame["comps"][c][0]:
                    raise Unsupported("scan component order")
                sel.append((seg[2 + 2 * c] >> 4, seg[2 + 2 * c] & 15))
            if (seg[1 + 2 * ns], seg[2 + 2 * ns], seg[3 + 2 * ns]) != (0, 63, 0):
                raise Unsupported("spectral selection / successive approximation")
            return frame, qt, hdc, hac, dri, sel, pos
        # everything else (APPn, COM, ...) is skipped


def info(data):
    frame = _parse(data)[0]
    dri = _parse(data)[4]
    return dict(width=frame["width"], height=frame["height"], components=len(frame["comps"]),
                h=[c[1] for c in frame["comps"]], v=[c[2] for c in frame["comps"]], restart_interval=dri)


def _geometry(frame):
    comps = frame["comps"]
    if len(comps) == 1:
        hv = [(1, 1)]       # a one-component scan is not interleaved: one block per MCU whatever the factors say
    else:
        hv = [(c[1], c[2]) for c in comps]
    hmax, vmax = max(h for h, _ in hv), max(v for _, v in hv)
    mx = -(-frame["width"] // (8 * hmax))
    my = -(-frame["height"] // (8 * vmax))
    return hv, hmax, vmax, mx, my


def coefficients(data):
    data = bytes(data)
    frame, qt, hdc, hac, dri, sel, pos = _parse(data)
    hv, hmax, vmax, mx, my = _geometry(frame)
    nc = len(hv)
    tables = []
    for c in range(nc):
        tq = frame["comps"][c][3]
        if tq not in qt:
            raise Invalid("missing quantisation table")
        tables.append(qt[tq])
        if sel[c][0] not in hdc or sel[c][1] not in hac:
            raise Invalid("missing Huffman table")
    planes = [np.zeros((my * v, mx * h, 64), np.int16) for h, v in hv]
    total = mx * my
    # split the scan at its markers
    segs = []
    start = pos
    i = pos
    n = len(data)
    end_marker = None
    while i < n:
        if data[i] != 0xFF:
            i += 1
            continue
        j = i
        while j < n and data[j] == 0xFF:
            j += 1
        if j >= n:
            break
        m = data[j]
        if m == 0x00 and j == i + 1:
            i = j + 1
            continue
        segs.append((start, i, m))
        start = j + 1
        i = j + 1
        if not (0xD0 <= m <= 0xD7):
            end_marker = m
            break
    if end_marker is None:
        raise Invalid("stream ends inside the scan")
    if end_marker != 0xD9:
        raise Unsupported("multi-scan or non-interleaved file") if end_marker in (0xDA, 0xC4, 0xDB) else Invalid("marker %02x in scan" % end_marker)
    per = dri if dri else total
    want = -(-total // per)
    if len(segs) != want:
        raise Invalid("restart marker count")
    for k, (a, b, m) in enumerate(segs):
        if k + 1 < len(segs) and m != 0xD0 + (k & 7):
            raise Invalid("wrong restart index")
        rd = _Bits(data[a:b])
        pred = [0] * nc
        for mcu in range(k * per, min((k + 1) * per, total)):
            my_, mx_ = divmod(mcu, mx)
            for c in range(nc):
                h, v = hv[c]
                for by in range(v):
                    for bx in range(h):
                        blk = planes[c][my_ * v + by, mx_ * h + bx]
                        s = rd.symbol(hdc[sel[c][0]])
                        if s > 15:
                            raise Invalid("DC size")
                        diff = _extend(rd.bits(s), s) if s else 0
                        pred[c] += diff
                        if not -32768 <= pred[c] <= 32767:
                            raise Invalid("coefficient out of range")
                        blk[0] = pred[c]
                        kk = 1
                        while kk < 64:
                            rs = rd.symbol(hac[sel[c][1]])
                            r, s = rs >> 4, rs & 15
                            if s == 0:
                                if r == 15:
                                    kk += 16
                                    if kk > 64:
                                        raise Invalid("zero run past coefficient 63")
                                    continue
                                break
                            kk += r
                            if kk > 63:
                                raise Invalid("zero run past coefficient 63")
                            blk[ZIGZAG[kk]] = _extend(rd.bits(s), s)
                            kk += 1
    inf = dict(width=frame["width"], height=frame["height"], components=nc, h=[c[1] for c in frame["comps"]],
               v=[c[2] for c in frame["comps"]], restart_interval=dri)
    return inf, planes, tables


C = {name: _fix(x, 13) for name, x in dict(
    c0298=0.298631336, c0390=0.390180644, c0541=0.541196100, c0765=0.765366865, c0899=0.899976223, c1175=1.175875602,
    c1501=1.501321110, c1847=1.847759065, c1961=1.961570560, c2053=2.053119869, c2562=2.562915447, c3072=3.072711026).items()}


def _pass(x, shift_in, descale):
    """One 1-D pass over the last axis of x (..., 8), int64."""
    z2, z3 = x[..., 2], x[..., 6]
    z1 = (z2 + z3) * C["c0541"]
    tmp2 = z1 - z3 * C["c1847"]
    tmp3 = z1 + z2 * C["c0765"]
    tmp0 = (x[..., 0] + x[..., 4]) << 13
    tmp1 = (x[..., 0] - x[..., 4]) << 13
    t10, t13, t11, t12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * C["c1175"]
    tmp0 = tmp0 * C["c0298"]
    tmp1 = tmp1 * C["c2053"]
    tmp2 = tmp2 * C["c3072"]
    tmp3 = tmp3 * C["c1501"]
    z1 = -z1 * C["c0899"]
    z2 = -z2 * C["c2562"]
    z3 = -z3 * C["c1961"] + z5
    z4 = -z4 * C["c0390"] + z5
    tmp0 = tmp0 + z1 + z3
    tmp1 = tmp1 + z2 + z4
    tmp2 = tmp2 + z2 + z3
    tmp3 = tmp3 + z1 + z4
    out = np.stack([t10 + tmp3, t11 + tmp2, t12 + tmp1, t13 + tmp0, t13 - tmp0, t12 - tmp1, t11 - tmp2, t10 - tmp3], axis=-1)
    return (out + (1 << (descale - 1))) >> descale


def idct_plane(blocks, table):
    """(by, bx, 64) int16 + table -> uint8 plane (by * 8, bx * 8)."""
    by, bx, _ = blocks.shape
    x = blocks.astype(np.int64) * table.astype(np.int64)
    x = x.reshape(by, bx, 8, 8)                            # [row u][col v]
    ws = _pass(np.swapaxes(x, -1, -2), 0, 11)              # columns: the pass runs along u for every v -> [v][y]
    out = _pass(np.swapaxes(ws, -1, -2), 0, 18)            # rows: along v for every y -> [y][x]
    out = np.clip(out + 128, 0, 255).astype(np.uint8)
    return out.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)


def _h2v1(p, cw):
    p = p[:, :cw].astype(np.int64)
    if cw <= 2:
        return np.repeat(p, 2, axis=1)
    out = np.zeros((p.shape[0], 2 * cw), np.int64)
    prev = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    nxt = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out[:, 0::2] = (3 * p + prev + 1) >> 2
    out[:, 1::2] = (3 * p + nxt + 2) >> 2
    out[:, 0] = p[:, 0]
    out[:, -1] = p[:, -1]
    return out


def _h2v2(p, cw, ch):
    p = p[:ch, :cw].astype(np.int64)
    if cw <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    up = np.concatenate([p[:1], p[:-1]], axis=0)
    dn = np.concatenate([p[1:], p[-1:]], axis=0)
    cs = np.zeros((2 * ch, cw), np.int64)
    cs[0::2] = 3 * p + up
    cs[1::2] = 3 * p + dn
    prev = np.concatenate([cs[:, :1], cs[:, :-1]], axis=1)
    nxt = np.concatenate([cs[:, 1:], cs[:, -1:]], axis=1)
    out = np.zeros((2 * ch, 2 * cw), np.int64)
    out[:, 0::2] = (3 * cs + prev + 8) >> 4
    out[:, 1::2] = (3 * cs + nxt + 7) >> 4
    out[:, 0] = (4 * cs[:, 0] + 8) >> 4
    out[:, -1] = (4 * cs[:, -1] + 7) >> 4
    return out


def decode(data):
    inf, planes, tables = coefficients(data)
    w, h = inf["width"], inf["height"]
    pix = [idct_plane(b, t) for b, t in zip(planes, tables)]
    if inf["components"] == 1:
        return pix[0][:h, :w].copy()
    hy, vy = inf["h"][0], inf["v"][0]
    cw, ch = -(-w // hy), -(-h // vy)
    y = pix[0][:h, :w].astype(np.int64)
    chroma = []
    for p in pix[1:]:
        if (hy, vy) == (1, 1):
            u = p.astype(np.int64)
        elif (hy, vy) == (2, 1):
            u = _h2v1(p, cw)
        else:
            u = _h2v2(p, cw, ch)
        chroma.append(u[:h, :w] - 128)
    cb, cr = chroma
    r = y + ((_fix(1.402, 16) * cr + 32768) >> 16)
    b = y + ((_fix(1.772, 16) * cb + 32768) >> 16)
    g = y + ((-_fix(0.34414, 16) * cb - _fix(0.71414, 16) * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)
