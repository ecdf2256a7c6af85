"""Independent numpy restatement of a baseline JPEG encode with libjpeg-turbo's defaults (JDCT_ISLOW, standard Huffman tables,
JFIF header), the reference of mis_jpeg_encode.  Written from the arithmetic alone: fixed-point RGB -> YCbCr, libjpeg's edge
replication and box downsampling, the int64 islow forward DCT, quantisation by rounded division, Annex K tables, and a bit-by-bit
entropy coder.  The entropy coder is a Python loop: meant for small images (the fixtures under tests/golden/jpeg_enc and one
small panorama).

    tables(quality)                                    -> [uint16 (64,) luminance, chrominance], natural order
    geometry(w, h, sampling)                           -> dict(hmax, vmax, mx, my, wb, hb): wb, hb the real blocks per component
    planes(rgb, quality, sampling)                     -> [int16 (blocks_y, blocks_x, 64) per component], natural order, dummy
                                                          blocks included (the layout of refimpl_jpeg.coefficients)
    entropy(planes, w, h, quality, sampling, restart)  -> bytes, the whole file
    encode(rgb, quality=95, sampling="420", restart_interval=0) -> bytes"""
import numpy as np

from refimpl_jpeg import ZIGZAG

SAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}

# Annex K.1, K.2
STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                     80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                     95, 98, 112, 100, 103, 99])
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                       99, 99, 99] + [99] * 32)
# Annex K.3 - K.6: code counts per length 1 .. 16, then the symbols
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125],
           [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36,
            51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73,
            74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132,
            133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178,
            179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217,
            218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119],
             [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240,
              21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70,
              71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121,
              122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167,
              168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213,
              214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])


def _fix(x, bits):
    return int(x * (1 << bits) + 0.5)


def tables(quality):
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return [np.clip((std * scale + 50) // 100, 1, 255).astype(np.uint16) for std in (STD_LUMA, STD_CHROMA)]


def geometry(w, h, sampling):
    hmax, vmax = SAMPLING[sampling]
    mx, my = -(-w // (8 * hmax)), -(-h // (8 * vmax))
    hv = [(hmax, vmax), (1, 1), (1, 1)]
    ceil = lambda a, b: -(-a // b)
    wb = [ceil(ceil(w * hc, hmax), 8) for hc, _ in hv]
    hb = [ceil(ceil(h * vc, vmax), 8) for _, vc in hv]
    return dict(hmax=hmax, vmax=vmax, mx=mx, my=my, hv=hv, wb=wb, hb=hb)


def _ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (_fix(.299, 16) * r + _fix(.587, 16) * g + _fix(.114, 16) * b + 32768) >> 16
    cb = (-_fix(.16874, 16) * r - _fix(.33126, 16) * g + _fix(.5, 16) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5, 16) * r - _fix(.41869, 16) * g - _fix(.08131, 16) * b + (128 << 16) + 32767) >> 16
    return [y, cb, cr]


def _edge(p, rows, cols):
    """p with its last row / column replicated out to rows x cols."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def component_samples(rgb, sampling):
    """The three sample planes the forward DCT reads: real block columns only (wb * 8), all my * v * 8 rows."""
    h, w = rgb.shape[:2]
    g = geometry(w, h, sampling)
    out = []
    for c, full in enumerate(_ycc(rgb)):
        hc, vc = g["hv"][c]
        fx, fy = g["hmax"] // hc, g["vmax"] // vc
        p = _edge(full, -(-h // g["vmax"]) * g["vmax"], g["wb"][c] * 8 * fx)
        if (fx, fy) == (2, 2):
            bias = np.tile([1, 2], p.shape[1] // 4 + 1)[:p.shape[1] // 2]
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        elif (fx, fy) == (2, 1):
            bias = np.tile([0, 1], p.shape[1] // 4 + 1)[:p.shape[1] // 2]
            p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
        out.append(_edge(p, g["my"] * vc * 8, p.shape[1]))
    return g, out


F = {k: _fix(v, 13) for k, v in dict(c0298=0.298631336, c0390=0.390180644, c0541=0.541196100, c0765=0.765366865, c0899=0.899976223,
                                     c1175=1.175875602, c1501=1.501321110, c1847=1.847759065, c1961=1.961570560, c2053=2.053119869,
                                     c2562=2.562915447, c3072=3.072711026).items()}


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(x, first):
    """One 1-D pass of jfdctint.c along the last axis of x (..., 8), int64."""
    d = [x[..., k] for k in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = (tmp10 + tmp11) << 2, (tmp10 - tmp11) << 2
    else:
        o[0], o[4] = _descale(tmp10 + tmp11, 2), _descale(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * F["c0541"]
    o[2] = _descale(z1 + tmp13 * F["c0765"], n)
    o[6] = _descale(z1 - tmp12 * F["c1847"], n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F["c1175"]
    t4, t5, t6, t7 = tmp4 * F["c0298"], tmp5 * F["c2053"], tmp6 * F["c3072"], tmp7 * F["c1501"]
    z1, z2 = -z1 * F["c0899"], -z2 * F["c2562"]
    z3, z4 = -z3 * F["c1961"] + z5, -z4 * F["c0390"] + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(samples, table):
    """uint plane (by * 8, bx * 8) -> int16 (by, bx, 64), natural order."""
    by, bx = samples.shape[0] // 8, samples.shape[1] // 8
    x = samples.astype(np.int64).reshape(by, 8, bx, 8).transpose(0, 2, 1, 3) - 128      # [row][col]
    x = _fdct_pass(x, True)                                                             # along each row
    x = np.swapaxes(_fdct_pass(np.swapaxes(x, -1, -2), False), -1, -2)                  # along each column
    qv = table.astype(np.int64).reshape(8, 8) << 3
    q = (np.abs(x) + (qv >> 1)) // qv
    return (np.sign(x) * q).astype(np.int16).reshape(by, bx, 64)


def planes(rgb, quality=95, sampling="420"):
    rgb = np.asarray(rgb)
    g, samples = component_samples(rgb, sampling)
    qt = tables(quality)
    out = []
    for c, s in enumerate(samples):
        hc, vc = g["hv"][c]
        real = fdct_quant(s, qt[0 if c == 0 else 1])
        plane = np.zeros((g["my"] * vc, g["mx"] * hc, 64), np.int16)
        plane[:, :real.shape[1]] = real
        # dummy blocks: no AC, the DC of the block before them in the MCU's scan order
        for my in range(g["my"]):
            for mx in range(g["mx"]):
                prev = None
                for j in range(my * vc, my * vc + vc):
                    for i in range(mx * hc, mx * hc + hc):
                        if i >= g["wb"][c] or j >= g["hb"][c]:
                            plane[j, i] = 0
                            plane[j, i, 0] = prev
                        prev = plane[j, i, 0]
        out.append(plane)
    return out


def _codes(counts, symbols):
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


def _segment(marker, payload):
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)


def headers(w, h, quality, sampling, restart_interval):
    hmax, vmax = SAMPLING[sampling]
    qt = tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate(qt):
        out += _segment(0xDB, bytes([i]) + bytes(int(v) for v in t[ZIGZAG]))
    out += _segment(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, hmax * 16 + vmax, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (counts, syms) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(counts) + bytes(syms))
    if restart_interval:
        out += _segment(0xDD, restart_interval.to_bytes(2, "big"))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0]))


class _Writer:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def entropy(coef, w, h, quality=95, sampling="420", restart_interval=0):
    g = geometry(w, h, sampling)
    dc = [_codes(*DC_LUMA), _codes(*DC_CHROMA)]
    ac = [_codes(*AC_LUMA), _codes(*AC_CHROMA)]
    wr = _Writer()
    pred = [0, 0, 0]
    zz = [np.asarray(p).reshape(p.shape[0], p.shape[1], 64)[:, :, ZIGZAG].astype(np.int64) for p in coef]
    count = rst = 0
    for my in range(g["my"]):
        for mx in range(g["mx"]):
            if restart_interval and count == restart_interval:
                wr.flush()
                wr.out += bytes([0xFF, 0xD0 + rst])
                rst = (rst + 1) & 7
                pred = [0, 0, 0]
                count = 0
            count += 1
            for c in range(3):
                hc, vc = g["hv"][c]
                t = 0 if c == 0 else 1
                for j in range(my * vc, my * vc + vc):
                    for i in range(mx * hc, mx * hc + hc):
                        blk = zz[c][j, i]
                        d = int(blk[0]) - pred[c]
                        pred[c] = int(blk[0])
                        cat = abs(d).bit_length()
                        if cat > 11:
                            raise ValueError("DC difference out of range")
                        wr.put(*dc[t][cat])
                        if cat:
                            wr.put(d if d >= 0 else d - 1, cat)
                        run = 0
                        nz = np.nonzero(blk[1:])[0] + 1
                        last = 0
                        for k in nz:
                            run = int(k) - last - 1
                            last = int(k)
                            while run > 15:
                                wr.put(*ac[t][0xF0])
                                run -= 16
                            v = int(blk[k])
                            cat = abs(v).bit_length()
                            if cat > 10:
                                raise ValueError("AC coefficient out of range")
                            wr.put(*ac[t][(run << 4) | cat])
                            wr.put(v if v >= 0 else v - 1, cat)
                        if last != 63:
                            wr.put(*ac[t][0x00])
    wr.flush()
    return headers(w, h, quality, sampling, restart_interval) + bytes(wr.out) + b"\xff\xd9"


def encode(rgb, quality=95, sampling="420", restart_interval=0):
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    return entropy(planes(rgb, quality, sampling), w, h, quality, sampling, restart_interval)
