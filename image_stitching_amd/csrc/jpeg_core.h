// jpeg_core.h -- the per-block and per-pixel arithmetic of the JPEG decode (jpeg.hip), host and device from one source:
// dequantisation + the islow inverse DCT of libjpeg's jidctint.c, the "fancy" (triangle) chroma upsampling of jdsample.c and the
// fixed-point YCbCr -> RGB of jdcolor.c, all as libjpeg-turbo runs them by default (JDCT_ISLOW, do_fancy_upsampling), bit for bit.
// No device-only construct: tests/harness/jpeg_host_harness.cpp compiles it with the host compiler alone.
//
// The IDCT in 32 bits.  libjpeg computes in `long`; here every sum and product is taken in uint32_t, i.e. modulo 2^32, and read
// as int32_t only where a value is descaled.  Ring arithmetic is exact modulo 2^32, so a descaled value is right whenever its true
// value fits an int32_t, whatever its partial sums did.  With x[u][v] the dequantised block, a(0) = 1, a(k) = 1.3871 (>= sqrt(2)
// cos(pi / 16), the largest gain of a basis function in one pass) and
//      S = sum over u, v of a(u) a(v) |x[u][v]|,
// the value descaled by the column pass is at most 8192 S and that of the row pass at most 8192 (4 S + 5.4) + 2^17 (5.4: the
// column pass's rounding, half a unit per term, through the row pass's gains).  Both fit when S <= JPEG_IDCT_S_MAX = 65000 (the
// limit is 65530; the rounding of the twelve FIX constants moves a gain by less than 0.0005, far inside that margin).  The
// entropy decoder (jpeg_host.h) accumulates S per block from integer weights that round a(u) a(v) up and refuses a stream with a
// block beyond the bound.  A block an encoder made from 8-bit samples has sum x^2 <= 64 * 128^2 before quantisation, hence
// sum |x| <= 8192, plus at most half a quantisation step (<= 127.5) per coefficient: S <= 1.924 (8192 + 64 * 127.5) < 31500.
//
// The range limit.  libjpeg indexes a table with (value & 1023) that wraps for |value| >= 512; no block inside the bound above
// made by an encoder reaches that, and this code clamps instead: clamp(value + 128, 0, 255).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#define JPEG_UNROLL _Pragma("unroll")
#else
#define JPEG_HD inline
#define JPEG_UNROLL
#endif

constexpr int JPEG_IDCT_S_MAX = 65000;
// a(u) a(v) in units of 1 / 1024, rounded up: 1, 1.3871, 1.3871^2
constexpr int JPEG_S_W00 = 1024, JPEG_S_W01 = 1421, JPEG_S_W11 = 1971;

// upsampling rules of one chroma plane (jdsample.c): the sampling layout and libjpeg's "downsampled width <= 2 replicates" rule
enum { JPEG_UP_COPY = 0, JPEG_UP_H2V1 = 1, JPEG_UP_H2V2 = 2, JPEG_UP_H2V1_REPLICATE = 3, JPEG_UP_H2V2_REPLICATE = 4 };

// FIX(x) = (int)(x * 8192 + 0.5)
constexpr uint32_t JF_0_298631336 = 2446, JF_0_390180644 = 3196, JF_0_541196100 = 4433, JF_0_765366865 = 6270, JF_0_899976223 = 7373,
                   JF_1_175875602 = 9633, JF_1_501321110 = 12299, JF_1_847759065 = 15137, JF_1_961570560 = 16069, JF_2_053119869 = 16819,
                   JF_2_562915447 = 20995, JF_3_072711026 = 25172;

JPEG_HD uint32_t jpeg_descale(uint32_t v, int n) { return (uint32_t)((int32_t)(v + (1u << (n - 1))) >> n); }

// one 1-D pass of jidctint.c over eight values (CONST_BITS = 13), descaled by n with rounding; in and out may be the same array
JPEG_HD void jpeg_idct_1d(const uint32_t in[8], uint32_t out[8], int n) {
    uint32_t z2 = in[2], z3 = in[6];
    uint32_t z1 = (z2 + z3) * JF_0_541196100;
    uint32_t tmp2 = z1 - z3 * JF_1_847759065;
    uint32_t tmp3 = z1 + z2 * JF_0_765366865;
    uint32_t tmp0 = (in[0] + in[4]) << 13;
    uint32_t tmp1 = (in[0] - in[4]) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    uint32_t z4 = tmp1 + tmp3;
    const uint32_t z5 = (z3 + z4) * JF_1_175875602;
    tmp0 *= JF_0_298631336; tmp1 *= JF_2_053119869; tmp2 *= JF_3_072711026; tmp3 *= JF_1_501321110;
    z1 *= 0u - JF_0_899976223; z2 *= 0u - JF_2_562915447; z3 *= 0u - JF_1_961570560; z4 *= 0u - JF_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    out[0] = jpeg_descale(tmp10 + tmp3, n); out[7] = jpeg_descale(tmp10 - tmp3, n);
    out[1] = jpeg_descale(tmp11 + tmp2, n); out[6] = jpeg_descale(tmp11 - tmp2, n);
    out[2] = jpeg_descale(tmp12 + tmp1, n); out[5] = jpeg_descale(tmp12 - tmp1, n);
    out[3] = jpeg_descale(tmp13 + tmp0, n); out[4] = jpeg_descale(tmp13 - tmp0, n);
}

JPEG_HD uint32_t jpeg_clamp255(int32_t v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// One block: ws holds the 64 dequantised coefficients in natural order (ws[8 u + v]) on entry; on return row[y] holds the eight
// samples of row y, sample x in byte x (two little-endian dwords).  Column pass descaled by 11, row pass by 18, + 128, clamped.
JPEG_HD void jpeg_idct_block(uint32_t ws[64], uint32_t row[8][2]) {
    JPEG_UNROLL
    for (int v = 0; v < 8; v++) {
        uint32_t col[8];
        JPEG_UNROLL
        for (int u = 0; u < 8; u++) col[u] = ws[8 * u + v];
        jpeg_idct_1d(col, col, 11);
        JPEG_UNROLL
        for (int u = 0; u < 8; u++) ws[8 * u + v] = col[u];
    }
    JPEG_UNROLL
    for (int y = 0; y < 8; y++) {
        uint32_t r[8];
        jpeg_idct_1d(ws + 8 * y, r, 18);
        JPEG_UNROLL
        for (int x = 0; x < 8; x++) r[x] = jpeg_clamp255((int32_t)r[x] + 128);
        row[y][0] = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
        row[y][1] = r[4] | (r[5] << 8) | (r[6] << 16) | (r[7] << 24);
    }
}

// The chroma sample of output pixel (x, y) from a component plane p (stride in bytes) whose real -- not padded -- size is cw x ch.
// The caller guarantees x < 2 cw (or cw for COPY) and y < 2 ch (or ch) as the layout implies: x < width, y < height.
JPEG_HD int jpeg_upsample_at(const uint8_t* p, size_t stride, int cw, int ch, int rule, int x, int y) {
    if (rule == JPEG_UP_COPY) return p[(size_t)y * stride + x];
    if (rule == JPEG_UP_H2V1_REPLICATE) return p[(size_t)y * stride + (x >> 1)];
    if (rule == JPEG_UP_H2V2_REPLICATE) return p[(size_t)(y >> 1) * stride + (x >> 1)];
    const int c = x >> 1, last = cw - 1;
    const int other = (x & 1) ? (c < last ? c + 1 : last) : (c > 0 ? c - 1 : 0);      // the neighbour column the triangle leans to
    if (rule == JPEG_UP_H2V1) {
        const uint8_t* r = p + (size_t)y * stride;
        if (x == 0 || x == 2 * cw - 1) return r[c];
        return (3 * r[c] + r[other] + ((x & 1) ? 2 : 1)) >> 2;
    }
    // h2v2: colsum = 3 * near row + far row, the far row clamped at the top and at the real bottom
    const int rn = y >> 1, rf = (y & 1) ? (rn < ch - 1 ? rn + 1 : ch - 1) : (rn > 0 ? rn - 1 : 0);
    const uint8_t *near = p + (size_t)rn * stride, *far = p + (size_t)rf * stride;
    const int cs = 3 * near[c] + far[c];
    if (x == 0) return (4 * cs + 8) >> 4;
    if (x == 2 * cw - 1) return (4 * cs + 7) >> 4;
    const int co = 3 * near[other] + far[other];
    return (3 * cs + co + ((x & 1) ? 7 : 8)) >> 4;
}

JPEG_HD uint32_t jpeg_load4(const uint8_t* p) {      // four samples at a 4-byte aligned address, sample k in byte k
    uint32_t w;
    __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
    return w;
}

// The h2v2 rule for a tile of 8 x 2 output pixels, x0 a multiple of 8 and y0 even, x0 < 2 cw, y0 < 2 ch: what jpeg_upsample_at gives
// for every pixel of the tile that lies inside 2 cw x 2 ch (the others get values nobody stores), from 9 loads per plane instead
// of 64: the near row and the two far rows as one dword of columns x0 / 2 .. x0 / 2 + 3 and the two columns beside it.  The plane's
// rows are 4-byte aligned and padded to whole blocks, so the dword lies inside its row; its samples past column cw - 1 only ever
// meet pixel 2 cw - 1, whose rule does not look at them.
JPEG_HD void jpeg_h2v2_tile(const uint8_t* p, size_t stride, int cw, int ch, int x0, int y0, int out[2][8]) {
    const int c0 = x0 >> 1, r = y0 >> 1, last = cw - 1;
    const int rows[3] = {r > 0 ? r - 1 : 0, r, r < ch - 1 ? r + 1 : ch - 1};
    int v[3][6];
    JPEG_UNROLL
    for (int i = 0; i < 3; i++) {
        const uint8_t* row = p + (size_t)rows[i] * stride;
        const uint32_t w = jpeg_load4(row + c0);
        v[i][0] = row[c0 > 0 ? c0 - 1 : 0];
        JPEG_UNROLL
        for (int k = 0; k < 4; k++) v[i][1 + k] = (int)((w >> (8 * k)) & 255u);
        v[i][5] = row[c0 + 4 <= last ? c0 + 4 : last];
    }
    JPEG_UNROLL
    for (int j = 0; j < 2; j++) {
        int cs[6];
        JPEG_UNROLL
        for (int m = 0; m < 6; m++) cs[m] = 3 * v[1][m] + v[2 * j][m];
        JPEG_UNROLL
        for (int k = 0; k < 8; k++) {
            const int x = x0 + k, c = 1 + (k >> 1);
            int val = (k & 1) ? (3 * cs[c] + cs[c + 1] + 7) >> 4 : (3 * cs[c] + cs[c - 1] + 8) >> 4;
            if (x == 0) val = (4 * cs[c] + 8) >> 4;
            if (x == 2 * cw - 1) val = (4 * cs[c] + 7) >> 4;
            out[j][k] = val;
        }
    }
}

// jdcolor.c: F(x) = (int)(x * 65536 + 0.5); cb, cr are the samples (0 .. 255), the result is B | G << 8 | R << 16
JPEG_HD uint32_t jpeg_ycc_to_bgr(int y, int cb, int cr) {
    cb -= 128; cr -= 128;
    const int r = y + ((91881 * cr + 32768) >> 16);
    const int b = y + ((116130 * cb + 32768) >> 16);
    const int g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    return jpeg_clamp255(b) | (jpeg_clamp255(g) << 8) | (jpeg_clamp255(r) << 16);
}
