// jpeg_enc_core.h -- the per-pixel and per-block arithmetic of the JPEG encode (jpeg_enc.hip) and its geometry, host and device
// from one source: the fixed-point RGB -> YCbCr of jccolor.c, the box downsampling of jcsample.c, the islow forward DCT of
// jfdctint.c and the quantisation of jcdctmgr.c, all as libjpeg-turbo runs them by default -- what cv::imwrite writes
// (image_stitching.cpp:1228), bit for bit.  Integers only.  No device-only construct: tests/harness/jpeg_enc_host_harness.cpp
// compiles it with the host compiler alone.
//
// Ranges.  Samples minus 128 lie in -128 .. 127.  The row pass multiplies sums of at most four of them (|.| <= 512) by constants
// below 2^15 and adds at most four such products: below 2^27.  Its results are at most 8 * 128 * 1.39 * 4 < 5700 in magnitude; the
// column pass forms sums of four (< 22800), products below 22800 * 25172 < 2^30 and sums of three products whose true value is
// bounded by the transform's gain (8 * 5700 * 1.39 * 8192 < 2^30): everything fits an int32_t, as libjpeg's own 32-bit builds rely on.
// A coefficient is at most 64 * 128 * 1.39^2 < 16000 in magnitude (they carry a factor 8, which quantisation by q << 3 removes).
//
// The quantiser divides by qv = q << 3 (8 .. 2040) through a reciprocal: with m = ceil(2^32 / qv) and a = |c| + (qv >> 1) < 2^15,
// m qv = 2^32 + e with 0 <= e < qv, so a m / 2^32 = a / qv + a e / (qv 2^32), and the floor is that of a / qv as long as
// a e < 2^32 -- here a e < 2^15 * 2^11.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_ENC_HD __host__ __device__ __forceinline__
#define JPEG_ENC_UNROLL _Pragma("unroll")
#else
#define JPEG_ENC_HD inline
#define JPEG_ENC_UNROLL
#endif

enum { JPEG_ENC_420 = 0, JPEG_ENC_422 = 1, JPEG_ENC_444 = 2 };      // MIS_JPEG_420, _422, _444

// Geometry of one image (section "Geometry" of the design): component 0 is luma (hmax x vmax blocks per MCU), 1 and 2 chroma (1 x 1).
struct JpegEncGeom {
    int w = 0, h = 0, hmax = 1, vmax = 1;
    int mx = 0, my = 0;             // MCUs
    int bw[3], bh[3];               // each component's plane in blocks: (my v_c) x (mx h_c)
    int wb[3], hb[3];               // the real blocks of it: the others are dummy blocks
    size_t blocks(int c) const { return (size_t)bw[c] * (size_t)bh[c]; }
};

inline JpegEncGeom jpeg_enc_geometry(int w, int h, int sampling) {
    JpegEncGeom g;
    g.w = w; g.h = h;
    g.hmax = sampling == JPEG_ENC_444 ? 1 : 2;
    g.vmax = sampling == JPEG_ENC_420 ? 2 : 1;
    g.mx = (w + 8 * g.hmax - 1) / (8 * g.hmax);
    g.my = (h + 8 * g.vmax - 1) / (8 * g.vmax);
    for (int c = 0; c < 3; c++) {
        const int hc = c ? 1 : g.hmax, vc = c ? 1 : g.vmax;
        g.bw[c] = g.mx * hc; g.bh[c] = g.my * vc;
        g.wb[c] = ((w * hc + g.hmax - 1) / g.hmax + 7) / 8;
        g.hb[c] = ((h * vc + g.vmax - 1) / g.vmax + 7) / 8;
    }
    return g;
}

// Annex K.1 / K.2 in natural order
static const uint8_t JPEG_ENC_STD_Q[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// jpeg_set_quality: table t (0 luminance, 1 chrominance) at quality 1 .. 100, natural order
inline void jpeg_enc_qtable(int quality, int t, uint16_t out[64]) {
    const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int scale = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int k = 0; k < 64; k++) {
        const int v = (JPEG_ENC_STD_Q[t][k] * scale + 50) / 100;
        out[k] = (uint16_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
    }
}

// what the quantiser needs of one table entry: ceil(2^32 / (q << 3)) and (q << 3) >> 1
inline void jpeg_enc_divisor(int q, uint32_t* recip, uint32_t* half) {
    const uint32_t qv = (uint32_t)q << 3;
    *recip = (uint32_t)(((1ull << 32) + qv - 1) / qv);
    *half = qv >> 1;
}

// jccolor.c: FIX(x) = (int)(x * 65536 + 0.5)
JPEG_ENC_HD int jpeg_enc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
JPEG_ENC_HD int jpeg_enc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
JPEG_ENC_HD int jpeg_enc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// FIX(x) = (int)(x * 8192 + 0.5)
constexpr int JE_0_298631336 = 2446, JE_0_390180644 = 3196, JE_0_541196100 = 4433, JE_0_765366865 = 6270, JE_0_899976223 = 7373,
              JE_1_175875602 = 9633, JE_1_501321110 = 12299, JE_1_847759065 = 15137, JE_1_961570560 = 16069, JE_2_053119869 = 16819,
              JE_2_562915447 = 20995, JE_3_072711026 = 25172;

JPEG_ENC_HD int jpeg_enc_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one 1-D pass of jfdctint.c over d[0], d[s], ..., d[7 s]: FIRST the row pass (even pair << 2, the rest descaled by 11), otherwise
// the column pass (descaled by 2 and 15)
template <bool FIRST>
JPEG_ENC_HD void jpeg_fdct_1d(int* d, int s) {
    const int tmp0 = d[0] + d[7 * s], tmp7 = d[0] - d[7 * s], tmp1 = d[s] + d[6 * s], tmp6 = d[s] - d[6 * s];
    const int tmp2 = d[2 * s] + d[5 * s], tmp5 = d[2 * s] - d[5 * s], tmp3 = d[3 * s] + d[4 * s], tmp4 = d[3 * s] - d[4 * s];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int n = FIRST ? 11 : 15;
    if (FIRST) {
        d[0] = (tmp10 + tmp11) * 4;
        d[4 * s] = (tmp10 - tmp11) * 4;
    } else {
        d[0] = jpeg_enc_descale(tmp10 + tmp11, 2);
        d[4 * s] = jpeg_enc_descale(tmp10 - tmp11, 2);
    }
    int z1 = (tmp12 + tmp13) * JE_0_541196100;
    d[2 * s] = jpeg_enc_descale(z1 + tmp13 * JE_0_765366865, n);
    d[6 * s] = jpeg_enc_descale(z1 - tmp12 * JE_1_847759065, n);
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * JE_1_175875602;
    const int t4 = tmp4 * JE_0_298631336, t5 = tmp5 * JE_2_053119869, t6 = tmp6 * JE_3_072711026, t7 = tmp7 * JE_1_501321110;
    z1 *= -JE_0_899976223; z2 *= -JE_2_562915447;
    z3 = z3 * -JE_1_961570560 + z5; z4 = z4 * -JE_0_390180644 + z5;
    d[7 * s] = jpeg_enc_descale(t4 + z1 + z3, n);
    d[5 * s] = jpeg_enc_descale(t5 + z2 + z4, n);
    d[3 * s] = jpeg_enc_descale(t6 + z2 + z3, n);
    d[s] = jpeg_enc_descale(t7 + z1 + z4, n);
}

JPEG_ENC_HD int jpeg_enc_quant(int c, uint32_t recip, uint32_t half) {
    const uint32_t a = (uint32_t)(c < 0 ? -c : c) + half;
    const int q = (int)(((uint64_t)a * recip) >> 32);
    return c < 0 ? -q : q;
}

// One block: x holds the 64 samples (0 .. 255) in natural order on entry, the quantised coefficients on return.
JPEG_ENC_HD void jpeg_fdct_quant_block(int x[64], const uint32_t* recip, const uint32_t* half) {
    JPEG_ENC_UNROLL
    for (int k = 0; k < 64; k++) x[k] -= 128;
    JPEG_ENC_UNROLL
    for (int r = 0; r < 8; r++) jpeg_fdct_1d<true>(x + 8 * r, 1);
    JPEG_ENC_UNROLL
    for (int c = 0; c < 8; c++) jpeg_fdct_1d<false>(x + c, 8);
    JPEG_ENC_UNROLL
    for (int k = 0; k < 64; k++) x[k] = jpeg_enc_quant(x[k], recip[k], half[k]);
}

// The block whose quantised DC a dummy block (i >= wb or j >= hb) of component c repeats: the block before it in the MCU's scan
// order, followed back to a real one.  A dummy row's first block follows the last block of the MCU's row above; a dummy block to
// the right follows its left neighbour.  (Chroma planes have no dummy blocks: wb = mx and hb = my.)
JPEG_ENC_HD void jpeg_enc_dummy_source(int i, int j, int wb, int hb, int hmax, int* si, int* sj) {
    int ii = j >= hb ? (i | (hmax - 1)) : i;
    *si = ii < wb ? ii : wb - 1;
    *sj = j < hb ? j : hb - 1;
}
