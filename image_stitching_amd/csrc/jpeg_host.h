// jpeg_host.h -- the host layer of the JPEG decode (jpeg.hip): marker parser and Huffman decoder of baseline streams, plain C++
// with no device code (tests/harness/jpeg_host_harness.cpp compiles it on its own, also under the address and undefined-behaviour
// sanitizers).  The input is untrusted: every read is checked against the buffer's end and no length field is believed.
//
//   jpeg_parse      headers up to the first SOS -> JpegHeader (geometry, tables); refuses what the library does not decode
//   jpeg_segments   the scan split at its restart markers, the marker count and indices checked, EOI required
//   jpeg_entropy    restart intervals [first, first + count) -> int16 blocks in natural order, 64 per block, each component a
//                   plane of (MCUs_y V) x (MCUs_x H) blocks; intervals are independent, so callers run them in parallel
// A one-component file is a non-interleaved scan: one block per MCU whatever its sampling factors say (libjpeg's rule).
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "jpeg_core.h"

constexpr int JPEG_OK = 0, JPEG_INVALID = -1, JPEG_UNSUPPORTED = -6;      // MIS_OK, MIS_E_INVALID, MIS_E_UNSUPPORTED

struct JpegError {
    int code = JPEG_OK;
    char text[160] = {0};
};

inline int jpeg_fail(JpegError* e, int code, const char* fmt, ...) {
    e->code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(e->text, sizeof(e->text), fmt, ap);
    va_end(ap);
    return code;
}

static const uint8_t JPEG_ZIGZAG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                        41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                        30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct JpegHuff {
    bool present = false;
    uint8_t vals[256];
    int total = 0;
    int32_t maxcode[17];        // largest code of each length, -1: none
    int32_t valoff[17];         // index of a length's first value minus its first code
    uint16_t fast[512];         // the next 9 bits -> length << 8 | value, 0: a longer code
};

struct JpegHeader {
    int width = 0, height = 0, ncomp = 0, restart_interval = 0;
    int file_h[3] = {0, 0, 0}, file_v[3] = {0, 0, 0};      // the sampling factors as written
    int h[3] = {1, 1, 1}, v[3] = {1, 1, 1};                // as decoded (1 x 1 for a one-component file)
    int tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0}, id[3] = {0, 0, 0};
    bool has_q[4] = {false, false, false, false};
    uint16_t q[4][64];                                     // natural order
    JpegHuff dc[4], ac[4];
    size_t scan = 0;                                       // first byte of the entropy-coded data
    int mcux = 0, mcuy = 0;
    int bw[3] = {0, 0, 0}, bh[3] = {0, 0, 0};              // each component's plane in blocks
    int cw = 0, ch = 0, rule = JPEG_UP_COPY;               // the chroma planes' real size and upsampling rule
    uint32_t sw[3][64];                                    // q * a(u) a(v) * 1024 per component: the weights of the IDCT bound S
    size_t blocks(int c) const { return (size_t)bw[c] * (size_t)bh[c]; }
    size_t intervals() const {
        const size_t total = (size_t)mcux * mcuy, per = restart_interval ? (size_t)restart_interval : total;
        return (total + per - 1) / per;
    }
};

struct JpegSegment { size_t begin, end; };      // entropy-coded bytes of one restart interval

inline int jpeg_build_huff(const uint8_t counts[16], const uint8_t* vals, int total, JpegHuff* t, JpegError* e) {
    memset(t->fast, 0, sizeof(t->fast));
    memcpy(t->vals, vals, (size_t)total);
    t->total = total;
    int32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        const int cnt = counts[len - 1];
        t->valoff[len] = k - code;
        if (code + cnt > (1 << len)) return jpeg_fail(e, JPEG_INVALID, "jpeg: over-subscribed Huffman table");
        for (int i = 0; i < cnt; i++, k++, code++)
            if (len <= 9)
                for (int f = 0; f < (1 << (9 - len)); f++) t->fast[(code << (9 - len)) | f] = (uint16_t)((len << 8) | vals[k]);
        t->maxcode[len] = cnt ? code - 1 : -1;
        code <<= 1;
    }
    t->present = true;
    return JPEG_OK;
}

inline int jpeg_parse(const uint8_t* d, size_t n, JpegHeader* H, JpegError* e) {
    if (!d || n < 4 || d[0] != 0xFF || d[1] != 0xD8) return jpeg_fail(e, JPEG_INVALID, "jpeg: no SOI marker");
    size_t pos = 2;
    bool have_frame = false;
    for (;;) {
        if (pos >= n) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (ends before the scan)");
        if (d[pos] != 0xFF) return jpeg_fail(e, JPEG_INVALID, "jpeg: marker expected at byte %zu", pos);
        while (pos < n && d[pos] == 0xFF) pos++;        // fill bytes
        if (pos >= n) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (ends inside a marker)");
        const int m = d[pos++];
        if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;      // no segment
        if (m == 0xD9) return jpeg_fail(e, JPEG_INVALID, "jpeg: EOI before the scan");
        if (n - pos < 2) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (segment length)");
        const size_t len = ((size_t)d[pos] << 8) | d[pos + 1];
        if (len < 2 || len > n - pos) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (segment of marker %02x)", m);
        const uint8_t* s = d + pos + 2;
        const size_t sl = len - 2;
        pos += len;
        if (m == 0xDB) {
            size_t i = 0;
            while (i < sl) {
                const int pq = s[i] >> 4, t = s[i] & 15;
                if (pq != 0) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: 16-bit quantisation table (Pq = %d)", pq);
                if (t > 3 || sl - i < 65) return jpeg_fail(e, JPEG_INVALID, "jpeg: bad DQT segment");
                for (int k = 0; k < 64; k++) H->q[t][JPEG_ZIGZAG[k]] = s[i + 1 + k];
                H->has_q[t] = true;
                i += 65;
            }
        } else if (m == 0xC4) {
            size_t i = 0;
            while (i < sl) {
                if (sl - i < 17) return jpeg_fail(e, JPEG_INVALID, "jpeg: bad DHT segment");
                const int tc = s[i] >> 4, th = s[i] & 15;
                int total = 0;
                for (int k = 0; k < 16; k++) total += s[i + 1 + k];
                if (tc > 1 || th > 3 || total > 256 || sl - i - 17 < (size_t)total) return jpeg_fail(e, JPEG_INVALID, "jpeg: bad DHT segment");
                if (int rc = jpeg_build_huff(s + i + 1, s + i + 17, total, tc ? &H->ac[th] : &H->dc[th], e)) return rc;
                i += 17 + (size_t)total;
            }
        } else if (m == 0xCC) {
            return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: arithmetic coding (DAC)");
        } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8) {
            if (m == 0xC2) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: progressive stream (SOF2)");
            if (m >= 0xC9) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: arithmetic coding (SOF%d)", m - 0xC0);
            if (m != 0xC0) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: extended, lossless or hierarchical stream (SOF%d)", m - 0xC0);
            if (have_frame) return jpeg_fail(e, JPEG_INVALID, "jpeg: two frame headers");
            if (sl < 6) return jpeg_fail(e, JPEG_INVALID, "jpeg: bad SOF0 segment");
            const int prec = s[0], nc = s[5];
            H->height = (s[1] << 8) | s[2];
            H->width = (s[3] << 8) | s[4];
            if (prec != 8) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: %d-bit precision", prec);
            if (nc == 4) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: 4 components (CMYK / YCCK)");
            if (nc != 1 && nc != 3) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: %d components", nc);
            if (sl != 6 + 3 * (size_t)nc) return jpeg_fail(e, JPEG_INVALID, "jpeg: bad SOF0 segment");
            if (H->width == 0 || H->height == 0) return jpeg_fail(e, JPEG_INVALID, "jpeg: zero dimension (%d x %d)", H->width, H->height);
            if ((uint64_t)H->width * (uint64_t)H->height >= (1ull << 31)) return jpeg_fail(e, JPEG_INVALID, "jpeg: %d x %d is 2^31 pixels or more", H->width, H->height);
            H->ncomp = nc;
            for (int c = 0; c < nc; c++) {
                H->id[c] = s[6 + 3 * c];
                H->file_h[c] = s[7 + 3 * c] >> 4; H->file_v[c] = s[7 + 3 * c] & 15;
                H->tq[c] = s[8 + 3 * c];
                if (H->file_h[c] < 1 || H->file_h[c] > 4 || H->file_v[c] < 1 || H->file_v[c] > 4 || H->tq[c] > 3)
                    return jpeg_fail(e, JPEG_INVALID, "jpeg: bad component %d in SOF0", c);
            }
            if (nc == 3) {
                const bool chroma11 = H->file_h[1] == 1 && H->file_v[1] == 1 && H->file_h[2] == 1 && H->file_v[2] == 1;
                const int lh = H->file_h[0], lv = H->file_v[0];
                if (!chroma11 || !((lh == 1 && lv == 1) || (lh == 2 && lv == 1) || (lh == 2 && lv == 2)))
                    return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: sampling layout %dx%d,%dx%d,%dx%d (4:4:4, 4:2:2 and 4:2:0 with 1x1 chroma only)", lh, lv,
                                     H->file_h[1], H->file_v[1], H->file_h[2], H->file_v[2]);
                for (int c = 0; c < 3; c++) { H->h[c] = H->file_h[c]; H->v[c] = H->file_v[c]; }
            }
            have_frame = true;
        } else if (m == 0xDD) {
            if (sl != 2) return jpeg_fail(e, JPEG_INVALID, "jpeg: bad DRI segment");
            H->restart_interval = (s[0] << 8) | s[1];
        } else if (m == 0xDA) {
            if (!have_frame) return jpeg_fail(e, JPEG_INVALID, "jpeg: SOS before SOF");
            if (sl < 1) return jpeg_fail(e, JPEG_INVALID, "jpeg: bad SOS segment");
            const int ns = s[0];
            if (ns != H->ncomp) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: multi-scan or non-interleaved file (a scan of %d of %d components)", ns, H->ncomp);
            if (sl != 4 + 2 * (size_t)ns) return jpeg_fail(e, JPEG_INVALID, "jpeg: bad SOS segment");
            for (int c = 0; c < ns; c++) {
                if (s[1 + 2 * c] != H->id[c]) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: scan components out of frame order");
                H->td[c] = s[2 + 2 * c] >> 4; H->ta[c] = s[2 + 2 * c] & 15;
                if (H->td[c] > 3 || H->ta[c] > 3) return jpeg_fail(e, JPEG_INVALID, "jpeg: bad table selector in SOS");
            }
            if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
                return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: spectral selection or successive approximation in a baseline scan");
            break;
        }
        // APPn, COM and everything else: skipped
    }
    for (int c = 0; c < H->ncomp; c++) {
        if (!H->has_q[H->tq[c]]) return jpeg_fail(e, JPEG_INVALID, "jpeg: missing quantisation table %d", H->tq[c]);
        if (!H->dc[H->td[c]].present || !H->ac[H->ta[c]].present) return jpeg_fail(e, JPEG_INVALID, "jpeg: missing Huffman table of component %d", c);
        for (int k = 0; k < 64; k++) {
            const int u = k >> 3, v = k & 7;
            H->sw[c][k] = (uint32_t)H->q[H->tq[c]][k] * (uint32_t)(u && v ? JPEG_S_W11 : (u || v ? JPEG_S_W01 : JPEG_S_W00));
        }
    }
    H->scan = pos;
    const int hmax = H->h[0], vmax = H->v[0];       // chroma is 1 x 1
    H->mcux = (H->width + 8 * hmax - 1) / (8 * hmax);
    H->mcuy = (H->height + 8 * vmax - 1) / (8 * vmax);
    for (int c = 0; c < H->ncomp; c++) { H->bw[c] = H->mcux * H->h[c]; H->bh[c] = H->mcuy * H->v[c]; }
    H->cw = (H->width + hmax - 1) / hmax;
    H->ch = (H->height + vmax - 1) / vmax;
    H->rule = hmax == 1 ? JPEG_UP_COPY : (vmax == 1 ? (H->cw <= 2 ? JPEG_UP_H2V1_REPLICATE : JPEG_UP_H2V1) : (H->cw <= 2 ? JPEG_UP_H2V2_REPLICATE : JPEG_UP_H2V2));
    return JPEG_OK;
}

// the scan split at its markers: one segment per restart interval, RSTn in order, then EOI
inline int jpeg_segments(const uint8_t* d, size_t n, const JpegHeader& H, std::vector<JpegSegment>* segs, JpegError* e) {
    segs->clear();
    const size_t want = H.intervals();
    size_t start = H.scan, i = H.scan;
    for (;;) {
        const uint8_t* f = i < n ? (const uint8_t*)memchr(d + i, 0xFF, n - i) : nullptr;
        if (!f) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (the scan has no EOI)");
        i = (size_t)(f - d);
        size_t j = i + 1;
        while (j < n && d[j] == 0xFF) j++;
        if (j >= n) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (the scan has no EOI)");
        const int m = d[j];
        if (m == 0x00 && j == i + 1) { i = j + 1; continue; }       // a stuffed FF
        if (segs->size() >= want) return jpeg_fail(e, JPEG_INVALID, "jpeg: more restart intervals than the frame has (%zu)", want);
        segs->push_back({start, i});
        start = i = j + 1;
        if (m >= 0xD0 && m <= 0xD7) {
            if (m != 0xD0 + (int)((segs->size() - 1) & 7)) return jpeg_fail(e, JPEG_INVALID, "jpeg: wrong restart index (RST%d after interval %zu)", m - 0xD0, segs->size() - 1);
            continue;
        }
        if (m == 0xD9) break;
        if (m == 0xDA || m == 0xC4 || m == 0xDB || m == 0xDD) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: multi-scan or non-interleaved file (marker %02x after the scan)", m);
        return jpeg_fail(e, JPEG_INVALID, "jpeg: marker %02x inside the scan", m);
    }
    if (segs->size() != want) return jpeg_fail(e, JPEG_INVALID, "jpeg: %zu restart intervals, the frame has %zu", segs->size(), want);
    // a block costs two bits at least (a DC code and an end of block): a frame header that promises more blocks than the scan can
    // hold is refused here, before anybody allocates the frame it describes
    size_t coded = 0, blocks = 0;
    for (const JpegSegment& s : *segs) coded += s.end - s.begin;
    for (int c = 0; c < H.ncomp; c++) blocks += H.blocks(c);
    if (blocks > 4 * coded) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (%zu coded bytes cannot hold the frame's %zu blocks)", coded, blocks);
    return JPEG_OK;
}

// bit reader over one segment: FF 00 is a stuffed FF; it never reads past `end` and never invents bits
struct JpegBits {
    const uint8_t *p, *end;
    uint64_t acc = 0;
    int cnt = 0;
    JpegBits(const uint8_t* b, const uint8_t* e_) : p(b), end(e_) {}
    void fill() {
        while (cnt <= 56 && p < end) {
            const uint8_t b = *p;
            if (b == 0xFF) {
                if (end - p >= 2 && p[1] == 0x00) p += 2;
                else { p = end; break; }
            } else p++;
            acc = (acc << 8) | b;
            cnt += 8;
        }
    }
    // the next 16 bits, zeros past the end (what is consumed is checked against cnt)
    uint32_t peek16() {
        if (cnt < 16) fill();
        return (uint32_t)(cnt >= 16 ? (acc >> (cnt - 16)) : (acc << (16 - cnt))) & 0xFFFFu;
    }
    bool skip(int nbits) { if (nbits > cnt) return false; cnt -= nbits; return true; }
    bool get(int nbits, int* out) {     // nbits 1 .. 15
        if (cnt < nbits) fill();
        if (cnt < nbits) return false;
        cnt -= nbits;
        *out = (int)((acc >> cnt) & ((1u << nbits) - 1));
        return true;
    }
};

// 0 .. 255, -1: the data ended inside the code, -2: no such code
inline int jpeg_symbol(JpegBits& br, const JpegHuff& t) {
    const uint32_t look = br.peek16();
    const uint16_t f = t.fast[look >> 7];
    if (f) return br.skip(f >> 8) ? (f & 255) : -1;
    for (int len = 10; len <= 16; len++) {
        const int32_t code = (int32_t)(look >> (16 - len));
        if (code <= t.maxcode[len]) {
            const int idx = t.valoff[len] + code;
            if (idx < 0 || idx >= t.total) return -2;
            return br.skip(len) ? t.vals[idx] : -1;
        }
    }
    return br.cnt < 16 ? -1 : -2;
}

inline int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// restart intervals [first, first + count) of the scan into the component planes
inline int jpeg_entropy(const uint8_t* d, const JpegHeader& H, const std::vector<JpegSegment>& segs, size_t first, size_t count, int16_t* const planes[3],
                        JpegError* e) {
    const size_t total = (size_t)H.mcux * H.mcuy, per = H.restart_interval ? (size_t)H.restart_interval : total;
    for (size_t k = first; k < first + count && k < segs.size(); k++) {
        JpegBits br(d + segs[k].begin, d + segs[k].end);
        int pred[3] = {0, 0, 0};
        const size_t m1 = (k + 1) * per < total ? (k + 1) * per : total;
        for (size_t mcu = k * per; mcu < m1; mcu++) {
            const size_t my = mcu / (size_t)H.mcux, mx = mcu % (size_t)H.mcux;
            for (int c = 0; c < H.ncomp; c++) {
                const JpegHuff &dc = H.dc[H.td[c]], &ac = H.ac[H.ta[c]];
                for (int by = 0; by < H.v[c]; by++)
                    for (int bx = 0; bx < H.h[c]; bx++) {
                        int16_t* blk = planes[c] + ((my * H.v[c] + by) * (size_t)H.bw[c] + mx * H.h[c] + bx) * 64;
                        memset(blk, 0, 64 * sizeof(int16_t));
                        int s = jpeg_symbol(br, dc);
                        if (s == -2 || s > 15) return jpeg_fail(e, JPEG_INVALID, "jpeg: Huffman code not in the DC table (MCU %zu)", mcu);
                        int bits = 0;
                        if (s < 0 || (s && !br.get(s, &bits))) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (entropy-coded data ends in MCU %zu)", mcu);
                        pred[c] += s ? jpeg_extend(bits, s) : 0;
                        if (pred[c] < -32768 || pred[c] > 32767) return jpeg_fail(e, JPEG_INVALID, "jpeg: DC coefficient out of the 16-bit range (MCU %zu)", mcu);
                        blk[0] = (int16_t)pred[c];
                        uint64_t S = (uint64_t)(pred[c] < 0 ? -pred[c] : pred[c]) * H.sw[c][0];
                        int kk = 1;
                        while (kk < 64) {
                            const int rs = jpeg_symbol(br, ac);
                            if (rs == -2) return jpeg_fail(e, JPEG_INVALID, "jpeg: Huffman code not in the AC table (MCU %zu)", mcu);
                            if (rs < 0) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (entropy-coded data ends in MCU %zu)", mcu);
                            const int r = rs >> 4;
                            s = rs & 15;
                            if (s == 0) {
                                if (r != 15) break;     // end of block
                                kk += 16;
                                if (kk > 64) return jpeg_fail(e, JPEG_INVALID, "jpeg: zero run past coefficient 63 (MCU %zu)", mcu);
                                continue;
                            }
                            kk += r;
                            if (kk > 63) return jpeg_fail(e, JPEG_INVALID, "jpeg: zero run past coefficient 63 (MCU %zu)", mcu);
                            if (!br.get(s, &bits)) return jpeg_fail(e, JPEG_INVALID, "jpeg: truncated stream (entropy-coded data ends in MCU %zu)", mcu);
                            const int val = jpeg_extend(bits, s), nat = JPEG_ZIGZAG[kk];
                            blk[nat] = (int16_t)val;
                            S += (uint64_t)(val < 0 ? -val : val) * H.sw[c][nat];
                            kk++;
                        }
                        if (S > (uint64_t)JPEG_IDCT_S_MAX * 1024u)
                            return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: a block of MCU %zu is beyond the 32-bit IDCT's bound (no encoder makes one)", mcu);
                    }
            }
        }
    }
    return JPEG_OK;
}
