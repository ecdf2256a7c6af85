// jpeg_enc_host.h -- the host layer of the JPEG encode (jpeg_enc.hip): parameter checks, headers and the Huffman coder of a baseline
// stream with the Annex K tables, plain C++ with no device code (tests/harness/jpeg_enc_host_harness.cpp compiles it on its own, also
// under the address and undefined-behaviour sanitizers).
//
//   jpeg_enc_check       the refusals of an image's geometry and of the parameters; fills in the defaults
//   jpeg_enc_headers     SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI (with a restart interval only), SOS
//   jpeg_enc_plan        the scan cut into chunks of whole MCU rows -- of whole restart intervals when there is an interval
//   jpeg_enc_code        one chunk: its starting DC predictors are read from the coefficient planes (0 after a restart), so chunks
//                        are independent and callers code them in parallel
//   jpeg_enc_join_*      the chunks joined -- at bit granularity, FF bytes stuffed after the join, because stuffing depends on byte
//                        alignment; bytewise with restart intervals, whose chunks are whole bytes already -- and EOI; chunk by
//                        chunk in two passes (count, write), so the join runs in parallel too
// The stream does not depend on the number of chunks.  Coefficients are int16 blocks of 64 in natural order, each component a plane
// of (MCUs_y V) x (MCUs_x H) blocks with its dummy blocks filled (no AC, the DC of the block before): what the device writes.
#pragma once
#include <string.h>
#include <vector>
#include "jpeg_enc_core.h"
#include "jpeg_host.h"      // JpegError, jpeg_fail, JPEG_ZIGZAG

struct JpegEncParams { int quality, sampling, restart_interval; };      // MisJpegEncodeParams, defaults filled in

constexpr int JPEG_ENC_DEFAULT_QUALITY = 95;      // cv::imwrite's

// p == nullptr: all defaults
inline int jpeg_enc_check(int width, int height, int channels, bool u8, const JpegEncParams* p, JpegEncParams* out, JpegError* e) {
    if (width <= 0 || height <= 0) return jpeg_fail(e, JPEG_INVALID, "jpeg: zero or negative size (%d x %d)", width, height);
    if (width > 65535 || height > 65535) return jpeg_fail(e, JPEG_INVALID, "jpeg: %d x %d, a dimension above 65535", width, height);
    if (channels == 1) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: 1-channel source (greyscale output)");
    if (channels == 4) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: 4-channel source");
    if (channels != 3 || !u8) return jpeg_fail(e, JPEG_INVALID, "jpeg: the source must be 8UC3 BGR (%d channels)", channels);
    JpegEncParams r = p ? *p : JpegEncParams{0, JPEG_ENC_420, 0};
    if (r.quality < 0 || r.quality > 100) return jpeg_fail(e, JPEG_INVALID, "jpeg: quality %d (1 .. 100, 0: the default)", r.quality);
    if (r.quality == 0) r.quality = JPEG_ENC_DEFAULT_QUALITY;
    if (r.sampling == 3) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: 4:4:0 sampling (4:2:0, 4:2:2 and 4:4:4 only)");
    if (r.sampling == 4) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: 4:1:1 sampling (4:2:0, 4:2:2 and 4:4:4 only)");
    if (r.sampling < 0 || r.sampling > 4) return jpeg_fail(e, JPEG_UNSUPPORTED, "jpeg: sampling %d (4:2:0, 4:2:2 and 4:4:4 only)", r.sampling);
    if (r.restart_interval < 0 || r.restart_interval > 65535)
        return jpeg_fail(e, JPEG_INVALID, "jpeg: restart interval %d (0 .. 65535 MCUs)", r.restart_interval);
    *out = r;
    return JPEG_OK;
}

// Annex K.3 - K.6: the number of codes of each length 1 .. 16, then the symbols; tables DC0, AC0, DC1, AC1
static const uint8_t JPEG_ENC_DC_BITS[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static const uint8_t JPEG_ENC_DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t JPEG_ENC_AC_BITS[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static const uint8_t JPEG_ENC_AC_VALS[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// code and length of every symbol of one table; length 0: no such symbol
struct JpegEncHuff {
    uint16_t code[256];
    uint8_t len[256];
    JpegEncHuff(const uint8_t bits[16], const uint8_t* vals) {
        memset(len, 0, sizeof(len));
        memset(code, 0, sizeof(code));
        unsigned c = 0;
        int k = 0;
        for (int l = 1; l <= 16; l++) {
            for (int i = 0; i < bits[l - 1]; i++, k++, c++) { code[vals[k]] = (uint16_t)c; len[vals[k]] = (uint8_t)l; }
            c <<= 1;
        }
    }
};

struct JpegEncTables {
    JpegEncHuff dc[2], ac[2];
    JpegEncTables()
        : dc{JpegEncHuff(JPEG_ENC_DC_BITS[0], JPEG_ENC_DC_VALS), JpegEncHuff(JPEG_ENC_DC_BITS[1], JPEG_ENC_DC_VALS)},
          ac{JpegEncHuff(JPEG_ENC_AC_BITS[0], JPEG_ENC_AC_VALS[0]), JpegEncHuff(JPEG_ENC_AC_BITS[1], JPEG_ENC_AC_VALS[1])} {}
};

inline void jpeg_enc_segment(std::vector<uint8_t>* out, int marker, const uint8_t* payload, size_t n) {
    const uint8_t head[4] = {0xFF, (uint8_t)marker, (uint8_t)((n + 2) >> 8), (uint8_t)(n + 2)};
    out->insert(out->end(), head, head + 4);
    out->insert(out->end(), payload, payload + n);
}

inline void jpeg_enc_headers(const JpegEncGeom& g, const JpegEncParams& p, std::vector<uint8_t>* out) {
    out->push_back(0xFF); out->push_back(0xD8);
    const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    jpeg_enc_segment(out, 0xE0, jfif, sizeof(jfif));
    for (int t = 0; t < 2; t++) {
        uint16_t q[64];
        jpeg_enc_qtable(p.quality, t, q);
        uint8_t seg[65] = {(uint8_t)t};
        for (int k = 0; k < 64; k++) seg[1 + k] = (uint8_t)q[JPEG_ZIGZAG[k]];
        jpeg_enc_segment(out, 0xDB, seg, sizeof(seg));
    }
    const uint8_t sof[15] = {8, (uint8_t)(g.h >> 8), (uint8_t)g.h, (uint8_t)(g.w >> 8), (uint8_t)g.w, 3, 1, (uint8_t)(g.hmax * 16 + g.vmax), 0, 2, 0x11, 1, 3, 0x11, 1};
    jpeg_enc_segment(out, 0xC0, sof, sizeof(sof));
    for (int t = 0; t < 2; t++) {
        uint8_t seg[1 + 16 + 162];
        seg[0] = (uint8_t)t;
        memcpy(seg + 1, JPEG_ENC_DC_BITS[t], 16);
        memcpy(seg + 17, JPEG_ENC_DC_VALS, 12);
        jpeg_enc_segment(out, 0xC4, seg, 17 + 12);
        seg[0] = (uint8_t)(0x10 | t);
        memcpy(seg + 1, JPEG_ENC_AC_BITS[t], 16);
        memcpy(seg + 17, JPEG_ENC_AC_VALS[t], 162);
        jpeg_enc_segment(out, 0xC4, seg, 17 + 162);
    }
    if (p.restart_interval) {
        const uint8_t dri[2] = {(uint8_t)(p.restart_interval >> 8), (uint8_t)p.restart_interval};
        jpeg_enc_segment(out, 0xDD, dri, 2);
    }
    const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0};
    jpeg_enc_segment(out, 0xDA, sos, sizeof(sos));
}

// MCUs [m0, m1) of the scan and what coding them gave: whole bytes, then `tail_bits` (< 8) more bits in the low end of `tail`.
// Without a restart interval the bytes are not stuffed yet (the join does that); with one they are final, markers included.
struct JpegEncChunk {
    size_t m0 = 0, m1 = 0;
    std::vector<uint8_t> bytes;
    size_t size = 0;            // bytes written (the vector is grown ahead of the writer)
    uint32_t tail = 0;
    int tail_bits = 0;
    JpegError err;
};

inline void jpeg_enc_plan(const JpegEncGeom& g, int restart_interval, int want, std::vector<JpegEncChunk>* chunks) {
    const size_t total = (size_t)g.mx * g.my, per = restart_interval ? (size_t)restart_interval : (size_t)g.mx;
    const size_t units = (total + per - 1) / per;
    const size_t n = want < 1 ? 1 : ((size_t)want < units ? (size_t)want : units);
    chunks->clear();
    chunks->resize(n);
    for (size_t k = 0; k < n; k++) {
        (*chunks)[k].m0 = (k * units / n) * per;
        (*chunks)[k].m1 = k + 1 == n ? total : ((k + 1) * units / n) * per;
    }
}

struct JpegEncBits {
    JpegEncChunk& c;
    const bool stuff;
    uint64_t acc = 0;
    int n = 0;
    JpegEncBits(JpegEncChunk& chunk, bool stuff_) : c(chunk), stuff(stuff_) {}
    // room for what one block can write: 64 codes of at most 26 bits, every byte stuffed, and a marker
    void reserve_block() { if (c.bytes.size() < c.size + 512) c.bytes.resize(c.bytes.size() * 2 + 4096); }
    void drain() {
        while (n >= 8) {
            const uint8_t b = (uint8_t)(acc >> (n - 8));
            c.bytes[c.size++] = b;
            if (stuff && b == 0xFF) c.bytes[c.size++] = 0;
            n -= 8;
        }
    }
    void put(uint32_t v, int len) {     // len <= 26; v has no bits above len
        acc = (acc << len) | v;
        n += len;
        if (n >= 32) drain();
    }
    void pad() { drain(); if (n) { put((1u << (8 - n)) - 1, 8 - n); drain(); } }
    void marker(int m) { c.bytes[c.size++] = 0xFF; c.bytes[c.size++] = (uint8_t)m; }
    void finish() { drain(); c.tail = (uint32_t)(acc & ((1u << n) - 1)); c.tail_bits = n; c.bytes.resize(c.size); }
};

inline int jpeg_enc_category(int v) {
    const unsigned a = (unsigned)(v < 0 ? -v : v);
    return a ? 32 - __builtin_clz(a) : 0;
}

inline int jpeg_enc_code(const int16_t* const coef[3], const JpegEncGeom& g, int restart_interval, const JpegEncTables& T, JpegEncChunk* chunk) {
    const size_t total = (size_t)g.mx * g.my, ri = (size_t)restart_interval;
    JpegEncBits bw(*chunk, ri != 0);
    chunk->size = 0;
    int pred[3] = {0, 0, 0};
    if (!ri && chunk->m0) {     // the last block of each component in the MCU before
        const size_t my = (chunk->m0 - 1) / (size_t)g.mx, mx = (chunk->m0 - 1) % (size_t)g.mx;
        for (int c = 0; c < 3; c++) {
            const int hc = c ? 1 : g.hmax, vc = c ? 1 : g.vmax;
            pred[c] = coef[c][((my * vc + vc - 1) * (size_t)g.bw[c] + mx * hc + hc - 1) * 64];
        }
    }
    for (size_t mcu = chunk->m0; mcu < chunk->m1; mcu++) {
        const size_t my = mcu / (size_t)g.mx, mx = mcu % (size_t)g.mx;
        if (ri && mcu % ri == 0) {
            bw.reserve_block();
            if (mcu) bw.marker(0xD0 + (int)((mcu / ri - 1) & 7));
            pred[0] = pred[1] = pred[2] = 0;
        }
        for (int c = 0; c < 3; c++) {
            const int hc = c ? 1 : g.hmax, vc = c ? 1 : g.vmax;
            const JpegEncHuff &dc = T.dc[c ? 1 : 0], &ac = T.ac[c ? 1 : 0];
            for (int by = 0; by < vc; by++)
                for (int bx = 0; bx < hc; bx++) {
                    const int16_t* blk = coef[c] + ((my * vc + by) * (size_t)g.bw[c] + mx * hc + bx) * 64;
                    bw.reserve_block();
                    const int d = blk[0] - pred[c];
                    pred[c] = blk[0];
                    int cat = jpeg_enc_category(d);
                    if (cat > 11) return jpeg_fail(&chunk->err, JPEG_INVALID, "jpeg: DC difference %d out of range (MCU %zu)", d, mcu);
                    bw.put(((uint32_t)dc.code[cat] << cat) | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << cat) - 1)), dc.len[cat] + cat);
                    uint64_t nz = 0;
                    for (int k = 1; k < 64; k++) nz |= (uint64_t)(blk[JPEG_ZIGZAG[k]] != 0) << k;
                    int last = 0;
                    while (nz) {
                        const int k = __builtin_ctzll(nz);
                        nz &= nz - 1;
                        int run = k - last - 1;
                        last = k;
                        for (; run > 15; run -= 16) bw.put(ac.code[0xF0], ac.len[0xF0]);
                        const int v = blk[JPEG_ZIGZAG[k]];
                        cat = jpeg_enc_category(v);
                        if (cat > 10) return jpeg_fail(&chunk->err, JPEG_INVALID, "jpeg: AC coefficient %d out of range (MCU %zu)", v, mcu);
                        const int rs = (run << 4) | cat;
                        bw.put(((uint32_t)ac.code[rs] << cat) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << cat) - 1)), ac.len[rs] + cat);
                    }
                    if (last != 63) bw.put(ac.code[0], ac.len[0]);
                }
        }
        if (ri && ((mcu + 1) % ri == 0 || mcu + 1 == total)) bw.pad();
    }
    bw.finish();
    return JPEG_OK;
}

// The join.  Without a restart interval the chunks' bits follow each other with no gap: chunk k begins at bit bit0[k] of the scan, and
// owns the scan's bytes whose first bit lies inside it -- a byte's other bits may be the next chunks', and past the scan's end they
// are ones.  jpeg_enc_join_count gives the bytes a chunk owns once every FF among them has its 00 behind it, jpeg_enc_join_layout
// turns the counts into offsets into the file (headers first, EOI last), jpeg_enc_join_write writes a chunk's bytes there: chunks
// are independent in both passes, so callers run them in parallel.  With a restart interval a chunk's bytes are final and it owns them.
struct JpegEncJoin {
    bool restart = false;
    std::vector<uint64_t> bit0;     // n + 1 entries: the first bit of each chunk, then the scan's length in bits
    std::vector<size_t> off;        // n + 1 entries: counts, then (jpeg_enc_join_layout) the file offset of each chunk's bytes and of EOI
    size_t bytes = 0;               // the whole file
};

inline void jpeg_enc_join_begin(const std::vector<JpegEncChunk>& chunks, int restart_interval, JpegEncJoin* J) {
    const size_t n = chunks.size();
    J->restart = restart_interval != 0;
    J->bit0.assign(n + 1, 0);
    J->off.assign(n + 1, 0);
    for (size_t k = 0; k < n; k++) J->bit0[k + 1] = J->bit0[k] + 8 * (uint64_t)chunks[k].bytes.size() + (uint64_t)chunks[k].tail_bits;
}

inline unsigned jpeg_enc_chunk_bit(const JpegEncChunk& c, uint64_t p) {
    const uint64_t nb = c.bytes.size();
    if (p < 8 * nb) return (c.bytes[p >> 3] >> (7 - (p & 7))) & 1u;
    return (c.tail >> (c.tail_bits - 1 - (int)(p - 8 * nb))) & 1u;
}

// the bytes chunk k owns, in order, handed to sink(byte)
template <class Sink>
inline void jpeg_enc_join_chunk(const std::vector<JpegEncChunk>& chunks, const JpegEncJoin& J, size_t k, Sink sink) {
    const JpegEncChunk& c = chunks[k];
    const uint64_t total = J.bit0.back();
    const uint64_t j0 = (J.bit0[k] + 7) / 8, j1 = (J.bit0[k + 1] + 7) / 8;
    if (j0 >= j1) return;
    const unsigned s = (unsigned)(8 * j0 - J.bit0[k]);      // the owned bytes begin at bit s of the chunk, all at the same shift
    const size_t nb = c.bytes.size();
    const uint8_t* b = c.bytes.data();
    uint64_t j = j0;
    if (s == 0) {
        for (; j < j1 && (size_t)(j - j0) < nb; j++) sink(b[j - j0]);
    } else {
        for (; j < j1 && (size_t)(j - j0) + 1 < nb; j++) sink((uint8_t)((b[j - j0] << s) | (b[j - j0 + 1] >> (8 - s))));
    }
    for (; j < j1; j++) {       // the bytes that reach into the chunk's last bits, the next chunks or the padding
        unsigned v = 0;
        size_t kk = k;
        for (int t = 0; t < 8; t++) {
            const uint64_t g = 8 * j + (uint64_t)t;
            if (g >= total) { v = (v << 1) | 1u; continue; }
            while (g >= J.bit0[kk + 1]) kk++;
            v = (v << 1) | jpeg_enc_chunk_bit(chunks[kk], g - J.bit0[kk]);
        }
        sink((uint8_t)v);
    }
}

inline void jpeg_enc_join_count(const std::vector<JpegEncChunk>& chunks, JpegEncJoin* J, size_t k) {
    size_t n = 0;
    if (J->restart) n = chunks[k].bytes.size();
    else jpeg_enc_join_chunk(chunks, *J, k, [&](uint8_t v) { n += v == 0xFF ? 2 : 1; });
    J->off[k + 1] = n;
}

inline void jpeg_enc_join_layout(JpegEncJoin* J, size_t head_bytes) {
    size_t at = head_bytes;
    for (size_t k = 0; k + 1 < J->off.size(); k++) { const size_t n = J->off[k + 1]; J->off[k] = at; at += n; }
    J->off.back() = at;
    J->bytes = at + 2;
}

inline void jpeg_enc_join_write(const std::vector<JpegEncChunk>& chunks, const JpegEncJoin& J, size_t k, uint8_t* file) {
    uint8_t* d = file + J.off[k];
    if (J.restart) { if (!chunks[k].bytes.empty()) memcpy(d, chunks[k].bytes.data(), chunks[k].bytes.size()); }
    else jpeg_enc_join_chunk(chunks, J, k, [&](uint8_t v) { *d++ = v; if (v == 0xFF) *d++ = 0; });
    if (k + 1 == chunks.size()) { file[J.off.back()] = 0xFF; file[J.off.back() + 1] = 0xD9; }
}

// the whole stream of one image from its coefficient planes, in `want` chunks at most, on the calling thread
inline int jpeg_enc_stream(const int16_t* const coef[3], const JpegEncGeom& g, const JpegEncParams& p, int want, std::vector<uint8_t>* out, JpegError* e) {
    static const JpegEncTables T;
    std::vector<JpegEncChunk> chunks;
    jpeg_enc_plan(g, p.restart_interval, want, &chunks);
    for (JpegEncChunk& c : chunks)
        if (jpeg_enc_code(coef, g, p.restart_interval, T, &c) != JPEG_OK) { *e = c.err; return e->code; }
    out->clear();
    jpeg_enc_headers(g, p, out);
    JpegEncJoin J;
    jpeg_enc_join_begin(chunks, p.restart_interval, &J);
    for (size_t k = 0; k < chunks.size(); k++) jpeg_enc_join_count(chunks, &J, k);
    jpeg_enc_join_layout(&J, out->size());
    out->resize(J.bytes);
    for (size_t k = 0; k < chunks.size(); k++) jpeg_enc_join_write(chunks, J, k, out->data());
    return JPEG_OK;
}
