// jpeg_enc_host_harness.cpp -- the JPEG encode's host layer (image_stitching_amd/csrc/jpeg_enc_host.h) and the host twin of its device
// arithmetic (jpeg_enc_core.h: the functions the kernels of jpeg_enc.hip call, compiled here by the host compiler) as a program of
// its own.
//
//   jpeg_enc_host_harness encode <w> <h> <quality> <sampling 0|1|2> <restart> <chunks> <in.bgr> <out.jpg>
//        the whole encode on the CPU from packed BGR rows: what the kernels do per block, then the entropy coder in <chunks> chunks
//   jpeg_enc_host_harness stress
//        the entropy coder over an all-zero plane, planes of extreme values (the largest categories the tables hold, and beyond
//        them: refused), a 1 x 1 image, a chunk count above the MCU row count and a restart interval of 1, every case at several
//        chunk counts whose streams must be equal; prints "stress OK".  Built with -fsanitize=address,undefined this is the
//        memory-safety check of the coder's buffers.
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../image_stitching_amd/csrc/jpeg_enc_host.h"

// what jpeg_enc_luma_kernel / jpeg_enc_chroma_kernel do, block by block
static void transform(const uint8_t* bgr, const JpegEncGeom& g, int quality, std::vector<int16_t> coef[3]) {
    auto px = [&](int x, int y, int k) { return (int)bgr[((size_t)std::min(y, g.h - 1) * g.w + std::min(x, g.w - 1)) * 3 + k]; };
    for (int c = 0; c < 3; c++) {
        uint16_t q[64];
        uint32_t recip[64], half[64];
        jpeg_enc_qtable(quality, c ? 1 : 0, q);
        for (int k = 0; k < 64; k++) jpeg_enc_divisor(q[k], &recip[k], &half[k]);
        coef[c].assign(g.blocks(c) * 64, 0);
        const int fx = c ? g.hmax : 1, fy = c ? g.vmax : 1, ch = (g.h + fy - 1) / fy;
        for (int j = 0; j < g.bh[c]; j++)
            for (int i = 0; i < g.bw[c]; i++) {
                const bool dummy = i >= g.wb[c] || j >= g.hb[c];
                int si = i, sj = j;
                if (dummy) jpeg_enc_dummy_source(i, j, g.wb[c], g.hb[c], g.hmax, &si, &sj);
                int x[64];
                for (int r = 0; r < 8; r++)
                    for (int k = 0; k < 8; k++) {
                        const int dy = std::min(sj * 8 + r, ch - 1), dx = si * 8 + k;
                        int sum = 0;
                        for (int t = 0; t < fy; t++)
                            for (int u = 0; u < fx; u++) {
                                const int X = dx * fx + u, Y = dy * fy + t, B = px(X, Y, 0), G = px(X, Y, 1), R = px(X, Y, 2);
                                sum += c == 0 ? jpeg_enc_y(R, G, B) : (c == 1 ? jpeg_enc_cb(R, G, B) : jpeg_enc_cr(R, G, B));
                            }
                        x[8 * r + k] = fx == 2 && fy == 2 ? (sum + 1 + (k & 1)) >> 2 : (fx == 2 ? (sum + (k & 1)) >> 1 : sum);
                    }
                jpeg_fdct_quant_block(x, recip, half);
                int16_t* out = coef[c].data() + ((size_t)j * g.bw[c] + i) * 64;
                for (int k = 0; k < 64; k++) out[k] = (int16_t)(dummy && k ? 0 : x[k]);
            }
    }
}

static int stream_of(const std::vector<int16_t> coef[3], const JpegEncGeom& g, const JpegEncParams& p, int chunks, std::vector<uint8_t>* out, JpegError* e) {
    const int16_t* planes[3] = {coef[0].data(), coef[1].data(), coef[2].data()};
    return jpeg_enc_stream(planes, g, p, chunks, out, e);
}

static bool stress_case(const char* name, int w, int h, int sampling, int restart, int value, int ac_value, int expect) {
    const JpegEncParams p{90, sampling, restart};
    const JpegEncGeom g = jpeg_enc_geometry(w, h, sampling);
    std::vector<int16_t> coef[3];
    for (int c = 0; c < 3; c++) {
        coef[c].assign(g.blocks(c) * 64, (int16_t)ac_value);
        for (size_t b = 0; b < g.blocks(c); b++) coef[c][b * 64] = (int16_t)((b & 1) ? -value : value);     // DC differences of 2 |value|
    }
    std::vector<uint8_t> first;
    for (int chunks : {1, 2, 3, 7, g.my, g.my + 5, 1000}) {
        std::vector<uint8_t> out;
        JpegError e;
        const int rc = stream_of(coef, g, p, chunks, &out, &e);
        if (rc != expect) { printf("%s: chunks %d returned %d (%s), expected %d\n", name, chunks, rc, e.text, expect); return false; }
        if (rc != JPEG_OK) continue;
        if (out.size() < 4 || out[0] != 0xFF || out[1] != 0xD8 || out[out.size() - 2] != 0xFF || out[out.size() - 1] != 0xD9) { printf("%s: no SOI / EOI\n", name); return false; }
        if (first.empty()) first = out;
        else if (out != first) { printf("%s: the stream depends on the chunk count (%d)\n", name, chunks); return false; }
    }
    printf("%s: %s\n", name, expect == JPEG_OK ? "coded" : "refused");
    return true;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "encode" && argc == 10) {
        const int w = atoi(argv[2]), h = atoi(argv[3]);
        const JpegEncParams in{atoi(argv[4]), atoi(argv[5]), atoi(argv[6])};
        JpegEncParams p;
        JpegError e;
        if (jpeg_enc_check(w, h, 3, true, &in, &p, &e) != JPEG_OK) { printf("%s\n", e.text); return 2; }
        std::vector<uint8_t> bgr((size_t)w * h * 3);
        FILE* f = fopen(argv[8], "rb");
        if (!f || fread(bgr.data(), 1, bgr.size(), f) != bgr.size()) { printf("cannot read %s\n", argv[8]); return 1; }
        fclose(f);
        const JpegEncGeom g = jpeg_enc_geometry(w, h, p.sampling);
        std::vector<int16_t> coef[3];
        transform(bgr.data(), g, p.quality, coef);
        std::vector<uint8_t> out;
        if (stream_of(coef, g, p, atoi(argv[7]), &out, &e) != JPEG_OK) { printf("%s\n", e.text); return 2; }
        f = fopen(argv[9], "wb");
        if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { printf("cannot write %s\n", argv[9]); return 1; }
        fclose(f);
        printf("%zu\n", out.size());
        return 0;
    }
    if (cmd == "stress") {
        bool ok = true;
        ok &= stress_case("all zero 131x77 4:2:0", 131, 77, JPEG_ENC_420, 0, 0, 0, JPEG_OK);
        ok &= stress_case("largest categories 131x77 4:2:0", 131, 77, JPEG_ENC_420, 0, 1023, -1023, JPEG_OK);     // DC differences of 2046: category 11; AC category 10
        ok &= stress_case("largest categories 47x31 4:4:4 restart 1", 47, 31, JPEG_ENC_444, 1, 1023, 1023, JPEG_OK);
        ok &= stress_case("DC beyond the table", 33, 19, JPEG_ENC_422, 0, 1024, 0, JPEG_INVALID);
        ok &= stress_case("AC beyond the table", 33, 19, JPEG_ENC_422, 0, 0, -1024, JPEG_INVALID);
        ok &= stress_case("int16 extremes", 16, 16, JPEG_ENC_420, 0, 32767, -32768, JPEG_INVALID);
        ok &= stress_case("1x1 4:2:0", 1, 1, JPEG_ENC_420, 0, 5, 0, JPEG_OK);
        ok &= stress_case("1x1 4:4:4 restart 1", 1, 1, JPEG_ENC_444, 1, -7, 1, JPEG_OK);
        ok &= stress_case("restart 1, 64x48 4:2:0", 64, 48, JPEG_ENC_420, 1, 100, 3, JPEG_OK);
        ok &= stress_case("restart 5 across MCU rows, 50x40 4:2:2", 50, 40, JPEG_ENC_422, 5, 100, 0, JPEG_OK);
        ok &= stress_case("restart 65535 (one interval)", 50, 40, JPEG_ENC_420, 65535, 9, 1, JPEG_OK);
        ok &= stress_case("one MCU row, many columns", 3000, 8, JPEG_ENC_444, 0, 300, 255, JPEG_OK);
        if (!ok) return 1;
        printf("stress OK\n");
        return 0;
    }
    printf("usage: %s encode <w> <h> <quality> <sampling> <restart> <chunks> <in.bgr> <out.jpg> | stress\n", argv[0]);
    return 64;
}
