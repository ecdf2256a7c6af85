// jpeg_host_harness.cpp -- the JPEG decode's host layer (image_stitching_amd/csrc/jpeg_host.h) and the host twin of its device
// arithmetic (jpeg_core.h: the functions the kernels of jpeg.hip call, compiled here by the host compiler) as a program of its own.
//
//   jpeg_host_harness decode <in.jpg> <out.bgr>     the whole decode on the CPU; prints "<width> <height>", writes packed BGR rows
//   jpeg_host_harness idct <in.i32> <out.u8>        jpeg_idct_block over raw blocks of 64 dequantised int32 coefficients (natural
//        order) -> 64 samples per block, row by row: the 32-bit IDCT by itself, for blocks no stream of the fixtures holds
//   jpeg_host_harness fuzz <seed> <count> <in.jpg>...
//        every file whole, every proper prefix of it and <count> seeded single-byte corruptions of it through the same decode;
//        prints the outcome counts per file.  A prefix that decodes is an error (exit 1).  Built with -fsanitize=address,undefined
//        this is the memory-safety check of the parser: it reads untrusted bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>
#include "../../image_stitching_amd/csrc/jpeg_host.h"

static int decode(const uint8_t* d, size_t n, std::vector<uint8_t>* bgr, int* w, int* h, JpegError* e) {
    JpegHeader H;
    std::vector<JpegSegment> segs;
    if (int rc = jpeg_parse(d, n, &H, e)) return rc;
    if (int rc = jpeg_segments(d, n, H, &segs, e)) return rc;
    std::vector<std::vector<int16_t>> coef(H.ncomp);
    int16_t* planes[3] = {nullptr, nullptr, nullptr};
    for (int c = 0; c < H.ncomp; c++) { coef[c].resize(H.blocks(c) * 64); planes[c] = coef[c].data(); }
    if (int rc = jpeg_entropy(d, H, segs, 0, segs.size(), planes, e)) return rc;
    // what jpeg_idct_kernel does per block
    std::vector<std::vector<uint8_t>> pix(H.ncomp);
    size_t stride[3] = {0, 0, 0};
    for (int c = 0; c < H.ncomp; c++) {
        stride[c] = (size_t)H.bw[c] * 8;
        pix[c].resize(stride[c] * H.bh[c] * 8);
        const uint16_t* q = H.q[H.tq[c]];
        for (size_t b = 0; b < H.blocks(c); b++) {
            uint32_t ws[64], row[8][2];
            for (int k = 0; k < 64; k++) ws[k] = (uint32_t)((int)planes[c][b * 64 + k] * (int)q[k]);
            jpeg_idct_block(ws, row);
            const size_t by = b / H.bw[c], bx = b % H.bw[c];
            for (int y = 0; y < 8; y++)
                for (int x = 0; x < 8; x++) pix[c][(by * 8 + y) * stride[c] + bx * 8 + x] = (uint8_t)(row[y][x >> 2] >> (8 * (x & 3)));
        }
    }
    // what jpeg_color_kernel does per tile of 8 x 2 pixels: the h2v2 rule through jpeg_h2v2_tile, the other rules pixel by pixel.  The
    // tile function must give what the per-pixel function gives wherever a pixel is stored: -2 if it ever does not.
    *w = H.width; *h = H.height;
    bgr->resize((size_t)H.width * H.height * 3);
    for (int y0 = 0; y0 < H.height; y0 += 2)
        for (int x0 = 0; x0 < H.width; x0 += 8) {
            int cb[2][8] = {{0}}, cr[2][8] = {{0}};
            if (H.ncomp == 3 && H.rule == JPEG_UP_H2V2) {
                jpeg_h2v2_tile(pix[1].data(), stride[1], H.cw, H.ch, x0, y0, cb);
                jpeg_h2v2_tile(pix[2].data(), stride[2], H.cw, H.ch, x0, y0, cr);
            }
            for (int r = 0; r < 2 && y0 + r < H.height; r++)
                for (int k = 0; k < 8 && x0 + k < H.width; k++) {
                    const int x = x0 + k, y = y0 + r, yy = pix[0][(size_t)y * stride[0] + x];
                    uint32_t px = (uint32_t)yy * 0x010101u;
                    if (H.ncomp == 3) {
                        const int b1 = jpeg_upsample_at(pix[1].data(), stride[1], H.cw, H.ch, H.rule, x, y);
                        const int r1 = jpeg_upsample_at(pix[2].data(), stride[2], H.cw, H.ch, H.rule, x, y);
                        if (H.rule == JPEG_UP_H2V2 && (b1 != cb[r][k] || r1 != cr[r][k])) return jpeg_fail(e, -2, "harness: jpeg_h2v2_tile differs from jpeg_upsample_at at (%d, %d)", x, y);
                        px = jpeg_ycc_to_bgr(yy, b1, r1);
                    }
                    uint8_t* o = bgr->data() + ((size_t)y * H.width + x) * 3;
                    o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16);
                }
        }
    return JPEG_OK;
}

static bool read_file(const char* path, std::vector<uint8_t>* out) {
    FILE* f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + got);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "decode" && argc == 4) {
        std::vector<uint8_t> d, bgr;
        if (!read_file(argv[2], &d)) { printf("can't read %s\n", argv[2]); return 2; }
        int w = 0, h = 0;
        JpegError e;
        if (decode(d.data(), d.size(), &bgr, &w, &h, &e) != JPEG_OK) { printf("refused (%d): %s\n", e.code, e.text); return 3; }
        FILE* f = fopen(argv[3], "wb");
        if (!f || fwrite(bgr.data(), 1, bgr.size(), f) != bgr.size()) { printf("can't write %s\n", argv[3]); return 2; }
        fclose(f);
        printf("%d %d\n", w, h);
        return 0;
    }
    if (mode == "idct" && argc == 4) {
        std::vector<uint8_t> d;
        if (!read_file(argv[2], &d) || d.size() % 256) { printf("can't read blocks from %s\n", argv[2]); return 2; }
        std::vector<uint8_t> out(d.size() / 4);
        for (size_t b = 0; b < d.size() / 256; b++) {
            uint32_t ws[64], row[8][2];
            for (int k = 0; k < 64; k++) {
                int32_t c;
                memcpy(&c, d.data() + b * 256 + 4 * k, 4);
                ws[k] = (uint32_t)c;
            }
            jpeg_idct_block(ws, row);
            for (int k = 0; k < 64; k++) out[b * 64 + k] = (uint8_t)(row[k >> 3][(k >> 2) & 1] >> (8 * (k & 3)));
        }
        FILE* f = fopen(argv[3], "wb");
        if (!f || fwrite(out.data(), 1, out.size(), f) != out.size()) { printf("can't write %s\n", argv[3]); return 2; }
        fclose(f);
        return 0;
    }
    if (mode == "fuzz" && argc >= 5) {
        uint64_t state = strtoull(argv[2], nullptr, 10) * 2 + 1;
        const long count = strtol(argv[3], nullptr, 10);
        auto rnd = [&]() { state = state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(state >> 33); };
        int bad = 0;
        for (int a = 4; a < argc; a++) {
            std::vector<uint8_t> d, bgr;
            if (!read_file(argv[a], &d)) { printf("can't read %s\n", argv[a]); return 2; }
            int w = 0, h = 0;
            JpegError e;
            const int whole = decode(d.data(), d.size(), &bgr, &w, &h, &e);
            long pre[3] = {0, 0, 0}, cor[3] = {0, 0, 0};        // ok, invalid, unsupported
            int twin = 0;       // -2 seen: the tile function and the per-pixel function disagreed
            auto slot = [&](int rc) { if (rc == -2) twin = 1; return rc == JPEG_OK ? 0 : (rc == JPEG_INVALID ? 1 : 2); };
            for (size_t n = 0; n < d.size(); n++) {
                // (a copy of exactly n bytes: a read past the prefix is a read past the allocation)
                std::vector<uint8_t> p(d.begin(), d.begin() + n);
                pre[slot(decode(p.data(), p.size(), &bgr, &w, &h, &e))]++;
            }
            for (long k = 0; k < count; k++) {
                std::vector<uint8_t> p(d);
                p[rnd() % p.size()] = (uint8_t)rnd();
                cor[slot(decode(p.data(), p.size(), &bgr, &w, &h, &e))]++;
            }
            printf("%s whole %d prefixes ok %ld invalid %ld unsupported %ld corruptions ok %ld invalid %ld unsupported %ld\n", argv[a], whole, pre[0], pre[1], pre[2],
                   cor[0], cor[1], cor[2]);
            if (pre[0] || twin || whole == -2) bad = 1;
        }
        return bad;
    }
    printf("usage: %s decode <in.jpg> <out.bgr> | idct <in.i32> <out.u8> | fuzz <seed> <count> <in.jpg>...\n", argv[0]);
    return 2;
}
