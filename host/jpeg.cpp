// jpeg.cpp -- imread of "<k>.jpg" for the host tools (declared in stitcher.hpp): the files' bytes through mis_jpeg_decode_batch, one
// call for all frames (host entropy decode, device IDCT / upsampling / colour), the pixels back as 8UC3 BGR host images; and imwrite
// of a .jpg (image_stitching.cpp:1228) through mis_jpeg_encode (device colour / DCT / quantisation, host Huffman coding)
#include <fstream>
#include <iterator>
#include <stdexcept>
#include "stitcher.hpp"

namespace mis {

std::vector<HostImage> decodeJPEGBatch(MisContext* ctx, const std::vector<std::string>& paths) {
    const int n = (int)paths.size();
    std::vector<std::vector<char>> bytes(n);
    std::vector<const void*> datas(n);
    std::vector<size_t> sizes(n);
    std::vector<HostImage> out(n);
    std::vector<MisImage> dsts(n);
    for (int i = 0; i < n; i++) {
        std::ifstream f(paths[i], std::ios::binary);
        if (!f) throw std::runtime_error("Can't open image " + paths[i]);
        bytes[i].assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
        datas[i] = bytes[i].data(); sizes[i] = bytes[i].size();
        MisJpegInfo info;
        if (mis_jpeg_info(datas[i], sizes[i], &info) != MIS_OK) throw std::runtime_error(paths[i] + ": " + mis_jpeg_last_error());
        out[i].width = info.width; out[i].height = info.height; out[i].channels = 3;
        out[i].data.resize((size_t)info.width * info.height * 3);
        dsts[i] = MisImage{out[i].data.data(), info.width, info.height, 3, (size_t)info.width * 3, MIS_U8, MIS_MEM_HOST};
    }
    if (n > 0 && mis_jpeg_decode_batch(ctx, datas.data(), sizes.data(), n, dsts.data()) != MIS_OK)
        throw std::runtime_error(std::string("mis_jpeg_decode_batch: ") + mis_last_error(ctx));
    return out;
}

HostImage decodeJPEG(MisContext* ctx, const std::string& path) { return std::move(decodeJPEGBatch(ctx, {path})[0]); }

std::vector<uint8_t> encodeJPEG(MisContext* ctx, const MisImage& bgr, const MisJpegEncodeParams& params) {
    MisJpegStream s{nullptr, 0};
    if (mis_jpeg_encode(ctx, &bgr, &params, &s) != MIS_OK) throw std::runtime_error(std::string("mis_jpeg_encode: ") + mis_last_error(ctx));
    std::vector<uint8_t> out(s.data, s.data + s.bytes);
    mis_jpeg_stream_free(&s);
    return out;
}

std::vector<uint8_t> encodeJPEG(MisContext* ctx, const HostImage& bgr, const MisJpegEncodeParams& params) {
    const MisImage img{const_cast<uint8_t*>(bgr.data.data()), bgr.width, bgr.height, bgr.channels, (size_t)bgr.width * bgr.channels, MIS_U8, MIS_MEM_HOST};
    return encodeJPEG(ctx, img, params);
}

std::vector<std::vector<uint8_t>> encodeJPEGBatch(MisContext* ctx, const std::vector<HostImage>& bgrs, const MisJpegEncodeParams& params) {
    std::vector<MisImage> imgs;
    for (const HostImage& b : bgrs) imgs.push_back(MisImage{const_cast<uint8_t*>(b.data.data()), b.width, b.height, b.channels, (size_t)b.width * b.channels, MIS_U8, MIS_MEM_HOST});
    std::vector<MisJpegStream> streams(imgs.size(), MisJpegStream{nullptr, 0});
    if (imgs.empty()) return {};
    if (mis_jpeg_encode_batch(ctx, imgs.data(), (int)imgs.size(), &params, streams.data()) != MIS_OK) throw std::runtime_error(std::string("mis_jpeg_encode_batch: ") + mis_last_error(ctx));
    std::vector<std::vector<uint8_t>> out;
    for (MisJpegStream& s : streams) {
        out.emplace_back(s.data, s.data + s.bytes);
        mis_jpeg_stream_free(&s);
    }
    return out;
}

void writeJPEG(const std::string& path, MisContext* ctx, const MisImage& bgr, const MisJpegEncodeParams& params) {
    const std::vector<uint8_t> bytes = encodeJPEG(ctx, bgr, params);
    std::ofstream f(path, std::ios::binary);
    f.write((const char*)bytes.data(), (std::streamsize)bytes.size());
    if (!f) throw std::runtime_error("Can't write " + path);
}

void writeJPEG(const std::string& path, MisContext* ctx, const HostImage& bgr, const MisJpegEncodeParams& params) {
    const MisImage img{const_cast<uint8_t*>(bgr.data.data()), bgr.width, bgr.height, bgr.channels, (size_t)bgr.width * bgr.channels, MIS_U8, MIS_MEM_HOST};
    writeJPEG(path, ctx, img, params);
}

}  // namespace mis
