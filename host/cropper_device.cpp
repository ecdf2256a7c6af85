// cropper_device.cpp -- the device forms of mis::crop (cropper.hpp) over mis_crop_rect / mis_crop (csrc/crop.hip)
#include "cropper.hpp"
#include <hip/hip_runtime_api.h>
#include <stdexcept>
#include <string>

namespace mis {

namespace {
Rect finish(MisContext* ctx, int rc, const int rect[4], int status) {
    if (rc != MIS_OK) throw std::runtime_error(std::string("mis_crop failed: ") + mis_last_error(ctx));
    if (status == 1) throw std::runtime_error("crop: the image is empty");
    if (status == 2) throw std::runtime_error("crop: no interior rectangle found");
    return Rect{rect[0], rect[1], rect[2], rect[3]};
}
void must_be_device_u8(const MisImage& img) {
    if (img.mem != MIS_MEM_DEVICE || img.dtype != MIS_U8) throw std::runtime_error("crop: an 8-bit image in device memory expected");
}
struct DeviceBuffer {
    void* p = nullptr;
    explicit DeviceBuffer(size_t bytes) { if (hipMalloc(&p, bytes) != hipSuccess) throw std::runtime_error("crop: hipMalloc failed"); }
    ~DeviceBuffer() { if (p) (void)hipFree(p); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
};
}  // namespace

Rect cropRectDevice(MisContext* ctx, const MisImage& src) {
    must_be_device_u8(src);
    int rect[4] = {0, 0, 0, 0}, status = 0;
    const int rc = mis_crop_rect(ctx, src.data, src.width, src.height, src.channels, src.stride, rect, &status);
    return finish(ctx, rc, rect, status);
}

Rect cropDevice(MisContext* ctx, const MisImage& src, MisImage* dst) {
    must_be_device_u8(src);
    if (!dst) throw std::runtime_error("crop: null output");
    must_be_device_u8(*dst);
    if (dst->height < src.height) throw std::runtime_error("crop: the output buffer needs the source's rows");
    int rect[4] = {0, 0, 0, 0}, status = 0;
    const int rc = mis_crop(ctx, src.data, src.width, src.height, src.channels, src.stride, dst->data, dst->stride, rect, &status);
    const Rect r = finish(ctx, rc, rect, status);
    dst->width = r.width; dst->height = r.height; dst->channels = src.channels;
    return r;
}

Rect cropDevice(MisContext* ctx, HostImage& source) {
    if (source.channels != 3 && source.channels != 1) throw std::runtime_error("crop: 8UC3 or 8UC1 image expected");
    if (source.width <= 0 || source.height <= 0) throw std::runtime_error("crop: the image is empty");
    const size_t row = (size_t)source.width * source.channels, bytes = row * source.height;
    DeviceBuffer in(bytes), out(bytes);
    if (hipMemcpy(in.p, source.data.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("crop: upload failed");
    const MisImage src{in.p, source.width, source.height, source.channels, row, MIS_U8, MIS_MEM_DEVICE};
    MisImage dst{out.p, source.width, source.height, source.channels, row, MIS_U8, MIS_MEM_DEVICE};
    const Rect r = cropDevice(ctx, src, &dst);
    HostImage res;
    res.width = r.width; res.height = r.height; res.channels = source.channels;
    res.data.resize((size_t)r.width * r.height * source.channels);
    if (hipMemcpy2D(res.data.data(), (size_t)r.width * source.channels, out.p, row, (size_t)r.width * source.channels, r.height, hipMemcpyDeviceToHost) != hipSuccess)
        throw std::runtime_error("crop: download failed");
    source = std::move(res);
    return r;
}

}  // namespace mis
