// seam_stage.h -- what the seam finders that look at the images (seam.hip, seam_gc.hip) share on their way in and out: the input
// contract, the packed device block of images and masks, and the copy of one frame into and out of its slot.  Which frames are
// gathered, and whether the block then crosses to the host, is each finder's own business.
#pragma once
#include "common.h"
#include "seam_plan.h"

// corners + the frames' sizes (images, or masks of the same size) as the pair plan takes them
inline std::vector<SeamFrame> seam_frames(const MisPoint* corners, const MisImage* sized, int n) {
    std::vector<SeamFrame> f((size_t)n);
    for (int i = 0; i < n; i++) f[i] = SeamFrame{corners[i].x, corners[i].y, sized[i].width, sized[i].height};
    return f;
}

// image i is 8UC3, mask i is 8U of the same size, both non-empty
inline int seam_check_input(MisContext* ctx, const MisImage& I, const MisImage& M, int i) {
    MIS_CHECK(ctx, I.data && M.data && I.dtype == MIS_U8 && I.channels == 3 && M.dtype == MIS_U8 && M.channels == 1 && I.width == M.width && I.height == M.height &&
                       I.width > 0 && I.height > 0, MIS_E_INVALID, "image %d: need an 8UC3 image and an 8U mask of the same size", i);
    return MIS_OK;
}

// The packed block: per frame an image slot and a mask slot of dense rows, each 256-byte aligned; `bytes` is where a finder's own
// regions may follow.
struct SeamSlots {
    std::vector<size_t> ioff, moff;
    size_t bytes = 0;
    SeamSlots(const MisImage* images, int n) : ioff((size_t)n), moff((size_t)n) {
        for (int i = 0; i < n; i++) {
            ioff[i] = bytes; bytes += mis_align_up((size_t)images[i].width * images[i].height * 3, 256);
            moff[i] = bytes; bytes += mis_align_up((size_t)images[i].width * images[i].height, 256);
        }
    }
};

// a caller's 8-bit image or mask, device or host, into its slot of the device block / a mask slot back to the caller's mask
inline hipError_t seam_gather(void* slot, const MisImage& src, hipStream_t stream) {
    const size_t row = (size_t)src.width * src.channels;
    return hipMemcpy2DAsync(slot, row, src.data, src.stride, row, src.height, src.mem == MIS_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream);
}
inline hipError_t seam_scatter(const MisImage& dst, const void* slot, hipStream_t stream) {
    const size_t row = (size_t)dst.width * dst.channels;
    return hipMemcpy2DAsync(dst.data, dst.stride, slot, row, row, dst.height, dst.mem == MIS_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream);
}
