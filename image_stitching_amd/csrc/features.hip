// features.hip -- device blocks of feature sets (MisFeatures), whichever finder fills them, and their transfers.
//
// A feature set owns one device block taken from its context's pool of recycled blocks (a hipMalloc / hipFree pair per frame
// would synchronise the whole device).  The registry below remembers what the pool gave for every live block, so that
// mis_features_free can hand it back without a synchronisation.
#include "common.h"
#include <algorithm>
#include <mutex>
#include <unordered_map>

namespace {

std::mutex g_feat_mutex;
std::unordered_map<void*, size_t> g_feat_sizes;  // block sizes of live feature sets (for the pool)

}  // namespace

MisFeatLayout mis_feat_layout(int cap, int desc_cols, int desc_dtype) {
    MisFeatLayout l;
    l.desc_off = mis_align_up(sizeof(MisKeyPoint) * (size_t)cap, 256);
    l.count_off = l.desc_off + mis_align_up((size_t)cap * desc_cols * mis_dtype_size(desc_dtype), 256);
    l.bytes = l.count_off + 256;
    return l;
}

int mis_feat_block_alloc(MisContext* ctx, size_t bytes, void** out, MisContext* errs) {
    size_t got = 0;
    const int rc = mis_pool_alloc(ctx, bytes, out, &got, errs);
    if (rc != MIS_OK) return rc;
    std::lock_guard<std::mutex> lock(g_feat_mutex);
    g_feat_sizes[*out] = got;
    return MIS_OK;
}

int mis_feat_alloc(MisContext* ctx, int cap, int desc_cols, int desc_dtype, MisFeatures* f) {
    const MisFeatLayout l = mis_feat_layout(cap, desc_cols, desc_dtype);
    void* mem = nullptr;
    const int rc = mis_feat_block_alloc(ctx, l.bytes, &mem);
    if (rc != MIS_OK) return rc;
    f->keypoints = (MisKeyPoint*)mem;
    f->descriptors = (uint8_t*)mem + l.desc_off;
    f->desc_cols = desc_cols; f->desc_dtype = desc_dtype;
    f->owner_ = mem;
    f->n = 0;
    return MIS_OK;
}

int* mis_feat_count(const MisFeatures* f, int cap) {
    return (int*)((uint8_t*)f->owner_ + mis_feat_layout(cap, f->desc_cols, f->desc_dtype).count_off);
}

extern "C" int mis_features_download(MisContext* ctx, const MisFeatures* f, MisKeyPoint* kps, void* desc) {
    if (!ctx || !f) return MIS_E_INVALID;
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    if (f->n > 0) {
        if (kps) MIS_HIP(ctx, hipMemcpyAsync(kps, f->keypoints, sizeof(MisKeyPoint) * (size_t)f->n, hipMemcpyDeviceToHost, ctx->stream));
        if (desc) MIS_HIP(ctx, hipMemcpyAsync(desc, f->descriptors, (size_t)f->n * f->desc_cols * mis_dtype_size(f->desc_dtype), hipMemcpyDeviceToHost, ctx->stream));
    }
    MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MIS_OK;
}

extern "C" int mis_features_upload(MisContext* ctx, int img_w, int img_h, int n, const MisKeyPoint* kps, const void* desc, int desc_cols,
                                   int desc_dtype, MisFeatures* out) {
    if (!ctx || !out) return MIS_E_INVALID;
    MIS_CHECK(ctx, n >= 0 && (n == 0 || (kps && desc)) && desc_cols > 0 && (desc_dtype == MIS_U8 || desc_dtype == MIS_F32), MIS_E_INVALID,
              "bad feature arrays");
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    memset(out, 0, sizeof(*out));
    out->img_w = img_w; out->img_h = img_h;
    int rc = mis_feat_alloc(ctx, std::max(n, 1), desc_cols, desc_dtype, out);
    if (rc != MIS_OK) return rc;
    if (n) {
        MIS_HIP(ctx, hipMemcpyAsync(out->keypoints, kps, sizeof(MisKeyPoint) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        MIS_HIP(ctx, hipMemcpyAsync(out->descriptors, desc, (size_t)n * desc_cols * mis_dtype_size(desc_dtype), hipMemcpyHostToDevice, ctx->stream));
        MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    out->n = n;
    return MIS_OK;
}

extern "C" int mis_features_free(MisContext* ctx, MisFeatures* f) {
    if (!ctx || !f) return MIS_E_INVALID;
    if (f->owner_) {
        mis_knn_ahead_drop(ctx, f->owner_);      // (the block may come back from the pool for another feature set)
        size_t bytes = 0;
        {
            std::lock_guard<std::mutex> lock(g_feat_mutex);
            auto it = g_feat_sizes.find(f->owner_);
            if (it != g_feat_sizes.end()) { bytes = it->second; g_feat_sizes.erase(it); }
        }
        if (bytes) mis_pool_free(ctx, f->owner_, bytes);  // recycled without synchronising the device
        else {
            MIS_HIP(ctx, hipSetDevice(ctx->device));
            MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));
            MIS_HIP(ctx, hipFree(f->owner_));
        }
    }
    f->owner_ = nullptr; f->keypoints = nullptr; f->descriptors = nullptr; f->n = 0;
    return MIS_OK;
}
