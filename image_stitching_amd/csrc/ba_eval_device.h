// ba_eval_device.h -- the device side of the adjusters that evaluate per observation (BundleAdjusterRay: motion_ray.hip, 3 errors
// per observation; BundleAdjusterAffinePartial: motion_affine.hip, 2).  Both have 4 parameters per camera, so an error row has 8
// non-zero Jacobian entries and an edge 44 sums (ba_ray.h: BA_RAY_JCOLS, BA_RAY_CHAINS, ba_ray_chain); what differs is the
// MODEL (BaRayObsModel, BaAffineObsModel): the record size, the errors per observation and the observation's arithmetic.
//   ba_eval_kernel<MODEL>     one thread per observation over the flat index: its ERRS errors and, in the Jacobian state, its
//                             ERRS x 8 Jacobian entries.  The keypoints are read where the finder left them.
//   ba_normal_kernel<ERRS>    one workgroup per edge, one thread per entry of the edge's 8 x 8 block of J^T J (upper triangle) and
//                             of J^T err: a sequential sum over the edge's ERRS * count rows in ascending order, staged through LDS
// No atomics; every trip count comes from the edge table; one stream synchronisation per evaluation.
#pragma once
#include "ba_ray.h"
#include "common.h"
#include <vector>

namespace {

constexpr int BA_EVAL_THREADS = 256;
constexpr int BA_NORMAL_THREADS = 64;      // 44 chains
constexpr int BA_NORMAL_ROWS = 64;         // rows of J (and err) staged in LDS at a time

// obs_count observations; rec: 9 n records with jac, else n; err: ERRS per observation; jac: ERRS * 8 per observation or nullptr
template <class MODEL>
__global__ __launch_bounds__(BA_EVAL_THREADS) void ba_eval_kernel(const double* __restrict__ rec, int n, const BaRayEdge* __restrict__ edges, const BaRayObs* __restrict__ obs,
                                                                   int obs_count, const MisKeyPoint* const* __restrict__ kps, double* __restrict__ err, double* __restrict__ jac) {
    const int m = blockIdx.x * BA_EVAL_THREADS + threadIdx.x;
    if (m >= obs_count) return;
    const BaRayObs o = obs[m];
    const BaRayEdge e = edges[o.edge];
    const MisKeyPoint* k1 = kps[e.i] + o.q;
    const MisKeyPoint* k2 = kps[e.j] + o.t;
    MODEL::observation(rec, n, e.i, e.j, (double)k1->x, (double)k1->y, (double)k2->x, (double)k2->y, err + (size_t)m * MODEL::ERRS,
                       jac ? jac + (size_t)m * MODEL::ERRS * BA_RAY_JCOLS : nullptr);
}

// block e: the 44 sums of edge e over its ERRS * count rows, rows staged through LDS BA_NORMAL_ROWS at a time.  The trip count is
// the edge table's; every thread of the block takes the same number of steps.
template <int ERRS>
__global__ __launch_bounds__(BA_NORMAL_THREADS) void ba_normal_kernel(const BaRayEdge* __restrict__ edges, const double* __restrict__ jac, const double* __restrict__ err,
                                                                       double* __restrict__ partials) {
    __shared__ double sj[BA_NORMAL_ROWS * BA_RAY_JCOLS];
    __shared__ double se[BA_NORMAL_ROWS];
    const BaRayEdge e = edges[blockIdx.x];
    const int t = threadIdx.x, rows = ERRS * e.count;
    const size_t row0 = (size_t)ERRS * e.first;
    int a = 0, b = 0;
    if (t < BA_RAY_CHAINS) ba_ray_chain(t, &a, &b);
    double s = 0.;
    for (int base = 0; base < rows; base += BA_NORMAL_ROWS) {
        const int cnt = min(BA_NORMAL_ROWS, rows - base);
        for (int q = t; q < cnt * BA_RAY_JCOLS; q += BA_NORMAL_THREADS) sj[q] = jac[(row0 + base) * BA_RAY_JCOLS + q];
        if (t < cnt) se[t] = err[row0 + base + t];
        __syncthreads();
        if (t < BA_RAY_CHAINS)
            for (int k = 0; k < cnt; k++) s = ba_ray_accumulate(s, sj[k * BA_RAY_JCOLS + a], b < 0 ? se[k] : sj[k * BA_RAY_JCOLS + b]);
        __syncthreads();
    }
    if (t < BA_RAY_CHAINS) partials[(size_t)blockIdx.x * BA_RAY_CHAINS + t] = s;
}

// The device side of an evaluation (the `Eval` of ba_ray_solve.h).  One block from the context's pool holds every device array of
// the call and goes back to the pool when the evaluator leaves its scope, on every exit path (after a wait for the stream: a
// kernel may still be reading it).
template <class MODEL>
struct BaDeviceEval {
    static constexpr int REC = MODEL::REC, ERRS = MODEL::ERRS;
    MisContext* ctx = nullptr;
    void* block = nullptr;
    size_t block_bytes = 0;
    int n = 0, ne = 0, total = 0;
    double *d_rec = nullptr, *d_err = nullptr, *d_jac = nullptr, *d_part = nullptr;
    BaRayEdge* d_edges = nullptr;
    BaRayObs* d_obs = nullptr;
    const MisKeyPoint** d_kps = nullptr;
    double *h_rec = nullptr, *h_err = nullptr, *h_part = nullptr;      // pinned
    BaDeviceEval() = default;
    BaDeviceEval(const BaDeviceEval&) = delete;
    BaDeviceEval& operator=(const BaDeviceEval&) = delete;
    ~BaDeviceEval() {
        if (!block) return;
        (void)hipStreamSynchronize(ctx->stream);
        mis_pool_free(ctx, block, block_bytes);
    }
    int prepare(MisContext* c, const MisFeatures* features, int n_, const std::vector<BaRayEdge>& edges, const std::vector<BaRayObs>& obs) {
        ctx = c; n = n_; ne = (int)edges.size(); total = (int)obs.size();
        const size_t rec_b = mis_align_up(sizeof(double) * 9 * n * REC, 256), err_b = mis_align_up(sizeof(double) * ERRS * total, 256),
                     jac_b = mis_align_up(sizeof(double) * ERRS * BA_RAY_JCOLS * total, 256), part_b = mis_align_up(sizeof(double) * BA_RAY_CHAINS * ne, 256),
                     edge_b = mis_align_up(sizeof(BaRayEdge) * ne, 256), obs_b = mis_align_up(sizeof(BaRayObs) * total, 256), kps_b = mis_align_up(sizeof(void*) * n, 256);
        // pinned: [records][err][partials], then the tables on their way up
        const size_t up_b = edge_b + obs_b + kps_b;
        void* hp = nullptr;
        if (int rc = mis_host_stage(ctx, rec_b + err_b + part_b + up_b, &hp)) return rc;
        h_rec = (double*)hp; h_err = (double*)((char*)hp + rec_b); h_part = (double*)((char*)hp + rec_b + err_b);
        char* up = (char*)hp + rec_b + err_b + part_b;
        memcpy(up, edges.data(), sizeof(BaRayEdge) * ne);
        memcpy(up + edge_b, obs.data(), sizeof(BaRayObs) * total);
        for (int i = 0; i < n; i++) ((const MisKeyPoint**)(up + edge_b + obs_b))[i] = features[i].keypoints;
        if (int rc = mis_pool_alloc(ctx, rec_b + err_b + jac_b + part_b + up_b, &block, &block_bytes)) return rc;
        char* d = (char*)block;
        d_rec = (double*)d; d += rec_b;
        d_err = (double*)d; d += err_b;
        d_jac = (double*)d; d += jac_b;
        d_part = (double*)d; d += part_b;
        d_edges = (BaRayEdge*)d; d_obs = (BaRayObs*)(d + edge_b); d_kps = (const MisKeyPoint**)(d + edge_b + obs_b);
        MIS_HIP(ctx, hipMemcpyAsync(d_edges, up, up_b, hipMemcpyHostToDevice, ctx->stream));
        return MIS_OK;
    }
    double* records() { return h_rec; }
    const double* err() const { return h_err; }
    const double* partials() const { return h_part; }
    int run(MisContext*, bool jac) {
        MIS_HIP(ctx, hipMemcpyAsync(d_rec, h_rec, sizeof(double) * (jac ? 9 : 1) * n * REC, hipMemcpyHostToDevice, ctx->stream));
        ba_eval_kernel<MODEL><<<(total + BA_EVAL_THREADS - 1) / BA_EVAL_THREADS, BA_EVAL_THREADS, 0, ctx->stream>>>(d_rec, n, d_edges, d_obs, total, d_kps, d_err, jac ? d_jac : nullptr);
        MIS_HIP(ctx, hipGetLastError());
        if (jac) {
            ba_normal_kernel<ERRS><<<ne, BA_NORMAL_THREADS, 0, ctx->stream>>>(d_edges, d_jac, d_err, d_part);
            MIS_HIP(ctx, hipGetLastError());
            MIS_HIP(ctx, hipMemcpyAsync(h_part, d_part, sizeof(double) * BA_RAY_CHAINS * ne, hipMemcpyDeviceToHost, ctx->stream));
        }
        MIS_HIP(ctx, hipMemcpyAsync(h_err, d_err, sizeof(double) * ERRS * total, hipMemcpyDeviceToHost, ctx->stream));
        MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the one wait of the evaluation
        return MIS_OK;
    }
};

}  // namespace
