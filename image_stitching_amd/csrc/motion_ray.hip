// motion_ray.hip -- BundleAdjusterRay: the adjuster behind ba_cost_func = "ray"
//   (*adjuster)(features, pairwise_matches, cameras) with BundleAdjusterRay        image_stitching/image_stitching.cpp:683-684
// The solver is the host's (ba_ray_solve.h over motion_host.h: CvLevMarq, the Jacobi SVD solve of the 4n x 4n system); what
// grows with the number of inlier matches runs here, once per evaluation, on the context's stream:
//   ba_ray_eval_kernel     one thread per observation: its 3 errors and, in the Jacobian state, its 3 x 8 Jacobian entries
//   ba_ray_normal_kernel   one workgroup per edge, one thread per entry of the edge's 8 x 8 block of J^T J (upper triangle) and
//                          of J^T err: a sequential sum over the edge's rows in ascending order
// The keypoints are read where the finder left them, in the features' device arrays.  The arithmetic is ba_ray.h's.
#include "ba_ray_solve.h"

namespace {

constexpr int EVAL_THREADS = 256;
constexpr int NORMAL_THREADS = 64;      // 44 chains
constexpr int NORMAL_ROWS = 64;         // rows of J (and err) staged in LDS at a time

// obs_count observations; rec: 9 n records with jac, else n; err: 3 per observation; jac: 24 per observation or nullptr
__global__ __launch_bounds__(EVAL_THREADS) void ba_ray_eval_kernel(const double* __restrict__ rec, int n, const BaRayEdge* __restrict__ edges, const BaRayObs* __restrict__ obs,
                                                                    int obs_count, const MisKeyPoint* const* __restrict__ kps, double* __restrict__ err, double* __restrict__ jac) {
    const int m = blockIdx.x * EVAL_THREADS + threadIdx.x;
    if (m >= obs_count) return;
    const BaRayObs o = obs[m];
    const BaRayEdge e = edges[o.edge];
    const MisKeyPoint* k1 = kps[e.i] + o.q;
    const MisKeyPoint* k2 = kps[e.j] + o.t;
    ba_ray_observation(rec, n, e.i, e.j, (double)k1->x, (double)k1->y, (double)k2->x, (double)k2->y, err + (size_t)m * 3, jac ? jac + (size_t)m * 3 * BA_RAY_JCOLS : nullptr);
}

// block e: the 44 sums of edge e over its 3 count rows, rows staged through LDS NORMAL_ROWS at a time.  The trip count is the
// edge table's; every thread of the block takes the same number of steps.
__global__ __launch_bounds__(NORMAL_THREADS) void ba_ray_normal_kernel(const BaRayEdge* __restrict__ edges, const double* __restrict__ jac, const double* __restrict__ err,
                                                                        double* __restrict__ partials) {
    __shared__ double sj[NORMAL_ROWS * BA_RAY_JCOLS];
    __shared__ double se[NORMAL_ROWS];
    const BaRayEdge e = edges[blockIdx.x];
    const int t = threadIdx.x, rows = 3 * e.count;
    const size_t row0 = (size_t)3 * e.first;
    int a = 0, b = 0;
    if (t < BA_RAY_CHAINS) ba_ray_chain(t, &a, &b);
    double s = 0.;
    for (int base = 0; base < rows; base += NORMAL_ROWS) {
        const int cnt = min(NORMAL_ROWS, rows - base);
        for (int q = t; q < cnt * BA_RAY_JCOLS; q += NORMAL_THREADS) sj[q] = jac[(row0 + base) * BA_RAY_JCOLS + q];
        if (t < cnt) se[t] = err[row0 + base + t];
        __syncthreads();
        if (t < BA_RAY_CHAINS)
            for (int k = 0; k < cnt; k++) s = ba_ray_accumulate(s, sj[k * BA_RAY_JCOLS + a], b < 0 ? se[k] : sj[k * BA_RAY_JCOLS + b]);
        __syncthreads();
    }
    if (t < BA_RAY_CHAINS) partials[(size_t)blockIdx.x * BA_RAY_CHAINS + t] = s;
}

// The device side of an evaluation.  One block from the context's pool holds every device array of the call and goes back to
// the pool when the evaluator leaves its scope, on every exit path (after a wait for the stream: a kernel may still be reading it).
struct DeviceEval {
    MisContext* ctx = nullptr;
    void* block = nullptr;
    size_t block_bytes = 0;
    int n = 0, ne = 0, total = 0;
    double *d_rec = nullptr, *d_err = nullptr, *d_jac = nullptr, *d_part = nullptr;
    BaRayEdge* d_edges = nullptr;
    BaRayObs* d_obs = nullptr;
    const MisKeyPoint** d_kps = nullptr;
    double *h_rec = nullptr, *h_err = nullptr, *h_part = nullptr;      // pinned
    DeviceEval() = default;
    DeviceEval(const DeviceEval&) = delete;
    DeviceEval& operator=(const DeviceEval&) = delete;
    ~DeviceEval() {
        if (!block) return;
        (void)hipStreamSynchronize(ctx->stream);
        mis_pool_free(ctx, block, block_bytes);
    }
    int prepare(MisContext* c, const MisFeatures* features, int n_, const std::vector<BaRayEdge>& edges, const std::vector<BaRayObs>& obs) {
        ctx = c; n = n_; ne = (int)edges.size(); total = (int)obs.size();
        const size_t rec_b = mis_align_up(sizeof(double) * 9 * n * BA_RAY_REC, 256), err_b = mis_align_up(sizeof(double) * 3 * total, 256),
                     jac_b = mis_align_up(sizeof(double) * 3 * BA_RAY_JCOLS * total, 256), part_b = mis_align_up(sizeof(double) * BA_RAY_CHAINS * ne, 256),
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
        MIS_HIP(ctx, hipMemcpyAsync(d_rec, h_rec, sizeof(double) * (jac ? 9 : 1) * n * BA_RAY_REC, hipMemcpyHostToDevice, ctx->stream));
        ba_ray_eval_kernel<<<(total + EVAL_THREADS - 1) / EVAL_THREADS, EVAL_THREADS, 0, ctx->stream>>>(d_rec, n, d_edges, d_obs, total, d_kps, d_err, jac ? d_jac : nullptr);
        MIS_HIP(ctx, hipGetLastError());
        if (jac) {
            ba_ray_normal_kernel<<<ne, NORMAL_THREADS, 0, ctx->stream>>>(d_edges, d_jac, d_err, d_part);
            MIS_HIP(ctx, hipGetLastError());
            MIS_HIP(ctx, hipMemcpyAsync(h_part, d_part, sizeof(double) * BA_RAY_CHAINS * ne, hipMemcpyDeviceToHost, ctx->stream));
        }
        MIS_HIP(ctx, hipMemcpyAsync(h_err, d_err, sizeof(double) * 3 * total, hipMemcpyDeviceToHost, ctx->stream));
        MIS_HIP(ctx, hipStreamSynchronize(ctx->stream));      // the one wait of the evaluation
        return MIS_OK;
    }
};

}  // namespace

extern "C" int mis_bundle_adjust_ray(MisContext* ctx, const MisFeatures* features, const MisMatchesInfo* pairwise, int n, float conf_thresh, MisCameraParams* cameras) {
    if (!ctx) return MIS_E_INVALID;
    MIS_CHECK(ctx, features && pairwise && cameras && n >= 2, MIS_E_INVALID, "null argument or fewer than two cameras");
    MIS_HIP(ctx, hipSetDevice(ctx->device));
    DeviceEval ev;
    return ba_ray_solve(ctx, features, pairwise, n, conf_thresh, cameras, ev);
}
