// knn_plan_harness.cpp -- the capacity plan of the matcher's 2-NN pass (image_stitching_amd/csrc/knn_plan.h) as a shared object for
// tests/test_knn_plan_cpu.py.  Plain C++, no HIP.
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#include "../../image_stitching_amd/csrc/knn_plan.h"

static KnnCapPlan g_plan;

// plans; returns the number of pairs.  *njobs: length of the workgroup table; *knn_total: queries in idx / dist; *xp_bytes: expanded forms
extern "C" int harness_plan(int n, const int* caps, const uint8_t* mask, int range_width, int rank, int world, int* njobs, long long* knn_total, long long* xp_bytes) {
    plan_knn_capacity(n, caps, mask, range_width, rank, world, &g_plan);
    *njobs = (int)g_plan.jobs.size();
    *knn_total = (long long)g_plan.knn_total;
    *xp_bytes = (long long)g_plan.xp_bytes;
    return (int)g_plan.pairs.size();
}
// pairs: (i, j, knn_off12, knn_off21) each; frames: (train_off, query_off) each; jobs: (pair, dir, q0, pad) each
extern "C" void harness_tables(long long* pairs, long long* frames, int* jobs) {
    for (size_t k = 0; k < g_plan.pairs.size(); k++) {
        const PairDesc& p = g_plan.pairs[k];
        pairs[4 * k] = p.i; pairs[4 * k + 1] = p.j; pairs[4 * k + 2] = (long long)p.knn_off12; pairs[4 * k + 3] = (long long)p.knn_off21;
    }
    for (size_t f = 0; f < g_plan.frames.size(); f++) { frames[2 * f] = (long long)g_plan.frames[f].train_off; frames[2 * f + 1] = (long long)g_plan.frames[f].query_off; }
    for (size_t q = 0; q < g_plan.jobs.size(); q++) { jobs[4 * q] = g_plan.jobs[q].pair; jobs[4 * q + 1] = g_plan.jobs[q].dir; jobs[4 * q + 2] = g_plan.jobs[q].q0; jobs[4 * q + 3] = g_plan.jobs[q].pad; }
}
extern "C" int harness_rowpad() { return HM_ROWPAD; }
