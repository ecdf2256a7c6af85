// homography.h -- internal interface of the batched cv::findHomography(RANSAC) engine (homography.hip).
#pragma once
#include "common.h"

// One findHomography problem: n correspondences src -> dst (f32 x,y pairs), optional inlier mask.
struct HomoCall {
    const float* src;
    const float* dst;
    uint8_t* mask;   // n bytes or null
    long long pt_off;  // offset of this problem's points in the batch-wide scratch arrays
    int n;
    int active;      // 0: skipped (result: ok = 0)
};

struct HomoResult {
    double H[9];
    int ok;
    int iters;   // RANSAC hypotheses evaluated
    int ninl;    // inliers of the best model
    int pad;
};

// Device workspace for a batch of problems (grow-only, owned by the caller).
struct HomoBatch {
    int count = 0;            // problems
    long long points = 0;     // total points over all problems
    int max_iters = 0;
    void* mem = nullptr;
    size_t bytes = 0;
    // carved pointers (device)
    HomoCall* calls = nullptr;
    HomoResult* results = nullptr;
    void* state = nullptr;
    int* sub_idx = nullptr;
    double* Hc = nullptr;
    int* valid = nullptr;
    int* good = nullptr;
    float* scr = nullptr;     // 4 floats per point: compressed inliers
    double* rec = nullptr;    // 10 doubles per point: per-point terms of the DLT / LM sums
    unsigned* draw_next = nullptr;  // per problem: stream-position tables of the subset drawing
    int* draw_idx = nullptr;
    int* fin = nullptr;       // per problem: RANSAC phase in which it finished (0 / 1), -1 while unfinished
    int2* work = nullptr;     // work list of a RANSAC phase: (problem, first hypothesis) of every block of hypotheses to solve and count
    unsigned* work_ctr = nullptr;  // at offset 0 of mem: list length, tickets taken by the solve / count launches (zero between phases)
};

int homo_batch_reserve(MisContext* ctx, HomoBatch* b, int count, long long points, int max_iters);
int homo_batch_debug_states(MisContext* ctx, const HomoBatch* b, int* out, int cap);
void homo_batch_release(HomoBatch* b);
// What one homo_batch_run call enqueues.  The matcher splits a batch into chains on several streams: a replay-only run of a RANSAC
// phase leaves the tails of the problems that end there pending, and the mask / refinement runs finish those of one phase.
enum HomoRun {
    HOMO_BOTH_PHASES = 2,     // hypotheses [0, PHASE0), replay and tails of the problems that finish there, then the same for the rest
    HOMO_PHASE0_REPLAY = 3,   // hypotheses [0, PHASE0) and replay; the finishers' tails are left pending
    HOMO_PHASE1_REPLAY = 6,   // hypotheses [PHASE0, max_iters) and replay; the finishers' tails are left pending
    HOMO_TAIL0_MASK = 10,     // the pending tails of phase w: 10 + 2 w = inlier mask + compaction, 11 + 2 w = DLT + LM refinement
    HOMO_TAIL0_REFINE = 11,
    HOMO_TAIL1_MASK = 12,
    HOMO_TAIL1_REFINE = 13,
};
// `calls` (device array of b->count entries) must be filled before this is enqueued on `stream` (nullptr: the context's stream).
// Optional ordering hooks of a run: rec is recorded behind the draw_kernel of the second phase (rec_pos 0) or of the first (2).
// Speculative drawing of the second phase's subsets (homography.hip, DRAW_SPEC): a HOMO_PHASE0_REPLAY run given spec_stream enqueues
// it there, behind spec_fork (recorded behind the first phase's draw) and in front of spec_join (and of spec_mark, a timing
// event, when set); the HOMO_PHASE1_REPLAY run of the same batch is given spec_join alone and queues its draw behind it.
struct HomoSync {
    hipEvent_t rec = nullptr; int rec_pos = 0;
    hipStream_t spec_stream = nullptr;
    hipEvent_t spec_fork = nullptr, spec_join = nullptr, spec_mark = nullptr;
};
int homo_batch_run(MisContext* ctx, HomoBatch* b, double thresh, int max_iters, double confidence, HomoRun run = HOMO_BOTH_PHASES,
                   hipStream_t stream = nullptr, const HomoSync* sync = nullptr);
