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
    int* draw_idx = nullptr;
    int* fin = nullptr;       // per problem: RANSAC phase in which it finished (a RansacPhase), -1 while unfinished
    int2* work = nullptr;     // work list of a RANSAC phase: (problem, first hypothesis) of every block of hypotheses to solve and count
    unsigned* work_ctr = nullptr;  // at offset 0 of mem: list length, tickets taken by the solve / count launches (zero between phases)
};

int homo_batch_reserve(MisContext* ctx, HomoBatch* b, int count, long long points, int max_iters);
int homo_batch_debug_states(MisContext* ctx, const HomoBatch* b, int* out, int cap);
void homo_batch_release(HomoBatch* b);
// The motion model of an estimation.  MODEL_HOMOGRAPHY: cv::findHomography, 4-point subsets (everything above).
// MODEL_AFFINE_PARTIAL: cv::estimateAffinePartial2D, 2-point subsets (calib3d ptsetreg.cpp, restated in homography.hip under
// "the affine-partial model"): the same draw / work list / replay / tail steps with kernels of its own -- a closed-form hypothesis
// solved and counted in one kernel (no Hc, no Jacobi), the replay with bar max(max_good, 1) and exponent 2, a 4-parameter LM tail.
// HomoResult::H then holds [a -b tx; b a ty; 0 0 1].
enum MotionModel { MODEL_HOMOGRAPHY = 0, MODEL_AFFINE_PARTIAL = 1 };
// The RANSAC parameters of an estimation; every entry below validates them (thresh <= 0: the default of 3 pixels).
// refine_iters: LM iterations of the affine-partial tail (0: the RANSAC model itself); the homography's refinement is fixed at 10.
struct HomoParams { double thresh; int max_iters; double confidence; MotionModel model = MODEL_HOMOGRAPHY; int refine_iters = 10; };
// Optional ordering hooks of a batch's phases.  after_first_draw / after_second_draw: recorded behind that phase's draw_kernel.
// Speculative drawing of the second phase's subsets (homography.hip, DRAW_SPEC): given spec_stream, the first phase enqueues it
// there, behind spec_fork (recorded behind its own draw) and in front of spec_join (and of spec_mark, a timing event, when set);
// the second phase queues its draw behind spec_join.
struct HomoHooks {
    hipEvent_t after_first_draw = nullptr, after_second_draw = nullptr;
    hipStream_t spec_stream = nullptr;
    hipEvent_t spec_fork = nullptr, spec_join = nullptr, spec_mark = nullptr;
};
// A phase covers the hypotheses [0, PHASE0) or [PHASE0, max_iters); a problem's tail is the inlier mask with the ordered
// compaction of the inliers, then the DLT + LM refinement on them.
enum RansacPhase { PHASE_FIRST = 0, PHASE_SECOND = 1 };      // (the values of HomoBatch::fin)
enum TailStep { TAIL_MASK, TAIL_REFINE };
// `calls` (device array of b->count entries) must be filled before any of these is enqueued on `stream` (nullptr: the context's).
// homo_solve: the whole estimation -- both phases, each with the tails of the problems that finish in it.
// The matcher splits a batch into chains on several streams instead: homo_phase enqueues one phase -- draw, solves, counts and the
// replay -- and leaves the tails of the problems that end there pending; homo_tails runs one step of the tails pending from
// `phase`, TAIL_MASK before TAIL_REFINE.
int homo_solve(MisContext* ctx, HomoBatch* b, const HomoParams& prm, hipStream_t stream = nullptr, const HomoHooks* hooks = nullptr);
int homo_phase(MisContext* ctx, HomoBatch* b, const HomoParams& prm, RansacPhase phase, hipStream_t stream, const HomoHooks* hooks = nullptr);
int homo_tails(MisContext* ctx, HomoBatch* b, const HomoParams& prm, RansacPhase phase, TailStep step, hipStream_t stream);
