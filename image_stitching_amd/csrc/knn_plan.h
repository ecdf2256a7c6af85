// knn_plan.h -- host-side layout of the matcher's 2-NN pass: the pair selection, the directed pairs' slots in the idx / dist
// arrays, the frames' expanded descriptor blocks and the workgroup table of the Hamming pass on the matrix cores.  Plain C++,
// no device code (tests/harness/knn_plan_harness.cpp compiles it on its own).
//
// No includes and no namespace of its own: match.hip includes it INSIDE its unnamed namespace, so that the kernels' parameter
// types -- and with them the kernels' symbols -- stay what they were.  The including file provides <stddef.h>, <stdint.h>,
// <algorithm> and <vector> first.

struct PairDesc {
    int i, j;            // image indices, i < j
    size_t knn_off12, knn_off21;  // offsets (in queries) into idx2 / dist2
    size_t m_off;        // offset into the per-pair match / point / mask arrays
    int cap;             // n_i + n_j
};

constexpr int HM_ROWPAD = 256;         // expanded blocks are padded with zero rows to a multiple of this
constexpr int HM_MAX_TRAINS = 8192;

struct HmFrame { size_t train_off, query_off; };   // byte offsets of a frame's two expanded forms

// One workgroup of the pass: 256 queries of a directed pair against all trains.  The table is ordered so that workgroup L runs on
// XCD L mod 8 (the dispatcher deals workgroups round-robin over the eight XCDs) and every XCD only ever sees the TRAIN sets of
// the frames t with t mod 8 = its number: two frames of a 16-frame job, 2 MB of expanded descriptors, resident in its 4 MB L2
// (with the (query block, pair) grid every XCD walked all 16 MB and every tile was a miss to the fabric: the tile loads' latency,
// not the matrix pipe, paced the loop).
struct HmJob { int pair, dir, q0, pad; };

// FeaturesMatcher::operator(): the mask (strict upper triangle, NULL: all) and BestOf2NearestRangeMatcher's range_width
// (-1: all, else j < i + range_width)
inline bool knn_pair_selected(int i, int j, int n, const uint8_t* mask, int range_width) {
    if (mask && !mask[(size_t)i * n + j]) return false;
    return range_width == -1 || j < i + range_width;
}

// The workgroup table for `pairs` over n frames of which frame f has (at most) nq[f] keypoints: eight lists by train frame mod 8,
// interleaved, padded with pair = -1 to a multiple of 8.  A query block past a frame's real count leaves at once (the kernel
// compares q0 with the count on the device), so nq may be a capacity.
inline void hm_job_table(const std::vector<PairDesc>& pairs, int n, const int* nq, std::vector<HmJob>* jobs) {
    const int np = (int)pairs.size();
    std::vector<HmJob> lists[8];
    for (int t = 0; t < n; t++)
        for (int k = 0; k < np; k++) {
            const int dir = pairs[k].j == t ? 0 : (pairs[k].i == t ? 1 : -1);      // direction 0: queries of i against the trains of j
            if (dir < 0) continue;
            const int nqf = nq[dir == 0 ? pairs[k].i : pairs[k].j];
            for (int q0 = 0; q0 < nqf; q0 += 256) lists[t & 7].push_back(HmJob{k, dir, q0, 0});
        }
    size_t longest = 0;
    for (auto& l : lists) longest = std::max(longest, l.size());
    jobs->assign(longest * 8, HmJob{-1, 0, 0, 0});
    for (int c = 0; c < 8; c++)
        for (size_t sl = 0; sl < lists[c].size(); sl++) (*jobs)[sl * 8 + c] = lists[c][sl];
}

// The 2-NN pass planned from the feature blocks' CAPACITIES, for a batch whose keypoint counts are still on the device only
// (mis_knn_ahead_enqueue): every selected i < j is a pair -- an empty frame cannot be skipped, its workgroups leave at once --,
// a directed pair's slot holds the query frame's capacity padded to HM_ROWPAD, and a frame's expanded forms hold its padded
// capacity in rows of 128 bytes (from offset 0, xp_bytes in all: every block is a multiple of 256 bytes).
struct KnnCapPlan {
    std::vector<PairDesc> pairs;       // knn_off12 / knn_off21 only (m_off and cap follow from the counts: the matcher call's)
    std::vector<HmFrame> frames;
    std::vector<HmJob> jobs;
    size_t knn_total = 0, xp_bytes = 0;
};
inline size_t knn_rows_padded(int n) { return (size_t)(std::max(n, 1) + HM_ROWPAD - 1) / HM_ROWPAD * HM_ROWPAD; }
inline void plan_knn_capacity(int n, const int* caps, const uint8_t* mask, int range_width, int rank, int world, KnnCapPlan* pl) {
    pl->pairs.clear(); pl->knn_total = 0;
    int pair_index = 0;
    for (int i = 0; i < n; i++)
        for (int j = i + 1; j < n; j++) {
            if (!knn_pair_selected(i, j, n, mask, range_width)) continue;
            if ((pair_index++ % world) != rank) continue;
            const size_t qi = knn_rows_padded(caps[i]), qj = knn_rows_padded(caps[j]);
            pl->pairs.push_back(PairDesc{i, j, pl->knn_total, pl->knn_total + qi, 0, 0});
            pl->knn_total += qi + qj;
        }
    pl->frames.resize(n);
    size_t off = 0;
    for (int i = 0; i < n; i++) {
        const size_t bytes = knn_rows_padded(caps[i]) * 128;
        pl->frames[i].train_off = off; off += bytes;
        pl->frames[i].query_off = off; off += bytes;
    }
    pl->xp_bytes = off;
    hm_job_table(pl->pairs, n, caps, &pl->jobs);
}
