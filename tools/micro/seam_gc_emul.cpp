// seam_gc_emul.cpp -- the graph-cut seam finder's kernels (csrc/seam_gc.hip) run on the host for one pair, thread by thread in the
// kernels' order, through the very per-node functions the kernels call (csrc/seam_gc_core.h): a round launch sees the heights of
// its start in the halos, pushes over a tile's border wait in the outbox for the absorb pass, the global relabel relaxes tile by
// tile until a sweep changes nothing.  Built and driven by tools/seam_gc_emul.py (with -fsanitize=address,undefined: every plane
// has its exact size, so an index past a plane is caught here and not on a GPU).
//   seam_gc_emul in.bin out.bin K        K: round sets between two global relabels
// in.bin: 12 ints (w1 h1 w2 h2 ox1 oy1 ox2 oy2 gw gh 0 0), 2 floats (terminal_cost, bad_region_penalty), img1, img2, mask1, mask2
// out.bin: 4 ints (round sets, relabels, sweeps, most sweeps of a relabel), the flow (int64), cap_right, cap_down, terminals
// (int32 planes), labels (bytes).  Checks on the way out: no negative excess, drain or residual; flow conserved.
#include "../../image_stitching_amd/csrc/seam_gc_core.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <cstring>

int main(int argc, char** argv) {
    FILE* f = argc == 4 ? fopen(argv[1], "rb") : nullptr;
    int hdr[12]; float costs[2];
    if (argc != 4 || !f || fread(hdr, 4, 12, f) != 12 || fread(costs, 4, 2, f) != 2) { fprintf(stderr, "usage: seam_gc_emul in.bin out.bin K\n"); return 1; }
    GcPair P{};
    P.w1 = hdr[0]; P.h1 = hdr[1]; P.w2 = hdr[2]; P.h2 = hdr[3]; P.ox1 = hdr[4]; P.oy1 = hdr[5]; P.ox2 = hdr[6]; P.oy2 = hdr[7]; P.gw = hdr[8]; P.gh = hdr[9];
    const int K = atoi(argv[3]);
    std::vector<uint8_t> i1((size_t)P.w1 * P.h1 * 3), i2((size_t)P.w2 * P.h2 * 3), m1((size_t)P.w1 * P.h1), m2((size_t)P.w2 * P.h2);
    if (fread(i1.data(), 1, i1.size(), f) != i1.size() || fread(i2.data(), 1, i2.size(), f) != i2.size() || fread(m1.data(), 1, m1.size(), f) != m1.size() || fread(m2.data(), 1, m2.size(), f) != m2.size()) return 1;
    fclose(f);
    P.img1 = i1.data(); P.img2 = i2.data(); P.mask1 = m1.data(); P.mask2 = m2.data();
    P.tiles_x = (P.gw + GC_T - 1) / GC_T; P.tiles_y = (P.gh + GC_T - 1) / GC_T; P.base = 0; P.hmax = P.gw * P.gh + 2;
    const size_t V = (size_t)P.gw * P.gh;
    std::vector<std::vector<int>> pl(13, std::vector<int>(V));   // exact size: ASan sees any overrun
    GcPlanes G;
    for (int d = 0; d < 4; d++) { G.res[d] = pl[d].data(); G.outbox[d] = pl[8 + d].data(); }
    G.excess = pl[4].data(); G.height = pl[5].data(); G.drain = pl[6].data(); G.term = pl[7].data();
    for (int y = 0; y < P.gh; y++) for (int x = 0; x < P.gw; x++) gc_build_node(P, G, costs[0], costs[1], x, y);
    std::vector<int> capR = pl[GC_R], capD = pl[GC_D], term = pl[7];
    std::vector<int> hs(GC_HS * GC_HS), ps(4 * GC_TN);
    std::vector<GcNode> nodes(GC_TN);
    int sets = 0, relabels = 0, sweeps_total = 0, max_sweeps = 0;
    long active = 0;
    for (;;) {
        // global relabel
        for (size_t k = 0; k < V; k++) G.height[k] = G.drain[k] > 0 ? 1 : P.hmax;
        int sweeps = 0;
        for (;;) {
            int changed = 0;
            for (int ty = 0; ty < P.tiles_y; ty++) for (int tx = 0; tx < P.tiles_x; tx++) {
                const int tx0 = tx * GC_T, ty0 = ty * GC_T;
                for (int i = 0; i < GC_HS * GC_HS; i++) gc_load_height(P, G, tx0, ty0, i, hs.data());
                std::vector<int> h0(GC_TN), h(GC_TN), nh(GC_TN);
                for (int t = 0; t < GC_TN; t++) { gc_node_load(P, G, tx0 + t % GC_T, ty0 + t / GC_T, nodes[t]); h0[t] = h[t] = hs[gc_hs_at(t % GC_T, t / GC_T)]; }
                for (int it = 0; it < GC_TN; it++) {
                    int any = 0;
                    for (int t = 0; t < GC_TN; t++) { nh[t] = nodes[t].in ? gc_relax(nodes[t].r, h[t], hs.data(), t % GC_T, t / GC_T) : h[t]; any |= nh[t] < h[t]; }
                    if (!any) break;
                    for (int t = 0; t < GC_TN; t++) { h[t] = nh[t]; hs[gc_hs_at(t % GC_T, t / GC_T)] = h[t]; }
                }
                // NOTE: emulating tiles one after another lets a later tile see an earlier tile's result of the same sweep
                // (the device sees last sweep's): convergence differs, the fixpoint does not
                for (int t = 0; t < GC_TN; t++) if (nodes[t].in && h[t] != h0[t]) { G.height[(size_t)(ty0 + t / GC_T) * P.gw + tx0 + t % GC_T] = h[t]; changed = 1; }
            }
            sweeps++;
            if (!changed) break;
        }
        relabels++; sweeps_total += sweeps; if (sweeps > max_sweeps) max_sweeps = sweeps;
        active = 0;
        for (size_t k = 0; k < V; k++) active += G.excess[k] > 0 && G.height[k] < P.hmax;
        if (!active) break;
        if (sets > 100000) { fprintf(stderr, "no convergence\n"); return 2; }
        for (int s = 0; s < K; s++) {
            // round kernel: every tile against the heights of the launch (snapshot)
            std::vector<int> hsnap(G.height, G.height + V);
            for (int ty = 0; ty < P.tiles_y; ty++) for (int tx = 0; tx < P.tiles_x; tx++) {
                const int tx0 = tx * GC_T, ty0 = ty * GC_T;
                GcPlanes S = G; S.height = hsnap.data();
                for (int i = 0; i < GC_HS * GC_HS; i++) gc_load_height(P, S, tx0, ty0, i, hs.data());
                for (int t = 0; t < GC_TN; t++) gc_node_load(P, S, tx0 + t % GC_T, ty0 + t / GC_T, nodes[t]);
                for (int r = 0; r < GC_INNER; r++) {
                    for (int t = 0; t < GC_TN; t++) gc_push(nodes[t], hs.data(), ps.data(), t % GC_T, t / GC_T, P.hmax);
                    for (int t = 0; t < GC_TN; t++) gc_absorb_relabel(nodes[t], hs.data(), ps.data(), t % GC_T, t / GC_T, P.hmax);
                    for (int t = 0; t < GC_TN; t++) hs[gc_hs_at(t % GC_T, t / GC_T)] = nodes[t].h;
                }
                for (int t = 0; t < GC_TN; t++) gc_node_store(P, G, tx0 + t % GC_T, ty0 + t / GC_T, nodes[t]);
            }
            for (int y = 0; y < P.gh; y++) for (int x = 0; x < P.gw; x++) gc_border_absorb(P, G, x, y);
            sets++;
        }
    }
    // invariants: conservation
    long long tot_e = 0, tot_drained = 0, tot_src = 0;
    for (size_t k = 0; k < V; k++) { tot_e += G.excess[k]; if (term[k] > 0) tot_drained += term[k] - G.drain[k]; else tot_src += -term[k]; if (G.excess[k] < 0 || G.drain[k] < 0) { fprintf(stderr, "negative state\n"); return 3; } for (int d = 0; d < 4; d++) if (G.res[d][k] < 0) { fprintf(stderr, "negative residual\n"); return 3; } }
    if (tot_e + tot_drained != tot_src) { fprintf(stderr, "flow not conserved\n"); return 4; }
    f = fopen(argv[2], "wb");
    int stats[4] = {sets, relabels, sweeps_total, max_sweeps};
    long long flow = tot_drained;
    fwrite(stats, 4, 4, f); fwrite(&flow, 8, 1, f);
    fwrite(capR.data(), 4, V, f); fwrite(capD.data(), 4, V, f); fwrite(term.data(), 4, V, f);
    std::vector<uint8_t> lab(V);
    for (size_t k = 0; k < V; k++) lab[k] = G.height[k] < P.hmax;
    fwrite(lab.data(), 1, V, f);
    fclose(f);
    return 0;
}
