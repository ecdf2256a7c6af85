// seam_plan_dump.cpp -- the seam finders' pair plan (csrc/seam_plan.h) on the host, for tests/test_seam_plan_cpu.py.
// stdin: any number of layouts, each "order n" (order: run | distance) followed by n frames "x y w h".
// stdout: per layout "plan <pairs> <levels>", then a line "i j level x0 y0 x1 y1" per pair in processing order.
#include "../../image_stitching_amd/csrc/seam_plan.h"
#include <cstdio>
#include <cstring>

int main() {
    char order[16];
    int n;
    while (scanf("%15s %d", order, &n) == 2) {
        if (n < 0 || (strcmp(order, "run") != 0 && strcmp(order, "distance") != 0)) { fprintf(stderr, "bad layout header: %s %d\n", order, n); return 2; }
        std::vector<SeamFrame> f((size_t)n);
        for (SeamFrame& s : f)
            if (scanf("%d %d %d %d", &s.x, &s.y, &s.w, &s.h) != 4) { fprintf(stderr, "truncated layout\n"); return 2; }
        const SeamPlan plan = seam_plan(f, strcmp(order, "run") == 0 ? SEAM_ORDER_RUN : SEAM_ORDER_DISTANCE);
        printf("plan %zu %d\n", plan.pairs.size(), plan.nlevels);
        for (const SeamPair& p : plan.pairs) printf("%d %d %d %d %d %d %d\n", p.i, p.j, p.level, p.roi.x0, p.roi.y0, p.roi.x1, p.roi.y1);
    }
    return 0;
}
