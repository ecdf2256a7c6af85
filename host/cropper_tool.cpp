// cropper_tool -- test aid (tests/test_host_cpp.py): reads a binary PGM/PPM (P5 / P6), then
//   cropper_tool contour IN.pgm            prints the external contours: one line "n x0 y0 x1 y1 ..." each
//   cropper_tool fill IN.pgm OUT.pgm       largest contour filled (drawContours FILLED)
//   cropper_tool crop IN.ppm OUT.ppm       crop(); prints "x y w h"
//   cropper_tool crop_time IN.ppm REPS     mis::crop() REPS times on copies of the image; prints the median in milliseconds (tools/crop_device_bench.py)
//   cropper_tool crop_device IN.ppm OUT.ppm   the same through mis::cropDevice (the library's kernels; needs a GPU)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include "cropper.hpp"

int main(int argc, char** argv) {
    try {
        if (argc == 3 && !std::strcmp(argv[1], "contour")) {
            mis::HostImage m = mis::readPPM(argv[2]);
            for (const auto& c : mis::findExternalContours(m)) {
                std::printf("%zu", c.size());
                for (const auto& p : c) std::printf(" %d %d", p.x, p.y);
                std::printf("\n");
            }
            return 0;
        }
        if (argc == 4 && !std::strcmp(argv[1], "fill")) {
            mis::HostImage m = mis::readPPM(argv[2]);
            auto cs = mis::findExternalContours(m);
            size_t id = 0;
            for (size_t i = 0; i < cs.size(); i++) if (cs[i].size() > cs[id].size()) id = i;
            mis::writePPM(argv[3], mis::fillContour(cs.at(id), m.width, m.height));
            return 0;
        }
        if (argc == 4 && !std::strcmp(argv[1], "crop")) {
            mis::HostImage m = mis::readPPM(argv[2]);
            mis::Rect r = mis::crop(m);
            mis::writePPM(argv[3], m);
            std::printf("%d %d %d %d\n", r.x, r.y, r.width, r.height);
            return 0;
        }
        if (argc == 4 && !std::strcmp(argv[1], "crop_time")) {
            const mis::HostImage m = mis::readPPM(argv[2]);
            std::vector<double> ms;
            for (int k = 0; k < std::max(1, std::atoi(argv[3])); k++) {
                mis::HostImage c = m;
                const auto t0 = std::chrono::steady_clock::now();
                mis::crop(c);
                ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            }
            std::sort(ms.begin(), ms.end());
            std::printf("%.4f\n", ms[ms.size() / 2]);
            return 0;
        }
        if (argc == 4 && !std::strcmp(argv[1], "crop_device")) {
            mis::HostImage m = mis::readPPM(argv[2]);
            MisContext* ctx = nullptr;
            if (mis_context_create(0, nullptr, &ctx) != MIS_OK) throw std::runtime_error("mis_context_create failed: no HIP device (there is no CPU fallback)");
            mis::Rect r;
            try { r = mis::cropDevice(ctx, m); } catch (...) { mis_context_destroy(ctx); throw; }
            mis_context_destroy(ctx);
            mis::writePPM(argv[3], m);
            std::printf("%d %d %d %d\n", r.x, r.y, r.width, r.height);
            return 0;
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: cropper_tool contour IN | fill IN OUT | crop IN OUT | crop_time IN REPS | crop_device IN OUT\n");
    return 1;
}
