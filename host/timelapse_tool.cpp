// timelapse_tool.cpp -- test aid: mis::Stitcher::timelapse on the frames "<k>.ppm" / cameras "<k>.txt" (k = 1 .. n) of a directory,
// the canvases written as raw PPM so that a test can compare them with the Python pipeline's pixel for pixel (stitch_main writes
// them as JPEG files only, image_stitching.cpp:1214):
//   timelapse_tool <dir> <n> <as_is|crop> <expos_comp_type> <out_prefix>
// writes <out_prefix><k>.ppm for every kept frame k and prints "dst_roi x y width height" and "kept k1 k2 ...".
#include <fstream>
#include <iostream>
#include <sstream>
#include "stitcher.hpp"

int main(int argc, char** argv) {
    if (argc != 6) { std::cout << "usage: " << argv[0] << " <dir> <n> <as_is|crop> <expos_comp_type> <out_prefix>\n"; return 2; }
    try {
        const std::string dir = argv[1];
        const int n = std::atoi(argv[2]);
        mis::StitchConfig cfg;
        cfg.timelapse = true;
        cfg.timelapse_type = argv[3];
        cfg.expos_comp_type = argv[4];
        std::vector<mis::HostImage> frames;
        std::vector<mis::CameraParams> cams;
        for (int k = 1; k <= n; k++) {
            frames.push_back(mis::readPPM(dir + "/" + std::to_string(k) + ".ppm"));
            std::ifstream f(dir + "/" + std::to_string(k) + ".txt");
            if (!f) throw std::runtime_error("no camera description for frame " + std::to_string(k));
            std::stringstream ss;
            ss << f.rdbuf();
            bool portrait = false;
            cams.push_back(mis::cameraFromImageDescription(ss.str(), &portrait));
        }
        mis::Stitcher st(0, cfg);
        const mis::TimelapseResult r = st.timelapse(frames, cams);
        for (size_t k = 0; k < r.frames.size(); k++) mis::writePPM(std::string(argv[5]) + std::to_string(r.indices[k] + 1) + ".ppm", r.frames[k]);
        std::cout << "dst_roi " << r.dst_roi.x << " " << r.dst_roi.y << " " << r.dst_roi.width << " " << r.dst_roi.height << "\nkept";
        for (int i : r.indices) std::cout << " " << i + 1;
        std::cout << "\n";
    } catch (const std::exception& e) {
        std::cout << e.what() << "\n";
        return 1;
    }
    return 0;
}
