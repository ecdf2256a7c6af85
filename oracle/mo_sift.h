/* mo_sift.h -- CPU restatement (TEST INFRASTRUCTURE, see mo_common.h) of cv::SIFT::create()->detectAndCompute
 * as the reference calls it: image_stitching/image_stitching.cpp:559 (`SIFT::create()`, features_type == "sift")
 * and :613 (`computeImageFeatures`).  OpenCV source restated from memory: features2d/src/sift.dispatch.cpp,
 * sift.simd.hpp (4.5+, float scale space: SIFT_FIXPT_SCALE = 1), imgproc GaussianBlur / resize.
 *
 * PINNED, against an independent reading: the semantics of every stage at every parameter path (tap counts and taps, the folded
 * REFLECT_101, the doubled base image, incremental sigmas, octave count, DoG, the 26-neighbour scan and its threshold,
 * adjustLocalExtrema with all its rejections, the keypoint fields and the packed octave, orientation histogram / smoothing / peaks,
 * duplicate removal, KeyPoint_LessThan, the firstOctave rescaling, the descriptor).  tests/refimpl_sift.py restates them in numpy
 * from OpenCV's documented behaviour on another numerical road (float64 with derived float32 bands), and
 * tests/test_refimpl_sift_cpu.py holds this file to it.  NOT PINNED (OpenCV is absent): OpenCV's own SIMD-dependent last
 * bits.  Deliberate restatement choices where OpenCV's result depends on its SIMD build, all inside the reference's bands:
 * separable Gaussian taps accumulated in ascending tap order without FMA; exp via the shared Cephes polynomial mo_expf
 * (cv::hal::exp32f is table based); 2^x via mo_expf(x ln 2).
 * A Gaussian kernel is never truncated (GaussianBlur has no cap on ksize): parameters whose largest kernel exceeds
 * MO_SIFT_MAX_TAPS get no finder.
 *
 * Defaults of SIFT::create(): nfeatures 0 (unbounded), nOctaveLayers 3, contrastThreshold 0.04, edgeThreshold 10,
 * sigma 1.6, firstOctave -1 (input doubled), descriptors CV_32F with integer values 0..255. */
#ifndef MO_SIFT_H
#define MO_SIFT_H
#include <stddef.h>
#include <stdint.h>
#include "mo_orb.h" /* MoKeyPoint */
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int nfeatures;             /* 0 */
    int n_octave_layers;       /* 3 */
    double contrast_threshold; /* 0.04 */
    double edge_threshold;     /* 10 */
    double sigma;              /* 1.6 */
} MoSiftParams;

typedef struct MoSift MoSift;

void mo_sift_default_params(MoSiftParams* p);
MoSift* mo_sift_create(const MoSiftParams* p, int width, int height);
void mo_sift_destroy(MoSift* s);
int mo_sift_run(MoSift* s, const uint8_t* bgr, size_t stride); /* -> number of keypoints, < 0 on error */
int mo_sift_num_keypoints(const MoSift* s);
const MoKeyPoint* mo_sift_keypoints(const MoSift* s);
const float* mo_sift_descriptors(const MoSift* s); /* n x 128 */
/* intermediates for stage-by-stage parity tests */
int mo_sift_num_octaves(const MoSift* s);
const float* mo_sift_gauss(const MoSift* s, int octave, int layer, int* w, int* h); /* layer 0 .. nOctaveLayers + 2 */
const float* mo_sift_dog(const MoSift* s, int octave, int layer, int* w, int* h);   /* layer 0 .. nOctaveLayers + 1 */
int mo_sift_num_raw_keypoints(const MoSift* s); /* before duplicate removal */
int mo_sift_num_candidates(const MoSift* s);    /* extrema of the scan, before adjustLocalExtrema */
int mo_sift_num_refined(const MoSift* s);       /* candidates that adjustLocalExtrema kept */

float mo_expf(float x);
/* Gaussian taps of GaussianBlur(sigma) for CV_32F images: ksize = cvRound(sigma * 8 + 1) | 1, uncapped; returns ksize, or -1
 * (nothing written) when ksize > MO_SIFT_MAX_TAPS.  mo_sift_create returns NULL for parameters that need such a kernel. */
#define MO_SIFT_MAX_TAPS 127
int mo_gaussian_ksize(double sigma);
int mo_gaussian_taps_f32(double sigma, float* taps /* >= MO_SIFT_MAX_TAPS */);
#ifdef __cplusplus
}
#endif
#endif
