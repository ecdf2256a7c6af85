// akaze_core.h -- the per-element arithmetic of the AKAZE finder's kernels (akaze.hip; SURVEY Appendix A.19 is the definition).
// Plain functions of one pixel, one candidate, one window or one lane, with no barrier inside: the kernels call them one element
// a thread, and a host program (tools/micro/akaze_emul.cpp) calls them element by element in the same order.  They compile as
// ordinary C++.  All image arithmetic is float32; the library is built without FMA contraction.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AKZ_HD __host__ __device__ __forceinline__
#else
#define AKZ_HD inline
#endif

enum { AKZ_MAX_LEVELS = 32, AKZ_MAX_FED = 256, AKZ_MAX_TAPS = 9, AKZ_DESC_BITS = 486, AKZ_DESC_BYTES = 61, AKZ_CELLS = 29, AKZ_ORI_GRID = 169, AKZ_ORI_WINDOWS = 42,
       AKZ_HIST_BINS = 300 };
// which plane mis_akaze_debug_level returns
enum { AKZ_LT = 0, AKZ_LSMOOTH = 1, AKZ_FLOW = 2, AKZ_LX = 3, AKZ_LY = 4, AKZ_LDET = 5, AKZ_PLANES = 6 };
#define AKZ_PI_F 3.14159265358979323846f

AKZ_HD int akz_fround(float x) { return (int)(x + 0.5f); }
AKZ_HD int akz_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
AKZ_HD int akz_reflect101(int p, int len) {     // one reflection is enough: every caller's reach is below len
    if (p < 0) p = -p;
    if (p >= len) p = 2 * len - 2 - p;
    return p;
}

// ---------------------------------------------------------------- step 1: levels ----------------
struct AkzLevel {
    int w, h, octave, sublevel, sigma_size, border, nsteps;
    float esigma, ratio, tau_div;      // ratio = 2^octave, tau_div = 4^octave
};
struct AkzPlan {
    int nlev, noct;
    AkzLevel lv[AKZ_MAX_LEVELS];
};
// false: more levels than AKZ_MAX_LEVELS.  (Host: the plan is made once per frame size.)
inline bool akz_plan(int w, int h, int n_octaves, int n_layers, AkzPlan* P) {
    P->nlev = 0; P->noct = 0;
    for (int o = 0; o < n_octaves; o++) {
        const int lw = (int)(w / (double)(1 << o)), lh = (int)(h / (double)(1 << o));
        if (o > 0 && (lw < 80 || lh < 40)) break;
        for (int j = 0; j < n_layers; j++) {
            if (P->nlev >= AKZ_MAX_LEVELS) return false;
            AkzLevel& L = P->lv[P->nlev++];
            L.w = lw; L.h = lh; L.octave = o; L.sublevel = j;
            L.ratio = (float)(1 << o); L.tau_div = (float)(1 << o) * (float)(1 << o);
            L.esigma = 1.6f * powf(2.f, (float)j / (float)n_layers + (float)o);
            L.sigma_size = (int)lrintf(L.esigma * 1.5f / L.ratio);            // cvRound: ties to even
            L.border = akz_fround(10.f * sqrtf(2.f) * (float)L.sigma_size);
            L.nsteps = 0;
        }
        P->noct = o + 1;
    }
    return true;
}

// ---------------------------------------------------------------- step 2: FED -------------------
// The schedule of the step from evolution time t0 to t1, reordered, as floats.  It is evaluated in double and stored as float (the
// f32 formula of the definition gives the same n away from exact ties; T = t1 - t0 cancels three digits in f32).  Returns n.
inline int akz_fed_schedule(double t0, double t1, float* tau /* AKZ_MAX_FED */) {
    const double T = t1 - t0, tau_max = 0.25;
    const int n = (int)(ceil(sqrt(3.0 * T / tau_max + 0.25) - 0.5 - 1.0e-8) + 0.5);
    if (n <= 0 || n > AKZ_MAX_FED) return n;
    const double scale = 3.0 * T / (tau_max * (double)(n * (n + 1)));
    double tauh[AKZ_MAX_FED];
    for (int k = 0; k < n; k++) {
        const double c = cos(3.14159265358979323846 * (double)(2 * k + 1) / (double)(4 * n + 2));
        tauh[k] = scale * tau_max / (2.0 * c * c);
    }
    const int kappa = n / 2;
    int prime = n + 1;
    for (;; prime++) {
        bool is_prime = prime >= 2;
        for (int d = 2; d * d <= prime; d++)
            if (prime % d == 0) { is_prime = false; break; }
        if (is_prime) break;
    }
    for (int k = 0, l = 0; l < n; k++, l++) {
        int index;
        while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
        tau[l] = (float)tauh[index];
    }
    return n;
}
inline double akz_etime(int n_layers, int octave, int sublevel) {
    const double es = 1.6 * pow(2.0, (double)sublevel / (double)n_layers + (double)octave);
    return 0.5 * es * es;
}

// ---------------------------------------------------------------- step 3: scale space -----------
AKZ_HD float akz_gray01(const uint8_t* bgr) {      // the project's 8-bit grey (15-bit coefficients), over 255
    return (float)((bgr[0] * 3735 + bgr[1] * 19235 + bgr[2] * 9798 + (1 << 14)) >> 15) / 255.f;
}
inline int akz_gauss_ksize(double sigma) {
    int k = (int)ceil(2.0 * (1.0 + (sigma - 0.8) / 0.3));
    return (k & 1) ? k : k + 1;
}
inline int akz_gauss_taps(double sigma, float* taps /* AKZ_MAX_TAPS */) {
    const int n = akz_gauss_ksize(sigma);
    double v[AKZ_MAX_TAPS], sum = 0;
    for (int i = 0; i < n; i++) { const double x = i - (n - 1) * 0.5; v[i] = exp(-0.5 * x * x / (sigma * sigma)); sum += v[i]; }
    for (int i = 0; i < n; i++) taps[i] = (float)(v[i] / sum);
    return n;
}
// INTER_AREA along one axis: destination d averages [d s, (d + 1) s) of n_src source samples (clipped to them); first source
// index, the count (<= 4 for 2 <= s < 3) and the overlap weights.  Returns the sum of the weights.
AKZ_HD float akz_area_span(int d, float s, int n_src, int* i0, int* cnt, float* wgt /* 4 */) {
    const float f0 = (float)d * s, f1 = fminf((float)(d + 1) * s, (float)n_src);
    const int a = (int)floorf(f0);
    int c = 0;
    float sum = 0.f;
    for (int i = a; (float)i < f1 && c < 4 && i < n_src; i++, c++) {
        const float wv = fminf((float)(i + 1), f1) - fmaxf((float)i, f0);
        wgt[c] = wv;
        sum += wv;
    }
    *i0 = a; *cnt = c;
    return sum;
}
AKZ_HD float akz_area_px(const float* src, int sw, int sh, float sx, float sy, int x, int y) {
    int ix, nx, iy, ny;
    float wx[4], wy[4];
    const float swx = akz_area_span(x, sx, sw, &ix, &nx, wx), swy = akz_area_span(y, sy, sh, &iy, &ny, wy);
    float acc = 0.f;
    for (int r = 0; r < ny; r++) {
        float ra = 0.f;
        for (int c = 0; c < nx; c++) ra += wx[c] * src[(size_t)(iy + r) * sw + ix + c];
        acc += wy[r] * ra;
    }
    return acc / (swx * swy);
}
// unnormalised 3 x 3 Scharr of a plane at (x, y), BORDER_REFLECT_101
AKZ_HD void akz_scharr(const float* p, int w, int h, int x, int y, float* lx, float* ly) {
    const int xm = akz_reflect101(x - 1, w), xp = akz_reflect101(x + 1, w), ym = akz_reflect101(y - 1, h), yp = akz_reflect101(y + 1, h);
    const float *r0 = p + (size_t)ym * w, *r1 = p + (size_t)y * w, *r2 = p + (size_t)yp * w;
    *lx = 3.f * (r0[xp] - r0[xm]) + 10.f * (r1[xp] - r1[xm]) + 3.f * (r2[xp] - r2[xm]);
    *ly = 3.f * (r2[xm] - r0[xm]) + 10.f * (r2[x] - r0[x]) + 3.f * (r2[xp] - r0[xp]);
}
AKZ_HD float akz_flow_g2(float lx, float ly, float k) { return 1.f / (1.f + (lx * lx + ly * ly) / (k * k)); }
AKZ_HD float akz_level_k(float k0, int octave) {      // k <- 0.75 k on every octave change
    for (int o = 0; o < octave; o++) k0 = 0.75f * k0;
    return k0;
}
AKZ_HD int akz_hist_bin(float m, float hmax) {
    const int b = (int)floorf((float)AKZ_HIST_BINS * (m / hmax));
    return b > AKZ_HIST_BINS - 1 ? AKZ_HIST_BINS - 1 : b;
}
// the k-contrast from the histogram of the non-zero gradient magnitudes (hmax == 0: a constant image, the value is never used)
AKZ_HD float akz_kcontrast(const unsigned* hist, float hmax) {
    unsigned npoints = 0;
    for (int b = 0; b < AKZ_HIST_BINS; b++) npoints += hist[b];
    if (!(hmax > 0.f)) return 0.03f;
    const unsigned nthreshold = (unsigned)((float)npoints * 0.7f);
    unsigned nelements = 0;
    int k = 0;
    for (; nelements < nthreshold && k < AKZ_HIST_BINS; k++) nelements += hist[k];
    if (nelements < nthreshold) return 0.03f;
    return hmax * ((float)k / (float)AKZ_HIST_BINS);
}
// one explicit diffusion update of a pixel: c and its neighbours (Lt), gc and theirs (the flow); has_*: the neighbour is inside
AKZ_HD float akz_diffuse(float c, float gc, float l, float gl, bool has_l, float r, float gr, bool has_r, float u, float gu, bool has_u, float d, float gd,
                         bool has_d, float tau) {
    const float fr = has_r ? (gc + gr) * (r - c) : 0.f, fl = has_l ? (gc + gl) * (l - c) : 0.f;
    const float fd = has_d ? (gc + gd) * (d - c) : 0.f, fu = has_u ? (gc + gu) * (u - c) : 0.f;
    return c + 0.5f * tau * (((fr + fl) + fd) + fu);
}

// ---------------------------------------------------------------- step 4: derivatives -----------
// The separable kernel pair at scale s has three non-zero taps a side: minus / plus are the plane's samples one derivative step
// (-s / +s) away, at the smoothing offsets -s, 0, +s across.
AKZ_HD float akz_deriv_norm(int s) { return 1.f / (2.f * (float)s * (10.f / 3.f + 2.f)); }
AKZ_HD float akz_deriv(const float* minus /* 3 */, const float* plus /* 3 */, float norm) {
    const float wn = (10.f / 3.f) * norm;
    return (norm * (plus[0] - minus[0]) + wn * (plus[1] - minus[1])) + norm * (plus[2] - minus[2]);
}
AKZ_HD float akz_deriv_x(const float* p, int w, int h, int x, int y, int s, float norm) {
    const int xm = akz_reflect101(x - s, w), xp = akz_reflect101(x + s, w);
    const int y0 = akz_reflect101(y - s, h), y2 = akz_reflect101(y + s, h);
    const float mi[3] = {p[(size_t)y0 * w + xm], p[(size_t)y * w + xm], p[(size_t)y2 * w + xm]};
    const float pl[3] = {p[(size_t)y0 * w + xp], p[(size_t)y * w + xp], p[(size_t)y2 * w + xp]};
    return akz_deriv(mi, pl, norm);
}
AKZ_HD float akz_deriv_y(const float* p, int w, int h, int x, int y, int s, float norm) {
    const int ym = akz_reflect101(y - s, h), yp = akz_reflect101(y + s, h);
    const int x0 = akz_reflect101(x - s, w), x2 = akz_reflect101(x + s, w);
    const float mi[3] = {p[(size_t)ym * w + x0], p[(size_t)ym * w + x], p[(size_t)ym * w + x2]};
    const float pl[3] = {p[(size_t)yp * w + x0], p[(size_t)yp * w + x], p[(size_t)yp * w + x2]};
    return akz_deriv(mi, pl, norm);
}
AKZ_HD float akz_ldet(float lxx, float lyy, float lxy, int s) {
    const float s2 = (float)(s * s);
    return (lxx * lyy - lxy * lxy) * (s2 * s2);
}

// ---------------------------------------------------------------- steps 5, 6: candidates --------
struct AkzCand { int x, y, level; float resp; };
AKZ_HD bool akz_is_candidate(const float* ldet, int w, int h, int x, int y, int border, float threshold) {
    if (x < border || y < border || x >= w - border || y >= h - border) return false;
    const float *r0 = ldet + (size_t)(y - 1) * w + x, *r1 = r0 + w, *r2 = r1 + w;
    const float v = r1[0];
    return v > threshold && v > r0[-1] && v > r0[0] && v > r0[1] && v > r1[-1] && v > r1[1] && v > r2[-1] && v > r2[0] && v > r2[1];
}
// q wins over p: (R_q, -order_q) > (R_p, -order_p), order = (level, y, x)
AKZ_HD bool akz_wins(const AkzCand& q, const AkzCand& p) {
    if (q.resp != p.resp) return q.resp > p.resp;
    if (q.level != p.level) return q.level < p.level;
    if (q.y != p.y) return q.y < p.y;
    return q.x < p.x;
}
// q suppresses p: a neighbouring level, inside p's radius (base coordinates), and it wins
AKZ_HD bool akz_suppresses(const AkzCand& q, float q_ratio, const AkzCand& p, float p_ratio, float p_radius) {
    const float dx = (float)q.x * q_ratio - (float)p.x * p_ratio, dy = (float)q.y * q_ratio - (float)p.y * p_ratio;
    return dx * dx + dy * dy <= p_radius * p_radius && akz_wins(q, p);
}

// ---------------------------------------------------------------- step 7: refinement ------------
AKZ_HD bool akz_refine(const float* ldet, int w, int x, int y, float* dx, float* dy) {
    const float *r0 = ldet + (size_t)(y - 1) * w + x, *r1 = r0 + w, *r2 = r1 + w;
    const float Dx = 0.5f * (r1[1] - r1[-1]), Dy = 0.5f * (r2[0] - r0[0]);
    const float Dxx = (r1[1] + r1[-1]) - 2.f * r1[0], Dyy = (r2[0] + r0[0]) - 2.f * r1[0];
    const float Dxy = 0.25f * (((r2[1] + r0[-1]) - r0[1]) - r2[-1]);
    const float det = Dxx * Dyy - Dxy * Dxy;
    *dx = (Dy * Dxy - Dx * Dyy) / det;
    *dy = (Dx * Dxy - Dy * Dxx) / det;
    return fabsf(*dx) <= 1.f && fabsf(*dy) <= 1.f;      // (a singular system gives inf / NaN: refused)
}

// ---------------------------------------------------------------- step 8: orientation -----------
AKZ_HD float akz_angle(float x, float y) {
    const float a = atan2f(y, x);
    return a < 0.f ? a + 2.f * AKZ_PI_F : a;
}
// grid position p of the 13 x 13 square (i = p / 13 - 6 outer, j = p % 13 - 6): the weighted responses and the angle of the sample,
// angle -1 (in no window) outside the disc i^2 + j^2 < 36
AKZ_HD void akz_ori_sample(const float* lx, const float* ly, int w, int h, float xf, float yf, int s, int p, float* rx, float* ry, float* ang) {
    const int i = p / 13 - 6, j = p % 13 - 6;
    if (i * i + j * j >= 36) { *rx = 0.f; *ry = 0.f; *ang = -1.f; return; }
    const int ix = akz_clampi(akz_fround(xf + (float)(i * s)), 0, w - 1), iy = akz_clampi(akz_fround(yf + (float)(j * s)), 0, h - 1);
    const float g = expf(-(float)(i * i + j * j) / 12.5f) / (12.5f * AKZ_PI_F);
    *rx = g * lx[(size_t)iy * w + ix];
    *ry = g * ly[(size_t)iy * w + ix];
    *ang = akz_angle(*rx, *ry);
}
AKZ_HD bool akz_in_window(float ang1, float ang) {
    const float two_pi = 2.f * AKZ_PI_F;
    const float ang2 = ang1 + AKZ_PI_F / 3.f > two_pi ? ang1 - 5.f * AKZ_PI_F / 3.f : ang1 + AKZ_PI_F / 3.f;
    if (ang1 < ang2) return ang1 < ang && ang < ang2;
    return (ang > 0.f && ang < ang2) || (ang > ang1 && ang < two_pi);
}
// window k (start 0.15 k): the sums over the samples in grid order, and the window's score
AKZ_HD float akz_window(const float* rx, const float* ry, const float* ang, int k, float* sum_x, float* sum_y) {
    const float ang1 = 0.15f * (float)k;
    float sx = 0.f, sy = 0.f;
    for (int p = 0; p < AKZ_ORI_GRID; p++)
        if (akz_in_window(ang1, ang[p])) { sx += rx[p]; sy += ry[p]; }
    *sum_x = sx; *sum_y = sy;
    return sx * sx + sy * sy;
}
AKZ_HD float akz_angle_degrees(float sum_x, float sum_y) {
    float d = akz_angle(sum_x, sum_y) * (180.f / AKZ_PI_F);
    if (d >= 360.f) d -= 360.f;
    return d;
}

// ---------------------------------------------------------------- step 9: MLDB ------------------
// cell c of 0 .. 28: grids of step 10, 7, 5 hold cells 0 .. 3, 4 .. 12, 13 .. 28 (i outer, j inner, from -10)
AKZ_HD void akz_cell(int c, int* step, int* i0, int* j0) {
    int per, base;
    if (c < 4) { *step = 10; per = 2; base = 0; }
    else if (c < 13) { *step = 7; per = 3; base = 4; }
    else { *step = 5; per = 4; base = 13; }
    *i0 = -10 + ((c - base) / per) * *step;
    *j0 = -10 + ((c - base) % per) * *step;
}
// one lane's share of a cell's sums: samples t = lane, lane + nlanes, ... of the step x step block (k = i0 + t / step outer)
AKZ_HD void akz_cell_lane_sums(const float* lt, const float* lx, const float* ly, int w, int h, float xf, float yf, int s, float co, float si, int c, int lane,
                               int nlanes, float* out /* 3 */) {
    int step, i0, j0;
    akz_cell(c, &step, &i0, &j0);
    float a = 0.f, bx = 0.f, by = 0.f;
    for (int t = lane; t < step * step; t += nlanes) {
        const int k = i0 + t / step, l = j0 + t % step;
        const int x = akz_clampi(akz_fround(xf + (-(float)l * si + (float)k * co) * (float)s), 0, w - 1);
        const int y = akz_clampi(akz_fround(yf + ((float)l * co + (float)k * si) * (float)s), 0, h - 1);
        const size_t o = (size_t)y * w + x;
        const float vx = lx[o], vy = ly[o];
        a += lt[o];
        bx += -vx * si + vy * co;
        by += vx * co + vy * si;
    }
    out[0] = a; out[1] = bx; out[2] = by;
}
// bit b of 0 .. 485 compares vals[3 * ca + ch] > vals[3 * cb + ch]: grid, then channel, then the cell pairs a < b
AKZ_HD void akz_bit_cells(int b, int* ca, int* cb, int* ch) {
    int base, n;
    if (b < 18) { base = 0; n = 4; }
    else if (b < 18 + 108) { b -= 18; base = 4; n = 9; }
    else { b -= 126; base = 13; n = 16; }
    const int pairs = n * (n - 1) / 2;
    *ch = b / pairs;
    int r = b % pairs, a = 0;
    while (r >= n - 1 - a) { r -= n - 1 - a; a++; }
    *ca = base + a;
    *cb = base + a + 1 + r;
}
AKZ_HD bool akz_bit(const float* vals /* 3 * AKZ_CELLS */, int b) {
    int ca, cb, ch;
    akz_bit_cells(b, &ca, &cb, &ch);
    return vals[3 * ca + ch] > vals[3 * cb + ch];
}
