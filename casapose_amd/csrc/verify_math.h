// Verifying an estimated pose against the network's own output: the estimate's rendered depth plane (masks.hip: one uint32 plane per rendered
// instance, the bit pattern of an fp32 depth) is compared with the filtered label map or slot map and with the vector field.  The arithmetic of
// the device kernel (pose_verify.hip), of its host twin and of the stand-alone self-test (verify_selftest.cpp), as __host__ __device__ code.
// Nothing here calls a library, takes a square root or divides: the host and the device cannot disagree.
//
// The rules, for one job (image m, plane p, label l) and one pixel (row i, column j):
//   1. frame           plane p is slot p % instances_max of frame p / instances_max; the planes that may hide it are the first
//                      min(max(inst_counts[frame], 0), instances_max) planes of that frame, p itself excepted
//   2. pixels walked   the job's bbox_obj (record words 2-5: x, y, w, h, or a negative w or h for "empty") clipped to the image; an empty box
//                      walks nothing
//   3. rendered        the job's plane word is not 0xffffffff
//   4. hidden          rendered, and a plane q of rule 1 has, at this pixel, a smaller word, or an equal word and q < p.  Depths are positive
//                      fp32, so comparing the words compares the depths; 0xffffffff is the largest word.  Plane q is read only at the pixels of
//                      its own clipped bbox_obj (the renderer hits nothing outside it)
//   5. visible         rendered and not hidden; the pixel's label L = labels[m][i][j] sorts it into on_label (L == l), on_background (L == 0)
//                      and on_other (anything else)
//   6. pairs           for an on_label pixel and keypoint k: d = (dy, dx) = the fp32 field words dir_off + 2k, dir_off + 2k + 1 of the pixel's
//                      record as fp64, e = (ky - (i + o), kx - (j + o)) with (ky, kx) = kp2d[job][k] and o = sample_offset; the pair counts when
//                      d.d and e.e are both > 0 and finite.  a.b = a_y * b_y + a_x * b_x in fp64, one rounding per operation, no contraction
//   7. inliers         of those, d.e >= 0 and (d.e) * (d.e) >= ((cos_min * cos_min) * (d.d)) * (e.e)
//   8. label_pixels    the pixels of the whole image m whose label is l (a histogram of the label maps, taken in the same call)
//   9. counts          int32 [8] per job: rendered, hidden, on_label, on_background, on_other, label_pixels, pairs, inliers.  Integers only:
//                      the result does not depend on the order of summation
//  10. refusals        a job whose image, plane or label (1..255) is out of range, or whose frame is not below `frames`, leaves zeros
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "plane_record.h"

#if defined(__HIPCC__)
#define VERIFY_HD __host__ __device__ inline
#else
#define VERIFY_HD inline
#endif

namespace cp_verify {

constexpr int COUNTS = 8;
constexpr int C_RENDERED = 0, C_HIDDEN = 1, C_ON_LABEL = 2, C_ON_BACKGROUND = 3, C_ON_OTHER = 4, C_LABEL_PIXELS = 5, C_PAIRS = 6, C_INLIERS = 7;
constexpr int TILE = 256;                 // pixels a block takes per step
constexpr int MAX_SPLIT = 64;             // blocks per job
constexpr int MAX_INSTANCES = 256;        // planes of a frame: cp_mask's limit
constexpr int MAX_KP = 32;
constexpr int BINS = 256;                 // label values
constexpr double LARGEST = 1.7976931348623157e308;
using cp_plane::Box, cp_plane::clipped_box, cp_plane::EMPTY, cp_plane::MAX_SIDE, cp_plane::R_BOX_OBJ, cp_plane::RECORD;

// the pixel rectangle a job walks and what it reads there
struct Job {
    int image, plane, label;
    int first, hiders;   // the frame's first plane and how many of its planes may hide (rule 1)
    bool walks;          // false: the box is empty, only label_pixels is counted
    Box box;
};

VERIFY_HD bool intersect(const Box& a, const Box& b, Box& out) {
    out.x0 = a.x0 > b.x0 ? a.x0 : b.x0, out.y0 = a.y0 > b.y0 ? a.y0 : b.y0;
    out.x1 = a.x1 < b.x1 ? a.x1 : b.x1, out.y1 = a.y1 < b.y1 ? a.y1 : b.y1;
    return out.x0 <= out.x1 && out.y0 <= out.y1;
}

// rules 1, 2 and 10: false when the job leaves zeros.  job: (image, plane, label, unused)
VERIFY_HD bool job_setup(const int32_t* job, const int32_t* records, int nplanes, const int32_t* inst_counts, int frames, int instances_max, int images,
                         int H, int W, Job& j) {
    j.image = job[0], j.plane = job[1], j.label = job[2];
    if (j.image < 0 || j.image >= images || j.plane < 0 || j.plane >= nplanes || j.label < 1 || j.label > 255) return false;
    const int frame = j.plane / instances_max;
    if (frame >= frames) return false;
    const int c = inst_counts[frame];
    j.first = frame * instances_max;
    j.hiders = c < 0 ? 0 : (c > instances_max ? instances_max : c);
    if (j.first + j.hiders > nplanes) j.hiders = nplanes - j.first;   // never a plane beyond the array
    j.walks = clipped_box(records + (size_t)j.plane * RECORD, H, W, 0, j.box);   // rule 2
    return true;
}

// the part of plane q's box inside the job's: false when q cannot hide anything of the job
VERIFY_HD bool hider_box(const Job& j, int q, const int32_t* records, int H, int W, Box& out) {
    Box b;
    if (q == j.plane || !clipped_box(records + (size_t)q * RECORD, H, W, 0, b)) return false;
    return intersect(j.box, b, out);
}

// rule 4 for one plane q whose box holds the pixel: w is the job's word (not EMPTY), wq is q's
VERIFY_HD bool hides(uint32_t wq, int q, uint32_t w, int p) { return wq < w || (wq == w && q < p); }

VERIFY_HD bool inside(const Box& b, int i, int j) { return j >= b.x0 && j <= b.x1 && i >= b.y0 && i <= b.y1; }

// rules 6 and 7 for one (pixel, keypoint) pair: bit 0 = the pair counts, bit 1 = it is an inlier.  ci, cj: the pixel's centre
VERIFY_HD int pair_bits(float dy32, float dx32, double ky, double kx, double ci, double cj, double cos2) {
#pragma clang fp contract(off)
    const double dy = (double)dy32, dx = (double)dx32;
    const double dd = dy * dy + dx * dx;
    if (!(dd > 0.0 && dd <= LARGEST)) return 0;
    const double ey = ky - ci, ex = kx - cj;
    const double ee = ey * ey + ex * ex;
    if (!(ee > 0.0 && ee <= LARGEST)) return 0;
    const double de = dy * ey + dx * ex;
    return (de >= 0.0 && de * de >= (cos2 * dd) * ee) ? 3 : 1;
}

VERIFY_HD double pixel_centre(int i, double sample_offset) {
#pragma clang fp contract(off)
    return (double)i + sample_offset;
}

// rule 8, serially: hist int32 [images][BINS], every word written
inline void histogram_serial(const uint8_t* labels, int images, int H, int W, int32_t* hist) {
    const size_t hw = (size_t)H * (size_t)W;
    for (size_t k = 0; k < (size_t)images * BINS; ++k) hist[k] = 0;
    for (int m = 0; m < images; ++m)
        for (size_t at = 0; at < hw; ++at) hist[(size_t)m * BINS + labels[(size_t)m * hw + at]] += 1;
}

// The serial scorer: the same rules, one loop nest.  Argument shapes as cp_pose_verify_i32's (include/casapose_hip.h).
inline void verify_serial(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const int32_t* inst_counts, int frames,
                          int instances_max, const uint8_t* labels, const float* field, int images, int ld, int dir_off, int kp, const double* kp2d,
                          const int32_t* jobs, int njobs, double sample_offset, double cos_min, int32_t* counts, int32_t* hist) {
#pragma clang fp contract(off)
    const size_t hw = (size_t)H * (size_t)W;
    const double cos2 = cos_min * cos_min;
    histogram_serial(labels, images, H, W, hist);
    for (int n = 0; n < njobs; ++n) {
        int32_t* out = counts + (size_t)n * COUNTS;
        for (int k = 0; k < COUNTS; ++k) out[k] = 0;
        Job j;
        if (!job_setup(jobs + 4 * (size_t)n, records, nplanes, inst_counts, frames, instances_max, images, H, W, j)) continue;
        out[C_LABEL_PIXELS] = hist[(size_t)j.image * BINS + j.label];
        if (!j.walks) continue;
        const uint32_t* mine = planes + (size_t)j.plane * hw;
        const uint8_t* lab = labels + (size_t)j.image * hw;
        const float* fld = field + (size_t)j.image * hw * (size_t)ld;
        const double* kps = kp2d + (size_t)n * 2 * (size_t)kp;
        for (int i = j.box.y0; i <= j.box.y1; ++i)
            for (int x = j.box.x0; x <= j.box.x1; ++x) {
                const size_t at = (size_t)i * W + x;
                const uint32_t w = mine[at];
                if (w == EMPTY) continue;
                out[C_RENDERED] += 1;
                bool hidden = false;
                for (int q = j.first; q < j.first + j.hiders && !hidden; ++q) {
                    Box b;
                    if (hider_box(j, q, records, H, W, b) && inside(b, i, x)) hidden = hides(planes[(size_t)q * hw + at], q, w, j.plane);
                }
                if (hidden) {
                    out[C_HIDDEN] += 1;
                    continue;
                }
                const int L = lab[at];
                if (L != j.label) {
                    out[L == 0 ? C_ON_BACKGROUND : C_ON_OTHER] += 1;
                    continue;
                }
                out[C_ON_LABEL] += 1;
                const float* rec = fld + at * (size_t)ld + dir_off;
                const double ci = pixel_centre(i, sample_offset), cj = pixel_centre(x, sample_offset);
                for (int k = 0; k < kp; ++k) {
                    const int bits = pair_bits(rec[2 * k], rec[2 * k + 1], kps[2 * k], kps[2 * k + 1], ci, cj, cos2);
                    out[C_PAIRS] += bits & 1;
                    out[C_INLIERS] += bits >> 1;
                }
            }
    }
}

}  // namespace cp_verify
