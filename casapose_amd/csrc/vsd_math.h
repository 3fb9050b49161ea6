// BOP's Visible Surface Discrepancy for (estimate, ground-truth instance) pairs, from depth planes the mask renderer left behind (masks.hip:
// one uint32 plane per rendered instance, the bit pattern of an fp32 depth) and the sensor's depth image.  The arithmetic of the device kernel
// (vsd.hip) and of the stand-alone self-test (vsd_selftest.cpp), as __host__ __device__ code.  Nothing here calls a library beyond <math.h>.
//
// The rules, for one pair (estimate plane e, ground-truth plane g, image m) and one pixel (row i, column j):
//   1. rendered depth  z_e, z_g are the fp32 depths of the two planes; a plane word of 0xffffffff means "not hit"
//   2. sensor depth    z_t is the sensor depth in millimetres, fp32; a value that is not > 0 (0, negative or NaN) means "missing".  BOP only
//                      knows 0; negative values and NaN are this project's addition
//   3. distances       c = sqrt((1 + ((j - cx) / fx)^2) + ((i - cy) / fy)^2) and d_x = (double) z_x * c, in fp64 without FMA contraction; pixel
//                      centres sit at integer coordinates (BOP's convention)
//   4. visibility      (BOP19 mode)  vis_g = hit_g && (missing_t || d_g - d_t <= delta)
//                                    vis_e = hit_e && (missing_t || d_e - d_t <= delta || vis_g)
//                                    inter = vis_g && vis_e,  uni = vis_g || vis_e
//   5. pixels walked   the union of the two planes' boxes (record words 2-5: x, y, w, h, or a negative w or h for "empty"), each clipped to
//                      the image first; a pixel outside both boxes has neither hit.  Two empty boxes: nothing is walked
//   6. counts          int32 [2 + ntau] per pair: the sum of uni, the sum of inter, and per k the pixels with
//                      inter && |d_g - d_e| / diameter >= tau_k.  Integers only: the result does not depend on the order of summation
//   7. refusals        a pair whose image or plane index is out of range, or whose diameter is not > 0, leaves zeros
//   8. error           e_k = (counts[2 + k] + counts[0] - counts[1]) / counts[0] in fp64, 1.0 where counts[0] == 0; on the host, from the
//                      integers (pose_estimation/bop_vsd.py)
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "plane_record.h"

#if defined(__HIPCC__)
#define VSD_HD __host__ __device__ inline
#else
#define VSD_HD inline
#endif

namespace cp_vsd {

constexpr int MAX_TAUS = 32;              // one bit per tau in Pixel::reached
constexpr int TILE = 256;                 // pixels a block takes per step
constexpr int MAX_SPLIT = 64;             // blocks per pair
using cp_plane::Box, cp_plane::Camera, cp_plane::clipped_box, cp_plane::depth_of, cp_plane::EMPTY, cp_plane::MAX_SIDE, cp_plane::R_BOX_OBJ, cp_plane::RECORD;

// the pixel rectangle [i0, i0 + bh) x [j0, j0 + bw) a pair walks, and what it reads there
struct Pair {
    int image, plane_e, plane_g;
    int i0, j0, bh, bw;
};

struct Pixel {
    bool uni, inter;
    uint32_t reached;   // bit k: inter && cost >= tau_k
};

// rules 5 and 7: false when the pair leaves zeros.  pair: (image, estimate plane, ground-truth plane, unused)
VSD_HD bool pair_setup(const int32_t* pair, const int32_t* records, int nplanes, int images, int H, int W, double diameter, Pair& p) {
    p.image = pair[0], p.plane_e = pair[1], p.plane_g = pair[2];
    if (p.image < 0 || p.image >= images || p.plane_e < 0 || p.plane_e >= nplanes || p.plane_g < 0 || p.plane_g >= nplanes) return false;
    if (!(diameter > 0.0)) return false;
    Box a, b;
    const bool has_a = clipped_box(records + (size_t)p.plane_e * RECORD, H, W, 0, a);
    const bool has_b = clipped_box(records + (size_t)p.plane_g * RECORD, H, W, 0, b);
    if (!has_a && !has_b) return false;
    if (!has_a) a = b;
    if (has_a && has_b) {
        if (b.x0 < a.x0) a.x0 = b.x0;
        if (b.y0 < a.y0) a.y0 = b.y0;
        if (b.x1 > a.x1) a.x1 = b.x1;
        if (b.y1 > a.y1) a.y1 = b.y1;
    }
    p.i0 = a.y0, p.j0 = a.x0, p.bh = a.y1 - a.y0 + 1, p.bw = a.x1 - a.x0 + 1;   // inside [0, H) x [0, W)
    return true;
}

// rule 3: the distance from the camera centre of a point at depth 1 on the ray of pixel (i, j)
VSD_HD double ray_scale(int i, int j, const Camera& cam) {
#pragma clang fp contract(off)
    const double x = ((double)j - cam.cx) / cam.fx, y = ((double)i - cam.cy) / cam.fy;
    return sqrt((1.0 + x * x) + y * y);
}

// rules 1-4 and the comparisons of rule 6 for one pixel
VSD_HD Pixel pixel(uint32_t bits_e, uint32_t bits_g, float z_t, int i, int j, const Camera& cam, double delta, double diameter, const double* taus,
                   int ntau) {
#pragma clang fp contract(off)
    Pixel r = {false, false, 0u};
    const bool hit_e = bits_e != EMPTY, hit_g = bits_g != EMPTY;
    if (!hit_e && !hit_g) return r;
    const bool missing = !(z_t > 0.f);
    const double c = ray_scale(i, j, cam);
    const double d_t = (double)z_t * c, d_e = (double)depth_of(bits_e) * c, d_g = (double)depth_of(bits_g) * c;
    const bool vis_g = hit_g && (missing || d_g - d_t <= delta);
    const bool vis_e = hit_e && (missing || d_e - d_t <= delta || vis_g);
    r.uni = vis_g || vis_e;
    r.inter = vis_g && vis_e;
    if (r.inter) {
        const double cost = fabs(d_g - d_e) / diameter;
        for (int k = 0; k < ntau; ++k)
            if (cost >= taus[k]) r.reached |= 1u << k;
    }
    return r;
}

// The serial scorer: the same rules, one loop nest.  planes uint32 [nplanes][H][W], records int32 [nplanes][RECORD], depth float
// [images][H][W], cams double [images][4], pairs int32 [npairs][4], diameters double [npairs], taus double [ntau], counts int32 [npairs][2 + ntau].
inline void vsd_serial(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth, const double* cams, int images,
                       const int32_t* pairs, const double* diameters, int npairs, double delta, const double* taus, int ntau, int32_t* counts) {
    const size_t hw = (size_t)H * (size_t)W;
    for (int n = 0; n < npairs; ++n) {
        int32_t* out = counts + (size_t)n * (2 + ntau);
        for (int k = 0; k < 2 + ntau; ++k) out[k] = 0;
        Pair p;
        if (!pair_setup(pairs + 4 * (size_t)n, records, nplanes, images, H, W, diameters[n], p)) continue;
        const Camera cam = {cams[4 * p.image], cams[4 * p.image + 1], cams[4 * p.image + 2], cams[4 * p.image + 3]};
        const uint32_t *pe = planes + (size_t)p.plane_e * hw, *pg = planes + (size_t)p.plane_g * hw;
        const float* pt = depth + (size_t)p.image * hw;
        for (int i = p.i0; i < p.i0 + p.bh; ++i)
            for (int j = p.j0; j < p.j0 + p.bw; ++j) {
                const size_t at = (size_t)i * W + j;
                const Pixel r = pixel(pe[at], pg[at], pt[at], i, j, cam, delta, diameters[n], taus, ntau);
                out[0] += r.uni;
                out[1] += r.inter;
                for (int k = 0; k < ntau; ++k) out[2 + k] += (r.reached >> k) & 1u;
            }
    }
}

}  // namespace cp_vsd
