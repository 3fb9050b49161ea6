// One pixel of one synthetic scene: SyntheticSceneDataset._render (data_handler/synthetic_scene.py) restated line for line in fp64, as
// __host__ __device__ code shared by the kernel (scenes.hip), its host twin (cp_render_scenes_host_f32) and the stand-alone self-test
// (scenes_selftest.cpp).  Nothing here calls a library beyond <math.h>.
//
// An image is described by one record of 8-byte words, HEADER words followed by OBJECT words per object:
//   [0] hc  [1] wc   crop origin (row, column) in the 480 x 640 frame
//   [2] fx  [3] fy  [4] cx  [5] cy   the camera
//   [6] the image seed: the bit pattern of a uint64 (the Philox key)
//   [7] the number of objects in this image, 0 <= n <= oc (anything else renders the background alone)
//   per object: R [9] row-major, t [3], 1 / semi-axes [3], colour [3]
// All of the geometry is fp64 without FMA contraction, so that silhouette decisions follow the host's as closely as fp64 allows; the one
// conversion to fp32 is the last step.  The noise is Philox4x32-10 (philox.h) keyed by the image seed and counted by (pixel, draw): the six
// normals of a pixel depend on nothing but (image seed, pixel), whatever block, batch position or shard renders it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "philox.h"

#if defined(__HIPCC__)
#define SCENE_HD __host__ __device__ inline
#else
#define SCENE_HD inline
#endif

namespace cp_scene {

constexpr int HEADER = 8, OBJECT = 18, DERIVED = 4;
constexpr int W_HC = 0, W_WC = 1, W_FX = 2, W_FY = 3, W_CX = 4, W_CY = 5, W_SEED = 6, W_COUNT = 7;
constexpr int O_R = 0, O_T = 9, O_INV = 12, O_COLOUR = 15;
constexpr int MAX_OBJECTS = 254;   // labels are uint8 with 0 for the background

SCENE_HD size_t record_words(int oc) { return (size_t)HEADER + (size_t)OBJECT * (size_t)oc; }

SCENE_HD uint64_t record_seed(const double* rec) {
    uint64_t s;
    __builtin_memcpy(&s, rec + W_SEED, sizeof s);
    return s;
}

SCENE_HD int record_objects(const double* rec, int oc) {
    const double n = rec[W_COUNT];
    return (n >= 0.0 && n <= (double)oc) ? (int)n : 0;   // false for NaN
}

// the pixel-independent part of one object: c = -(R^T t) * inv_axes (the camera centre in the unit-sphere frame) and cq = c.c - 1
SCENE_HD void object_terms(const double* obj, double* der) {
#pragma clang fp contract(off)
    const double *R = obj + O_R, *t = obj + O_T, *inv = obj + O_INV;
    for (int j = 0; j < 3; ++j) der[j] = -((R[j] * t[0] + R[3 + j] * t[1]) + R[6 + j] * t[2]) * inv[j];
    der[3] = ((der[0] * der[0] + der[1] * der[1]) + der[2] * der[2]) - 1.0;
}

// the ray of crop pixel (y, x): ((x + wc + 0.5 - cx) / fx, (y + hc + 0.5 - cy) / fy, 1); xs, ys are the frame coordinates of the pixel centre
SCENE_HD void pixel_ray(const double* rec, int y, int x, double& xs, double& ys, double& rx, double& ry) {
#pragma clang fp contract(off)
    xs = ((double)x + rec[W_WC]) + 0.5;
    ys = ((double)y + rec[W_HC]) + 0.5;
    rx = (xs - rec[W_CX]) / rec[W_FX];
    ry = (ys - rec[W_CY]) / rec[W_FY];
}

// one object against one ray: objects are visited in index order and a later one wins only when strictly nearer
SCENE_HD void visit_object(const double* obj, const double* der, int o, double rx, double ry, double& depth, int& label, double& shade) {
#pragma clang fp contract(off)
    const double *R = obj + O_R, *inv = obj + O_INV;
    const double d0 = ((rx * R[0] + ry * R[3]) + R[6]) * inv[0];   // (r R) * inv_axes with r_z = 1
    const double d1 = ((rx * R[1] + ry * R[4]) + R[7]) * inv[1];
    const double d2 = ((rx * R[2] + ry * R[5]) + R[8]) * inv[2];
    const double a = (d0 * d0 + d1 * d1) + d2 * d2;
    const double bq = (d0 * der[0] + d1 * der[1]) + d2 * der[2];
    const double disc = bq * bq - a * der[3];
    if (disc > 0.0) {
        const double s = (-bq - sqrt(disc)) / a;   // the ray parameter = the depth (r_z = 1)
        if (s > 0.0 && s < depth) {
            depth = s;
            label = o + 1;
            shade = 0.55 + 0.45 * fabs(der[2] + d2 * s);   // |z| of the unit-sphere normal
        }
    }
}

// label and shade of one pixel; der holds DERIVED words per object (object_terms)
SCENE_HD void trace_pixel(const double* rec, const double* der, int n, double rx, double ry, int& label, double& shade) {
    double depth = (double)INFINITY;
    label = 0;
    shade = 0.0;
    for (int o = 0; o < n; ++o) visit_object(rec + HEADER + OBJECT * o, der + DERIVED * o, o, rx, ry, depth, label, shade);
}

// the six standard normals of a pixel: two Philox blocks (draw 0 and 1), Box-Muller in fp32 with both branches of each uniform pair.
// normals[0..2] perturb a background pixel's channels, normals[3..5] every pixel's.
SCENE_HD void pixel_normals(uint64_t seed, uint32_t pixel, float* normals) {
    const float two_pi = 6.2831853071795865f;
    const cp::philox4 a = cp::philox4x32_10(pixel, 0u, 0u, 0u, seed), b = cp::philox4x32_10(pixel, 1u, 0u, 0u, seed);
    const float r0 = sqrtf(-2.f * logf(cp::u01(a.v[0]))), t0 = two_pi * cp::u01(a.v[1]);
    const float r1 = sqrtf(-2.f * logf(cp::u01(a.v[2]))), t1 = two_pi * cp::u01(a.v[3]);
    const float r2 = sqrtf(-2.f * logf(cp::u01(b.v[0]))), t2 = two_pi * cp::u01(b.v[1]);
    normals[0] = r0 * cosf(t0);
    normals[1] = r0 * sinf(t0);
    normals[2] = r1 * cosf(t1);
    normals[3] = r1 * sinf(t1);
    normals[4] = r2 * cosf(t2);
    normals[5] = r2 * sinf(t2);
}

// the procedural background at frame coordinates (xs, ys) of a pixel centre (shade_math.h draws the same wave behind its meshes)
SCENE_HD double background_wave(double xs, double ys) {
#pragma clang fp contract(off)
    return 0.35 + (0.1 * sin(xs / 37.0)) * cos(ys / 53.0);
}

// the last steps of one pixel whose channels v are in [0, 1] before noise: N(0, 0.02) when it is a background pixel, N(0, 0.01) on every
// pixel, clip(., 0, 1) * 2 - 1 and the one rounding to fp32.  noise = false reads no normal.
SCENE_HD void finish_pixel(const double* v, bool background, bool noise, const float* normals, float* rgb) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double b = background && noise ? v[c] + 0.02 * (double)normals[c] : v[c];
        double w = noise ? b + 0.01 * (double)normals[3 + c] : b;
        w = w < 0.0 ? 0.0 : (w > 1.0 ? 1.0 : w);
        rgb[c] = (float)(w * 2.0 - 1.0);
    }
}

// the colour of one pixel in [-1, 1]: colours[label - 1] * shade or the background wave, N(0, 0.02) on background pixels, N(0, 0.01)
// everywhere, clip(., 0, 1) * 2 - 1.  noise = false gives the noise-free image and reads no normal.
SCENE_HD void shade_pixel(const double* rec, int label, double shade, double xs, double ys, bool noise, const float* normals, float* rgb) {
#pragma clang fp contract(off)
    double v[3];
    if (label > 0) {
        const double* colour = rec + HEADER + OBJECT * (label - 1) + O_COLOUR;
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = colour[c] * shade;
    } else {
        const double bg = background_wave(xs, ys);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = bg;
    }
    finish_pixel(v, label == 0, noise, normals, rgb);
}

// one image, serially: what cp_render_scenes_host_f32 runs per record.  der is caller-provided scratch of DERIVED * oc words.
SCENE_HD void render_image_serial(const double* rec, int oc, int H, int W, int noise, double* der, float* img, uint8_t* label, float* target_seg,
                                  int32_t* counts) {
    const int n = record_objects(rec, oc), K = oc + 1;
    const uint64_t seed = record_seed(rec);
    for (int o = 0; o < n; ++o) object_terms(rec + HEADER + OBJECT * o, der + DERIVED * o);
    for (int o = 0; o < oc; ++o) counts[o] = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * (size_t)W + (size_t)x;
            double xs, ys, rx, ry, shade;
            int lab;
            float normals[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            pixel_ray(rec, y, x, xs, ys, rx, ry);
            trace_pixel(rec, der, n, rx, ry, lab, shade);
            if (noise) pixel_normals(seed, (uint32_t)p, normals);
            shade_pixel(rec, lab, shade, xs, ys, noise != 0, normals, img + 3 * p);
            label[p] = (uint8_t)lab;
            for (int k = 0; k < K; ++k) target_seg[p * (size_t)K + (size_t)k] = k == lab ? 1.f : 0.f;
            if (lab > 0) counts[lab - 1] += 1;
        }
}

}  // namespace cp_scene
