// Shaded pictures of meshes: mask_math.h's rasteriser with a colour output.  The arithmetic of the device kernels (shade.hip), of their host
// twin (cp_render_shaded_host_f32) and of the stand-alone self-test (shade_selftest.cpp), as __host__ __device__ code.  Nothing here calls a
// library beyond <math.h>.
//
// The rules, fixed so that the device, the twin and a NumPy restatement agree (integers bit for bit, the image to fp32 rounding):
//   1. projection, coverage, depth   cp_mask::setup_triangle, edge and sample_depth as they are (rules 1-6 of mask_math.h)
//   2. visibility     one 64-bit key per pixel and frame, key = depth_bits << 32 | instance << 24 | triangle, with depth_bits rule 5's fp32
//                     pattern, instance < 256 and triangle < 2^24; the smallest key wins: the smallest depth, then the lowest instance (mask_math.h
//                     rule 7), then the lowest triangle index.  The winner does not depend on the order of arrival.  Empty is all ones.
//   3. attributes     the winning triangle is rebuilt with setup_triangle (the same snapped vertices and E_k as in the raster pass);
//                     q_k = (double)E_k / z_k, lambda_k = q_k / ((q_0 + q_1) + q_2); albedo_c = (lambda_0 c_0 + lambda_1 c_1) + lambda_2 c_2 with
//                     c_k = (double)u8 / 255.0 from the per-vertex colours, or the object's flat colour (fp32 widened) without them
//   4. normal         the flat face normal in camera space from the three camera points of mask_math.h rule 1: n = (P1 - P0) x (P2 - P0),
//                     divided by its length, with the sign that makes n . P0 <= 0 (two-sided).  A zero-length normal shades with n . l = 0
//   5. shade          s = ambient + diffuse * max(0, n . l), l the frame's unit light direction in camera space; the channel is
//                     clip(albedo_c * s, 0, 1) * 2 - 1
//   6. background     (u8 / 255.0) from the background image when there is one, otherwise scene_math.h's wave at the frame's crop origin
//   7. noise          scene_math.h / philox.h as they are, keyed by the frame's seed and counted by pixel: N(0, 0.02) on background pixels,
//                     then N(0, 0.01) everywhere, before the clip; noise = 0 draws nothing.  The image is rounded to fp32 once, at the end
//   8. depth          optional fp32 output: the winning fp32 depth, 0 on background
// A frame's record is FRAME_WORDS fp64 words: the light direction (3), ambient, diffuse, the seed's bit pattern, crop row, crop column.
// A key that decodes to an instance, object, triangle or vertex out of range renders as background.
#pragma once
#include "mask_math.h"
#include "scene_math.h"

#if defined(__HIPCC__)
#define SHADE_HD __host__ __device__ inline
#else
#define SHADE_HD inline
#endif

namespace cp_shade {

using cp_mask::Camera;
using cp_mask::Tri;

constexpr int FRAME_WORDS = 8;
constexpr int F_LIGHT = 0, F_AMBIENT = 3, F_DIFFUSE = 4, F_SEED = 5, F_CROP_ROW = 6, F_CROP_COL = 7;
constexpr uint64_t KEY_EMPTY = ~(uint64_t)0;
constexpr int MAX_TRIANGLES = 1 << 24;

SHADE_HD size_t workspace_bytes(int frames, int H, int W) { return (size_t)frames * (size_t)H * (size_t)W * sizeof(uint64_t); }

// rule 2; instance < 256 and tri < 2^24 are the caller's (checked before any launch)
SHADE_HD uint64_t make_key(uint32_t depth_bits, int instance, int tri) {
    return (uint64_t)depth_bits << 32 | (uint64_t)(uint32_t)instance << 24 | (uint64_t)(uint32_t)tri;
}

SHADE_HD uint64_t frame_seed(const double* frame) {
    uint64_t s;
    __builtin_memcpy(&s, frame + F_SEED, sizeof s);
    return s;
}

// what a pixel is made of once its key is decoded
struct Surface {
    int label;          // the instance's label, 0: background
    float depth;        // rule 8
    double albedo[3];   // rule 3
    double shade;       // rule 5's s
};

// the meshes, the instance tables and the colours: the arguments of cp_render_shaded_f32 that every pixel reads
struct Scene {
    const float* verts;
    const int32_t* vert_counts;
    int Vmax;
    const int32_t* faces;
    const int32_t* face_counts;
    int Tmax, objects;
    const double* cams;
    const int32_t* inst_counts;
    const int32_t* inst_obj;
    const int32_t* inst_label;
    const double* poses;
    int instances_max, H, W;
    double near;
    int64_t S;
    const uint8_t* colors;       // [objects][Vmax][3] or null
    const float* flat_colors;    // [objects][3]
};

// rules 4 and 5: s for the triangle with camera points p0, p1, p2 under the light l
SHADE_HD double face_shade(const double* p0, const double* p1, const double* p2, const double* l, double ambient, double diffuse) {
#pragma clang fp contract(off)
    const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
    const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
    double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    double ndl = 0.0;
    if (len > 0.0) {   // false for NaN
        nx = nx / len, ny = ny / len, nz = nz / len;
        if ((nx * p0[0] + ny * p0[1]) + nz * p0[2] > 0.0) nx = -nx, ny = -ny, nz = -nz;
        ndl = (nx * l[0] + ny * l[1]) + nz * l[2];
    }
    return ambient + diffuse * (ndl > 0.0 ? ndl : 0.0);
}

// rules 2-5 and 8 for the key of pixel (i, j) of frame f; false: background (an empty key, or one that decodes to something out of range)
SHADE_HD bool decode_surface(const Scene& sc, const double* frame, int f, int i, int j, uint64_t key, Surface& out) {
#pragma clang fp contract(off)
    if (key == KEY_EMPTY) return false;
    const int k = (int)((key >> 24) & 255u), tri = (int)(key & 0xffffffu);
    if (k >= cp_mask::clamp_count(sc.inst_counts[f], sc.instances_max)) return false;
    const size_t slot = (size_t)f * sc.instances_max + k;
    const int obj = sc.inst_obj[slot], lab = sc.inst_label[slot];
    if (!cp_mask::instance_valid(obj, lab, sc.objects)) return false;
    const int vcount = cp_mask::clamp_count(sc.vert_counts[obj], sc.Vmax), tcount = cp_mask::clamp_count(sc.face_counts[obj], sc.Tmax);
    if (tri >= tcount) return false;
    const float* ov = sc.verts + (size_t)obj * sc.Vmax * 3;
    const int32_t* face = sc.faces + ((size_t)obj * sc.Tmax + tri) * 3;
    const double* P = sc.poses + slot * 12;
    const Camera cam = {sc.cams[4 * f], sc.cams[4 * f + 1], sc.cams[4 * f + 2], sc.cams[4 * f + 3]};
    Tri t;
    if (cp_mask::setup_triangle(ov, vcount, face, P, cam, sc.near, sc.S, sc.H, sc.W, t) != cp_mask::TRI_DRAW) return false;   // checks the face's indices
    const int64_t px = 256 * (int64_t)j + sc.S, py = 256 * (int64_t)i + sc.S;
    const int64_t E0 = cp_mask::edge(t.x1, t.y1, t.x2, t.y2, px, py), E1 = cp_mask::edge(t.x2, t.y2, t.x0, t.y0, px, py),
                  E2 = cp_mask::edge(t.x0, t.y0, t.x1, t.y1, px, py);
    if (E0 + E1 + E2 == 0) return false;
    const double q0 = (double)E0 / t.z0, q1 = (double)E1 / t.z1, q2 = (double)E2 / t.z2;
    const double sum = (q0 + q1) + q2;
    const double l0 = q0 / sum, l1 = q1 / sum, l2 = q2 / sum;
    const int a = face[0], b = face[1], c = face[2];   // in [0, vcount): setup_triangle drew
    if (sc.colors) {
        const uint8_t* oc = sc.colors + (size_t)obj * sc.Vmax * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            out.albedo[ch] = (l0 * ((double)oc[3 * (size_t)a + ch] / 255.0) + l1 * ((double)oc[3 * (size_t)b + ch] / 255.0)) +
                             l2 * ((double)oc[3 * (size_t)c + ch] / 255.0);
    } else {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out.albedo[ch] = (double)sc.flat_colors[3 * (size_t)obj + ch];
    }
    double p0[3], p1[3], p2[3];
    cp_mask::camera_point(ov + 3 * (size_t)a, P, p0[0], p0[1], p0[2]);
    cp_mask::camera_point(ov + 3 * (size_t)b, P, p1[0], p1[1], p1[2]);
    cp_mask::camera_point(ov + 3 * (size_t)c, P, p2[0], p2[1], p2[2]);
    out.shade = face_shade(p0, p1, p2, frame + F_LIGHT, frame[F_AMBIENT], frame[F_DIFFUSE]);
    const uint32_t bits = (uint32_t)(key >> 32);
    __builtin_memcpy(&out.depth, &bits, sizeof bits);
    out.label = lab & 255;
    return true;
}

// rules 2-8 for one pixel: rgb[3], the label byte and the depth.  background: the frame's [H][W][3] bytes or null
SHADE_HD void shade_pixel(const Scene& sc, const double* frame, int f, int i, int j, uint64_t key, const uint8_t* background, bool noise,
                          float* rgb, uint8_t& label, float& depth) {
#pragma clang fp contract(off)
    Surface s;
    const bool hit = decode_surface(sc, frame, f, i, j, key, s);
    const size_t p = (size_t)i * (size_t)sc.W + (size_t)j;
    double v[3];
    if (hit) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = s.albedo[c] * s.shade;
    } else if (background) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (double)background[3 * p + c] / 255.0;
    } else {
        const double xs = ((double)j + frame[F_CROP_COL]) + 0.5, ys = ((double)i + frame[F_CROP_ROW]) + 0.5;   // cp_scene::pixel_ray's centres
        const double bg = cp_scene::background_wave(xs, ys);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = bg;
    }
    float normals[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (noise) cp_scene::pixel_normals(frame_seed(frame), (uint32_t)p, normals);
    cp_scene::finish_pixel(v, !hit, noise, normals, rgb);
    label = hit ? (uint8_t)s.label : (uint8_t)0;
    depth = hit ? s.depth : 0.f;
}

// The serial renderer: the same key planes, the same rules, one loop nest.  keys: workspace_bytes(frames, H, W) bytes.
inline void render_shaded_serial(const Scene& sc, int frames, double far, const double* lights, const uint8_t* background, int noise, float* img,
                                 uint8_t* label, float* depth, int32_t* dropped, uint64_t* keys) {
    const size_t hw = (size_t)sc.H * (size_t)sc.W;
    for (int f = 0; f < frames; ++f) {
        uint64_t* plane = keys + (size_t)f * hw;
        for (size_t p = 0; p < hw; ++p) plane[p] = KEY_EMPTY;
        dropped[f] = 0;
        const int n = cp_mask::clamp_count(sc.inst_counts[f], sc.instances_max);
        const Camera cam = {sc.cams[4 * f], sc.cams[4 * f + 1], sc.cams[4 * f + 2], sc.cams[4 * f + 3]};
        for (int k = 0; k < n; ++k) {
            const size_t slot = (size_t)f * sc.instances_max + k;
            const int obj = sc.inst_obj[slot];
            if (!cp_mask::instance_valid(obj, sc.inst_label[slot], sc.objects)) continue;
            const int vcount = cp_mask::clamp_count(sc.vert_counts[obj], sc.Vmax), tcount = cp_mask::clamp_count(sc.face_counts[obj], sc.Tmax);
            const float* ov = sc.verts + (size_t)obj * sc.Vmax * 3;
            const int32_t* of = sc.faces + (size_t)obj * sc.Tmax * 3;
            for (int tri = 0; tri < tcount; ++tri) {
                Tri t;
                const int st = cp_mask::setup_triangle(ov, vcount, of + 3 * (size_t)tri, sc.poses + slot * 12, cam, sc.near, sc.S, sc.H, sc.W, t);
                if (st == cp_mask::TRI_DROPPED) dropped[f] += 1;
                if (st != cp_mask::TRI_DRAW) continue;
                for (int i = t.i0; i <= t.i1; ++i)
                    for (int j = t.j0; j <= t.j1; ++j) {
                        uint32_t bits;
                        if (!cp_mask::sample_depth(t, i, j, sc.S, sc.near, far, bits)) continue;
                        const uint64_t key = make_key(bits, k, tri);
                        if (key < plane[(size_t)i * sc.W + j]) plane[(size_t)i * sc.W + j] = key;
                    }
            }
        }
        const double* frame = lights + (size_t)f * FRAME_WORDS;
        const uint8_t* bg = background ? background + (size_t)f * hw * 3 : nullptr;
        for (int i = 0; i < sc.H; ++i)
            for (int j = 0; j < sc.W; ++j) {
                const size_t p = (size_t)f * hw + (size_t)i * sc.W + j;
                float d;
                shade_pixel(sc, frame, f, i, j, plane[(size_t)i * sc.W + j], bg, noise != 0, img + 3 * p, label[p], d);
                if (depth) depth[p] = d;
            }
    }
}

}  // namespace cp_shade
