// Segmentation masks of a BOP frame: every instance's mesh rasterised at its ground-truth pose, the nearest instance per pixel.  The arithmetic of
// the device kernels (masks.hip), of their host twin (cp_render_masks_host_u8) and of the stand-alone self-test (masks_selftest.cpp), as
// __host__ __device__ code.  Nothing here calls a library beyond <math.h>.
//
// The rules, fixed so that the device, the twin and a NumPy restatement agree bit for bit:
//   1. camera point   X = ((R00 x + R01 y) + R02 z) + tx (rows 1, 2 alike), fp64 without FMA contraction; the fp32 vertex widens exactly
//   2. projection     u = (fx X) / Z + cx, v = (fy Y) / Z + cy, then U = rint(256 u), V = rint(256 v) as int64 (round half to even)
//   3. sample point   pixel (row i, column j) is sampled at (256 j + S, 256 i + S), S = rint(256 sample_offset)
//   4. coverage       E_k = (x_b - x_a)(p_y - y_a) - (y_b - y_a)(p_x - x_a) in int64 for the edges (1,2), (2,0), (0,1); covered when
//                     E0 + E1 + E2 != 0 and all three are >= 0 or all three are <= 0 (both windings, closed edges)
//   5. depth          z = A / ((E0 / z0 + E1 / z1) + E2 / z2) in fp64 with A = E0 + E1 + E2, rounded once to fp32; kept when near <= z <= far
//   6. near plane     a triangle with a vertex at Z < near (or NaN) is dropped whole and counted.  So is one that cannot be represented: a face
//                     index outside the object's vertices, or |256 u| or |256 v| above 2^28 (which keeps every int64 product below 2^60)
//   7. visibility     the smallest fp32 depth wins a pixel, the lowest instance index on a tie; compared as bit patterns, which order like the
//                     numbers because every kept depth is positive (near > 0)
//   8. records        per instance int32 [RECORD]: px_count_all, px_count_visib, bbox_obj (x, y, w, h), bbox_visib (x, y, w, h),
//                     dropped_triangles; a box is (xmin, ymin, xmax - xmin, ymax - ymin) of its pixel set -- the BOP toolkit's calc_2d_bbox --
//                     or (-1, -1, -1, -1) when the set is empty
// An instance whose object index is outside [0, objects) or whose label is outside [0, 255] renders nothing and keeps an empty record.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "plane_record.h"

#if defined(__HIPCC__)
#define MASK_HD __host__ __device__ inline
#else
#define MASK_HD inline
#endif

namespace cp_mask {

using cp_plane::Camera, cp_plane::EMPTY, cp_plane::MAX_SIDE, cp_plane::R_BOX_OBJ, cp_plane::RECORD;   // what the planes' readers share
constexpr int R_ALL = 0, R_VISIB = 1, R_BOX_VISIB = 6, R_DROPPED = 10;
constexpr int MAX_INSTANCES = 256;     // per frame: the resolve kernel keeps ten LDS words per instance
constexpr int LANE_SAMPLES = 1024;     // a triangle whose clipped bounding box holds more samples is walked by a whole wave
constexpr double SNAP_LIMIT = 268435456.0;   // 2^28
constexpr int TRI_EMPTY = 0, TRI_DRAW = 1, TRI_DROPPED = 2;
constexpr int32_t BOX_NONE = 0x7fffffff;

// a projected triangle: snapped vertices, camera depths, and the pixel rectangle [i0, i1] x [j0, j1] whose samples its bounding box holds
struct Tri {
    int64_t x0, y0, x1, y1, x2, y2;
    double z0, z1, z2;
    int i0, i1, j0, j1;
};

MASK_HD int clamp_count(int n, int hi) { return n < 0 ? 0 : (n > hi ? hi : n); }

MASK_HD size_t workspace_bytes(int frames, int instances_max, int H, int W) {
    return (size_t)frames * (size_t)instances_max * (size_t)H * (size_t)W * sizeof(uint32_t);
}

MASK_HD int64_t sample_origin(double sample_offset) { return (int64_t)rint(256.0 * sample_offset); }

// rule 1: the camera point of one vertex (shade_math.h takes its face normals from the same three points)
MASK_HD void camera_point(const float* v, const double* P, double& X, double& Y, double& Z) {
#pragma clang fp contract(off)
    const double x = (double)v[0], y = (double)v[1], z = (double)v[2];
    X = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    Y = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    Z = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
}

// rules 1, 2 and 6 for one vertex; false: the triangle is dropped
MASK_HD bool camera_vertex(const float* v, const double* P, const Camera& cam, double near, int64_t& U, int64_t& V, double& Z) {
#pragma clang fp contract(off)
    double X, Y;
    camera_point(v, P, X, Y, Z);
    if (!(Z >= near)) return false;   // also NaN
    const double su = 256.0 * ((cam.fx * X) / Z + cam.cx);
    const double sv = 256.0 * ((cam.fy * Y) / Z + cam.cy);
    if (!(fabs(su) <= SNAP_LIMIT && fabs(sv) <= SNAP_LIMIT)) return false;
    U = (int64_t)rint(su);
    V = (int64_t)rint(sv);
    return true;
}

MASK_HD int64_t min3(int64_t a, int64_t b, int64_t c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
MASK_HD int64_t max3(int64_t a, int64_t b, int64_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
// floor / ceiling of a / 256 for either sign (|a| < 2^29)
MASK_HD int64_t floor256(int64_t a) { return (a - (((a % 256) + 256) % 256)) / 256; }
MASK_HD int64_t ceil256(int64_t a) { return floor256(a + 255); }

// One triangle of one instance: TRI_DRAW with `t` filled, TRI_EMPTY (zero area, or no sample of the image inside its bounding box) or
// TRI_DROPPED.  verts: the object's [vcount][3]; face: its three vertex indices; P: the [3,4] pose, row-major.
MASK_HD int setup_triangle(const float* verts, int vcount, const int32_t* face, const double* P, const Camera& cam, double near, int64_t S, int H,
                           int W, Tri& t) {
    const int a = face[0], b = face[1], c = face[2];
    if (a < 0 || a >= vcount || b < 0 || b >= vcount || c < 0 || c >= vcount) return TRI_DROPPED;
    const bool ok0 = camera_vertex(verts + 3 * (size_t)a, P, cam, near, t.x0, t.y0, t.z0);
    const bool ok1 = camera_vertex(verts + 3 * (size_t)b, P, cam, near, t.x1, t.y1, t.z1);
    const bool ok2 = camera_vertex(verts + 3 * (size_t)c, P, cam, near, t.x2, t.y2, t.z2);
    if (!(ok0 && ok1 && ok2)) return TRI_DROPPED;
    if ((t.x1 - t.x0) * (t.y2 - t.y0) - (t.y1 - t.y0) * (t.x2 - t.x0) == 0) return TRI_EMPTY;   // = E0 + E1 + E2 at every sample
    int64_t j0 = ceil256(min3(t.x0, t.x1, t.x2) - S), j1 = floor256(max3(t.x0, t.x1, t.x2) - S);
    int64_t i0 = ceil256(min3(t.y0, t.y1, t.y2) - S), i1 = floor256(max3(t.y0, t.y1, t.y2) - S);
    if (j0 < 0) j0 = 0;
    if (i0 < 0) i0 = 0;
    if (j1 > W - 1) j1 = W - 1;
    if (i1 > H - 1) i1 = H - 1;
    if (j0 > j1 || i0 > i1) return TRI_EMPTY;
    t.i0 = (int)i0, t.i1 = (int)i1, t.j0 = (int)j0, t.j1 = (int)j1;
    return TRI_DRAW;
}

MASK_HD int64_t edge(int64_t xa, int64_t ya, int64_t xb, int64_t yb, int64_t px, int64_t py) { return (xb - xa) * (py - ya) - (yb - ya) * (px - xa); }

// rules 3-5 for the sample of pixel (i, j): true with the fp32 depth's bit pattern when the triangle covers it inside [near, far]
MASK_HD bool sample_depth(const Tri& t, int i, int j, int64_t S, double near, double far, uint32_t& bits) {
#pragma clang fp contract(off)
    const int64_t px = 256 * (int64_t)j + S, py = 256 * (int64_t)i + S;
    const int64_t E0 = edge(t.x1, t.y1, t.x2, t.y2, px, py), E1 = edge(t.x2, t.y2, t.x0, t.y0, px, py), E2 = edge(t.x0, t.y0, t.x1, t.y1, px, py);
    const int64_t A = E0 + E1 + E2;
    if (A == 0) return false;
    if (!((E0 >= 0 && E1 >= 0 && E2 >= 0) || (E0 <= 0 && E1 <= 0 && E2 <= 0))) return false;
    const double z = (double)A / (((double)E0 / t.z0 + (double)E1 / t.z1) + (double)E2 / t.z2);
    const float zf = (float)z;
    if (!((double)zf >= near && (double)zf <= far)) return false;
    __builtin_memcpy(&bits, &zf, sizeof bits);
    return true;
}

// an instance that renders: its object index and label are in range
MASK_HD bool instance_valid(int obj, int label, int objects) { return obj >= 0 && obj < objects && label >= 0 && label <= 255; }

// a record while it accumulates: the two counts, then (xmin, ymin, xmax, ymax) twice, then the dropped triangles
MASK_HD void record_clear(int32_t* r) {
    r[R_ALL] = r[R_VISIB] = r[R_DROPPED] = 0;
    r[R_BOX_OBJ] = r[R_BOX_OBJ + 1] = r[R_BOX_VISIB] = r[R_BOX_VISIB + 1] = BOX_NONE;
    r[R_BOX_OBJ + 2] = r[R_BOX_OBJ + 3] = r[R_BOX_VISIB + 2] = r[R_BOX_VISIB + 3] = -1;
}

MASK_HD void box_finish(int32_t* box, int32_t count) {
    if (count == 0) {
        box[0] = box[1] = box[2] = box[3] = -1;
    } else {
        box[2] -= box[0];
        box[3] -= box[1];
    }
}

MASK_HD void record_finish(int32_t* r) {
    box_finish(r + R_BOX_OBJ, r[R_ALL]);
    box_finish(r + R_BOX_VISIB, r[R_VISIB]);
}

MASK_HD void box_add(int32_t* box, int x, int y) {
    if (x < box[0]) box[0] = x;
    if (y < box[1]) box[1] = y;
    if (x > box[2]) box[2] = x;
    if (y > box[3]) box[3] = y;
}

// The serial renderer: the same planes, the same rules, one loop nest.  planes: workspace_bytes(frames, instances_max, H, W) bytes.
inline void render_serial(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts, int Tmax,
                          int objects, const double* cams, const int32_t* inst_counts, const int32_t* inst_obj, const int32_t* inst_label,
                          const double* poses, int frames, int instances_max, int H, int W, double near, double far, double sample_offset,
                          uint8_t* label, int32_t* records, uint32_t* planes) {
    const size_t hw = (size_t)H * (size_t)W;
    const int64_t S = sample_origin(sample_offset);
    for (int f = 0; f < frames; ++f) {
        const int n = clamp_count(inst_counts[f], instances_max);
        const Camera cam = {cams[4 * f], cams[4 * f + 1], cams[4 * f + 2], cams[4 * f + 3]};
        uint32_t* fplanes = planes + (size_t)f * instances_max * hw;
        int32_t* frec = records + (size_t)f * instances_max * RECORD;
        for (int k = 0; k < instances_max; ++k) record_clear(frec + (size_t)k * RECORD);
        for (int k = 0; k < n; ++k) {
            uint32_t* plane = fplanes + (size_t)k * hw;
            for (size_t p = 0; p < hw; ++p) plane[p] = EMPTY;
            const size_t slot = (size_t)f * instances_max + k;
            const int obj = inst_obj[slot];
            if (!instance_valid(obj, inst_label[slot], objects)) continue;
            const int vcount = clamp_count(vert_counts[obj], Vmax), tcount = clamp_count(face_counts[obj], Tmax);
            const float* ov = verts + (size_t)obj * Vmax * 3;
            const int32_t* of = faces + (size_t)obj * Tmax * 3;
            for (int tri = 0; tri < tcount; ++tri) {
                Tri t;
                const int st = setup_triangle(ov, vcount, of + 3 * (size_t)tri, poses + slot * 12, cam, near, S, H, W, t);
                if (st == TRI_DROPPED) frec[(size_t)k * RECORD + R_DROPPED] += 1;
                if (st != TRI_DRAW) continue;
                for (int i = t.i0; i <= t.i1; ++i)
                    for (int j = t.j0; j <= t.j1; ++j) {
                        uint32_t bits;
                        if (sample_depth(t, i, j, S, near, far, bits) && bits < plane[(size_t)i * W + j]) plane[(size_t)i * W + j] = bits;
                    }
            }
        }
        for (int i = 0; i < H; ++i)
            for (int j = 0; j < W; ++j) {
                const size_t p = (size_t)i * W + j;
                uint32_t best = EMPTY;
                int winner = -1;
                for (int k = 0; k < n; ++k) {
                    const uint32_t b = fplanes[(size_t)k * hw + p];
                    if (b == EMPTY) continue;
                    int32_t* r = frec + (size_t)k * RECORD;
                    r[R_ALL] += 1;
                    box_add(r + R_BOX_OBJ, j, i);
                    if (b < best) best = b, winner = k;
                }
                uint8_t lab = 0;
                if (winner >= 0) {
                    int32_t* r = frec + (size_t)winner * RECORD;
                    r[R_VISIB] += 1;
                    box_add(r + R_BOX_VISIB, j, i);
                    lab = (uint8_t)inst_label[(size_t)f * instances_max + winner];
                }
                label[(size_t)f * hw + p] = lab;
            }
        for (int k = 0; k < instances_max; ++k) record_finish(frec + (size_t)k * RECORD);
    }
}

}  // namespace cp_mask
