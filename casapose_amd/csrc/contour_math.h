// Contour alignment of rendered poses against the network's own label map: the distance field of an object's trusted silhouette boundary and
// one 2-D Gauss-Newton step per (image, render plane) job on the rendered contour.  The arithmetic of the device kernels (mask_contour.hip), of
// their host twins (cp_mask_edt_host_u16, cp_contour_step_host_f64) and of the stand-alone self-test (contour_selftest.cpp), as __host__
// __device__ code.  Part A is integers only and exact; part B is fp64 without FMA contraction, + - * / in the sums (sqrt only in the solve and
// the RMS, through icp_math.h), in a fixed order of summation: the device and the host give the same bytes.
//
// A. The field, for one job (image m, label l) and the gate G in whole pixels, 1 <= G <= 255:
//   A1. seeds      the pixels with labels[m][y][x] == l that have at least one 4-neighbour inside the image whose label is 0.  A neighbour
//                  with another object's label (an occlusion edge) and a neighbour outside the image (the border) make no seed
//   A2. field      D2(p) = min(min over seeds s of |p - s|^2, G G + 1), uint16.  No seeds: G G + 1 everywhere
//   A3. how        rows first: R(x, y) = min(d d, G G + 1) for the smallest d <= G with a seed at (x - d, y) or (x + d, y); then columns:
//                  D2(x, y) = min(G G + 1, min over rows y' in the image of R(x, y') + (y' - y)^2).  A seed more than G columns or rows away
//                  adds more than G G, so the clamp makes both windows exact, and a minimum over more rows than y - G .. y + G changes nothing
//   A4. refusal    image outside [0, images) or label outside [1, 255]: status ST_REFUSED, not a byte of the job's plane or rows is written
// B. The step, for one job (image m, render plane s, field plane f, gate G) and one pixel (x, y):
//   B1. pixels     as icp_math.h rule 1: the plane's bbox_obj clipped to [1, W-2] x [1, H-2]
//   B2. contour    the plane is hit at the pixel and not hit at one or more of its left, right, upper and lower neighbours
//   B3. used       the rendered depth z is > 0 and D2 at the pixel and at its four neighbours are all <= G G
//   B4. residual   e = ((D2(x+1, y) - D2(x-1, y)) / 4, (D2(x, y+1) - D2(x, y-1)) / 4): exact, and c - s wherever the five share their seed s
//   B5. point      p = P(x, y, z) of icp_math.h rule 3 with cx - o and cy - o in place of cx and cy, o = the rasteriser's sample offset in whole
//                  256ths of a pixel (the subtraction is made once per job): the plane was sampled at (x + o, y + o).
//                  a = fx / Z, b = fy / Z, c = -((a X) / Z), d = -((b Y) / Z): the projection's Jacobian rows (a, 0, c) and (0, b, d);
//                  times [-[p]x | I] for the left twist (omega, v):
//                  Ju = (c Y, a Z - c X, -(a Y), a, 0, c),  Jv = (d Y - b Z, -(d X), b X, 0, b, d);  g = ex Ju + ey Jv  (= J^T e)
//   B6. sums       ee = ex ex + ey ey.  With ee > 0: A_ab += g_a (g_b / ee) for a <= b (21), b_a -= g_a (6), see += ee (1).  With ee = 0 the
//                  pixel is counted as used and adds nothing.  Two integer counts: used pixels, contour pixels.  The order is icp_math.h rule 7
//   B7. solve, update   icp_math.h rules 8 and 9 on these sums (cp_icp::solve_update)
//   B8. statuses   ST_REFUSED: image, plane or field index out of range or the gate outside [1, 255] (nothing is read for the job; its stats
//                  are zeros); ST_FEW: fewer than min_pixels used pixels; ST_SINGULAR: a pivot was not > 0.  Every status but ST_OK leaves
//                  the pose as it is
//   B9. stats      fp64 [4]: used pixels, sqrt(see / used) in pixels (0 without pixels), contour pixels, see
#pragma once
#include "icp_math.h"

namespace cp_contour {

using cp_icp::Camera, cp_icp::EMPTY, cp_icp::Job, cp_icp::LANES, cp_icp::MAX_SIDE, cp_icp::MAX_SPLIT, cp_icp::N_A, cp_icp::N_B, cp_icp::SUMS, cp_icp::TILE;
using cp_icp::ST_FEW, cp_icp::ST_OK, cp_icp::ST_REFUSED, cp_icp::ST_SINGULAR;
using cp_icp::add_tiles, cp_icp::PARTIAL, cp_icp::step_serial, cp_icp::workspace_bytes;   // the step, on Contour's terms (part B)

constexpr int MAX_GATE = 255;

// ---- A. the field ---------------------------------------------------------------------------------------------------------------------------
ICP_HD int clamp_of(int G) { return G * G + 1; }

// bytes of the row pass's values: uint16 [njobs][H][W]
ICP_HD size_t edt_workspace_bytes(int njobs, int H, int W) { return (size_t)njobs * (size_t)H * (size_t)W * sizeof(uint16_t); }

// rule A4.  job: (image, label)
ICP_HD bool edt_job_ok(const int32_t* job, int images) { return job[0] >= 0 && job[0] < images && job[1] >= 1 && job[1] <= 255; }

// rule A1 for pixel (x, y) of one image, 0 <= x < W, 0 <= y < H
ICP_HD bool is_seed(const uint8_t* lab, int H, int W, int x, int y, int l) {
    const size_t at = (size_t)y * W + x;
    if (lab[at] != l) return false;
    return (x > 0 && lab[at - 1] == 0) || (x + 1 < W && lab[at + 1] == 0) || (y > 0 && lab[at - W] == 0) || (y + 1 < H && lab[at + W] == 0);
}

// rule A3, rows: flags[c - base] says whether column c of the row is a seed; every column of [max(x - G, 0), min(x + G, W - 1)] must be there
ICP_HD uint16_t row_value(const uint8_t* flags, int base, int W, int x, int G) {
    for (int d = 0; d <= G; ++d) {
        const int a = x - d, b = x + d;
        if ((a >= 0 && flags[a - base]) || (b < W && flags[b - base])) return (uint16_t)(d * d);
    }
    return (uint16_t)clamp_of(G);
}

// rule A3, columns: one row's value v, dy rows away, onto a running minimum
ICP_HD int col_min(int best, int v, int dy) {
    const int c = v + dy * dy;
    return c < best ? c : best;
}

// The serial field: labels uint8 [images][H][W], jobs int32 [njobs][2], planes uint16 [njobs][H][W], status int32 [njobs], rows: the workspace
inline void edt_serial(const uint8_t* labels, int images, int H, int W, const int32_t* jobs, int njobs, int G, uint16_t* planes, int32_t* status,
                       uint16_t* rows, uint8_t* flags /* [W] */) {
    const size_t hw = (size_t)H * (size_t)W;
    for (int n = 0; n < njobs; ++n) {
        if (!edt_job_ok(jobs + 2 * (size_t)n, images)) {
            status[n] = ST_REFUSED;
            continue;
        }
        status[n] = ST_OK;
        const uint8_t* lab = labels + (size_t)jobs[2 * (size_t)n] * hw;
        const int l = jobs[2 * (size_t)n + 1];
        uint16_t* R = rows + (size_t)n * hw;
        uint16_t* D = planes + (size_t)n * hw;
        for (int y = 0; y < H; ++y) {
            for (int x = 0; x < W; ++x) flags[x] = is_seed(lab, H, W, x, y, l);
            for (int x = 0; x < W; ++x) R[(size_t)y * W + x] = row_value(flags, 0, W, x, G);
        }
        for (int y = 0; y < H; ++y) {
            const int lo = y - G < 0 ? 0 : y - G, hi = y + G > H - 1 ? H - 1 : y + G;
            for (int x = 0; x < W; ++x) {
                int best = clamp_of(G);
                for (int yy = lo; yy <= hi; ++yy) best = col_min(best, R[(size_t)yy * W + x], yy - y);
                D[(size_t)y * W + x] = (uint16_t)best;
            }
        }
    }
}

// ---- B. the step ----------------------------------------------------------------------------------------------------------------------------
// rules B1 and B8: false when the job is refused.  job: (image, plane, field, gate).  Reads the plane's record only when it returns true.
ICP_HD bool job_setup(const int32_t* job, const int32_t* records, int nplanes, int nfields, int images, int H, int W, Job& j, int& field, int& G) {
    field = job[2], G = job[3];
    const bool mine = field >= 0 && field < nfields && G >= 1 && G <= MAX_GATE;
    return cp_icp::job_setup(job, mine ? 1.0 : 0.0, records, nplanes, images, H, W, j);
}

// rule B5: an image's camera (fx, fy, cx, cy) moved by the sample offset
ICP_HD Camera job_camera(const double* cam, double sample) {
#pragma clang fp contract(off)
    const Camera c = {cam[0], cam[1], cam[2] - sample, cam[3] - sample};
    return c;
}

// one used pixel's terms: g = J^T e and e . e
struct Terms {
    double g[6], ee;
};

// rules B2-B5 for pixel (x, y) -> 0: no contour pixel, 1: a contour pixel that is not used, 2: used (t is set)
ICP_HD int pixel(uint32_t bc, uint32_t bl, uint32_t br, uint32_t bu, uint32_t bd, int dc, int dl, int dr, int du, int dd, int x, int y,
                 const Camera& cam, int G, Terms& t) {
#pragma clang fp contract(off)
    if (bc == EMPTY || !(bl == EMPTY || br == EMPTY || bu == EMPTY || bd == EMPTY)) return 0;
    const int g2 = G * G;
    const double z = (double)cp_icp::depth_of(bc);
    if (!(z > 0.0) || dc > g2 || dl > g2 || dr > g2 || du > g2 || dd > g2) return 1;
    const double ex = (double)(dr - dl) / 4.0, ey = (double)(dd - du) / 4.0;
    double p[3];
    cp_icp::back_project(x, y, z, cam, p);
    const double a = cam.fx / p[2], b = cam.fy / p[2], c = -((a * p[0]) / p[2]), d = -((b * p[1]) / p[2]);
    const double Ju[6] = {c * p[1], a * p[2] - c * p[0], -(a * p[1]), a, 0.0, c};
    const double Jv[6] = {d * p[1] - b * p[2], -(d * p[0]), b * p[0], 0.0, b, d};
#pragma unroll
    for (int k = 0; k < 6; ++k) t.g[k] = ex * Ju[k] + ey * Jv[k];
    t.ee = ex * ex + ey * ey;
    return 2;
}

// rule B6 for one used pixel: its terms onto a lane's sums
ICP_HD void add_terms(const Terms& t, double* s) {
#pragma clang fp contract(off)
    if (!(t.ee > 0.0)) return;
    double h[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) h[a] = t.g[a] / t.ee;
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
            s[k] = s[k] + t.g[a] * h[b];
            ++k;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) s[N_A + a] = s[N_A + a] - t.g[a];
    s[N_A + N_B] = s[N_A + N_B] + t.ee;
}

// pixel s of a job's box, read from the render plane and the field: every address lies inside the clipped box grown by one pixel, which is
// inside the image (cp_icp::job_setup)
ICP_HD int job_pixel(const Job& j, int s, const uint32_t* plane, const uint16_t* field, int W, const Camera& cam, int G, Terms& t) {
    const int dy = (int)((unsigned)s / (unsigned)j.bw), y = j.y0 + dy, x = j.x0 + (s - dy * j.bw);
    const size_t at = (size_t)y * W + x;
    const uint32_t bc = plane[at];
    if (bc == EMPTY) return 0;
    const uint32_t bl = plane[at - 1], br = plane[at + 1], bu = plane[at - W], bd = plane[at + W];
    if (!(bl == EMPTY || br == EMPTY || bu == EMPTY || bd == EMPTY)) return 0;
    return pixel(bc, bl, br, bu, bd, field[at], field[at - 1], field[at + 1], field[at - W], field[at + W], x, y, cam, G, t);
}

// rules B7-B9: the step of one job from its sums.  pose: row-major [3, 4], rewritten only with ST_OK and update != 0.  -> the status
ICP_HD int solve_update(const double* sums, long long used, long long contour, double damping, int min_pixels, int update, double* pose, double* stats) {
    const int code = cp_icp::solve_update(sums, used, damping, min_pixels, update, pose, stats);
    stats[2] = (double)contour, stats[3] = sums[N_A + N_B];
    return code;
}

// The contour refiner's terms for cp_icp's step (icp_math.h says what each member is).  Args: planes uint32 [nplanes][H][W], records int32
// [nplanes][RECORD], fields uint16 [nfields][H][W], cams double [images][4], jobs int32 [njobs][4], sample: the sample offset (a multiple of 1 / 256)
struct Contour {
    static constexpr int COUNTS = 2;   // used pixels, contour pixels
    struct Args {
        const uint32_t* planes;
        const int32_t* records;
        int nplanes, H, W;
        const uint16_t* fields;
        int nfields;
        const double* cams;
        int images;
        const int32_t* jobs;
        double sample;
    };
    struct Context {
        const uint32_t* plane;
        const uint16_t* field;
        int W;
        Camera cam;
        int G;
    };
    static ICP_HD bool setup(const Args& a, size_t n, Job& j, Context& c) {
        int field, G;
        if (!job_setup(a.jobs + 4 * n, a.records, a.nplanes, a.nfields, a.images, a.H, a.W, j, field, G)) return false;
        const size_t hw = (size_t)a.H * (size_t)a.W;
        c = {a.planes + (size_t)j.plane * hw, a.fields + (size_t)field * hw, a.W, job_camera(a.cams + 4 * (size_t)j.image, a.sample), G};
        return true;
    }
    static ICP_HD void add(const Job& j, const Context& c, int s, double* sums, int* counts) {
        Terms t;
        const int kind = job_pixel(j, s, c.plane, c.field, c.W, c.cam, c.G, t);
        if (kind == 0) return;
        counts[1] += 1;
        if (kind != 2) return;
        add_terms(t, sums);
        counts[0] += 1;
    }
    static ICP_HD int solve(const double* sums, const long long* counts, double damping, int min_pixels, int update, double* pose, double* stats) {
        return solve_update(sums, counts[0], counts[1], damping, min_pixels, update, pose, stats);
    }
};

}  // namespace cp_contour
