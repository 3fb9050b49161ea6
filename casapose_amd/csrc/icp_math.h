// Projective point-to-plane ICP of rendered poses against the sensor's depth image: one Gauss-Newton step per (image, render plane) job, from
// the depth planes the mask renderer left behind (masks.hip: one uint32 plane per rendered instance, the bit pattern of an fp32 depth).  The
// arithmetic of the device kernels (depth_icp.hip), of their host twin (cp_depth_icp_step_host_f64) and of the stand-alone self-test
// (icp_selftest.cpp), as __host__ __device__ code.  fp64 throughout, no FMA contraction, only + - * / and sqrt: nothing here calls libm, so the
// device and the host agree bit for bit.
//
// The rules, for one job (image m, plane s, gate g in millimetres) and one pixel (column x, row y); pixel centres sit at integer coordinates:
//   1. pixels walked   the plane's bbox_obj (record words 2-5: x, y, w, h, or a negative w or h for "empty") clipped to [1, W-2] x [1, H-2]
//   2. rendered depth  z, z_L, z_R, z_U, z_D: the plane at the pixel and at its left, right, upper and lower neighbour; a word of 0xffffffff
//                      means "not hit".  The pixel is skipped unless all five are hit and |z_R - z_L| < jump g and |z_D - z_U| < jump g
//                      (jump is in gates; the product is taken once per job)
//   3. back-projection P(x, y, z) = (((x - cx) z) / fx, ((y - cy) z) / fy, z);  p, p_L, p_R, p_U, p_D
//   4. normal          n = (p_R - p_L) x (p_D - p_U), divided by its length; skipped when the length is not > 0
//   5. sensor depth    d, fp32 millimetres; the pixel is used only if d > 0 (a NaN fails) and |d - z| < g.  q = P(x, y, d)
//   6. terms           r = n . (q - p),  J = (p x n, n);  dot products as (a0 b0 + a1 b1) + a2 b2
//   7. sums            SUMS = 28 fp64 sums per job: the upper triangle of J J^T row by row (21), J r (6), r r (1); and an integer count.
//                      Order: the clipped box in row-major order is cut into tiles of TILE pixels.  Within a tile lane l of 64 adds its
//                      pixels l, l + 64, ... in order, starting from +0; the 64 lane sums combine pairwise, lane l taking lane l + off for off =
//                      32, 16, 8, 4, 2, 1; the tiles' sums are then added serially in index order, starting from +0.  Nothing else is allowed:
//                      the result does not depend on the launch shape
//   8. solve           (A + damping diag(A)) xi = b by Cholesky (serial sums, lowest index first); xi = (omega, v)
//   9. update          the quaternion (1, omega / 2) divided by its length -> dR;  R <- dR R,  t <- dR t + v
//  10. statuses        ST_REFUSED: the image or plane index is out of range or the gate is not > 0 (nothing is read for the job; its stats
//                      are zeros); ST_FEW: fewer than min_pixels pixels were used; ST_SINGULAR: a pivot was not > 0 (a NaN included).  Every
//                      status but ST_OK leaves the pose as it is
//  11. stats           fp64 [4]: the pixels used, sqrt(sum r r / pixels) before the update (0 without pixels), |omega|, |v| (0 unless ST_OK)
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define ICP_HD __host__ __device__ inline
#else
#define ICP_HD inline
#endif

// sqrt without <math.h>: one correctly rounded instruction on the host, the device library's correctly rounded fp64 root on the device
#define ICP_SQRT(x) __builtin_sqrt(x)

namespace cp_icp {

constexpr int TILE = 1024;               // pixels of a tile: 16 per lane
constexpr int LANES = 64;
constexpr int SUMS = 28, N_A = 21, N_B = 6;
constexpr int PARTIAL = SUMS + 1;        // fp64 words of a tile's record in the workspace: the sums, then the count (exact: <= TILE)
constexpr int MAX_SPLIT = 64;            // blocks per job
constexpr int MAX_SIDE = 16384;          // H, W: cp_mask::MAX_SIDE
constexpr int RECORD = 11, R_BOX = 2;    // cp_mask::RECORD, R_BOX_OBJ
constexpr uint32_t EMPTY = 0xffffffffu;  // cp_mask::EMPTY
constexpr int ST_OK = 0, ST_FEW = 1, ST_SINGULAR = 2, ST_REFUSED = 3;

struct Camera {
    double fx, fy, cx, cy;
};

// the pixel rectangle [y0, y0 + bh) x [x0, x0 + bw) a job walks (total = bh * bw pixels in tiles tiles; all zero for an empty box)
struct Job {
    int image, plane;
    int x0, y0, bw, bh, total, tiles;
};

// one used pixel's terms
struct Terms {
    double J[6], r;
};

ICP_HD double absd(double a) { return a < 0.0 ? -a : a; }

ICP_HD float depth_of(uint32_t bits) {
    float z;
    __builtin_memcpy(&z, &bits, sizeof z);
    return z;
}

// the tiles of the largest clipped box of an H x W image: what the workspace holds per job
ICP_HD long long max_tiles(int H, int W) {
    if (H < 3 || W < 3) return 1;
    return ((long long)(H - 2) * (long long)(W - 2) + TILE - 1) / TILE;
}

ICP_HD size_t workspace_bytes(int njobs, int H, int W) { return (size_t)njobs * (size_t)max_tiles(H, W) * PARTIAL * sizeof(double); }

// rules 1 and 10: false when the job is refused.  job: (image, plane, unused, unused).  Reads the plane's record only when it returns true.
ICP_HD bool job_setup(const int32_t* job, double gate, const int32_t* records, int nplanes, int images, int H, int W, Job& j) {
    j.image = job[0], j.plane = job[1];
    j.x0 = j.y0 = j.bw = j.bh = j.total = j.tiles = 0;
    if (j.image < 0 || j.image >= images || j.plane < 0 || j.plane >= nplanes) return false;
    if (!(gate > 0.0)) return false;
    const int32_t* rec = records + (size_t)j.plane * RECORD;
    const int64_t x = rec[R_BOX], y = rec[R_BOX + 1], w = rec[R_BOX + 2], h = rec[R_BOX + 3];
    if (w < 0 || h < 0) return true;
    const int64_t x0 = x < 1 ? 1 : x, y0 = y < 1 ? 1 : y;
    const int64_t x1 = x + w > W - 2 ? W - 2 : x + w, y1 = y + h > H - 2 ? H - 2 : y + h;
    if (x0 > x1 || y0 > y1) return true;
    j.x0 = (int)x0, j.y0 = (int)y0, j.bw = (int)(x1 - x0 + 1), j.bh = (int)(y1 - y0 + 1);   // inside [1, W-2] x [1, H-2]
    j.total = j.bw * j.bh;   // < 2^28
    j.tiles = (j.total + TILE - 1) / TILE;
    return true;
}

ICP_HD double dot3(const double* a, const double* b) {
#pragma clang fp contract(off)
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

ICP_HD void cross3(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// rule 3
ICP_HD void back_project(int x, int y, double z, const Camera& cam, double* p) {
#pragma clang fp contract(off)
    p[0] = (((double)x - cam.cx) * z) / cam.fx;
    p[1] = (((double)y - cam.cy) * z) / cam.fy;
    p[2] = z;
}

// rules 2-6 for pixel (x, y): false when the pixel is skipped
ICP_HD bool pixel(uint32_t bc, uint32_t bl, uint32_t br, uint32_t bu, uint32_t bd, float sensor, int x, int y, const Camera& cam, double gate,
                  double jump, Terms& t) {
#pragma clang fp contract(off)
    if (bc == EMPTY || bl == EMPTY || br == EMPTY || bu == EMPTY || bd == EMPTY) return false;
    if (!(sensor > 0.f)) return false;
    const double z = (double)depth_of(bc), zl = (double)depth_of(bl), zr = (double)depth_of(br), zu = (double)depth_of(bu), zd = (double)depth_of(bd);
    const double d = (double)sensor;
    if (!(absd(zr - zl) < jump) || !(absd(zd - zu) < jump) || !(absd(d - z) < gate)) return false;
    double p[3], pl[3], pr[3], pu[3], pd[3], q[3];
    back_project(x, y, z, cam, p);
    back_project(x - 1, y, zl, cam, pl);
    back_project(x + 1, y, zr, cam, pr);
    back_project(x, y - 1, zu, cam, pu);
    back_project(x, y + 1, zd, cam, pd);
    const double a[3] = {pr[0] - pl[0], pr[1] - pl[1], pr[2] - pl[2]}, b[3] = {pd[0] - pu[0], pd[1] - pu[1], pd[2] - pu[2]};
    double n[3];
    cross3(a, b, n);
    const double len = ICP_SQRT(dot3(n, n));
    if (!(len > 0.0)) return false;
    n[0] = n[0] / len, n[1] = n[1] / len, n[2] = n[2] / len;
    back_project(x, y, d, cam, q);
    const double e[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
    t.r = dot3(n, e);
    cross3(p, n, t.J);
    t.J[3] = n[0], t.J[4] = n[1], t.J[5] = n[2];
    return true;
}

// rule 7 for one pixel: its terms onto a lane's sums
ICP_HD void add_terms(const Terms& t, double* s) {
#pragma clang fp contract(off)
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
            s[k] = s[k] + t.J[a] * t.J[b];
            ++k;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a) s[N_A + a] = s[N_A + a] + t.J[a] * t.r;
    s[N_A + N_B] = s[N_A + N_B] + t.r * t.r;
}

// pixel s of a job's box, read from the plane and the sensor image: every address lies inside the clipped box grown by one pixel, which is
// inside the image (job_setup)
ICP_HD bool job_pixel(const Job& j, int s, const uint32_t* plane, const float* sensor, int W, const Camera& cam, double gate, double jump, Terms& t) {
    const int dy = (int)((unsigned)s / (unsigned)j.bw), y = j.y0 + dy, x = j.x0 + (s - dy * j.bw);
    const size_t at = (size_t)y * W + x;
    const uint32_t bc = plane[at];
    if (bc == EMPTY) return false;
    return pixel(bc, plane[at - 1], plane[at + 1], plane[at - W], plane[at + W], sensor[at], x, y, cam, gate, jump, t);
}

// rule 7 for one tile on the host: the lanes one after the other, then the tree -> sums [SUMS], count
inline void tile_serial(const Job& j, int tile, const uint32_t* plane, const float* sensor, int W, const Camera& cam, double gate, double jump,
                        double* sums, int& count) {
#pragma clang fp contract(off)
    double lane[LANES][SUMS];
    int cnt[LANES];
    for (int l = 0; l < LANES; ++l) {
        cnt[l] = 0;
        for (int k = 0; k < SUMS; ++k) lane[l][k] = 0.0;
        for (int s = tile * TILE + l; s < (tile + 1) * TILE && s < j.total; s += LANES) {
            Terms t;
            if (!job_pixel(j, s, plane, sensor, W, cam, gate, jump, t)) continue;
            add_terms(t, lane[l]);
            cnt[l] += 1;
        }
    }
    for (int off = LANES / 2; off >= 1; off /= 2)
        for (int l = 0; l < off; ++l) {
            for (int k = 0; k < SUMS; ++k) lane[l][k] = lane[l][k] + lane[l + off][k];
            cnt[l] += cnt[l + off];
        }
    for (int k = 0; k < SUMS; ++k) sums[k] = lane[0][k];
    count = cnt[0];
}

// rule 7's last step: a job's tile records (PARTIAL words each) added in index order -> sums [SUMS], count
ICP_HD void add_tiles(const double* partials, int tiles, double* sums, long long& count) {
#pragma clang fp contract(off)
    for (int k = 0; k < SUMS; ++k) sums[k] = 0.0;
    count = 0;
    for (int t = 0; t < tiles; ++t) {
        const double* p = partials + (size_t)t * PARTIAL;
        for (int k = 0; k < SUMS; ++k) sums[k] = sums[k] + p[k];
        count += (long long)p[SUMS];
    }
}

// rules 8-11: the step of one job from its sums.  pose: row-major [3, 4], rewritten only with ST_OK and update != 0.  -> the status
ICP_HD int solve_update(const double* sums, long long count, double damping, int min_pixels, int update, double* pose, double* stats) {
#pragma clang fp contract(off)
    stats[0] = (double)count;
    stats[1] = count > 0 ? ICP_SQRT(sums[N_A + N_B] / (double)count) : 0.0;
    stats[2] = stats[3] = 0.0;
    if (count < (long long)min_pixels) return ST_FEW;
    double L[6][6];
    int k = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) L[b][a] = sums[k++];   // the lower triangle of A
    for (int a = 0; a < 6; ++a) L[a][a] = L[a][a] + damping * L[a][a];
    for (int c = 0; c < 6; ++c) {
        double s = L[c][c];
        for (int m = 0; m < c; ++m) s = s - L[c][m] * L[c][m];
        if (!(s > 0.0)) return ST_SINGULAR;
        const double piv = ICP_SQRT(s);
        L[c][c] = piv;
        for (int r = c + 1; r < 6; ++r) {
            double v = L[r][c];
            for (int m = 0; m < c; ++m) v = v - L[r][m] * L[c][m];
            L[r][c] = v / piv;
        }
    }
    double y[6], xi[6];
    for (int r = 0; r < 6; ++r) {
        double v = sums[N_A + r];
        for (int m = 0; m < r; ++m) v = v - L[r][m] * y[m];
        y[r] = v / L[r][r];
    }
    for (int r = 5; r >= 0; --r) {
        double v = y[r];
        for (int m = r + 1; m < 6; ++m) v = v - L[m][r] * xi[m];
        xi[r] = v / L[r][r];
    }
    stats[2] = ICP_SQRT(dot3(xi, xi));
    stats[3] = ICP_SQRT(dot3(xi + 3, xi + 3));
    if (!update) return ST_OK;
    const double hx = xi[0] / 2.0, hy = xi[1] / 2.0, hz = xi[2] / 2.0;
    const double qn = ICP_SQRT(1.0 + ((hx * hx + hy * hy) + hz * hz));
    const double w = 1.0 / qn, x = hx / qn, yq = hy / qn, z = hz / qn;
    const double dR[9] = {1.0 - 2.0 * (yq * yq + z * z), 2.0 * (x * yq - w * z),        2.0 * (x * z + w * yq),
                          2.0 * (x * yq + w * z),        1.0 - 2.0 * (x * x + z * z),   2.0 * (yq * z - w * x),
                          2.0 * (x * z - w * yq),        2.0 * (yq * z + w * x),        1.0 - 2.0 * (x * x + yq * yq)};
    double out[12];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) {
            const double col[3] = {pose[c], pose[4 + c], pose[8 + c]};
            out[4 * r + c] = dot3(dR + 3 * r, col);
        }
    out[3] = out[3] + xi[3], out[7] = out[7] + xi[4], out[11] = out[11] + xi[5];
    for (int i = 0; i < 12; ++i) pose[i] = out[i];
    return ST_OK;
}

// The serial step: the same rules, one loop nest (what the host twin runs).  planes uint32 [nplanes][H][W], records int32 [nplanes][RECORD],
// depth float [images][H][W], cams double [images][4], jobs int32 [njobs][4], gates double [njobs], poses double [nplanes][12], stats double
// [njobs][4], status int32 [njobs], partials: workspace_bytes(njobs, H, W) bytes.
inline void step_serial(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth, const double* cams,
                        int images, const int32_t* jobs, const double* gates, int njobs, double jump, double damping, int min_pixels, int update,
                        double* poses, double* stats, int32_t* status, double* partials) {
    const size_t hw = (size_t)H * (size_t)W, per_job = (size_t)max_tiles(H, W) * PARTIAL;
    for (int n = 0; n < njobs; ++n) {
        Job j;
        double* st = stats + 4 * (size_t)n;
        if (!job_setup(jobs + 4 * (size_t)n, gates[n], records, nplanes, images, H, W, j)) {
            st[0] = st[1] = st[2] = st[3] = 0.0;
            status[n] = ST_REFUSED;
            continue;
        }
        const Camera cam = {cams[4 * j.image], cams[4 * j.image + 1], cams[4 * j.image + 2], cams[4 * j.image + 3]};
        double* part = partials + (size_t)n * per_job;
        for (int t = 0; t < j.tiles; ++t) {
            int count;
            tile_serial(j, t, planes + (size_t)j.plane * hw, depth + (size_t)j.image * hw, W, cam, gates[n], jump * gates[n], part + (size_t)t * PARTIAL, count);
            part[(size_t)t * PARTIAL + SUMS] = (double)count;
        }
        double sums[SUMS];
        long long count;
        add_tiles(part, j.tiles, sums, count);
        status[n] = solve_update(sums, count, damping, min_pixels, update, poses + 12 * (size_t)j.plane, st);
    }
}

}  // namespace cp_icp
