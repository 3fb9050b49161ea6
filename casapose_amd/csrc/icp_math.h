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
//
// Rules 7-11 do not depend on what a pixel contributes, and contour_math.h has other terms on the same sums.  So the second half of this
// header is the step of any such refiner, once: the host's tile and job loop, and for hipcc the two kernels and the argument checks that
// depth_icp.hip and mask_contour.hip share.  A refiner hands them its terms as a struct (Depth below, cp_contour::Contour).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "plane_record.h"

#if defined(__HIPCC__)
#include "common.h"   // CP_REQUIRE, for check_step
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
constexpr int MAX_SPLIT = 64;            // blocks per job
constexpr int ST_OK = 0, ST_FEW = 1, ST_SINGULAR = 2, ST_REFUSED = 3;
using cp_plane::Box, cp_plane::Camera, cp_plane::clipped_box, cp_plane::depth_of, cp_plane::EMPTY, cp_plane::MAX_SIDE, cp_plane::R_BOX_OBJ, cp_plane::RECORD;

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

// the tiles of the largest clipped box of an H x W image: what the workspace holds per job
ICP_HD long long max_tiles(int H, int W) {
    if (H < 3 || W < 3) return 1;
    return ((long long)(H - 2) * (long long)(W - 2) + TILE - 1) / TILE;
}

// rules 1 and 10: false when the job is refused.  job: (image, plane, unused, unused).  Reads the plane's record only when it returns true.
ICP_HD bool job_setup(const int32_t* job, double gate, const int32_t* records, int nplanes, int images, int H, int W, Job& j) {
    j.image = job[0], j.plane = job[1];
    j.x0 = j.y0 = j.bw = j.bh = j.total = j.tiles = 0;
    if (j.image < 0 || j.image >= images || j.plane < 0 || j.plane >= nplanes) return false;
    if (!(gate > 0.0)) return false;
    Box b;
    if (!clipped_box(records + (size_t)j.plane * RECORD, H, W, 1, b)) return true;   // nothing to walk is no refusal
    j.x0 = b.x0, j.y0 = b.y0, j.bw = b.x1 - b.x0 + 1, j.bh = b.y1 - b.y0 + 1;        // inside [1, W-2] x [1, H-2]
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

// The depth refiner's terms, as the step below takes them from any refiner:
//   COUNTS   the integer counts of a tile's record, after its SUMS sums (each exact: <= TILE)
//   Args     one call's arrays and settings (H and W among them): planes uint32 [nplanes][H][W], records int32 [nplanes][RECORD], depth float
//            [images][H][W], cams double [images][4], jobs int32 [njobs][4], gates double [njobs]
//   Context  one job's values, its data pointers resolved: what the walk reads
//   setup    job n of a call -> false when it is refused (nothing is read for it then, and c is left alone)
//   add      pixel s of the job's box: its terms onto a lane's sums and counts, or nothing
//   solve    rules 8-11 from a job's totals
struct Depth {
    static constexpr int COUNTS = 1;   // the pixels used
    struct Args {
        const uint32_t* planes;
        const int32_t* records;
        int nplanes, H, W;
        const float* depth;
        const double* cams;
        int images;
        const int32_t* jobs;
        const double* gates;
        double jump;
    };
    struct Context {
        const uint32_t* plane;
        const float* sensor;
        int W;
        Camera cam;
        double gate, step;   // step = jump gate (rule 2)
    };
    static ICP_HD bool setup(const Args& a, size_t n, Job& j, Context& c) {
#pragma clang fp contract(off)
        const double gate = a.gates[n];
        if (!job_setup(a.jobs + 4 * n, gate, a.records, a.nplanes, a.images, a.H, a.W, j)) return false;
        const size_t hw = (size_t)a.H * (size_t)a.W;
        const double* cam = a.cams + 4 * (size_t)j.image;
        c = {a.planes + (size_t)j.plane * hw, a.depth + (size_t)j.image * hw, a.W, {cam[0], cam[1], cam[2], cam[3]}, gate, a.jump * gate};
        return true;
    }
    static ICP_HD void add(const Job& j, const Context& c, int s, double* sums, int* counts) {
        Terms t;
        if (!job_pixel(j, s, c.plane, c.sensor, c.W, c.cam, c.gate, c.step, t)) return;
        add_terms(t, sums);
        counts[0] += 1;
    }
    static ICP_HD int solve(const double* sums, const long long* counts, double damping, int min_pixels, int update, double* pose, double* stats) {
        return solve_update(sums, counts[0], damping, min_pixels, update, pose, stats);
    }
};

// ---- the step of a refiner P: rule 7's order, once for the host and once for the device -----------------------------------------------------
template <class P>
constexpr int PARTIAL = SUMS + P::COUNTS;   // fp64 words of a tile's record in the workspace: the sums, then the counts

template <class P>
ICP_HD size_t workspace_bytes(int njobs, int H, int W) {
    return (size_t)njobs * (size_t)max_tiles(H, W) * PARTIAL<P> * sizeof(double);
}

// rule 7 for one tile on the host: the lanes one after the other, then the tree -> the tile's record
template <class P>
inline void tile_serial(const Job& j, const typename P::Context& c, int tile, double* record) {
#pragma clang fp contract(off)
    double lane[LANES][SUMS];
    int cnt[LANES][P::COUNTS];
    for (int l = 0; l < LANES; ++l) {
        for (int k = 0; k < SUMS; ++k) lane[l][k] = 0.0;
        for (int k = 0; k < P::COUNTS; ++k) cnt[l][k] = 0;
        for (int s = tile * TILE + l; s < (tile + 1) * TILE && s < j.total; s += LANES) P::add(j, c, s, lane[l], cnt[l]);
    }
    for (int off = LANES / 2; off >= 1; off /= 2)
        for (int l = 0; l < off; ++l) {
            for (int k = 0; k < SUMS; ++k) lane[l][k] = lane[l][k] + lane[l + off][k];
            for (int k = 0; k < P::COUNTS; ++k) cnt[l][k] += cnt[l + off][k];
        }
    for (int k = 0; k < SUMS; ++k) record[k] = lane[0][k];
    for (int k = 0; k < P::COUNTS; ++k) record[SUMS + k] = (double)cnt[0][k];
}

// rule 7's last step: a job's tile records (SUMS + NCOUNTS words each) added in index order -> sums [SUMS], counts [NCOUNTS]
template <int NCOUNTS>
ICP_HD void add_tiles(const double* partials, int tiles, double* sums, long long* counts) {
#pragma clang fp contract(off)
    for (int k = 0; k < SUMS; ++k) sums[k] = 0.0;
    for (int k = 0; k < NCOUNTS; ++k) counts[k] = 0;
    for (int t = 0; t < tiles; ++t) {
        const double* p = partials + (size_t)t * (SUMS + NCOUNTS);
        for (int k = 0; k < SUMS; ++k) sums[k] = sums[k] + p[k];
        for (int k = 0; k < NCOUNTS; ++k) counts[k] += (long long)p[SUMS + k];
    }
}

// The serial step: the same rules, one loop nest (what the host twins run).  poses double [nplanes][12], stats double [njobs][4], status int32
// [njobs], partials: workspace_bytes<P>(njobs, H, W) bytes.
template <class P>
inline void step_serial(const typename P::Args& a, int njobs, double damping, int min_pixels, int update, double* poses, double* stats, int32_t* status,
                        double* partials) {
    const size_t per_job = (size_t)max_tiles(a.H, a.W) * PARTIAL<P>;
    for (int n = 0; n < njobs; ++n) {
        Job j;
        typename P::Context c;
        double* st = stats + 4 * (size_t)n;
        if (!P::setup(a, (size_t)n, j, c)) {
            st[0] = st[1] = st[2] = st[3] = 0.0;
            status[n] = ST_REFUSED;
            continue;
        }
        double* part = partials + (size_t)n * per_job;
        for (int t = 0; t < j.tiles; ++t) tile_serial<P>(j, c, t, part + (size_t)t * PARTIAL<P>);
        double sums[SUMS];
        long long counts[P::COUNTS];
        add_tiles<P::COUNTS>(part, j.tiles, sums, counts);
        status[n] = P::solve(sums, counts, damping, min_pixels, update, poses + 12 * (size_t)j.plane, st);
    }
}

#if defined(__HIPCC__)
// The same step on the device, two launches.
// accumulate_kernel: grid (split * jobs) on x, part-major (block b is part b / jobs of job b % jobs: neighbouring blocks are different jobs, so
//   the parts that have tiles -- often only part 0 -- spread over the XCDs for every split), 256 threads = 4 waves.  A tile of TILE = 1024 pixels
//   of the job's clipped box belongs to one wave: wave w of block `part` takes tiles part * 4 + w, + split * 4, ...  Pixel s of the box is row
//   s / bw, column s % bw, so the lanes of a wave read runs of consecutive words of a row of the plane and of the rows above and below.  Lane l
//   keeps the 28 fp64 sums and the counts of its 16 pixels of the tile, the 64 lanes combine by an xor butterfly (both partners of a pair add
//   the same two numbers, so every lane ends with the bits of rule 7's tree), and lane k stores word k of the tile's record.  No LDS, no
//   atomics, and every tile of a job is written: the workspace needs no initialisation and the bits do not depend on split.
// solve_kernel: one wave per job.  Lane k adds word k of the job's tile records in index order; lane 0 takes the totals from LDS, solves,
//   rewrites the pose in place (only with ST_OK and update) and writes stats and status.  A refused job gets zeros and ST_REFUSED.
// Every index read from device memory is range-checked before it addresses anything (P::setup).
constexpr int THREADS = 256, WAVES = THREADS / LANES;

template <class P>
__global__ void __launch_bounds__(THREADS) accumulate_kernel(const typename P::Args a, int njobs, int split, long long per_job, double* __restrict__ partials) {
    const int lane = threadIdx.x & (LANES - 1), wave = threadIdx.x / LANES;
    const size_t n = blockIdx.x % (unsigned)njobs;
    const int part = (int)(blockIdx.x / (unsigned)njobs);
    Job j;
    typename P::Context c;
    if (!P::setup(a, n, j, c)) return;   // block-uniform
    double* __restrict__ out = partials + n * (size_t)per_job;

    for (int tile = part * WAVES + wave; tile < j.tiles; tile += split * WAVES) {   // wave-uniform
        double acc[SUMS];
        int cnt[P::COUNTS];
#pragma unroll
        for (int k = 0; k < SUMS; ++k) acc[k] = 0.0;
#pragma unroll
        for (int k = 0; k < P::COUNTS; ++k) cnt[k] = 0;
        for (int s = tile * TILE + lane; s < (tile + 1) * TILE && s < j.total; s += LANES) P::add(j, c, s, acc, cnt);
#pragma unroll
        for (int off = LANES / 2; off >= 1; off >>= 1) {
#pragma unroll
            for (int k = 0; k < SUMS; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], off);
#pragma unroll
            for (int k = 0; k < P::COUNTS; ++k) cnt[k] += __shfl_xor(cnt[k], off);
        }
        double mine = (double)cnt[P::COUNTS - 1];   // words SUMS .. of the record are the counts
#pragma unroll
        for (int k = 0; k < P::COUNTS - 1; ++k)
            if (lane == SUMS + k) mine = (double)cnt[k];
#pragma unroll
        for (int k = 0; k < SUMS; ++k)
            if (lane == k) mine = acc[k];
        if (lane < PARTIAL<P>) out[(size_t)tile * PARTIAL<P> + lane] = mine;
    }
}

template <class P>
__global__ void __launch_bounds__(LANES) solve_kernel(const typename P::Args a, double damping, int min_pixels, int update, long long per_job,
                                                      const double* __restrict__ partials, double* __restrict__ poses, double* __restrict__ stats,
                                                      int32_t* __restrict__ status) {
    __shared__ double s_sums[PARTIAL<P>];
    const int lane = threadIdx.x;
    const size_t n = blockIdx.x;
    Job j;
    typename P::Context c;
    if (!P::setup(a, n, j, c)) {   // block-uniform
        if (lane < 4) stats[4 * n + lane] = 0.0;
        if (lane == 0) status[n] = ST_REFUSED;
        return;
    }
    if (lane < PARTIAL<P>) {
        const double* __restrict__ p = partials + n * (size_t)per_job + lane;
        double sum = 0.0;
        for (int t = 0; t < j.tiles; ++t) sum = sum + p[(size_t)t * PARTIAL<P>];
        s_sums[lane] = sum;
    }
    __syncthreads();
    if (lane != 0) return;
    double sums[SUMS], pose[12], st[4];
    long long counts[P::COUNTS];
#pragma unroll
    for (int k = 0; k < SUMS; ++k) sums[k] = s_sums[k];
#pragma unroll
    for (int k = 0; k < P::COUNTS; ++k) counts[k] = (long long)s_sums[SUMS + k];
    double* __restrict__ pp = poses + 12 * (size_t)j.plane;
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = pp[k];
    const int code = P::solve(sums, counts, damping, min_pixels, update, pose, st);
    if (code == ST_OK && update) {
#pragma unroll
        for (int k = 0; k < 12; ++k) pp[k] = pose[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) stats[4 * n + k] = st[k];
    status[n] = code;
}

// what both entry points ask of their arguments, after their own null-pointer and count checks; query: the name of the workspace's size call
inline int check_step(const char* fn, int nplanes, int H, int W, int njobs, double damping, int min_pixels, int update, int split, size_t workspace_bytes,
                      const char* query, size_t needed) {
    CP_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "%s: H and W must lie in [1, %d] (got %d x %d)", fn, MAX_SIDE, H, W);
    CP_REQUIRE((long long)nplanes < (1ll << 31) / 12, "%s: nplanes %d is too large", fn, nplanes);
    CP_REQUIRE(damping >= 0.0 && damping <= 1.7976931348623157e308, "%s: damping must be finite and not negative (got %g)", fn, damping);
    CP_REQUIRE(min_pixels >= 1, "%s: min_pixels must be positive (got %d)", fn, min_pixels);
    CP_REQUIRE(update == 0 || update == 1, "%s: update must be 0 or 1 (got %d)", fn, update);
    CP_REQUIRE(split >= 1 && split <= MAX_SPLIT, "%s: split must lie in [1, %d] blocks per job (got %d)", fn, MAX_SPLIT, split);
    CP_REQUIRE((long long)njobs * split <= 0x7fffffffLL, "%s: njobs %d x split %d is above 2^31 - 1 blocks; split the call", fn, njobs, split);
    CP_REQUIRE(workspace_bytes >= needed, "%s: workspace_bytes %zu is below %s = %zu", fn, workspace_bytes, query, needed);
    return CP_OK;
}
#endif

}  // namespace cp_icp
