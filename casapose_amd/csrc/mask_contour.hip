// Contour alignment against the network's label map (contour_math.h states the rules): the distance field of every (image, label) job's trusted
// silhouette boundary, and one 2-D Gauss-Newton step per (image, render plane) job on the rendered contour.  The render planes and records are
// what cp_render_masks_u8 left behind, the poses are the renderer's own device array; this file is the schedule.
//
// edt_rows_kernel: one block of 256 threads per (job, row, 256 columns).  The seed flags of the columns x0 - G .. x0 + 255 + G of the row go to
//   LDS (each from five label bytes, the lanes on consecutive columns), then thread x scans outwards from its column in LDS, at most G steps,
//   and stores the clamped squared distance as uint16 to the workspace.  The first block of a job writes its status.
// edt_cols_kernel: one block per (job, 32 rows x 64 columns).  The rows of the workspace that lie within G of the tile are staged in LDS 128 at
//   a time (a row of the stage is 64 uint16 = 128 bytes, read from global memory by one wave); thread (column, row group) reads each staged
//   value once and updates its eight output rows' running minima, so a staged row serves all 32 output rows.  The lanes of a wave read
//   consecutive uint16 of one staged row: no bank conflicts.  Integers only, no atomics, every pixel of the plane is written exactly once.
// The step's two launches and its host loop are icp_math.h's (accumulate_kernel, solve_kernel, step_serial), on cp_contour::Contour's terms.
// Every index read from device memory (image, label, plane, field, gate, the box corners) is range-checked before it addresses anything.
#include <cmath>
#include <vector>

#include "common.h"
#include "contour_math.h"

namespace {

using namespace cp_contour;

constexpr int THREADS = 256;
constexpr int COL_TX = 64, COL_TY = 32, COL_STAGE = 128, COL_GROUPS = THREADS / COL_TX, COL_OUT = COL_TY / COL_GROUPS;

__global__ void __launch_bounds__(THREADS) edt_rows_kernel(const uint8_t* __restrict__ labels, int images, int H, int W, const int32_t* __restrict__ jobs,
                                                          int G, uint16_t* __restrict__ rows, int32_t* __restrict__ status) {
    __shared__ uint8_t s_flags[THREADS + 2 * MAX_GATE + 2];
    const unsigned segs = (unsigned)(W + THREADS - 1) / THREADS, per_job = (unsigned)H * segs;
    const size_t n = blockIdx.x / per_job;
    const unsigned rem = blockIdx.x % per_job;
    const int y = (int)(rem / segs), x0 = (int)(rem % segs) * THREADS, tid = threadIdx.x;
    const bool ok = edt_job_ok(jobs + 2 * n, images);   // block-uniform
    if (rem == 0 && tid == 0) status[n] = ok ? ST_OK : ST_REFUSED;
    if (!ok) return;
    const size_t hw = (size_t)H * (size_t)W;
    const uint8_t* __restrict__ lab = labels + (size_t)jobs[2 * n] * hw;
    const int l = jobs[2 * n + 1], base = x0 - G;
    for (int i = tid; i < THREADS + 2 * G; i += THREADS) {
        const int c = base + i;
        s_flags[i] = (c >= 0 && c < W) ? (uint8_t)is_seed(lab, H, W, c, y, l) : (uint8_t)0;
    }
    __syncthreads();
    const int x = x0 + tid;
    if (x < W) rows[n * hw + (size_t)y * W + x] = row_value(s_flags, base, W, x, G);   // indices 0 .. 255 + 2 G of s_flags
}

__global__ void __launch_bounds__(THREADS) edt_cols_kernel(const int32_t* __restrict__ jobs, int images, int H, int W, int G,
                                                          const uint16_t* __restrict__ rows, uint16_t* __restrict__ planes) {
    __shared__ uint16_t s_win[COL_STAGE][COL_TX];
    const unsigned tiles_x = (unsigned)(W + COL_TX - 1) / COL_TX, per_job = tiles_x * ((unsigned)(H + COL_TY - 1) / COL_TY);
    const size_t n = blockIdx.x / per_job;
    const unsigned rem = blockIdx.x % per_job;
    if (!edt_job_ok(jobs + 2 * n, images)) return;   // block-uniform
    const int y0 = (int)(rem / tiles_x) * COL_TY, x0 = (int)(rem % tiles_x) * COL_TX;
    const int tx = threadIdx.x & (COL_TX - 1), group = threadIdx.x / COL_TX, x = x0 + tx;
    const size_t hw = (size_t)H * (size_t)W;
    const uint16_t* __restrict__ R = rows + n * hw;
    const int clamp = clamp_of(G);
    const int first = y0 - G < 0 ? 0 : y0 - G, last = y0 + COL_TY - 1 + G > H - 1 ? H - 1 : y0 + COL_TY - 1 + G;   // rows of the image: first <= last
    int best[COL_OUT];
#pragma unroll
    for (int k = 0; k < COL_OUT; ++k) best[k] = clamp;
    for (int c0 = first; c0 <= last; c0 += COL_STAGE) {
        const int here = last - c0 + 1 < COL_STAGE ? last - c0 + 1 : COL_STAGE;
        for (int r = group; r < here; r += COL_GROUPS) s_win[r][tx] = x < W ? R[(size_t)(c0 + r) * W + x] : (uint16_t)clamp;
        __syncthreads();
        for (int r = 0; r < here; ++r) {
            const int v = s_win[r][tx], dy = c0 + r - (y0 + group);
#pragma unroll
            for (int k = 0; k < COL_OUT; ++k) best[k] = col_min(best[k], v, dy - k * COL_GROUPS);
        }
        __syncthreads();
    }
    if (x < W) {
        uint16_t* __restrict__ D = planes + n * hw;
#pragma unroll
        for (int k = 0; k < COL_OUT; ++k) {
            const int y = y0 + group + k * COL_GROUPS;
            if (y < H) D[(size_t)y * W + x] = (uint16_t)best[k];
        }
    }
}

// the rasteriser's sample point in whole 256ths of a pixel (cp_mask::sample_origin), as pixels
double sample_of(double sample_offset) { return rint(256.0 * sample_offset) / 256.0; }

long long edt_row_blocks(int njobs, int H, int W) { return (long long)njobs * H * ((W + THREADS - 1) / THREADS); }
long long edt_col_blocks(int njobs, int H, int W) { return (long long)njobs * ((H + COL_TY - 1) / COL_TY) * ((W + COL_TX - 1) / COL_TX); }

int check_edt(const char* fn, const uint8_t* labels, int images, int H, int W, const int32_t* jobs, int njobs, int gate, uint16_t* planes, int32_t* status,
              void* workspace, size_t workspace_bytes) {
    CP_REQUIRE(labels && jobs && planes && status && workspace, "%s: null pointer", fn);
    CP_REQUIRE(images >= 1 && njobs >= 1, "%s: images and njobs must be positive (got %d, %d)", fn, images, njobs);
    CP_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "%s: H and W must lie in [1, %d] (got %d x %d)", fn, MAX_SIDE, H, W);
    CP_REQUIRE(gate >= 1 && gate <= MAX_GATE, "%s: gate must lie in [1, %d] pixels (got %d)", fn, MAX_GATE, gate);
    CP_REQUIRE(edt_row_blocks(njobs, H, W) <= 0x7fffffffLL && edt_col_blocks(njobs, H, W) <= 0x7fffffffLL,
               "%s: njobs %d at %d x %d is above 2^31 - 1 blocks; split the call", fn, njobs, H, W);
    CP_REQUIRE(workspace_bytes >= edt_workspace_bytes(njobs, H, W), "%s: workspace_bytes %zu is below cp_mask_edt_workspace_bytes = %zu", fn,
               workspace_bytes, edt_workspace_bytes(njobs, H, W));
    CP_REQUIRE(((uintptr_t)jobs & 3) == 0 && ((uintptr_t)status & 3) == 0, "%s: jobs and status must be 4-byte aligned", fn);
    CP_REQUIRE(((uintptr_t)planes & 1) == 0 && ((uintptr_t)workspace & 1) == 0, "%s: planes and workspace must be 2-byte aligned", fn);
    return CP_OK;
}

int check_step(const char* fn, const Contour::Args& a, int njobs, double sample_offset, double damping, int min_pixels, int update, int split, double* poses,
               double* stats, int32_t* status, void* workspace, size_t workspace_bytes) {
    CP_REQUIRE(a.planes && a.records && a.fields && a.cams && a.jobs && poses && stats && status && workspace, "%s: null pointer", fn);
    CP_REQUIRE(a.nplanes >= 1 && a.nfields >= 1 && a.images >= 1 && njobs >= 1, "%s: nplanes, nfields, images and njobs must be positive (got %d, %d, %d, %d)",
               fn, a.nplanes, a.nfields, a.images, njobs);
    if (int rc = cp_icp::check_step(fn, a.nplanes, a.H, a.W, njobs, damping, min_pixels, update, split, workspace_bytes, "cp_contour_step_workspace_bytes",
                                    cp_contour::workspace_bytes<Contour>(njobs, a.H, a.W)))
        return rc;
    CP_REQUIRE(sample_offset >= 0.0 && sample_offset <= 1.0, "%s: sample_offset must lie in [0, 1] (got %g)", fn, sample_offset);
    CP_REQUIRE(((uintptr_t)a.planes & 3) == 0 && ((uintptr_t)a.records & 3) == 0 && ((uintptr_t)a.jobs & 3) == 0 && ((uintptr_t)status & 3) == 0,
               "%s: planes, records, jobs and status must be 4-byte aligned", fn);
    CP_REQUIRE(((uintptr_t)a.fields & 1) == 0, "%s: fields must be 2-byte aligned", fn);
    CP_REQUIRE(((uintptr_t)a.cams & 7) == 0 && ((uintptr_t)poses & 7) == 0 && ((uintptr_t)stats & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
               "%s: cams, poses, stats and workspace must be 8-byte aligned", fn);
    return CP_OK;
}

}  // namespace

extern "C" int cp_contour_tile(void) { return TILE; }

extern "C" size_t cp_mask_edt_workspace_bytes(int njobs, int H, int W) {
    if (njobs < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return 0;
    if (edt_row_blocks(njobs, H, W) > 0x7fffffffLL || edt_col_blocks(njobs, H, W) > 0x7fffffffLL) return 0;
    return edt_workspace_bytes(njobs, H, W);
}

extern "C" size_t cp_contour_step_workspace_bytes(int njobs, int H, int W) {
    if (njobs < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return 0;
    return workspace_bytes<Contour>(njobs, H, W);
}

extern "C" int cp_mask_edt_u16(const uint8_t* labels, int images, int H, int W, const int32_t* jobs, int njobs, int gate, uint16_t* planes,
                               int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_edt("cp_mask_edt_u16", labels, images, H, W, jobs, njobs, gate, planes, status, workspace, workspace_bytes)) return rc;
    hipStream_t st = (hipStream_t)stream;
    CP_LAUNCH(edt_rows_kernel, dim3((unsigned)edt_row_blocks(njobs, H, W)), dim3(THREADS), 0, st, labels, images, H, W, jobs, gate, (uint16_t*)workspace,
              status);
    if (int rc = cp::check_launch("cp_mask_edt_u16 (rows)")) return rc;
    CP_LAUNCH(edt_cols_kernel, dim3((unsigned)edt_col_blocks(njobs, H, W)), dim3(THREADS), 0, st, jobs, images, H, W, gate, (const uint16_t*)workspace,
              planes);
    return cp::check_launch("cp_mask_edt_u16 (columns)");
}

extern "C" int cp_mask_edt_host_u16(const uint8_t* labels, int images, int H, int W, const int32_t* jobs, int njobs, int gate, uint16_t* planes,
                                    int32_t* status, void* workspace, size_t workspace_bytes) {
    if (int rc = check_edt("cp_mask_edt_host_u16", labels, images, H, W, jobs, njobs, gate, planes, status, workspace, workspace_bytes)) return rc;
    std::vector<uint8_t> flags((size_t)W);
    edt_serial(labels, images, H, W, jobs, njobs, gate, planes, status, (uint16_t*)workspace, flags.data());
    return CP_OK;
}

extern "C" int cp_contour_step_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const uint16_t* fields, int nfields,
                                   const double* cams, int images, const int32_t* jobs, int njobs, double sample_offset, double damping, int min_pixels, int update,
                                   int split, double* poses, double* stats, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    const Contour::Args a = {planes, records, nplanes, H, W, fields, nfields, cams, images, jobs, sample_of(sample_offset)};
    if (int rc = check_step("cp_contour_step_f64", a, njobs, sample_offset, damping, min_pixels, update, split, poses, stats, status, workspace, workspace_bytes))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long per_job = cp_icp::max_tiles(H, W) * PARTIAL<Contour>;
    CP_LAUNCH(cp_icp::accumulate_kernel<Contour>, dim3((unsigned)((long long)njobs * split)), dim3(cp_icp::THREADS), 0, st, a, njobs, split, per_job,
              (double*)workspace);
    if (int rc = cp::check_launch("cp_contour_step_f64 (accumulate)")) return rc;
    CP_LAUNCH(cp_icp::solve_kernel<Contour>, dim3((unsigned)njobs), dim3(LANES), 0, st, a, damping, min_pixels, update, per_job, (const double*)workspace, poses,
              stats, status);
    return cp::check_launch("cp_contour_step_f64 (solve)");
}

extern "C" int cp_contour_step_host_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const uint16_t* fields, int nfields,
                                        const double* cams, int images, const int32_t* jobs, int njobs, double sample_offset, double damping, int min_pixels,
                                        int update, int split, double* poses, double* stats, int32_t* status, void* workspace, size_t workspace_bytes) {
    const Contour::Args a = {planes, records, nplanes, H, W, fields, nfields, cams, images, jobs, sample_of(sample_offset)};
    if (int rc = check_step("cp_contour_step_host_f64", a, njobs, sample_offset, damping, min_pixels, update, split, poses, stats, status, workspace,
                            workspace_bytes))
        return rc;
    step_serial<Contour>(a, njobs, damping, min_pixels, update, poses, stats, status, (double*)workspace);
    return CP_OK;
}
