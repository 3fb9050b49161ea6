// One projective point-to-plane ICP step per (image, render plane) job against the sensor's depth image (icp_math.h states the rules).  The
// planes and records are what cp_render_masks_u8 left behind, the poses are the renderer's own device array; this file is the schedule.
//
// icp_accumulate_kernel: grid (split * jobs) on x, part-major (block b is part b / jobs of job b % jobs: neighbouring blocks are different jobs,
//   so the parts that have tiles -- often only part 0 -- spread over the XCDs for every split), 256 threads = 4 waves.  A tile of TILE = 1024
//   pixels of the job's clipped box belongs to one wave: wave w of block `part` takes tiles part * 4 + w, + split * 4, ...  Pixel s of the
//   box is row s / bw, column s % bw, so the lanes of a wave read runs of consecutive words of a row of the plane, of the rows above and below
//   and of the sensor depth.  Lane l keeps 28 fp64 sums and a count over its 16 pixels of the tile, the 64 lanes combine by an xor butterfly
//   (both partners of a pair add the same two numbers, so every lane ends with the bits of icp_math.h's tree), and lanes 0..28 store the
//   tile's record, one word each.  No LDS, no atomics, and every tile of a job is written: the workspace needs no initialisation and the
//   bits do not depend on split.
// icp_solve_kernel: one wave per job.  Lane k < 29 adds word k of the job's tile records in index order; lane 0 takes the 29 totals from LDS,
//   solves, rewrites the pose in place and writes stats and status.
// Every index read from device memory (image, plane, the box corners) is range-checked before it addresses anything (job_setup).
#include "common.h"
#include "icp_math.h"

namespace {

using namespace cp_icp;

constexpr int THREADS = 256, WAVE = LANES, WAVES = THREADS / WAVE;

__global__ void __launch_bounds__(THREADS) icp_accumulate_kernel(const uint32_t* __restrict__ planes, const int32_t* __restrict__ records, int nplanes,
                                                                int H, int W, const float* __restrict__ depth, const double* __restrict__ cams,
                                                                int images, const int32_t* __restrict__ jobs, const double* __restrict__ gates,
                                                                int njobs, double jump, int split, long long per_job,
                                                                double* __restrict__ partials) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const size_t n = blockIdx.x % (unsigned)njobs;
    const int part = (int)(blockIdx.x / (unsigned)njobs);
    const double gate = gates[n], step = jump * gate;
    Job j;
    if (!job_setup(jobs + 4 * n, gate, records, nplanes, images, H, W, j)) return;   // block-uniform
    const size_t hw = (size_t)H * (size_t)W;
    const Camera cam = {cams[4 * j.image], cams[4 * j.image + 1], cams[4 * j.image + 2], cams[4 * j.image + 3]};
    const uint32_t* __restrict__ plane = planes + (size_t)j.plane * hw;
    const float* __restrict__ sensor = depth + (size_t)j.image * hw;
    double* __restrict__ out = partials + n * (size_t)per_job;

    for (int tile = part * WAVES + wave; tile < j.tiles; tile += split * WAVES) {   // wave-uniform
        double acc[SUMS];
#pragma unroll
        for (int k = 0; k < SUMS; ++k) acc[k] = 0.0;
        int cnt = 0;
        for (int s = tile * TILE + lane; s < (tile + 1) * TILE && s < j.total; s += WAVE) {
            Terms t;
            if (!job_pixel(j, s, plane, sensor, W, cam, gate, step, t)) continue;
            add_terms(t, acc);
            cnt += 1;
        }
#pragma unroll
        for (int off = WAVE / 2; off >= 1; off >>= 1) {
#pragma unroll
            for (int k = 0; k < SUMS; ++k) acc[k] = acc[k] + __shfl_xor(acc[k], off);
            cnt += __shfl_xor(cnt, off);
        }
        double mine = (double)cnt;   // word SUMS
#pragma unroll
        for (int k = 0; k < SUMS; ++k)
            if (lane == k) mine = acc[k];
        if (lane < PARTIAL) out[(size_t)tile * PARTIAL + lane] = mine;
    }
}

__global__ void __launch_bounds__(WAVE) icp_solve_kernel(const int32_t* __restrict__ records, int nplanes, int H, int W, int images,
                                                         const int32_t* __restrict__ jobs, const double* __restrict__ gates, double damping,
                                                         int min_pixels, int update, long long per_job, const double* __restrict__ partials,
                                                         double* __restrict__ poses, double* __restrict__ stats, int32_t* __restrict__ status) {
    __shared__ double s_sums[PARTIAL];
    const int lane = threadIdx.x;
    const size_t n = blockIdx.x;
    Job j;
    if (!job_setup(jobs + 4 * n, gates[n], records, nplanes, images, H, W, j)) {   // block-uniform
        if (lane < 4) stats[4 * n + lane] = 0.0;
        if (lane == 0) status[n] = ST_REFUSED;
        return;
    }
    if (lane < PARTIAL) {
        const double* __restrict__ p = partials + n * (size_t)per_job + lane;
        double sum = 0.0;
        for (int t = 0; t < j.tiles; ++t) sum = sum + p[(size_t)t * PARTIAL];
        s_sums[lane] = sum;
    }
    __syncthreads();
    if (lane != 0) return;
    double sums[SUMS], pose[12], st[4];
#pragma unroll
    for (int k = 0; k < SUMS; ++k) sums[k] = s_sums[k];
    double* __restrict__ P = poses + 12 * (size_t)j.plane;
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = P[k];
    const int code = solve_update(sums, (long long)s_sums[SUMS], damping, min_pixels, update, pose, st);
    if (code == ST_OK && update) {
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = pose[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) stats[4 * n + k] = st[k];
    status[n] = code;
}

int check_arguments(const char* fn, const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth, const double* cams,
                    int images, const int32_t* jobs, const double* gates, int njobs, double jump, double damping, int min_pixels, int update, int split,
                    double* poses, double* stats, int32_t* status, void* workspace, size_t workspace_bytes) {
    CP_REQUIRE(planes && records && depth && cams && jobs && gates && poses && stats && status && workspace, "%s: null pointer", fn);
    CP_REQUIRE(nplanes >= 1 && images >= 1 && njobs >= 1, "%s: nplanes, images and njobs must be positive (got %d, %d, %d)", fn, nplanes, images, njobs);
    CP_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "%s: H and W must lie in [1, %d] (got %d x %d)", fn, MAX_SIDE, H, W);
    CP_REQUIRE((long long)nplanes < (1ll << 31) / 12, "%s: nplanes %d is too large", fn, nplanes);
    CP_REQUIRE(jump > 0.0, "%s: jump must be positive (got %g)", fn, jump);
    CP_REQUIRE(damping >= 0.0 && damping <= 1.7976931348623157e308, "%s: damping must be finite and not negative (got %g)", fn, damping);
    CP_REQUIRE(min_pixels >= 1, "%s: min_pixels must be positive (got %d)", fn, min_pixels);
    CP_REQUIRE(update == 0 || update == 1, "%s: update must be 0 or 1 (got %d)", fn, update);
    CP_REQUIRE(split >= 1 && split <= MAX_SPLIT, "%s: split must lie in [1, %d] blocks per job (got %d)", fn, MAX_SPLIT, split);
    CP_REQUIRE((long long)njobs * split <= 0x7fffffffLL, "%s: njobs %d x split %d is above 2^31 - 1 blocks; split the call", fn, njobs, split);
    CP_REQUIRE(workspace_bytes >= cp_icp::workspace_bytes(njobs, H, W), "%s: workspace_bytes %zu is below cp_depth_icp_workspace_bytes = %zu", fn,
               workspace_bytes, cp_icp::workspace_bytes(njobs, H, W));
    CP_REQUIRE(((uintptr_t)planes & 3) == 0 && ((uintptr_t)records & 3) == 0 && ((uintptr_t)depth & 3) == 0 && ((uintptr_t)jobs & 3) == 0 &&
                   ((uintptr_t)status & 3) == 0,
               "%s: planes, records, depth, jobs and status must be 4-byte aligned", fn);
    CP_REQUIRE(((uintptr_t)cams & 7) == 0 && ((uintptr_t)gates & 7) == 0 && ((uintptr_t)poses & 7) == 0 && ((uintptr_t)stats & 7) == 0 &&
                   ((uintptr_t)workspace & 7) == 0,
               "%s: cams, gates, poses, stats and workspace must be 8-byte aligned", fn);
    return CP_OK;
}

}  // namespace

extern "C" int cp_depth_icp_tile(void) { return TILE; }

extern "C" size_t cp_depth_icp_workspace_bytes(int njobs, int H, int W) {
    if (njobs < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return 0;
    return cp_icp::workspace_bytes(njobs, H, W);
}

extern "C" int cp_depth_icp_step_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth, const double* cams,
                                     int images, const int32_t* jobs, const double* gates, int njobs, double jump, double damping, int min_pixels,
                                     int update, int split, double* poses, double* stats, int32_t* status, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    if (int rc = check_arguments("cp_depth_icp_step_f64", planes, records, nplanes, H, W, depth, cams, images, jobs, gates, njobs, jump, damping,
                                 min_pixels, update, split, poses, stats, status, workspace, workspace_bytes))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long per_job = max_tiles(H, W) * PARTIAL;
    CP_LAUNCH(icp_accumulate_kernel, dim3((unsigned)((long long)njobs * split)), dim3(THREADS), 0, st, planes, records, nplanes, H, W, depth, cams,
              images, jobs, gates, njobs, jump, split, per_job, (double*)workspace);
    if (int rc = cp::check_launch("cp_depth_icp_step_f64 (accumulate)")) return rc;
    CP_LAUNCH(icp_solve_kernel, dim3((unsigned)njobs), dim3(WAVE), 0, st, records, nplanes, H, W, images, jobs, gates, damping, min_pixels, update,
              per_job, (const double*)workspace, poses, stats, status);
    return cp::check_launch("cp_depth_icp_step_f64 (solve)");
}

extern "C" int cp_depth_icp_step_host_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth,
                                          const double* cams, int images, const int32_t* jobs, const double* gates, int njobs, double jump,
                                          double damping, int min_pixels, int update, int split, double* poses, double* stats, int32_t* status,
                                          void* workspace, size_t workspace_bytes) {
    if (int rc = check_arguments("cp_depth_icp_step_host_f64", planes, records, nplanes, H, W, depth, cams, images, jobs, gates, njobs, jump, damping,
                                 min_pixels, update, split, poses, stats, status, workspace, workspace_bytes))
        return rc;
    step_serial(planes, records, nplanes, H, W, depth, cams, images, jobs, gates, njobs, jump, damping, min_pixels, update, poses, stats, status,
                (double*)workspace);
    return CP_OK;
}
