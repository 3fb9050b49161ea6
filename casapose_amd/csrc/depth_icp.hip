// One projective point-to-plane ICP step per (image, render plane) job against the sensor's depth image.  The planes and records are what
// cp_render_masks_u8 left behind, the poses are the renderer's own device array.  icp_math.h states the rules and holds the schedule: the two
// launches (accumulate_kernel, solve_kernel) and the host twin's loop, on cp_icp::Depth's terms.  This file is the entry points.
#include "common.h"
#include "icp_math.h"

namespace {

using namespace cp_icp;

int check_arguments(const char* fn, const Depth::Args& a, int njobs, double damping, int min_pixels, int update, int split, double* poses, double* stats,
                    int32_t* status, void* workspace, size_t workspace_bytes) {
    CP_REQUIRE(a.planes && a.records && a.depth && a.cams && a.jobs && a.gates && poses && stats && status && workspace, "%s: null pointer", fn);
    CP_REQUIRE(a.nplanes >= 1 && a.images >= 1 && njobs >= 1, "%s: nplanes, images and njobs must be positive (got %d, %d, %d)", fn, a.nplanes, a.images,
               njobs);
    if (int rc = check_step(fn, a.nplanes, a.H, a.W, njobs, damping, min_pixels, update, split, workspace_bytes, "cp_depth_icp_workspace_bytes",
                            cp_icp::workspace_bytes<Depth>(njobs, a.H, a.W)))
        return rc;
    CP_REQUIRE(a.jump > 0.0, "%s: jump must be positive (got %g)", fn, a.jump);
    CP_REQUIRE(((uintptr_t)a.planes & 3) == 0 && ((uintptr_t)a.records & 3) == 0 && ((uintptr_t)a.depth & 3) == 0 && ((uintptr_t)a.jobs & 3) == 0 &&
                   ((uintptr_t)status & 3) == 0,
               "%s: planes, records, depth, jobs and status must be 4-byte aligned", fn);
    CP_REQUIRE(((uintptr_t)a.cams & 7) == 0 && ((uintptr_t)a.gates & 7) == 0 && ((uintptr_t)poses & 7) == 0 && ((uintptr_t)stats & 7) == 0 &&
                   ((uintptr_t)workspace & 7) == 0,
               "%s: cams, gates, poses, stats and workspace must be 8-byte aligned", fn);
    return CP_OK;
}

}  // namespace

extern "C" int cp_depth_icp_tile(void) { return TILE; }

extern "C" size_t cp_depth_icp_workspace_bytes(int njobs, int H, int W) {
    if (njobs < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return 0;
    return cp_icp::workspace_bytes<Depth>(njobs, H, W);
}

extern "C" int cp_depth_icp_step_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth, const double* cams,
                                     int images, const int32_t* jobs, const double* gates, int njobs, double jump, double damping, int min_pixels,
                                     int update, int split, double* poses, double* stats, int32_t* status, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    const Depth::Args a = {planes, records, nplanes, H, W, depth, cams, images, jobs, gates, jump};
    if (int rc = check_arguments("cp_depth_icp_step_f64", a, njobs, damping, min_pixels, update, split, poses, stats, status, workspace, workspace_bytes))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const long long per_job = max_tiles(H, W) * PARTIAL<Depth>;
    CP_LAUNCH(accumulate_kernel<Depth>, dim3((unsigned)((long long)njobs * split)), dim3(THREADS), 0, st, a, njobs, split, per_job, (double*)workspace);
    if (int rc = cp::check_launch("cp_depth_icp_step_f64 (accumulate)")) return rc;
    CP_LAUNCH(solve_kernel<Depth>, dim3((unsigned)njobs), dim3(LANES), 0, st, a, damping, min_pixels, update, per_job, (const double*)workspace, poses,
              stats, status);
    return cp::check_launch("cp_depth_icp_step_f64 (solve)");
}

extern "C" int cp_depth_icp_step_host_f64(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth,
                                          const double* cams, int images, const int32_t* jobs, const double* gates, int njobs, double jump,
                                          double damping, int min_pixels, int update, int split, double* poses, double* stats, int32_t* status,
                                          void* workspace, size_t workspace_bytes) {
    const Depth::Args a = {planes, records, nplanes, H, W, depth, cams, images, jobs, gates, jump};
    if (int rc = check_arguments("cp_depth_icp_step_host_f64", a, njobs, damping, min_pixels, update, split, poses, stats, status, workspace,
                                 workspace_bytes))
        return rc;
    step_serial<Depth>(a, njobs, damping, min_pixels, update, poses, stats, status, (double*)workspace);
    return CP_OK;
}
