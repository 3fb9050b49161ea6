// Device PnP: voted keypoints -> 6-DoF poses for every (image, object) pair of a batch, and its host twin.  The arithmetic is pnp_math.h
// (casapose_amd/pose_estimation/pnp.py restated in fp64); this file is the parallel schedule around it.
//
// pnp_kernel: one block of 256 threads per pair, one thread per hypothesis (a 5-point minimal set from the caller's table, H <= 256).
//   The pair's points are loaded once into LDS (fp64, crop->image affine applied).  The consensus stage (pnp_consensus.h, shared with
//   bpnp.hip): thread h runs EPnP on its five points and scores the pose on all n points; the scores go to LDS and a tree reduction with a total order (most inliers, smallest sum of squared inlier errors,
//   lowest index; idle slots lose against everything) picks the consensus.  No atomics: two calls give the same bits.  Thread 0 then runs
//   EPnP on the consensus set and LM over all points -- a few thousand fp64 operations, not worth a second schedule.
//   The working set of EPnP (the 12x12 M^T M, its eigenvectors, the barycentric coordinates: ~500 doubles) is private memory, i.e. scratch:
//   the problem is a few thousand threads per batch, and every loop has a fixed trip count, so the kernel ends whatever its input.
// cp_pnp_host_f64: the same functions in a serial loop over pairs and hypotheses, on host pointers; it launches nothing.
#include "common.h"
#include "pnp_consensus.h"
#include "pnp_math.h"

namespace {

using namespace cp_pnp;

constexpr int THREADS = CONSENSUS_THREADS;

__global__ void __launch_bounds__(THREADS) pnp_kernel(const float* __restrict__ points_xy, const float* __restrict__ points_3d,
                                                      const float* __restrict__ K, int k_per_image, const double* __restrict__ affine,
                                                      const int32_t* __restrict__ solve, const uint8_t* __restrict__ table, int oc, int n, int H,
                                                      double reprojection_error, float* __restrict__ poses, int32_t* __restrict__ info,
                                                      float* __restrict__ cost) {
    __shared__ Problem P;
    __shared__ Consensus S;
    const int pair = blockIdx.x, tid = threadIdx.x, image = pair / oc;
    float* pose = poses + (size_t)pair * 12;
    int32_t* inf = info + (size_t)pair * 4;
    float* cst = cost + (size_t)pair * 2;
    if (solve[pair] == 0) {   // block-uniform
        if (tid == 0) zero_outputs(SKIPPED, pose, inf, cst);
        return;
    }
    if (tid < n) load_point(P, tid, points_xy + (size_t)pair * n * 2, points_3d + (size_t)pair * n * 3, affine ? affine + (size_t)image * 6 : nullptr);
    if (tid < 9) P.K[tid] = (double)K[(k_per_image ? (size_t)image * 9 : 0) + tid];
    if (tid == 0) P.n = n;
    __syncthreads();
    const int status = consensus_stage(P, S, table, H, reprojection_error);
    if (status != OK) {   // block-uniform
        if (tid == 0) zero_outputs(status, pose, inf, cst);
        return;
    }
    if (tid == 0) {
        const Score best = {S.count[0], S.sse[0], S.mask[0]};
        finish_pair(P, S.index[0], best, pose, inf, cst);
    }
}

}  // namespace

namespace cp_pnp {
// declared in pnp_consensus.h; pnp_weighted.hip applies the same rules
int check_arguments(const char* fn, const void* points_xy, const void* points_3d, const void* K, const void* solve, const void* table, int b, int oc,
                    int n, int H, float reprojection_error, const void* poses, const void* info, const void* cost) {
    CP_REQUIRE(points_xy && points_3d && K && solve && table && poses && info && cost, "%s: null pointer", fn);
    CP_REQUIRE(b >= 1 && oc >= 1, "%s: b and oc must be positive (got %d, %d)", fn, b, oc);
    CP_REQUIRE((long long)b * oc <= 65535, "%s: more than 65535 (image, object) pairs in one call (b %d x oc %d)", fn, b, oc);
    CP_REQUIRE(n >= MIN_POINTS && n <= MAX_POINTS, "%s: n must lie in [%d, %d] (got %d); fewer than 5 points stay with the host path", fn, MIN_POINTS,
               MAX_POINTS, n);
    CP_REQUIRE(H >= 1 && H <= MAX_HYPOTHESES, "%s: H must lie in [1, %d] (got %d)", fn, MAX_HYPOTHESES, H);
    CP_REQUIRE(reprojection_error > 0.f, "%s: reprojection_error must be positive (got %g)", fn, (double)reprojection_error);   // false for NaN
    return CP_OK;
}
}  // namespace cp_pnp

extern "C" int cp_pnp_f64(const float* points_xy, const float* points_3d, const float* K, int k_per_image, const double* affine, const int32_t* solve,
                          const uint8_t* table, int b, int oc, int n, int H, float reprojection_error, float* poses, int32_t* info, float* cost,
                          void* stream) {
    if (int rc = check_arguments("cp_pnp_f64", points_xy, points_3d, K, solve, table, b, oc, n, H, reprojection_error, poses, info, cost)) return rc;
    CP_LAUNCH(pnp_kernel, dim3(b * oc), dim3(THREADS), 0, (hipStream_t)stream, points_xy, points_3d, K, k_per_image, affine, solve, table, oc, n, H,
              (double)reprojection_error, poses, info, cost);
    return cp::check_launch("cp_pnp_f64");
}

extern "C" int cp_pnp_host_f64(const float* points_xy, const float* points_3d, const float* K, int k_per_image, const double* affine,
                               const int32_t* solve, const uint8_t* table, int b, int oc, int n, int H, float reprojection_error, float* poses,
                               int32_t* info, float* cost) {
    if (int rc = check_arguments("cp_pnp_host_f64", points_xy, points_3d, K, solve, table, b, oc, n, H, reprojection_error, poses, info, cost)) return rc;
    for (int i = 0; i < H * SET_POINTS; ++i)
        CP_REQUIRE((int)table[i] < n, "cp_pnp_host_f64: hypothesis %d names point %d of %d", i / SET_POINTS, (int)table[i], n);
    for (int pair = 0; pair < b * oc; ++pair) {
        float* pose = poses + (size_t)pair * 12;
        int32_t* inf = info + (size_t)pair * 4;
        float* cst = cost + (size_t)pair * 2;
        if (solve[pair] == 0) {
            zero_outputs(SKIPPED, pose, inf, cst);
            continue;
        }
        const int image = pair / oc;
        solve_pair_serial(points_xy + (size_t)pair * n * 2, points_3d + (size_t)pair * n * 3, K + (k_per_image ? (size_t)image * 9 : 0),
                          affine ? affine + (size_t)image * 6 : nullptr, n, table, H, (double)reprojection_error, pose, inf, cst);
    }
    return CP_OK;
}
