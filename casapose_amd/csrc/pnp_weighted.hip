// Uncertainty-weighted device PnP (cp_pnp_weighted_f64) and its host twin: pnp.hip's schedule with the final LM weighted by the keypoint
// covariances (pnp_math.h: load_whitening, residual_normal_weighted, finish_pair_t<true>).  It is a translation unit of its own so that
// pnp_kernel is compiled exactly as before: the two kernels share every function of pnp_math.h, and in one unit the inliner treats them
// differently once there are two callers.
#include "common.h"
#include "pnp_consensus.h"
#include "pnp_math.h"

namespace {

using namespace cp_pnp;

constexpr int THREADS = CONSENSUS_THREADS;

// pnp_kernel (pnp.hip) with two additions: thread i < n also factors point i's covariance, and thread 0 takes the weighted LM when every point's
// factor exists, cp_pnp_f64's own finish otherwise.
__global__ void __launch_bounds__(THREADS) pnp_weighted_kernel(const float* __restrict__ points_xy, const float* __restrict__ points_3d,
                                                               const float* __restrict__ K, int k_per_image, const double* __restrict__ affine,
                                                               const int32_t* __restrict__ solve, const uint8_t* __restrict__ table, int oc, int n,
                                                               int H, double reprojection_error, const float* __restrict__ cov, double cov_floor,
                                                               float* __restrict__ poses, int32_t* __restrict__ info, float* __restrict__ cost,
                                                               int32_t* __restrict__ weighted) {
    __shared__ Problem P;
    __shared__ Consensus S;
    __shared__ Whitening Wt;
    __shared__ int w_ok[MAX_POINTS];
    const int pair = blockIdx.x, tid = threadIdx.x, image = pair / oc;
    float* pose = poses + (size_t)pair * 12;
    int32_t* inf = info + (size_t)pair * 4;
    float* cst = cost + (size_t)pair * 2;
    if (tid == 0) weighted[pair] = 0;   // (the same thread writes 1 below when the pair is solved with weights)
    if (solve[pair] == 0) {   // block-uniform
        if (tid == 0) zero_outputs(SKIPPED, pose, inf, cst);
        return;
    }
    const double* aff = affine ? affine + (size_t)image * 6 : nullptr;
    if (tid < n) {
        load_point(P, tid, points_xy + (size_t)pair * n * 2, points_3d + (size_t)pair * n * 3, aff);
        w_ok[tid] = load_whitening(Wt, tid, cov + ((size_t)pair * n + tid) * 3, cov_floor, aff) ? 1 : 0;
    }
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
        bool usable = true;
        for (int i = 0; i < n; ++i) usable = usable && w_ok[i] != 0;
        if (usable) finish_pair_t<true>(P, &Wt, S.index[0], best, pose, inf, cst);
        else finish_pair(P, S.index[0], best, pose, inf, cst);
        weighted[pair] = usable ? 1 : 0;
    }
}

int check_weighted_arguments(const char* fn, const void* cov, float cov_floor, const void* weighted) {
    CP_REQUIRE(cov, "%s: cov is a null pointer; callers without covariances use cp_pnp_f64", fn);
    CP_REQUIRE(weighted, "%s: weighted is a null pointer", fn);
    CP_REQUIRE(cov_floor >= 0.f && cov_floor <= 3.4028234e38f, "%s: cov_floor must be finite and not negative (got %g)", fn, (double)cov_floor);
    return CP_OK;
}

}  // namespace

extern "C" int cp_pnp_weighted_f64(const float* points_xy, const float* points_3d, const float* K, int k_per_image, const double* affine,
                                   const int32_t* solve, const uint8_t* table, int b, int oc, int n, int H, float reprojection_error, const float* cov,
                                   float cov_floor, float* poses, int32_t* info, float* cost, int32_t* weighted, void* stream) {
    if (int rc = check_arguments("cp_pnp_weighted_f64", points_xy, points_3d, K, solve, table, b, oc, n, H, reprojection_error, poses, info, cost)) return rc;
    if (int rc = check_weighted_arguments("cp_pnp_weighted_f64", cov, cov_floor, weighted)) return rc;
    CP_LAUNCH(pnp_weighted_kernel, dim3(b * oc), dim3(THREADS), 0, (hipStream_t)stream, points_xy, points_3d, K, k_per_image, affine, solve, table, oc,
              n, H, (double)reprojection_error, cov, (double)cov_floor, poses, info, cost, weighted);
    return cp::check_launch("cp_pnp_weighted_f64");
}

extern "C" int cp_pnp_weighted_host_f64(const float* points_xy, const float* points_3d, const float* K, int k_per_image, const double* affine,
                                        const int32_t* solve, const uint8_t* table, int b, int oc, int n, int H, float reprojection_error,
                                        const float* cov, float cov_floor, float* poses, int32_t* info, float* cost, int32_t* weighted) {
    if (int rc = check_arguments("cp_pnp_weighted_host_f64", points_xy, points_3d, K, solve, table, b, oc, n, H, reprojection_error, poses, info, cost))
        return rc;
    if (int rc = check_weighted_arguments("cp_pnp_weighted_host_f64", cov, cov_floor, weighted)) return rc;
    for (int i = 0; i < H * SET_POINTS; ++i)
        CP_REQUIRE((int)table[i] < n, "cp_pnp_weighted_host_f64: hypothesis %d names point %d of %d", i / SET_POINTS, (int)table[i], n);
    solve_batch_weighted_serial(points_xy, points_3d, K, k_per_image, affine, solve, table, b, oc, n, H, (double)reprojection_error, cov, (double)cov_floor,
                                poses, info, cost, weighted);
    return CP_OK;
}
