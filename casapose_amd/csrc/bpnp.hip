// BPnP keypoint loss on the device: voted keypoints -> loss and d loss / d keypoints through the PnP optimum, for every (image, object) pair of
// a batch, and its host twin.  The arithmetic is bpnp_math.h (training.bpnp_reprojection_loss_host restated in fp64); this file is the schedule.
//
// bpnp_pair_kernel: one block of 256 threads per pair.
//   1. the pair's keypoints go to LDS as fp64 image pixels (the fp32 crop->image affine applied), with the ground-truth projections;
//   2. the consensus stage of pnp_kernel (pnp_consensus.h): one thread per 5-point hypothesis, a tree reduction with a total order;
//   3. thread 0: EPnP on the consensus set, LM, the tightening LM; the optimum y goes to LDS;
//   4. lanes 0..11 (wave 0): one evaluation g(y +- h e_k) of the central-difference Hessian each; lanes 64..64+n (wave 1): keypoint j's
//      residual, Jacobian rows, loss and explicit gradient terms.  The two waves run side by side;
//   5. thread 0: g_pose = J^T g_r, H symmetrised, H v = g_pose, the pair's loss, pose and info;
//   6. lanes j < n: keypoint j's two gradient entries g_direct + J v, back through the affine, as (y, x).
//   Every exit before a barrier is block-uniform, and a block that leaves early still writes its zeros.  No atomics.
// bpnp_finish_kernel: one block.  na = the solved pairs (a fixed-order tree sum), loss = sum of pair losses / na, g_yx = weight / na x the
//   un-normalised gradient of solved pairs and 0 elsewhere (every element is written), counts = {solved, available but unsolved}.
// Like pnp_kernel this is latency-bound private-memory fp64: EPnP's working set (~500 doubles) is scratch, the serial tail runs on one lane.
// cp_bpnp_loss_host_f64: the same header functions in a serial loop on host pointers; it launches nothing.
#include "bpnp_math.h"
#include "common.h"
#include "pnp_consensus.h"

namespace {

using namespace cp_pnp;

constexpr int THREADS = CONSENSUS_THREADS, POINT_LANE0 = 64;

// the workspace: fp64 [pairs][2 kp] un-normalised gradients (y, x), then fp64 [pairs] pair losses
__host__ __device__ inline size_t ws_loss_offset(int pairs, int kp) { return (size_t)pairs * 2 * kp; }

__global__ void __launch_bounds__(THREADS) bpnp_pair_kernel(const float* __restrict__ coords_yx, const float* __restrict__ gt_xy,
                                                            const float* __restrict__ affine, const float* __restrict__ avail,
                                                            const float* __restrict__ points_3d, const float* __restrict__ K,
                                                            const uint8_t* __restrict__ table, int oc, int n, int H, double reprojection_error,
                                                            double max_pixel_error, double* __restrict__ ws, float* __restrict__ poses,
                                                            int32_t* __restrict__ info) {
    __shared__ Problem P;
    __shared__ Consensus S;
    __shared__ double s_gt[MAX_POINTS * 2], s_y[6], s_G[12 * 6], s_v[6], s_R[9], s_Jl[9];
    __shared__ PointTerm s_T[MAX_POINTS];
    __shared__ int s_ok, s_iters;
    const int pair = blockIdx.x, tid = threadIdx.x, image = pair / oc, pairs = gridDim.x;
    double* g_pair = ws + (size_t)pair * 2 * n;
    double* loss_pair = ws + ws_loss_offset(pairs, n) + pair;
    float* pose = poses + (size_t)pair * 12;
    int32_t* inf = info + (size_t)pair * 4;
    const float* aff = affine + (size_t)image * 6;
    if (avail[pair] == 0.f) {   // block-uniform
        if (tid == 0) zero_pair(SKIPPED, n, g_pair, loss_pair, pose, inf);
        return;
    }
    if (tid < n) load_point_yx(P, s_gt, tid, coords_yx + (size_t)pair * n * 2, points_3d + (size_t)pair * n * 3, gt_xy + (size_t)pair * n * 2, aff);
    if (tid < 9) P.K[tid] = (double)K[tid];
    if (tid == 0) P.n = n;
    __syncthreads();
    const int status = consensus_stage(P, S, table, H, reprojection_error);
    if (status != OK) {   // block-uniform
        if (tid == 0) zero_pair(status, n, g_pair, loss_pair, pose, inf);
        return;
    }
    if (tid == 0) {
        const Score best = {S.count[0], S.sse[0], S.mask[0]};
        double y[6], R[9], Jl[9];
        int iters = 0;
        const bool ok = tightened_optimum(P, best, y, iters);
        s_ok = ok ? 1 : 0;
        s_iters = iters;
        if (ok) {
            rotation_and_left_jacobian(y, R, Jl);
            for (int i = 0; i < 6; ++i) s_y[i] = y[i];
            for (int i = 0; i < 9; ++i) { s_R[i] = R[i]; s_Jl[i] = Jl[i]; }
        }
    }
    __syncthreads();
    if (!s_ok) {   // block-uniform
        if (tid == 0) zero_pair(NO_SOLUTION, n, g_pair, loss_pair, pose, inf);
        return;
    }
    if (tid < 12) {
        double g[6];
        shifted_gradient(P, s_y, tid, g);
        for (int a = 0; a < 6; ++a) s_G[tid * 6 + a] = g[a];
    } else if (tid >= POINT_LANE0 && tid < POINT_LANE0 + n) {
        PointTerm T;
        point_term(P, s_gt, s_y, s_R, s_Jl, tid - POINT_LANE0, max_pixel_error, T);
        s_T[tid - POINT_LANE0] = T;
    }
    __syncthreads();
    if (tid == 0) {
        double g_pose[6], v[6], total = 0.0;
        for (int a = 0; a < 6; ++a) g_pose[a] = 0.0;
        for (int j = 0; j < n; ++j) {
            total += s_T[j].l;
            for (int a = 0; a < 6; ++a) g_pose[a] += s_T[j].ju[a] * s_T[j].g_r[0] + s_T[j].jv[a] * s_T[j].g_r[1];
        }
        const bool ok = implicit_solve(s_y, s_G, g_pose, v) && finite(total);
        s_ok = ok ? 1 : 0;
        if (ok) {
            for (int a = 0; a < 6; ++a) s_v[a] = v[a];
            *loss_pair = total / n;
            pose_from_optimum(s_y, s_R, pose);
            inf[0] = OK; inf[1] = S.index[0]; inf[2] = S.count[0] < 0 ? 0 : S.count[0]; inf[3] = s_iters;
        }
    }
    __syncthreads();
    if (!s_ok) {   // block-uniform
        if (tid == 0) zero_pair(NO_SOLUTION, n, g_pair, loss_pair, pose, inf);
        return;
    }
    if (tid < n) point_gradient(s_T[tid], s_v, aff, g_pair + 2 * tid);
}

__global__ void __launch_bounds__(THREADS) bpnp_finish_kernel(const float* __restrict__ avail, const int32_t* __restrict__ info,
                                                              const double* __restrict__ ws, int pairs, int kp, double weight,
                                                              float* __restrict__ g_yx, double* __restrict__ loss_out, int32_t* __restrict__ counts) {
    __shared__ double s_loss[THREADS];
    __shared__ int s_solved[THREADS], s_unsolved[THREADS];
    const int tid = threadIdx.x;
    const double* pair_loss = ws + ws_loss_offset(pairs, kp);
    double l = 0.0;
    int solved = 0, unsolved = 0;
    for (int p = tid; p < pairs; p += THREADS) {   // a fixed order: thread t sums pairs t, t + 256, ..., then the tree
        const bool av = avail[p] != 0.f, ok = av && info[4 * p] == OK;
        if (ok) l += pair_loss[p];
        solved += ok ? 1 : 0;
        unsolved += (av && !ok) ? 1 : 0;
    }
    s_loss[tid] = l;
    s_solved[tid] = solved;
    s_unsolved[tid] = unsolved;
    __syncthreads();
#pragma unroll 1
    for (int half = THREADS / 2; half >= 1; half >>= 1) {
        if (tid < half) {
            s_loss[tid] += s_loss[tid + half];
            s_solved[tid] += s_solved[tid + half];
            s_unsolved[tid] += s_unsolved[tid + half];
        }
        __syncthreads();
    }
    const int na = s_solved[0];
    if (tid == 0) {
        *loss_out = na > 0 ? s_loss[0] / (double)na : 0.0;
        counts[0] = na;
        counts[1] = s_unsolved[0];
    }
    const int per = 2 * kp;
    for (long long i = tid; i < (long long)pairs * per; i += THREADS) {
        const int p = (int)(i / per);
        g_yx[i] = finished_gradient(ws[i], avail[p] != 0.f && info[4 * p] == OK, weight, na);
    }
}

int check_arguments(const char* fn, const void* coords_yx, const void* gt_xy, const void* affine, const void* avail, const void* points_3d, const void* K,
                    const void* table, int batch, int objects, int kp, int H, float reprojection_error, float max_pixel_error, float weight,
                    const void* g_yx, const void* loss_out, const void* poses, const void* info, const void* counts, const void* workspace) {
    CP_REQUIRE(coords_yx && gt_xy && affine && avail && points_3d && K && table && g_yx && loss_out && poses && info && counts && workspace,
               "%s: null pointer", fn);
    CP_REQUIRE(batch >= 1 && objects >= 1, "%s: batch and objects must be positive (got %d, %d)", fn, batch, objects);
    CP_REQUIRE((long long)batch * objects <= 65535, "%s: more than 65535 (image, object) pairs in one call (batch %d x objects %d)", fn, batch, objects);
    CP_REQUIRE(kp >= MIN_POINTS && kp <= MAX_POINTS, "%s: kp must lie in [%d, %d] (got %d); other point counts stay with the host path", fn, MIN_POINTS,
               MAX_POINTS, kp);
    CP_REQUIRE(H >= 1 && H <= MAX_HYPOTHESES, "%s: H must lie in [1, %d] (got %d)", fn, MAX_HYPOTHESES, H);
    CP_REQUIRE(reprojection_error > 0.f, "%s: reprojection_error must be positive (got %g)", fn, (double)reprojection_error);   // false for NaN
    CP_REQUIRE(max_pixel_error > 0.f, "%s: max_pixel_error must be positive (got %g)", fn, (double)max_pixel_error);
    CP_REQUIRE(weight == weight && fabsf(weight) <= 3.4028234e38f, "%s: weight must be finite (got %g)", fn, (double)weight);
    return CP_OK;
}

}  // namespace

extern "C" size_t cp_bpnp_loss_workspace_bytes(int batch, int objects, int kp) {
    if (batch < 1 || objects < 1 || kp < 1) return 0;
    return ((size_t)batch * objects * 2 * kp + (size_t)batch * objects) * sizeof(double);
}

extern "C" int cp_bpnp_loss_f64(const float* coords_yx, const float* gt_xy, const float* affine, const float* avail, const float* points_3d,
                                const float* K, const uint8_t* table, int batch, int objects, int kp, int H, float reprojection_error,
                                float max_pixel_error, float weight, float* g_yx, double* loss_out, float* poses, int32_t* info, int32_t* counts,
                                void* workspace, void* stream) {
    if (int rc = check_arguments("cp_bpnp_loss_f64", coords_yx, gt_xy, affine, avail, points_3d, K, table, batch, objects, kp, H, reprojection_error,
                                 max_pixel_error, weight, g_yx, loss_out, poses, info, counts, workspace))
        return rc;
    CP_REQUIRE(((uintptr_t)workspace & 7) == 0, "cp_bpnp_loss_f64: the workspace must be 8-byte aligned");
    const int pairs = batch * objects;
    CP_LAUNCH(bpnp_pair_kernel, dim3(pairs), dim3(THREADS), 0, (hipStream_t)stream, coords_yx, gt_xy, affine, avail, points_3d, K, table, objects, kp, H,
              (double)reprojection_error, (double)max_pixel_error, (double*)workspace, poses, info);
    if (int rc = cp::check_launch("cp_bpnp_loss_f64 (pairs)")) return rc;
    CP_LAUNCH(bpnp_finish_kernel, dim3(1), dim3(THREADS), 0, (hipStream_t)stream, avail, info, (const double*)workspace, pairs, kp, (double)weight, g_yx,
              loss_out, counts);
    return cp::check_launch("cp_bpnp_loss_f64 (finish)");
}

extern "C" int cp_bpnp_loss_host_f64(const float* coords_yx, const float* gt_xy, const float* affine, const float* avail, const float* points_3d,
                                     const float* K, const uint8_t* table, int batch, int objects, int kp, int H, float reprojection_error,
                                     float max_pixel_error, float weight, float* g_yx, double* loss_out, float* poses, int32_t* info, int32_t* counts,
                                     void* workspace) {
    if (int rc = check_arguments("cp_bpnp_loss_host_f64", coords_yx, gt_xy, affine, avail, points_3d, K, table, batch, objects, kp, H,
                                 reprojection_error, max_pixel_error, weight, g_yx, loss_out, poses, info, counts, workspace))
        return rc;
    CP_REQUIRE(((uintptr_t)workspace & 7) == 0, "cp_bpnp_loss_host_f64: the workspace must be 8-byte aligned");
    for (int i = 0; i < H * SET_POINTS; ++i)
        CP_REQUIRE((int)table[i] < kp, "cp_bpnp_loss_host_f64: hypothesis %d names point %d of %d", i / SET_POINTS, (int)table[i], kp);
    const int pairs = batch * objects;
    double* ws = (double*)workspace;
    double* pair_loss = ws + ws_loss_offset(pairs, kp);
    for (int pair = 0; pair < pairs; ++pair) {
        double* g_pair = ws + (size_t)pair * 2 * kp;
        float* pose = poses + (size_t)pair * 12;
        int32_t* inf = info + (size_t)pair * 4;
        if (avail[pair] == 0.f) {
            zero_pair(SKIPPED, kp, g_pair, pair_loss + pair, pose, inf);
            continue;
        }
        const size_t at = (size_t)pair * kp;
        bpnp_pair_serial(coords_yx + at * 2, gt_xy + at * 2, affine + (size_t)(pair / objects) * 6, points_3d + at * 3, K, kp, table, H,
                         (double)reprojection_error, (double)max_pixel_error, g_pair, pair_loss + pair, pose, inf);
    }
    int na = 0, unsolved = 0;
    double total = 0.0;
    for (int pair = 0; pair < pairs; ++pair) {
        const bool av = avail[pair] != 0.f, ok = av && info[4 * pair] == OK;
        if (ok) total += pair_loss[pair];
        na += ok ? 1 : 0;
        unsolved += (av && !ok) ? 1 : 0;
    }
    *loss_out = na > 0 ? total / (double)na : 0.0;
    counts[0] = na;
    counts[1] = unsolved;
    for (size_t i = 0; i < (size_t)pairs * 2 * kp; ++i)
        g_yx[i] = finished_gradient(ws[i], avail[i / (2 * kp)] != 0.f && info[4 * (i / (2 * kp))] == OK, (double)weight, na);
    return CP_OK;
}
