// The consensus stage of the device PnP, shared by pnp_kernel (pnp.hip) and bpnp_pair_kernel (bpnp.hip): one block of 256 threads per pair, one
// thread per hypothesis.  Thread h runs EPnP on its five points and scores the pose on all n points; a tree reduction with a total order (most
// inliers, smallest sum of squared inlier errors, lowest index; idle slots lose against everything) picks the winner.  No atomics.
#pragma once
#include "common.h"
#include "pnp_math.h"

namespace cp_pnp {

constexpr int CONSENSUS_THREADS = MAX_HYPOTHESES;

// the argument rules of cp_pnp_f64, cp_pnp_weighted_f64 and their twins (defined in pnp.hip, host only)
int check_arguments(const char* fn, const void* points_xy, const void* points_3d, const void* K, const void* solve, const void* table, int b, int oc,
                    int n, int H, float reprojection_error, const void* poses, const void* info, const void* cost);

struct Consensus {   // LDS of one block
    int status;
    int count[CONSENSUS_THREADS], index[CONSENSUS_THREADS];
    double sse[CONSENSUS_THREADS];
    uint32_t mask[CONSENSUS_THREADS];
};

// Every thread of the block calls it after P is complete in LDS (a barrier lies between).  Returns check_problem's status, the same in every
// thread; OK leaves the winner in slot 0 of S (index[0], count[0], sse[0], mask[0]) and ends with a barrier.
__device__ inline int consensus_stage(const Problem& P, Consensus& S, const uint8_t* __restrict__ table, int H, double reprojection_error) {
    const int tid = threadIdx.x;
    if (tid == 0) S.status = check_problem(P);
    __syncthreads();
    if (S.status != OK) return S.status;   // block-uniform
    Score s = {-2, 0.0, 0u};   // an idle slot: below a hypothesis without a pose (-1)
    if (tid < H) s = score_hypothesis(P, table + (size_t)tid * SET_POINTS, reprojection_error);
    S.count[tid] = s.count;
    S.sse[tid] = s.sse;
    S.mask[tid] = s.mask;
    S.index[tid] = tid;
    __syncthreads();
#pragma unroll 1
    for (int half = CONSENSUS_THREADS / 2; half >= 1; half >>= 1) {
        if (tid < half && better(S.count[tid + half], S.sse[tid + half], S.index[tid + half], S.count[tid], S.sse[tid], S.index[tid])) {
            S.count[tid] = S.count[tid + half];
            S.sse[tid] = S.sse[tid + half];
            S.mask[tid] = S.mask[tid + half];
            S.index[tid] = S.index[tid + half];
        }
        __syncthreads();
    }
    return OK;
}

}  // namespace cp_pnp
