// The assignment rule of the instance evaluator (cp_pose_match_f32, pose_match.hip): which of up to 16 estimates of one object in one image is
// compared with which of up to 16 ground-truth instances, as __host__ __device__ code free of HIP types.  match_assign_kernel and the
// stand-alone self-test (match_selftest.cpp) call the same function.  Nothing here calls a library.
//
// The rule is greedy, BOP's and COCO's scheme: repeatedly take the smallest finite cost among the estimates and instances that are still
// free; on ties the smaller instance g, then the smaller estimate e.  There is no distance gate: a far match is a match, and simply no true
// positive.  Greedy is not the optimal (Hungarian) assignment.  With costs
//        g0   g1
//   e0    1    2
//   e1    2  100
// greedy takes (e0, g0) and is left with (e1, g1) = 100, where the optimum pairs (e0, g1) and (e1, g0) at 2 + 2: under a threshold of 3 greedy
// finds one instance and the optimum two.  For a recall thresholded at 0.1 diameters the two can differ only where one estimate lies within the
// threshold of two instances, that is where two instances lie within 0.2 diameters of each other, which physical objects do not.
#pragma once

#if defined(__HIPCC__)
#define MATCH_HD __host__ __device__ __forceinline__
#else
#define MATCH_HD inline
#endif

namespace cp_match {

constexpr int MAX_SIDE = 16;                  // the bound on estimates and on instances per (image, object)
constexpr int UNMATCHED = -1, EMPTY = -2;     // est_match of a non-empty estimate without an instance (a false positive), of an empty slot

// x - x is 0 for every finite x and NaN for an infinity or a NaN
template <typename T>
MATCH_HD bool finite_cost(T x) {
    return x - x == (T)0;
}

// cost[e * stride + g] for e < estimates, g < instances; live: bit e set where estimate e is not empty.
// est_match [estimates] <- the instance of e, UNMATCHED or EMPTY;  gt_match [instances] <- the estimate of g or UNMATCHED.  Returns the matches.
// The two outputs are written through the pointers only (a kernel hands global or LDS memory: no private array is indexed here).
template <typename T>
MATCH_HD int greedy_match(const T* cost, int estimates, int instances, int stride, unsigned live, int* est_match, int* gt_match) {
    unsigned free_e = 0u, free_g = 0u;
    for (int e = 0; e < estimates; ++e) {
        const bool on = (live >> e) & 1u;
        est_match[e] = on ? UNMATCHED : EMPTY;
        if (on) free_e |= 1u << e;
    }
    for (int g = 0; g < instances; ++g) {
        gt_match[g] = UNMATCHED;
        free_g |= 1u << g;
    }
    int matched = 0;
    while (free_e != 0u && free_g != 0u) {
        int be = -1, bg = -1;
        T best = (T)0;
        for (int g = 0; g < instances; ++g) {
            if (!((free_g >> g) & 1u)) continue;
            for (int e = 0; e < estimates; ++e) {
                if (!((free_e >> e) & 1u)) continue;
                const T c = cost[e * stride + g];
                if (finite_cost(c) && (bg < 0 || c < best)) best = c, be = e, bg = g;   // strict: the first of equal costs stays
            }
        }
        if (bg < 0) break;   // nothing finite is left
        est_match[be] = bg;
        gt_match[bg] = be;
        free_e &= ~(1u << be);
        free_g &= ~(1u << bg);
        ++matched;
    }
    return matched;
}

}  // namespace cp_match
