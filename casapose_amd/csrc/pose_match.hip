// Pose statistics for several instances of one object per image: for every group = (image, object) up to R estimated poses are compared with up
// to I ground-truth instances -- the 2-D reprojection distance and ADD (ADD-S where the object's `symmetric` flag is set) of every (estimate,
// instance) pair -- and matched greedily by the 3-D error (match_math.h).  cp_pose_eval_f32 (pose_eval.hip) is the one-estimate, instance-0 form;
// the per-point arithmetic and the order of every sum are its own (pose_eval_math.h), so an error here equals its record on the same pair bit
// for bit.
//
// match_points_kernel<G>: grid (ceil(vmax / 256), groups * R), 256 threads, one thread per model point, one block per (chunk, estimate e).  The
//   group's ground-truth poses are staged in LDS once per block; a thread keeps its point under all of them in registers (3 G floats) and forms
//   the G 2-D and 3-D distances to estimate e's point.  ADD-S walks estimate e's transformed points in LDS tiles once and updates all G running
//   minima per read: one broadcast ds_read_b128 serves G x 6 VALU operations where pose_points_kernel has one read per 6, and R x I pairs cost R
//   walks instead of R x I.  G is I rounded up to 1, 2, 4, 8 or 16; entries g >= the group's count are carried as zeros.  Per-(e, g) fp64
//   partial sums per chunk: wave shuffle tree, waves in index order.  No atomics.
// match_assign_kernel: one wave per group sums the chunks (lane-strided, then the shuffle tree), divides by the count, and lane 0 assigns
//   (cp_match::greedy_match on the fp64 3-D means) and writes the four outputs.
#include "common.h"
#include "match_math.h"
#include "pose_eval_math.h"

namespace {

using namespace cp_pose;
constexpr int MAX_SIDE = cp_match::MAX_SIDE;
constexpr int WAVES = THREADS / 64;

__device__ __forceinline__ int clamped_instances(const int* __restrict__ gt_counts, int group, int instances) {
    const int c = gt_counts[group];
    return c < 0 ? 0 : (c > instances ? instances : c);
}

template <int G>
__global__ void __launch_bounds__(THREADS) match_points_kernel(const float* __restrict__ points, const int* __restrict__ counts,
                                                               const int* __restrict__ symmetric, int objects, int vmax,
                                                               const float* __restrict__ est, int slots, const float* __restrict__ gt,
                                                               int instances, const int* __restrict__ gt_counts,
                                                               const float* __restrict__ cams, double* __restrict__ partial) {
    __shared__ float4 tile[EST_TILE];
    __shared__ float gt_pose[G][12];
    __shared__ double wsum[2 * G][WAVES];
    const int row = blockIdx.y, chunk = blockIdx.x, tid = threadIdx.x;   // row = group * slots + e
    const int group = row / slots, o = group % objects, b = group / objects;
    const int i = chunk * THREADS + tid;
    const int cnt = clamped_count(counts, o, vmax);
    const int ng = clamped_instances(gt_counts, group, instances);
    float pe[12], k[9];
#pragma unroll
    for (int j = 0; j < 12; ++j) pe[j] = est[(size_t)row * 12 + j];
#pragma unroll
    for (int j = 0; j < 9; ++j) k[j] = cams[(size_t)b * 9 + j];
    double* out = partial + ((size_t)row * gridDim.x + chunk) * instances * 2;   // [instances][2]
    if (pose_abs_sum(pe) < 1e-4 || ng == 0 || chunk * THREADS >= cnt) {   // block-uniform
        if (tid < 2 * instances) out[tid] = 0.0;
        return;
    }
    if (tid < ng * 12) gt_pose[tid / 12][tid % 12] = gt[(size_t)group * instances * 12 + tid];   // ng * 12 <= 192 < THREADS
    __syncthreads();
    const float* obj = points + (size_t)o * vmax * 3;
    const bool active = i < cnt;
    float3 tg[G];
    float e2[G], e3[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        tg[g] = make_float3(0.f, 0.f, 0.f);
        e2[g] = e3[g] = 0.f;
    }
    if (active) {
        const float x = obj[3 * (size_t)i], y = obj[3 * (size_t)i + 1], z = obj[3 * (size_t)i + 2];
        const float3 es = transform(pe, x, y, z);
        const float2 pix = project(k, es);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g < ng) {   // block-uniform
                tg[g] = transform(gt_pose[g], x, y, z);
                e2[g] = pixel_distance(project(k, tg[g]), pix);
                e3[g] = add_distance(tg[g], es);
            }
        }
    }
    if (symmetric[o] != 0) {
        float best[G];
#pragma unroll
        for (int g = 0; g < G; ++g) best[g] = __builtin_inff();
        for (int t0 = 0; t0 < cnt; t0 += EST_TILE) {
            __syncthreads();   // the previous tile has been read
            const int padded = fill_tile(tile, obj, pe, t0, cnt, tid);
            __syncthreads();
            if (active) {
                for (int j = 0; j < padded; j += TILE_UNROLL) {
#pragma unroll
                    for (int u = 0; u < TILE_UNROLL; ++u) {
                        const float4 q = tile[j + u];
#pragma unroll
                        for (int g = 0; g < G; ++g) best[g] = fminf(best[g], squared_distance(tg[g], q.x, q.y, q.z));
                    }
                }
            }
        }
        if (active) {
#pragma unroll
            for (int g = 0; g < G; ++g)
                if (g < ng) e3[g] = adds_distance(best[g]);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const double s2 = wave_sum((double)e2[g]), s3 = wave_sum((double)e3[g]);
        if ((tid & 63) == 0) {
            wsum[2 * g][tid >> 6] = s2;
            wsum[2 * g + 1][tid >> 6] = s3;
        }
    }
    __syncthreads();
    if (tid < 2 * instances) {   // instances <= G
        double a = 0.0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w) a += wsum[tid][w];
        out[tid] = a;   // zeros for g >= ng: nothing was added
    }
}

__global__ void __launch_bounds__(64) match_assign_kernel(const int* __restrict__ counts, int objects, int vmax, int chunks,
                                                          const float* __restrict__ est, int slots, int instances,
                                                          const int* __restrict__ gt_counts, const float* __restrict__ diameters,
                                                          float allowed_error_2d, const double* __restrict__ partial, float* __restrict__ err,
                                                          float* __restrict__ gt_rec, int* __restrict__ est_match, int* __restrict__ tally) {
    __shared__ double mean2[MAX_SIDE * MAX_SIDE], mean3[MAX_SIDE * MAX_SIDE];   // [e * instances + g]
    __shared__ int gt_match[MAX_SIDE];
    const int group = blockIdx.x, lane = threadIdx.x, o = group % objects;
    const int ng = clamped_instances(gt_counts, group, instances);
    const double n = (double)clamped_count(counts, o, vmax);   // an empty mesh gives NaN means, which are never matched
    const double inf = (double)__builtin_inff();
    unsigned live = 0u;
    for (int e = 0; e < slots; ++e) {
        const size_t row = (size_t)group * slots + e;
        float pe[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) pe[j] = est[row * 12 + j];
        const bool on = !(pose_abs_sum(pe) < 1e-4);   // wave-uniform
        if (on) live |= 1u << e;
        for (int g = 0; g < instances; ++g) {
            double s2 = inf, s3 = inf;
            if (on && g < ng) {
                const double* in = partial + (row * chunks * instances + g) * 2;
                s2 = s3 = 0.0;
                for (int c = lane; c < chunks; c += 64) {
                    s2 += in[(size_t)c * instances * 2];
                    s3 += in[(size_t)c * instances * 2 + 1];
                }
                s2 = wave_sum(s2) / n;
                s3 = wave_sum(s3) / n;
            }
            if (lane == 0) {
                mean2[e * instances + g] = s2;
                mean3[e * instances + g] = s3;
                err[(row * instances + g) * 2] = (float)s2;
                err[(row * instances + g) * 2 + 1] = (float)s3;
            }
        }
    }
    if (lane != 0) return;
    int* em = est_match + (size_t)group * slots;
    const int matched = cp_match::greedy_match(mean3, slots, ng, instances, live, em, gt_match);
    const double diameter = (double)diameters[o];
    int tp3 = 0, tp2 = 0;
    for (int g = 0; g < instances; ++g) {
        float* r = gt_rec + ((size_t)group * instances + g) * 5;
        const int e = g < ng ? gt_match[g] : cp_match::UNMATCHED;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (e >= 0) {
            const double e2 = mean2[e * instances + g], e3 = mean3[e * instances + g];
            v[0] = (float)e2;
            v[1] = (float)e3;
            v[2] = e3 < diameter * 0.1 ? 1.f : 0.f;
            v[3] = e2 < (double)allowed_error_2d ? 1.f : 0.f;
            tp3 += v[2] != 0.f;
            tp2 += v[3] != 0.f;
        }
        r[0] = (float)e;
#pragma unroll
        for (int j = 0; j < 4; ++j) r[1 + j] = v[j];
    }
    int* t = tally + (size_t)group * 5;
    t[0] = ng;
    t[1] = __popc(live);
    t[2] = matched;
    t[3] = tp3;
    t[4] = tp2;
}

template <int G>
void launch_points(dim3 grid, hipStream_t st, const float* points, const int32_t* counts, const int32_t* symmetric, int objects, int vmax,
                   const float* est, int slots, const float* gt, int instances, const int32_t* gt_counts, const float* cams, double* partial) {
    CP_LAUNCH(match_points_kernel<G>, grid, dim3(THREADS), 0, st, points, counts, symmetric, objects, vmax, est, slots, gt, instances, gt_counts,
              cams, partial);
}

}  // namespace

extern "C" size_t cp_pose_match_workspace_bytes(int batch, int objects, int vmax, int slots, int instances) {
    if (batch < 1 || objects < 1 || vmax < 1 || slots < 1 || slots > MAX_SIDE || instances < 1 || instances > MAX_SIDE) return 0;
    return (size_t)batch * objects * slots * chunks_of(vmax) * instances * 2 * sizeof(double);
}

extern "C" int cp_pose_match_f32(const float* points, const int32_t* counts, const int32_t* symmetric, int objects, int vmax, const float* est,
                                 int slots, const float* gt, int instances, const int32_t* gt_counts, const float* cams, const float* diameters,
                                 int batch, float allowed_error_2d, void* workspace, float* err, float* gt_rec, int32_t* est_match, int32_t* tally,
                                 void* stream) {
    CP_REQUIRE(points && counts && symmetric && est && gt && gt_counts && cams && diameters && workspace && err && gt_rec && est_match && tally,
               "cp_pose_match_f32: null pointer");
    CP_REQUIRE(objects >= 1 && batch >= 1 && vmax >= 1, "cp_pose_match_f32: objects, batch and vmax must be positive (got %d, %d, %d)", objects,
               batch, vmax);
    CP_REQUIRE(slots >= 1 && slots <= MAX_SIDE && instances >= 1 && instances <= MAX_SIDE,
               "cp_pose_match_f32: slots and instances must lie in 1..%d (got %d, %d)", MAX_SIDE, slots, instances);
    CP_REQUIRE((long long)batch * objects * slots <= 65535,
               "cp_pose_match_f32: more than 65535 (image, object, slot) rows in one call (batch %d x objects %d x slots %d)", batch, objects, slots);
    CP_REQUIRE(vmax <= (1 << 24), "cp_pose_match_f32: vmax %d is above 2^24 points", vmax);
    CP_REQUIRE(((uintptr_t)workspace & 7) == 0, "cp_pose_match_f32: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int groups = batch * objects, chunks = chunks_of(vmax);
    const dim3 grid(chunks, groups * slots);
    double* partial = (double*)workspace;
#define CP_MATCH_POINTS(G) launch_points<G>(grid, st, points, counts, symmetric, objects, vmax, est, slots, gt, instances, gt_counts, cams, partial)
    if (instances <= 1) CP_MATCH_POINTS(1);
    else if (instances <= 2) CP_MATCH_POINTS(2);
    else if (instances <= 4) CP_MATCH_POINTS(4);
    else if (instances <= 8) CP_MATCH_POINTS(8);
    else CP_MATCH_POINTS(16);
#undef CP_MATCH_POINTS
    if (int rc = cp::check_launch("cp_pose_match_f32 (points)")) return rc;
    CP_LAUNCH(match_assign_kernel, dim3(groups), dim3(64), 0, st, counts, objects, vmax, chunks, est, slots, instances, gt_counts, diameters,
              allowed_error_2d, (const double*)partial, err, gt_rec, est_match, tally);
    return cp::check_launch("cp_pose_match_f32 (assign)");
}
