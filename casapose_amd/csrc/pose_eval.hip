// Pose statistics on the device: the per-(image, object) record of map_estimates (casapose/pose_estimation/ransac_voting.py:561-625 of the
// reference; the host counterpart is evaluate_poses in casapose_amd/pose_estimation/pose_evaluation.py).  For every pair: the mean 2-D
// reprojection distance and the mean ADD distance of the evaluation mesh under the estimated and the ground-truth pose -- ADD-S (distance to
// the nearest estimated point) where the object's `symmetric` flag is set -- and the miss / false-positive bookkeeping.
//
// fp32 VALU, no MFMA.  Distances are direct differences (ax-bx)^2 + (ay-by)^2 + (az-bz)^2: camera-frame coordinates are ~1e3 mm, so the
// |a|^2 - 2 a.b + |b|^2 form (which the reference evaluates in fp64) would cancel squares of 1e6 down to ~0.1 mm^2 in fp32.  The per-pair
// sums are fp64, reduced in a fixed order (wave shuffle tree, waves in index order, chunks in lane-strided index order): no atomics, so two
// calls on the same input give bit-identical records.
//
// pose_points_kernel: grid (ceil(vmax / 256), pairs), 256 threads, one thread per target point.  ADD-S walks the estimated-pose points in LDS
//   tiles of EST_TILE float4 {x, y, z, 0}, already transformed and written cooperatively; every lane reads the same address per step (a
//   broadcast: conflict-free), and keeps a running minimum of d^2.  Brute force is 7862^2 = 62 M point pairs of 8 VALU operations for the largest
//   symmetric LM mesh: VALU-bound, tens of microseconds over 256 CUs.  16 KB of LDS per block leaves the wave limit (8 blocks per CU) binding.
// pose_record_kernel: one wave per pair sums the chunk partials, divides by the count, classifies and writes the record.
#include "common.h"
#include "pose_eval_math.h"

namespace {

using namespace cp_pose;   // the per-point arithmetic, the tile and the order of the sums: pose_eval_math.h, shared with pose_match.hip
constexpr int PAIR_FLOATS = 36, RECORD_FLOATS = 6;

struct Pair {
    float est[12], gt[12], k[9], diameter, valid;
};

__device__ __forceinline__ Pair load_pair(const float* __restrict__ rec) {
    Pair p;
#pragma unroll
    for (int i = 0; i < 12; ++i) p.est[i] = rec[i];
#pragma unroll
    for (int i = 0; i < 12; ++i) p.gt[i] = rec[12 + i];
#pragma unroll
    for (int i = 0; i < 9; ++i) p.k[i] = rec[24 + i];
    p.diameter = rec[33];
    p.valid = rec[34];
    return p;
}

// a pair whose record is fixed by its flags alone: not in the ground truth, or in it with the zero pose
__device__ __forceinline__ bool pair_skipped(const Pair& p) { return p.valid == 0.f || pose_abs_sum(p.est) < 1e-4; }

__global__ void __launch_bounds__(THREADS) pose_points_kernel(const float* __restrict__ points, const int* __restrict__ counts,
                                                              const int* __restrict__ symmetric, int objects, int vmax,
                                                              const float* __restrict__ pairs, double* __restrict__ partial,
                                                              float* __restrict__ point_err2, float* __restrict__ point_err3) {
    __shared__ float4 tile[EST_TILE];
    __shared__ double wsum[2][THREADS / 64];
    const int pair = blockIdx.y, chunk = blockIdx.x, o = pair % objects, tid = threadIdx.x;
    const int i = chunk * THREADS + tid;
    const Pair p = load_pair(pairs + (size_t)pair * PAIR_FLOATS);
    const int cnt = clamped_count(counts, o, vmax);
    double* out = partial + ((size_t)pair * gridDim.x + chunk) * 2;
    if (pair_skipped(p) || chunk * THREADS >= cnt) {   // block-uniform
        if (tid == 0) out[0] = out[1] = 0.0;
        if (i < vmax) {
            if (point_err2) point_err2[(size_t)pair * vmax + i] = 0.f;
            if (point_err3) point_err3[(size_t)pair * vmax + i] = 0.f;
        }
        return;
    }
    const float* obj = points + (size_t)o * vmax * 3;
    const bool active = i < cnt;
    float3 tg = make_float3(0.f, 0.f, 0.f);
    float e2 = 0.f, e3 = 0.f;
    if (active) {
        const float x = obj[3 * (size_t)i], y = obj[3 * (size_t)i + 1], z = obj[3 * (size_t)i + 2];
        const float3 es = transform(p.est, x, y, z);
        tg = transform(p.gt, x, y, z);
        e2 = pixel_distance(project(p.k, tg), project(p.k, es));
        e3 = add_distance(tg, es);
    }
    if (symmetric[o] != 0) {
        float best = __builtin_inff();
        for (int t0 = 0; t0 < cnt; t0 += EST_TILE) {
            __syncthreads();   // the previous tile has been read
            const int padded = fill_tile(tile, obj, p.est, t0, cnt, tid);
            __syncthreads();
            if (active) {
                for (int j = 0; j < padded; j += TILE_UNROLL) {
#pragma unroll
                    for (int u = 0; u < TILE_UNROLL; ++u) {
                        const float4 q = tile[j + u];
                        best = fminf(best, squared_distance(tg, q.x, q.y, q.z));
                    }
                }
            }
        }
        if (active) e3 = adds_distance(best);
    }
    if (active) {
        if (point_err2) point_err2[(size_t)pair * vmax + i] = e2;
        if (point_err3) point_err3[(size_t)pair * vmax + i] = e3;
    } else if (i < vmax) {
        if (point_err2) point_err2[(size_t)pair * vmax + i] = 0.f;
        if (point_err3) point_err3[(size_t)pair * vmax + i] = 0.f;
    }
    const double s2 = wave_sum((double)e2), s3 = wave_sum((double)e3);
    if ((tid & 63) == 0) {
        wsum[0][tid >> 6] = s2;
        wsum[1][tid >> 6] = s3;
    }
    __syncthreads();
    if (tid == 0) {
        double a = 0.0, b = 0.0;
#pragma unroll
        for (int w = 0; w < THREADS / 64; ++w) {
            a += wsum[0][w];
            b += wsum[1][w];
        }
        out[0] = a;
        out[1] = b;
    }
}

__global__ void __launch_bounds__(64) pose_record_kernel(const int* __restrict__ counts, int objects, int vmax, int chunks,
                                                         const float* __restrict__ pairs, float allowed_error_2d,
                                                         const double* __restrict__ partial, float* __restrict__ records) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    const Pair p = load_pair(pairs + (size_t)pair * PAIR_FLOATS);
    const double* in = partial + (size_t)pair * chunks * 2;
    double s2 = 0.0, s3 = 0.0;
    for (int c = lane; c < chunks; c += 64) {
        s2 += in[2 * c];
        s3 += in[2 * c + 1];
    }
    s2 = wave_sum(s2);
    s3 = wave_sum(s3);
    if (lane != 0) return;
    float* r = records + (size_t)pair * RECORD_FLOATS;
    float v[RECORD_FLOATS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p.valid == 0.f) {
        v[5] = pose_abs_sum(p.est) > 1e-4 ? 1.f : 0.f;
    } else if (pair_skipped(p)) {
        v[0] = 99.9f;
        v[1] = 999.9f;
        v[4] = 1.f;
    } else {
        const double n = (double)clamped_count(counts, pair % objects, vmax);   // an empty mesh gives NaN means, as the host's mean of nothing
        const double e2 = s2 / n, e3 = s3 / n;
        v[0] = (float)e2;
        v[1] = (float)e3;
        v[2] = e3 < (double)p.diameter * 0.1 ? 1.f : 0.f;
        v[3] = e2 < (double)allowed_error_2d ? 1.f : 0.f;
    }
#pragma unroll
    for (int i = 0; i < RECORD_FLOATS; ++i) r[i] = v[i];
}

}  // namespace

extern "C" size_t cp_pose_eval_workspace_bytes(int batch, int objects, int vmax) {
    if (batch < 1 || objects < 1 || vmax < 1) return 0;
    return (size_t)batch * objects * chunks_of(vmax) * 2 * sizeof(double);
}

extern "C" int cp_pose_eval_est_tile(void) { return EST_TILE; }

extern "C" int cp_pose_eval_f32(const float* points, const int32_t* counts, const int32_t* symmetric, int objects, int vmax, const float* pairs,
                                int batch, float allowed_error_2d, void* workspace, float* records, float* point_err2, float* point_err3,
                                void* stream) {
    CP_REQUIRE(points && counts && symmetric && pairs && workspace && records, "cp_pose_eval_f32: null pointer");
    CP_REQUIRE(objects >= 1 && batch >= 1 && vmax >= 1, "cp_pose_eval_f32: objects, batch and vmax must be positive (got %d, %d, %d)", objects, batch,
               vmax);
    CP_REQUIRE((long long)batch * objects <= 65535, "cp_pose_eval_f32: more than 65535 (image, object) pairs in one call (batch %d x objects %d)",
               batch, objects);
    CP_REQUIRE(vmax <= (1 << 24), "cp_pose_eval_f32: vmax %d is above 2^24 points", vmax);
    CP_REQUIRE(((uintptr_t)workspace & 7) == 0, "cp_pose_eval_f32: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int npairs = batch * objects, chunks = chunks_of(vmax);
    CP_LAUNCH(pose_points_kernel, dim3(chunks, npairs), dim3(THREADS), 0, st, points, counts, symmetric, objects, vmax, pairs, (double*)workspace,
              point_err2, point_err3);
    if (int rc = cp::check_launch("cp_pose_eval_f32 (points)")) return rc;
    CP_LAUNCH(pose_record_kernel, dim3(npairs), dim3(64), 0, st, counts, objects, vmax, chunks, pairs, allowed_error_2d, (const double*)workspace,
              records);
    return cp::check_launch("cp_pose_eval_f32 (records)");
}
