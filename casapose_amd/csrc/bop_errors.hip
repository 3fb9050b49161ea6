// BOP pose errors on the device: e_MSSD and e_MSPD (bop_math.h states both and the rules of the arithmetic) for arbitrary (estimate, ground-truth
// instance) pairs, each a minimum over the object's symmetry transforms of a maximum over every vertex of its evaluation mesh.  A sibling of
// pose_eval.hip: the same pair record, pose transform and projection, fp32 VALU, no MFMA, no atomics.
//
// bop_max_kernel: grid (pairs * ceil(smax / SYM_GROUP)), 256 threads.  A block owns one pair and SYM_GROUP = 16 consecutive symmetries.  It
//   composes their P_ S in fp64 (one entry per thread, rounded once to fp32) into LDS, then walks the mesh in steps of TILE = 1024 vertices: a
//   thread keeps VERTS_PER_THREAD = 4 vertices, their estimated-pose points and pixels in registers -- none of which depends on the symmetry --
//   and walks the block's symmetries, reading each composed 3x4 from LDS at one address per step (a broadcast, as pose_points_kernel reads its
//   tile) and keeping 2 * SYM_GROUP running maxima of squared distances.  Vertex slots past the mesh repeat its last vertex, symmetry slots past
//   the object's count repeat the block's last symmetry: neither changes a maximum and the inner loops need no guards.  The maxima are reduced
//   in a fixed order (wave shuffle tree, then the four waves in index order) and written to the workspace [pairs][smax][2].
// bop_min_kernel: one wave per pair takes the root of every maximum, writes the optional per-symmetry array and reduces the minimum.
#include "bop_math.h"
#include "common.h"

namespace {

using namespace cp_bop;

struct Skip {
    bool skip;
    int o, cnt, sc;
};

// block-uniform: what both kernels decide from a pair's record and its object before they touch a vertex
__device__ __forceinline__ Skip classify(const float* __restrict__ rec, const int* __restrict__ object_index, const int* __restrict__ counts,
                                         const int* __restrict__ sym_counts, int objects, int vmax, int smax, size_t pair) {
    Skip s = {true, object_index[pair], 0, 0};
    if (s.o < 0 || s.o >= objects) return s;
    s.cnt = clamp_count(counts[s.o], vmax);
    s.sc = clamp_count(sym_counts[s.o], smax);
    s.skip = s.cnt < 1 || no_estimate(rec);
    return s;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m));
    return v;
}

__global__ void __launch_bounds__(THREADS) bop_max_kernel(const float* __restrict__ points, const int* __restrict__ counts,
                                                          const float* __restrict__ syms, const int* __restrict__ sym_counts, int objects,
                                                          int vmax, int smax, int groups, const float* __restrict__ pairs,
                                                          const int* __restrict__ object_index, float* __restrict__ maxima) {
    __shared__ float mat[SYM_GROUP * 12];
    __shared__ float red[THREADS / 64][SYM_GROUP * 2];
    const int tid = threadIdx.x;
    const size_t pair = blockIdx.x / (unsigned)groups;
    const int s0 = (int)(blockIdx.x % (unsigned)groups) * SYM_GROUP;
    const float* rec = pairs + pair * PAIR_FLOATS;
    const Skip c = classify(rec, object_index, counts, sym_counts, objects, vmax, smax, pair);
    if (c.skip || s0 >= c.sc) return;   // block-uniform; bop_min_kernel reads nothing of what is not written here
    const int ng = min(SYM_GROUP, c.sc - s0);
    if (tid < SYM_GROUP * 12) {
        const int g = min(tid / 12, ng - 1);
        mat[tid] = compose_entry(rec + 12, syms + ((size_t)c.o * smax + s0 + g) * 12, tid % 12);
    }
    float est[12], k[9];
#pragma unroll
    for (int i = 0; i < 12; ++i) est[i] = rec[i];
#pragma unroll
    for (int i = 0; i < 9; ++i) k[i] = rec[24 + i];
    float m3[SYM_GROUP], m2[SYM_GROUP];
#pragma unroll
    for (int g = 0; g < SYM_GROUP; ++g) m3[g] = m2[g] = 0.f;
    __syncthreads();
    const float* obj = points + (size_t)c.o * vmax * 3;
    for (int v0 = 0; v0 < c.cnt; v0 += TILE) {
        // The composed matrices are re-read from LDS in every step.  Without this the compiler hoists all SYM_GROUP * 12 reads out of the loop:
        // 256 VGPRs and 13 AGPRs, one wave per SIMD.
        asm volatile("" ::: "memory");
        float x[VERTS_PER_THREAD], y[VERTS_PER_THREAD], z[VERTS_PER_THREAD];
        P3 a[VERTS_PER_THREAD];
        P2 pa[VERTS_PER_THREAD];
#pragma unroll
        for (int u = 0; u < VERTS_PER_THREAD; ++u) {
            const size_t j = (size_t)min(v0 + u * THREADS + tid, c.cnt - 1);
            x[u] = obj[3 * j];
            y[u] = obj[3 * j + 1];
            z[u] = obj[3 * j + 2];
            a[u] = transform(est, x[u], y[u], z[u]);
            pa[u] = project(k, a[u]);
        }
#pragma unroll
        for (int g = 0; g < SYM_GROUP; ++g) {
            float m[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) m[i] = mat[g * 12 + i];
#pragma unroll
            for (int u = 0; u < VERTS_PER_THREAD; ++u) {
                const P3 b = transform(m, x[u], y[u], z[u]);
                m3[g] = fmaxf(m3[g], dist2(a[u], b));
                m2[g] = fmaxf(m2[g], dist2(pa[u], project(k, b)));
            }
        }
    }
#pragma unroll
    for (int g = 0; g < SYM_GROUP; ++g) {
        const float w3 = wave_max(m3[g]), w2 = wave_max(m2[g]);
        if ((tid & 63) == 0) {
            red[tid >> 6][2 * g] = w3;
            red[tid >> 6][2 * g + 1] = w2;
        }
    }
    __syncthreads();
    if (tid < 2 * ng) {
        float v = red[0][tid];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) v = fmaxf(v, red[w][tid]);
        maxima[(pair * smax + s0) * 2 + tid] = v;
    }
}

__global__ void __launch_bounds__(64) bop_min_kernel(const int* __restrict__ counts, const int* __restrict__ sym_counts, int objects, int vmax,
                                                     int smax, const float* __restrict__ pairs, const int* __restrict__ object_index,
                                                     const float* __restrict__ maxima, float* __restrict__ errors,
                                                     float* __restrict__ per_symmetry) {
    const size_t pair = blockIdx.x;
    const int lane = threadIdx.x;
    const Skip c = classify(pairs + pair * PAIR_FLOATS, object_index, counts, sym_counts, objects, vmax, smax, pair);
    const int sc = c.skip ? 0 : c.sc;
    const float inf = __builtin_inff();
    float e3 = inf, e2 = inf;
    for (int s = lane; s < smax; s += 64) {
        float d3 = inf, d2 = inf;
        if (s < sc) {
            d3 = sqrtf(maxima[(pair * smax + s) * 2]);
            d2 = sqrtf(maxima[(pair * smax + s) * 2 + 1]);
        }
        if (per_symmetry) {
            per_symmetry[(pair * smax + s) * 2] = d3;
            per_symmetry[(pair * smax + s) * 2 + 1] = d2;
        }
        e3 = fminf(e3, d3);
        e2 = fminf(e2, d2);
    }
    e3 = wave_min(e3);
    e2 = wave_min(e2);
    if (lane == 0) {
        errors[2 * pair] = e3;
        errors[2 * pair + 1] = e2;
    }
}

inline int groups_of(int smax) { return (smax + SYM_GROUP - 1) / SYM_GROUP; }

}  // namespace

extern "C" size_t cp_bop_errors_workspace_bytes(int npairs, int smax) {
    if (npairs < 1 || smax < 1) return 0;
    return (size_t)npairs * (size_t)smax * 2 * sizeof(float);
}

extern "C" int cp_bop_errors_tile(void) { return TILE; }
extern "C" int cp_bop_errors_sym_group(void) { return SYM_GROUP; }

extern "C" int cp_bop_errors_f32(const float* points, const int32_t* counts, int objects, int vmax, const float* syms, const int32_t* sym_counts,
                                 int smax, const float* pairs, const int32_t* object_index, int npairs, void* workspace, float* errors,
                                 float* per_symmetry, void* stream) {
    CP_REQUIRE(points && counts && syms && sym_counts && pairs && object_index && workspace && errors, "cp_bop_errors_f32: null pointer");
    CP_REQUIRE(objects >= 1 && vmax >= 1 && smax >= 1 && npairs >= 1,
               "cp_bop_errors_f32: objects, vmax, smax and npairs must be positive (got %d, %d, %d, %d)", objects, vmax, smax, npairs);
    CP_REQUIRE(vmax <= (1 << 24), "cp_bop_errors_f32: vmax %d is above 2^24 points", vmax);
    CP_REQUIRE(smax <= (1 << 16), "cp_bop_errors_f32: smax %d is above 2^16 transforms", smax);
    CP_REQUIRE((long long)npairs * groups_of(smax) <= 0xffffffLL,
               "cp_bop_errors_f32: npairs %d x %d symmetry groups is above 2^24 - 1 blocks; split the call", npairs, groups_of(smax));
    CP_REQUIRE(((uintptr_t)workspace & 7) == 0, "cp_bop_errors_f32: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int groups = groups_of(smax);
    CP_LAUNCH(bop_max_kernel, dim3((unsigned)(npairs * groups)), dim3(THREADS), 0, st, points, counts, syms, sym_counts, objects, vmax, smax, groups,
              pairs, object_index, (float*)workspace);
    if (int rc = cp::check_launch("cp_bop_errors_f32 (maxima)")) return rc;
    CP_LAUNCH(bop_min_kernel, dim3((unsigned)npairs), dim3(64), 0, st, counts, sym_counts, objects, vmax, smax, pairs, object_index,
              (const float*)workspace, errors, per_symmetry);
    return cp::check_launch("cp_bop_errors_f32 (minima)");
}
