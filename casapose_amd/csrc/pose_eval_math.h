// The per-point arithmetic of the pose statistics, shared by pose_eval.hip (one estimate against one ground-truth pose) and pose_match.hip (up
// to 16 estimates against up to 16 ground-truth instances): one copy, so that an error of the matcher equals the record of cp_pose_eval_f32 on
// the same pair bit for bit.  Device code; nothing here knows how a kernel packs its poses.
//
// fp32 VALU.  Distances are direct differences (ax-bx)^2 + (ay-by)^2 + (az-bz)^2: camera-frame coordinates are ~1e3 mm, so the
// |a|^2 - 2 a.b + |b|^2 form (which the reference evaluates in fp64) would cancel squares of 1e6 down to ~0.1 mm^2 in fp32.  Sums are fp64 in a
// fixed order: wave_sum's shuffle tree, waves in index order, chunks in lane-strided index order.
#pragma once
#include <hip/hip_runtime.h>

namespace cp_pose {

constexpr int THREADS = 256;     // one thread per target point; a chunk is the points of one block
constexpr int EST_TILE = 1024;   // points per LDS tile (16 KB); a multiple of TILE_UNROLL
constexpr int TILE_UNROLL = 8;

inline int chunks_of(int vmax) { return (vmax + THREADS - 1) / THREADS; }

// |sum of the 12 pose entries| (map_estimates :576,:579).  "Zero pose" is decided here and nowhere else: every kernel classifies an estimate
// from it, by pose_abs_sum(...) < 1e-4.
__device__ __forceinline__ double pose_abs_sum(const float* pose) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) s += (double)pose[i];
    return fabs(s);
}

__device__ __forceinline__ int clamped_count(const int* __restrict__ counts, int o, int vmax) {
    const int c = counts[o];
    return c < 0 ? 0 : (c > vmax ? vmax : c);
}

__device__ __forceinline__ float3 transform(const float* rt, float x, float y, float z) {
    return make_float3(fmaf(rt[0], x, fmaf(rt[1], y, fmaf(rt[2], z, rt[3]))), fmaf(rt[4], x, fmaf(rt[5], y, fmaf(rt[6], z, rt[7]))),
                       fmaf(rt[8], x, fmaf(rt[9], y, fmaf(rt[10], z, rt[11]))));
}

// project_tf (:173-182): pixel = (K cam).xy / (K cam).z, 0 where that z is exactly 0 (divide_no_nan)
__device__ __forceinline__ float2 project(const float* k, float3 c) {
    const float u = fmaf(k[0], c.x, fmaf(k[1], c.y, k[2] * c.z)), v = fmaf(k[3], c.x, fmaf(k[4], c.y, k[5] * c.z));
    const float w = fmaf(k[6], c.x, fmaf(k[7], c.y, k[8] * c.z));
    return w != 0.f ? make_float2(u / w, v / w) : make_float2(0.f, 0.f);
}

// the 2-D distance of a target point's pixel from the estimated point's
__device__ __forceinline__ float pixel_distance(float2 pt, float2 pe) {
    const float du = pt.x - pe.x, dv = pt.y - pe.y;
    return sqrtf(fmaf(du, du, dv * dv));
}

// squared camera-frame distance of a target point from an estimated point
__device__ __forceinline__ float squared_distance(float3 tg, float qx, float qy, float qz) {
    const float dx = tg.x - qx, dy = tg.y - qy, dz = tg.z - qz;
    return fmaf(dx, dx, fmaf(dy, dy, dz * dz));
}

// ADD per point
__device__ __forceinline__ float add_distance(float3 tg, float3 es) { return sqrtf(squared_distance(tg, es.x, es.y, es.z)); }

// ADD-S per point from the smallest squared distance (:610)
__device__ __forceinline__ float adds_distance(float best) { return sqrtf(fabsf(best) + 1e-5f); }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// One LDS tile of the ADD-S walk: points t0 .. t0+n-1 of `obj` under `pose`, written cooperatively as float4 {x, y, z, 0}.  Slots n .. padded-1
// repeat the tile's first point: the minimum does not change and the walk needs no remainder loop.  Returns padded (<= EST_TILE).  The caller
// puts a barrier before (the previous tile has been read) and after.
__device__ __forceinline__ int fill_tile(float4* tile, const float* __restrict__ obj, const float* pose, int t0, int cnt, int tid) {
    const int n = min(EST_TILE, cnt - t0);
    const int padded = (n + TILE_UNROLL - 1) / TILE_UNROLL * TILE_UNROLL;
    for (int j = tid; j < padded; j += THREADS) {
        const size_t s = (size_t)(t0 + (j < n ? j : 0));
        const float3 q = transform(pose, obj[3 * s], obj[3 * s + 1], obj[3 * s + 2]);
        tile[j] = make_float4(q.x, q.y, q.z, 0.f);
    }
    return padded;
}

}  // namespace cp_pose
