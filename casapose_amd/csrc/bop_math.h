// BOP pose errors with object symmetries: e_MSSD = min_S max_x |P^ x - P_ S x| (millimetres) and e_MSPD = min_S max_x |proj(P^ x) - proj(P_ S x)|
// (pixels), for an estimated pose P^, a ground-truth pose P_, a camera matrix K and the symmetry transforms S of the object.  The per-point
// arithmetic of the device kernels (bop_errors.hip) and of the stand-alone self-test (bop_selftest.cpp), as __host__ __device__ code: one copy.
//
// The rules:
//   1. zero pose     a pair whose estimated pose has |sum of its 12 entries| < 1e-4 (summed in fp64, as pose_eval.hip's pose_abs_sum) is "no
//                    estimate": both errors are +inf.  A sum that is not finite is treated the same way: a maximum would skip its NaNs.
//   2. composition   P_ S = [R_ R_s | R_ t_s + t_] is formed once per (pair, symmetry) in fp64 from the fp32 inputs and rounded once to fp32
//   3. transform     three fp32 FMAs per coordinate, as pose_eval.hip's transform
//   4. projection    (u, v, w) = K c with a general 3x3 K; pixel = (u, v) * (1 / w), and (0, 0) where w is exactly 0.  The reciprocal is
//                    v_rcp_f32 on the device (1 ulp) and 1.0f / w on the host: about 2^-23 * 640 = 8e-5 px, a thirtieth of the 2-D test gate
//   5. distances     direct coordinate differences, squared; the maximum over the vertices is taken on the squares and the root once per
//                    (pair, symmetry): sqrt is monotone
//   6. padding       vertices at index >= count and symmetries at index >= sym_count take no part; an object without vertices gives +inf
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BOP_HD __host__ __device__ inline
#else
#define BOP_HD inline
#endif

namespace cp_bop {

constexpr int PAIR_FLOATS = 36;        // estimated pose 12, ground-truth pose 12, K 9, three pads: the record of cp_pose_eval_f32
constexpr int THREADS = 256;
constexpr int VERTS_PER_THREAD = 4;    // vertices a thread keeps in registers (raw, transformed and projected) while it walks the symmetries
constexpr int TILE = THREADS * VERTS_PER_THREAD;   // vertices per block and step
constexpr int SYM_GROUP = 16;          // symmetries per block: 2 * SYM_GROUP running maxima per thread

BOP_HD int clamp_count(int n, int hi) { return n < 0 ? 0 : (n > hi ? hi : n); }

// rule 1
BOP_HD bool no_estimate(const float* pose) {
    double s = 0.0;
    for (int i = 0; i < 12; ++i) s += (double)pose[i];
    s = fabs(s);
    return !(s >= 1e-4 && s < (double)INFINITY);
}

// rule 2: entry e (row-major 3x4) of gt * sym
BOP_HD float compose_entry(const float* gt, const float* sym, int e) {
    const int r = e >> 2, c = e & 3;
    double v = (double)gt[4 * r] * (double)sym[c] + (double)gt[4 * r + 1] * (double)sym[4 + c] + (double)gt[4 * r + 2] * (double)sym[8 + c];
    if (c == 3) v += (double)gt[4 * r + 3];
    return (float)v;
}

struct P3 {
    float x, y, z;
};
struct P2 {
    float u, v;
};

// rule 3; rt is a row-major 3x4
BOP_HD P3 transform(const float* rt, float x, float y, float z) {
    return {fmaf(rt[0], x, fmaf(rt[1], y, fmaf(rt[2], z, rt[3]))), fmaf(rt[4], x, fmaf(rt[5], y, fmaf(rt[6], z, rt[7]))),
            fmaf(rt[8], x, fmaf(rt[9], y, fmaf(rt[10], z, rt[11])))};
}

BOP_HD float reciprocal(float w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(w);
#else
    return 1.0f / w;
#endif
}

// rule 4
BOP_HD P2 project(const float* k, P3 c) {
    const float u = fmaf(k[0], c.x, fmaf(k[1], c.y, k[2] * c.z)), v = fmaf(k[3], c.x, fmaf(k[4], c.y, k[5] * c.z));
    const float w = fmaf(k[6], c.x, fmaf(k[7], c.y, k[8] * c.z));
    const float r = reciprocal(w);
    return {w != 0.f ? u * r : 0.f, w != 0.f ? v * r : 0.f};
}

// rule 5
BOP_HD float dist2(P3 a, P3 b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return fmaf(dx, dx, fmaf(dy, dy, dz * dz));
}
BOP_HD float dist2(P2 a, P2 b) {
    const float du = a.u - b.u, dv = a.v - b.v;
    return fmaf(du, du, dv * dv);
}

// What the two kernels compute for one pair, as a plain loop (the self-test runs it under the sanitizers).  points [count][3], syms
// [sym_count][12], pair [PAIR_FLOATS]; per_symmetry is NULL or [smax][2] and gets +inf from sym_count on.  errors [2] = (e_MSSD, e_MSPD).
inline void pair_errors_serial(const float* points, int count, const float* syms, int sym_count, int smax, const float* pair, float* errors,
                               float* per_symmetry) {
    const float inf = INFINITY;
    errors[0] = errors[1] = inf;
    if (per_symmetry)
        for (int s = 0; s < 2 * smax; ++s) per_symmetry[s] = inf;
    if (no_estimate(pair) || count < 1) return;
    const float *est = pair, *gt = pair + 12, *k = pair + 24;
    for (int s = 0; s < sym_count && s < smax; ++s) {
        float m[12];
        for (int e = 0; e < 12; ++e) m[e] = compose_entry(gt, syms + 12 * (size_t)s, e);
        float m3 = 0.f, m2 = 0.f;
        for (int i = 0; i < count; ++i) {
            const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
            const P3 a = transform(est, x, y, z), b = transform(m, x, y, z);
            m3 = fmaxf(m3, dist2(a, b));
            m2 = fmaxf(m2, dist2(project(k, a), project(k, b)));
        }
        const float e3 = sqrtf(m3), e2 = sqrtf(m2);
        if (per_symmetry) {
            per_symmetry[2 * s] = e3;
            per_symmetry[2 * s + 1] = e2;
        }
        errors[0] = fminf(errors[0], e3);
        errors[1] = fminf(errors[1], e2);
    }
}

}  // namespace cp_bop
