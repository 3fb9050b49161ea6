// Keypoints and models_info of a set of meshes: per object the axis-aligned box, the largest vertex distance (BOP's `diameter`), and the box
// centre followed by farthest-point samples of the vertices (the reference's obj_NNNNNN_keypoints.ply).  The arithmetic of the device kernels
// (models.hip), of their host twin (cp_model_prep_host_f32) and of the stand-alone self-test (models_selftest.cpp), as __host__ __device__ code.
// Nothing here calls a library beyond <math.h>.
//
// The rules, fixed so that the device, the twin and a NumPy restatement agree bit for bit:
//   1. box        per-axis min and max of the object's N fp32 vertices, in fp32; between -0 and +0 the minimum is -0 and the maximum +0
//   2. centre     c = 0.5 * ((double)min + (double)max) per axis; keypoint 0 is c rounded to fp32
//   3. distance   d2(a, b) = (dx*dx + dy*dy) + dz*dz with dx = (double)a.x - (double)b.x, every product and sum rounded to fp64 (no FMA)
//   4. diameter   the maximum of d2 over all vertex pairs (0 for N = 1); the caller takes the square root.  A maximum does not depend on the
//                 order it is taken in: the pairs are walked as the upper triangle of TILE x TILE tiles, tile pair p of an object <-> (ta <= tb)
//   5. keypoints  m_i = d2(P_i, c); K - 1 times: j = the vertex with the largest m, the lowest index among equals; keypoint = P_j unchanged,
//                 index = j; m_i = min(m_i, d2(P_i, P_j)).  A largest m that is not above 0 when a pick is due means fewer distinct vertices
//                 than keypoints: status ST_TOO_FEW, this pick and the later ones are zero (keypoints and indices)
//   6. limits     2 <= K <= 32 (K counts the centre), 1 <= N <= 2^22, at most 1024 objects per call; tile-pair counts are 64-bit
// An object whose vertex range [offset, offset + N) does not lie inside the vertex array, or whose N is outside rule 6, gets status ST_BAD_COUNT
// and zeros everywhere; nothing of it is read.  Memory beyond an object's own N is never treated as a point.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MODEL_HD __host__ __device__ inline
#else
#define MODEL_HD inline
#endif

namespace cp_model {

constexpr int MIN_POINTS = 2, MAX_POINTS = 32;
constexpr int MAX_VERTICES = 1 << 22;
constexpr int MAX_OBJECTS = 1024;
constexpr int TILE = 256;   // vertices per tile of the diameter's pair walk
constexpr int ST_OK = 0, ST_BAD_COUNT = 1, ST_TOO_FEW = 2;

// the workspace: tile-pair prefix sums int64 [objects + 1], then the running minima m fp64 [total]
MODEL_HD size_t workspace_bytes(int objects, long long total) { return ((size_t)objects + 1) * sizeof(int64_t) + (size_t)total * sizeof(double); }

MODEL_HD bool object_valid(long long offset, int n, long long total) { return n >= 1 && n <= MAX_VERTICES && offset >= 0 && offset <= total - n; }

MODEL_HD double dist2(double ax, double ay, double az, double bx, double by, double bz) {
#pragma clang fp contract(off)
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// rule 1's order of fp32 values: -0 below +0, NaN below and above nothing
MODEL_HD bool below(float v, float m) { return v < m || (v == m && __builtin_signbit(v) && !__builtin_signbit(m)); }

MODEL_HD void box_add(float* mn, float* mx, const float* p) {
    for (int a = 0; a < 3; ++a) {
        if (below(p[a], mn[a])) mn[a] = p[a];
        if (below(mx[a], p[a])) mx[a] = p[a];
    }
}

MODEL_HD double centre(float mn, float mx) {
#pragma clang fp contract(off)
    return 0.5 * ((double)mn + (double)mx);
}

// rule 5's order of (m, index) candidates
MODEL_HD bool better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

MODEL_HD int tiles(int n) { return (n + TILE - 1) / TILE; }
MODEL_HD int64_t tile_pairs(int n) { return (int64_t)tiles(n) * (tiles(n) + 1) / 2; }

// pair p of an object's upper triangle, 0 <= p < tile_pairs(n): p = tb (tb + 1) / 2 + ta with ta <= tb.  p < 2^28, so the fp64 root is within one
// of the answer and the two loops settle it.
MODEL_HD void tile_of_pair(int64_t p, int& ta, int& tb) {
    int64_t t = (int64_t)((sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while (t > 0 && t * (t + 1) / 2 > p) --t;
    while ((t + 1) * (t + 2) / 2 <= p) ++t;
    tb = (int)t;
    ta = (int)(p - t * (t + 1) / 2);
}

// rule 5's failure from pick `first` on (keypoint first, index first - 1): zeros
MODEL_HD void zero_picks(float* kps, int32_t* idx, int K, int first) {
    for (int k = first; k < K; ++k) {
        kps[3 * k] = kps[3 * k + 1] = kps[3 * k + 2] = 0.f;
        if (k >= 1) idx[k - 1] = 0;
    }
}

// The serial twin: the same rules, one loop nest.  workspace: workspace_bytes(objects, total) bytes, 8-byte aligned.
inline void prep_serial(const float* verts, long long total, const long long* offsets, const int32_t* counts, int objects, int K, double* diameter_sq,
                        float* box, float* keypoints, int32_t* indices, int32_t* status, void* workspace) {
    int64_t* prefix = (int64_t*)workspace;
    double* m_all = (double*)(prefix + objects + 1);
    prefix[0] = 0;
    for (int o = 0; o < objects; ++o) prefix[o + 1] = prefix[o] + (object_valid(offsets[o], counts[o], total) ? tile_pairs(counts[o]) : 0);
    for (int o = 0; o < objects; ++o) {
        float* obox = box + 6 * (size_t)o;
        float* okp = keypoints + 3 * (size_t)K * o;
        int32_t* oidx = indices + (size_t)(K - 1) * o;
        const int n = counts[o];
        diameter_sq[o] = 0.0;
        if (!object_valid(offsets[o], n, total)) {
            status[o] = ST_BAD_COUNT;
            for (int a = 0; a < 6; ++a) obox[a] = 0.f;
            zero_picks(okp, oidx, K, 0);
            continue;
        }
        const float* P = verts + 3 * (size_t)offsets[o];
        double* m = m_all + offsets[o];
        // rules 1, 2
        float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int i = 0; i < n; ++i) box_add(mn, mx, P + 3 * (size_t)i);
        double c[3];
        for (int a = 0; a < 3; ++a) obox[a] = mn[a], obox[3 + a] = mx[a], c[a] = centre(mn[a], mx[a]), okp[a] = (float)c[a];
        // rule 5
        double bv = -1.0;
        int bi = 0x7fffffff;
        for (int i = 0; i < n; ++i) {
            m[i] = dist2((double)P[3 * (size_t)i], (double)P[3 * (size_t)i + 1], (double)P[3 * (size_t)i + 2], c[0], c[1], c[2]);
            if (better(m[i], i, bv, bi)) bv = m[i], bi = i;
        }
        status[o] = ST_OK;
        for (int k = 1; k < K; ++k) {
            if (!(bv > 0.0)) {
                status[o] = ST_TOO_FEW;
                zero_picks(okp, oidx, K, k);
                break;
            }
            const int j = bi;
            const float* Q = P + 3 * (size_t)j;
            okp[3 * k] = Q[0], okp[3 * k + 1] = Q[1], okp[3 * k + 2] = Q[2];
            oidx[k - 1] = j;
            if (k == K - 1) break;
            bv = -1.0, bi = 0x7fffffff;
            for (int i = 0; i < n; ++i) {
                const double d = dist2((double)P[3 * (size_t)i], (double)P[3 * (size_t)i + 1], (double)P[3 * (size_t)i + 2], (double)Q[0], (double)Q[1],
                                       (double)Q[2]);
                if (d < m[i]) m[i] = d;
                if (better(m[i], i, bv, bi)) bv = m[i], bi = i;
            }
        }
        // rule 4, in the kernel's tile order
        double best = 0.0;
        for (int64_t p = 0; p < prefix[o + 1] - prefix[o]; ++p) {
            int ta, tb;
            tile_of_pair(p, ta, tb);
            const int a1 = (ta + 1) * TILE < n ? (ta + 1) * TILE : n, b1 = (tb + 1) * TILE < n ? (tb + 1) * TILE : n;
            for (int i = ta * TILE; i < a1; ++i) {
                const double ax = (double)P[3 * (size_t)i], ay = (double)P[3 * (size_t)i + 1], az = (double)P[3 * (size_t)i + 2];
                for (int j = ta == tb ? i + 1 : tb * TILE; j < b1; ++j) {
                    const double d = dist2(ax, ay, az, (double)P[3 * (size_t)j], (double)P[3 * (size_t)j + 1], (double)P[3 * (size_t)j + 2]);
                    if (d > best) best = d;
                }
            }
        }
        diameter_sq[o] = best;
    }
}

}  // namespace cp_model
