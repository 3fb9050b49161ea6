// Splitting touching instances of one object by their centre votes: the per-pixel and per-peak arithmetic of the device kernels (vote_split.hip)
// and of the stand-alone self-test (vote_split_selftest.cpp), as __host__ __device__ code.  THE RULE stands in include/casapose_hip.h
// (cp_vote_split_labels) and is not restated here; every function names the step of the rule it carries out.  All fp32 arithmetic is one
// rounding per operation, without FMA contraction (the pragmas, and -ffp-contract=off for a compiler that does not read them).  Nothing here
// calls a library beyond <math.h>.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VS_HD __host__ __device__ inline
#else
#define VS_HD inline
#endif

namespace cp_vs {

constexpr int MAX_INST = 16, MAX_SLOTS = 254;   // cp_ccl_instance_labels' limits: slot ids are bytes
constexpr int MAX_SIDE = 16384;
constexpr int MAX_CELLS = 36864;                // cells of one object's grid: 147 456 bytes of the 160 KB of LDS a workgroup may have
constexpr int BAND = 32;                        // image rows an accumulate block owns
constexpr int MAX_STRIDE = 4, MAX_NMS = 4;

VS_HD bool finite32(float v) { return fabsf(v) <= 3.4028234663852886e38f; }   // false for NaN

VS_HD int cell_shift(int cell) { return cell == 2 ? 1 : cell == 4 ? 2 : 3; }

// step 1 for one pixel: the ray from the pixel's centre along its direction, on the axis of the larger component
struct Ray {
    float a0, b0, m, s;      // start on the major and the minor axis, minor per major, the sign of the major component
    float ea, eb;            // extents of the two axes
    bool major_y;
};

// false for a direction that does not vote (a component not finite, or both zero)
VS_HD bool ray_setup(int y, int x, float dy, float dx, int h, int w, Ray& r) {
#pragma clang fp contract(off)
    if (!finite32(dy) || !finite32(dx) || (dy == 0.f && dx == 0.f)) return false;
    r.major_y = fabsf(dy) >= fabsf(dx);
    const float dmaj = r.major_y ? dy : dx, dmin = r.major_y ? dx : dy;
    r.m = dmin / dmaj;
    r.s = dmaj > 0.f ? 1.f : -1.f;
    r.a0 = (float)(r.major_y ? y : x) + 0.5f;
    r.b0 = (float)(r.major_y ? x : y) + 0.5f;
    r.ea = (float)(r.major_y ? h : w);
    r.eb = (float)(r.major_y ? w : h);
    return true;
}

// step k of a ray: false once it has left the image, else the cell (cy, cx) it votes for
VS_HD bool ray_cell(const Ray& r, int k, int cell, int shift, int& cy, int& cx) {
#pragma clang fp contract(off)
    const float t = r.s * (float)(cell * k);
    const float a = r.a0 + t;
    const float p = t * r.m;
    const float b = r.b0 + p;
    if (!(a >= 0.f && a < r.ea && b >= 0.f && b < r.eb)) return false;
    const int ca = (int)a >> shift, cb = (int)b >> shift;   // floor(a / cell): a >= 0 and cell is a power of two
    cy = r.major_y ? ca : cb;
    cx = r.major_y ? cb : ca;
    return true;
}

// step 2: the key of a cell; a larger key is an earlier rank, and no two cells of a grid share one
VS_HD unsigned long long cell_key(int votes, int index) {
    return ((unsigned long long)(unsigned)votes << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)index);
}
VS_HD int key_votes(unsigned long long key) { return (int)(key >> 32); }
VS_HD int key_index(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)); }

// step 2: is the cell a candidate -- at least min_votes votes and the largest key of its clipped window
VS_HD bool is_candidate(const int32_t* acc, int gh, int gw, int cy, int cx, int min_votes, int nms) {
    const int v = acc[cy * gw + cx];
    if (v < min_votes) return false;
    const unsigned long long key = cell_key(v, cy * gw + cx);
    const int y0 = cy - nms < 0 ? 0 : cy - nms, y1 = cy + nms > gh - 1 ? gh - 1 : cy + nms;
    const int x0 = cx - nms < 0 ? 0 : cx - nms, x1 = cx + nms > gw - 1 ? gw - 1 : cx + nms;
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx)
            if (cell_key(acc[yy * gw + xx], yy * gw + xx) > key) return false;
    return true;
}

// step 2: does a ranked candidate survive the cut against the first rank's votes
VS_HD bool passes_cut(int votes, int top_votes, int rel_percent) { return (long long)votes * 100 >= (long long)rel_percent * top_votes; }

// step 2: the peak's position, the vote-weighted centroid of the clipped 3 x 3 cells around it, in fp64, rounded once to fp32
VS_HD void peak_position(const int32_t* acc, int gh, int gw, int cy, int cx, int cell, float& py, float& px) {
#pragma clang fp contract(off)
    long long sv = 0, sy = 0, sx = 0;
    for (int yy = cy - 1; yy <= cy + 1; ++yy)
        for (int xx = cx - 1; xx <= cx + 1; ++xx) {
            if (yy < 0 || yy >= gh || xx < 0 || xx >= gw) continue;
            const long long v = acc[yy * gw + xx];
            sv += v;
            sy += v * (2 * yy + 1);
            sx += v * (2 * xx + 1);
        }
    const double half = 0.5 * (double)cell;
    py = (float)((double)sy / (double)sv * half);
    px = (float)((double)sx / (double)sv * half);
}

// step 3: the squared distance of a peak from the pixel's line of sight (or from the pixel, where the direction says nothing)
VS_HD float peak_dist2(int y, int x, float dy, float dx, float py, float px) {
#pragma clang fp contract(off)
    const float ey = py - ((float)y + 0.5f), ex = px - ((float)x + 0.5f);
    const float eyy = ey * ey, exx = ex * ex;
    const float e2 = eyy + exx;
    const float dyy = dy * dy, dxx = dx * dx;
    const float n2 = dyy + dxx;
    const float d0 = ey * dy, d1 = ex * dx;
    const float dot = d0 + d1;
    if (finite32(n2) && n2 > 0.f && dot > 0.f) {
        const float c0 = ey * dx, c1 = ex * dy;
        const float cr = c0 - c1;
        const float cc = cr * cr;
        return cc / n2;
    }
    return e2;
}

// step 3 for one pixel of an object with `npeaks` surviving peaks (y, x pairs in rank order): the rank it takes, or -1
VS_HD int assign_rank(int y, int x, float dy, float dx, const float* peaks, int npeaks, float gate) {
#pragma clang fp contract(off)
    const float g2 = gate * gate;
    int best = -1;
    float bd = 0.f;
    for (int r = 0; r < npeaks; ++r) {
        const float d2 = peak_dist2(y, x, dy, dx, peaks[2 * r], peaks[2 * r + 1]);
        if (d2 <= g2 && (best < 0 || d2 < bd)) best = r, bd = d2;
    }
    return best;
}

// ---- the serial loops of the self-test: what the kernels of vote_split.hip carry out, one image at a time -------------------------------------
// step 1: acc int32 [objects][gh][gw], zeroed here
inline void accumulate_serial(const uint8_t* labels, const float* field, int ld, int dir_at, int h, int w, int objects, int cell, int vote_stride,
                              int32_t* acc) {
    const int gh = (h + cell - 1) / cell, gw = (w + cell - 1) / cell, shift = cell_shift(cell);
    for (size_t i = 0; i < (size_t)objects * gh * gw; ++i) acc[i] = 0;
    for (int y = 0; y < h; y += vote_stride)
        for (int x = 0; x < w; x += vote_stride) {
            const int l = labels[(size_t)y * w + x];
            if (l < 1 || l > objects) continue;
            const float* d = field + ((size_t)y * w + x) * ld + dir_at;
            Ray r;
            if (!ray_setup(y, x, d[0], d[1], h, w, r)) continue;
            int cy, cx;
            for (int k = 0; ray_cell(r, k, cell, shift, cy, cx); ++k) acc[((size_t)(l - 1) * gh + cy) * gw + cx] += 1;
        }
}

// step 2 for one object's grid: inst int32 [R][4] = (0, votes, cy, cx) or (0, 0, -1, -1); peaks fp32 [R][2]; returns the surviving peaks
inline int peaks_serial(const int32_t* acc, int gh, int gw, int cell, int R, int min_votes, int rel_percent, int nms, int32_t* inst, float* peaks) {
    unsigned long long below = ~0ull;
    int np = 0, top = 0;
    for (int r = 0; r < R; ++r) {
        unsigned long long best = 0;
        for (int cy = 0; cy < gh; ++cy)
            for (int cx = 0; cx < gw; ++cx) {
                if (!is_candidate(acc, gh, gw, cy, cx, min_votes, nms)) continue;
                const unsigned long long key = cell_key(acc[cy * gw + cx], cy * gw + cx);
                if (key < below && key > best) best = key;
            }
        below = best;
        if (r == 0) top = key_votes(best);
        if (best != 0 && passes_cut(key_votes(best), top, rel_percent)) {
            const int at = key_index(best), cy = at / gw, cx = at % gw;
            inst[4 * r] = 0, inst[4 * r + 1] = key_votes(best), inst[4 * r + 2] = cy, inst[4 * r + 3] = cx;
            peak_position(acc, gh, gw, cy, cx, cell, peaks[2 * r], peaks[2 * r + 1]);
            np = r + 1;
        } else {
            inst[4 * r] = 0, inst[4 * r + 1] = 0, inst[4 * r + 2] = -1, inst[4 * r + 3] = -1;
            peaks[2 * r] = peaks[2 * r + 1] = 0.f;
            if (best == 0) below = 0;   // no later rank either
        }
    }
    return np;
}

}  // namespace cp_vs
