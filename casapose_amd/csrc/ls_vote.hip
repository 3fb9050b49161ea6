// Confidence-weighted least-squares keypoint voting (CoordLSVotingWeighted.calc,
// casapose/pose_estimation/voting_layers_2d.py:83-122) as one streaming reduction.
//
// The reference broadcasts R = w(I - n n^T) to [B,H,W,objects,kp,2,2] and reduces in fp64;
// here every pixel is read exactly once (algorithmic bytes = H*W*ld*4 per image) and only
// the five distinct sums per (image, object, keypoint) are kept:
//     S00 = sum w(1-ny^2)   S01 = sum -w ny nx   S11 = sum w(1-nx^2)
//     T0  = sum (R c)_y     T1  = sum (R c)_x          c = ((y+.5)/H, (x+.5)/H)
// Per-pixel terms are formed in fp32 exactly as the reference does (:89-105) and
// accumulated in fp64 (:113-114).
//
// Work decomposition: a wave owns a strip of 64 columns x ROWS rows; lane l walks DOWN
// column x0+l, so the 64 lanes of each step read 64 consecutive pixels (one contiguous
// 64*ld*4-byte span, staged through LDS with 16-byte accesses) while each lane's object
// label stays constant for long runs.  A lane accumulates privately in fp64 registers and
// only flushes (LDS fp64 atomics) when its label changes or the strip ends; the block then
// adds its LDS table to the global fp64 sums with one atomic per entry.
#include "common.h"
#include "ls_cov_math.h"
#include "ls_robust_math.h"
#include <cmath>
#include <cstdlib>

namespace {

constexpr int ROWS = 16;        // rows per strip
constexpr int MAXKP = 9;        // compile-time bound for the private accumulators
constexpr int WAVES = 4;
// the production record [9 logits | 18 directions | 9 confidences]: 36 floats = nine 16-byte vectors, directions at 9, confidences at 27
constexpr int REC_LD = 36, REC_NV = REC_LD / 4, REC_DIR = 9, REC_CONF = 27;

// softplus = max(x,0) + log1p(exp(-|x|)) on the hardware exp2 / log2 units: with t = exp(-|x|) in (0,1] and u = fl(1 + t),
// log1p(t) = log(u) + (t - (u - 1)) / u restores the bits the addition drops (error ~1e-7 of the result)
__device__ __forceinline__ float softplus_fast(float x) {
    const float t = __expf(-fabsf(x));
    const float u = 1.0f + t;
    return fmaxf(x, 0.f) + (__logf(u) + (t - (u - 1.0f)) * __frcp_rn(u));
}

// ---- what the two forward kernels share ----

// the strip of this wave: strip id -> (image, strip row, strip column); all 4 waves of a block work on ONE image.  A kernel branches on find()
// and calls decode() inside the branch, so a wave without a strip does none of the divisions
struct LsStrip {
    int img, sidx;          // every wave: the block's image (its commit needs it) and the wave's strip id
    int x0, y0, x, ncols;   // a wave with a strip, after decode(): the strip's corner, the lane's column, the columns inside the image

    // tells whether the wave has a strip
    __device__ __forceinline__ bool find(int wave, int strips_x, int strips_y) {
        const int strips_per_img = strips_x * strips_y;
        const int blocks_per_img = (strips_per_img + WAVES - 1) / WAVES;
        img = blockIdx.x / blocks_per_img;
        sidx = (blockIdx.x % blocks_per_img) * WAVES + wave;
        return sidx < strips_per_img;
    }
    __device__ __forceinline__ void decode(int lane, int strips_x, int W) {
        const int sy = sidx / strips_x, sx = sidx % strips_x;
        x0 = sx * 64, y0 = sy * ROWS;
        x = x0 + lane;
        ncols = min(64, W - x0);
    }
    // the lane's column centre; divide like the reference: (v + 0.5) / H in fp32
    __device__ __forceinline__ float cx(int H) const { return ((float)x + 0.5f) / (float)H; }
};

// a lane's private sums of the run of equal labels it is in
template <int KP>
struct LsAcc {
    double a[KP][5] = {};
    int cur = 0;
    double* const table;
    __device__ __forceinline__ explicit LsAcc(double* acc_lds) : table(acc_lds) {}
    __device__ __forceinline__ void flush() {
        if (cur > 0) {
            double* dst = table + (size_t)(cur - 1) * KP * 5;
#pragma unroll
            for (int j = 0; j < KP; ++j)
#pragma unroll
                for (int c = 0; c < 5; ++c) {
                    atomicAdd(dst + j * 5 + c, a[j][c]);
                    a[j][c] = 0.0;
                }
        }
    }
    __device__ __forceinline__ void enter(int lab) {
        if (lab != cur) {
            flush();
            cur = lab;
        }
    }
};

// the block's LDS table [objects][KP][5]
__device__ __forceinline__ void ls_table_zero(double* acc_lds, int nacc) {
    for (int i = threadIdx.x; i < nacc; i += blockDim.x) acc_lds[i] = 0.0;
    __syncthreads();
}

__device__ __forceinline__ void ls_table_commit(const double* acc_lds, int nacc, double* __restrict__ gdst) {
    __syncthreads();
    for (int i = threadIdx.x; i < nacc; i += blockDim.x) {
        double v = acc_lds[i];
        if (v != 0.0) atomicAdd(gdst + i, v);
    }
}

// the five terms of one keypoint of one pixel: R = w (I - n n^T) and R c
__device__ __forceinline__ void ls_add_terms(double (&a)[5], float ny, float nx, float w, float cy, float cx) {
    const float r00 = (1.0f - ny * ny) * w;
    const float r01 = (0.0f - ny * nx) * w;
    const float r11 = (1.0f - nx * nx) * w;
    const float q0 = r00 * cy + r01 * cx;  // (:103-105)
    const float q1 = r01 * cy + r11 * cx;
    a[0] += (double)r00;
    a[1] += (double)r01;
    a[2] += (double)r11;
    a[3] += (double)q0;
    a[4] += (double)q1;
}

// A reweighted pass of the robust voter (cp_ls_vote_slots_robust_f32; ls_robust_math.h has the weight and why it is what it is) walks the pixels
// as the plain pass does and hands ls_add_terms w * rho in place of w.  The moments pass of cp_ls_slot_covariance_f32 (ls_cov_math.h) makes the
// same walk against estimates handed in and sums (A00, A01, A11, Q, Wall) in place of (S00, S01, S11, T0, T1).  The mode is a template parameter
// of the two kernels that walk a slot map: the plain instantiation carries none of what follows, the reweighted one none of the moments' work.
enum LsMode { LS_PLAIN = 0, LS_REWEIGHTED = 1, LS_MOMENTS = 2 };
//
// The estimates of the keypoints of a lane's current slot, in the voter's normalised coordinates (pixels / H): 18 registers, reloaded from the
// keypoints of the pass before when the lane's label changes -- as rarely as its accumulators are flushed.  A table of estimates in LDS would
// not fit beside 254 slots' sums and the staging buffer of ld = 64.
template <int MODE, int KP>
struct LsEst {
    static constexpr bool USED = MODE != LS_PLAIN;
    float p[USED ? KP : 1][2];
    // est_img: fp32 [slots][KP][2] in (y, x) pixels, the image's rows of the keypoints buffer
    __device__ __forceinline__ void load(const float* __restrict__ est_img, int lab, int H) {
        const float2* e = reinterpret_cast<const float2*>(est_img + (size_t)(lab - 1) * KP * 2);
#pragma unroll
        for (int j = 0; j < (USED ? KP : 0); ++j) {
            const float2 v = e[j];
            p[j][0] = v.x / (float)H;
            p[j][1] = v.y / (float)H;
        }
    }
};

// one keypoint of one labelled pixel: plain, reweighted, or the moments (rscale = 0 there: no cut-off)
template <int MODE>
__device__ __forceinline__ void ls_add_pixel(double (&a)[5], float2 n, float w, float cy, float cx, const float (&p)[2], float rscale) {
    if (MODE == LS_MOMENTS) {
        const cp_lsc::Moment m = cp_lsc::moment(p[0], p[1], cy, cx, n.x, n.y, w, rscale);
        a[0] += (double)((1.0f - n.x * n.x) * m.omega);   // as ls_add_terms forms them, omega in place of w
        a[1] += (double)((0.0f - n.x * n.y) * m.omega);
        a[2] += (double)((1.0f - n.y * n.y) * m.omega);
        a[3] += (double)m.q;
        a[4] += (double)m.wall;
        return;
    }
    if (MODE == LS_REWEIGHTED) w *= cp_lsr::rho(p[0], p[1], cy, cx, n.x, n.y, rscale);
    ls_add_terms(a, n.x, n.y, w, cy, cx);
}

// The two arithmetic choices.  Exact (generic kernel): libm weights and d / sqrt(d.d).  Fast (36-float kernel): softplus_fast and
// d * rsqrt(d.d), one reciprocal square root for both components -- the libm calls cost as much as the whole memory stream.
__device__ __forceinline__ float ls_weight_exact(float cf, int sigmoid) {
    return sigmoid ? 1.0f / (1.0f + expf(-cf))                    // sigmoid_weights=True (:32-33, sigmoid_scale = 1)
                   : fmaxf(cf, 0.f) + log1pf(expf(-fabsf(cf)));   // softplus (:35)
}

__device__ __forceinline__ float2 ls_normal_exact(float dy, float dx) {
    const float nrm = sqrtf(dy * dy + dx * dx);
    return make_float2((nrm > 0.f) ? dy / nrm : 0.f, (nrm > 0.f) ? dx / nrm : 0.f);  // divide_no_nan (:90)
}

__device__ __forceinline__ float2 ls_normal_fast(float dy, float dx) {
    const float n2 = dy * dy + dx * dx;
    const float inv = (n2 > 0.f) ? __frsqrt_rn(n2) : 0.f;  // divide_no_nan (:90)
    return make_float2(dy * inv, dx * inv);
}

// MODE other than LS_PLAIN (given labels only): est is the keypoints buffer of the pass before (the moments: the keypoints handed in), fp32
// [B][objects][KP][2], rscale = H / cutoff
template <int KP, int MODE = LS_PLAIN>
__global__ __launch_bounds__(256) void ls_accumulate_kernel(const float* __restrict__ field, int ld, int seg_off,
                                                            int dir_off, int conf_off, const uint8_t* __restrict__ labels,
                                                            int B, int H, int W, int objects, double* __restrict__ sums,
                                                            int strips_x, int strips_y, int sigmoid, const float* __restrict__ est,
                                                            float rscale) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* acc_lds = reinterpret_cast<double*>(smem_raw);                         // [objects][KP][5]
    float* stage = reinterpret_cast<float*>(smem_raw + sizeof(double) * objects * KP * 5);  // [WAVES][64*ld]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nacc = objects * KP * 5;
    ls_table_zero(acc_lds, nacc);

    float* wstage = stage + (size_t)wave * 64 * ld;
    LsStrip s;
    if (s.find(wave, strips_x, strips_y)) {
        s.decode(lane, strips_x, W);
        const int img = s.img, x0 = s.x0, y0 = s.y0, x = s.x, ncols = s.ncols;
        const float cx = s.cx(H);
        const int classes = objects + 1;
        LsAcc<KP> acc(acc_lds);
        LsEst<MODE, KP> pe;

        const int y_end = min(y0 + ROWS, H);
        // with given labels a row segment without a non-zero label contributes nothing: its records are not read.  The strip's labels are
        // fetched up front (independent loads, one round trip) so that no row waits for its own label before its records are requested.
        unsigned rowmask = 0xffffu;
        if (labels) {
            rowmask = 0;
#pragma unroll
            for (int ry = 0; ry < ROWS; ++ry) {
                const int l = (y0 + ry < y_end && lane < ncols) ? (int)labels[((size_t)img * H + y0 + ry) * W + x] : 0;
                rowmask |= (__builtin_amdgcn_ballot_w64(l != 0) != 0ull ? 1u : 0u) << ry;
            }
        }
        for (int y = y0; y < y_end; ++y) {
            const bool rd = (rowmask >> (y - y0)) & 1u;  // wave-uniform; a row that is not read has label 0 in every lane, as before
            // ---- stage this row segment: ncols*ld contiguous floats, 16 B per lane per step ----
            const float* g = field + (((size_t)img * H + y) * W + x0) * ld;
            const int nvec = rd ? (ncols * ld) >> 2 : 0;  // ld % 4 == 0
            for (int v = lane; v < nvec; v += 64)
                reinterpret_cast<float4*>(wstage)[v] = reinterpret_cast<const float4*>(g)[v];
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): LDS writes landed before the reads below
            int lab = 0;
            const float* px = wstage + lane * ld;
            if (rd && lane < ncols) {
                if (labels) {
                    lab = labels[((size_t)img * H + y) * W + x];
                    if (MODE != LS_PLAIN && lab > objects) lab = 0;   // no row of estimates to read
                } else {
                    float best = px[seg_off];
                    for (int k = 1; k < classes; ++k) {
                        float v = px[seg_off + k];
                        if (v > best) { best = v; lab = k; }
                    }
                }
            }
            const bool moved = lab != acc.cur;
            acc.enter(lab);
            if (lab > 0) {
                if (MODE != LS_PLAIN && moved) pe.load(est + (size_t)img * objects * KP * 2, lab, H);
                const float cy = ((float)y + 0.5f) / (float)H;
#pragma unroll
                for (int j = 0; j < KP; ++j) {
                    const float dy = px[dir_off + 2 * j], dx = px[dir_off + 2 * j + 1];
                    const float w = ls_weight_exact(px[conf_off + j], sigmoid);
                    const float2 n = ls_normal_exact(dy, dx);
                    ls_add_pixel<MODE>(acc.a[j], n, w, cy, cx, pe.p[MODE != LS_PLAIN ? j : 0], rscale);
                }
            }
            __builtin_amdgcn_wave_barrier();  // all lanes done reading before the next row overwrites
        }
        acc.flush();
    }
    ls_table_commit(acc_lds, nacc, sums + (size_t)s.img * nacc);
}

// ---- the strip walk of the kernels for the production record (ld = 36, 9 keypoints): same strip decomposition and arithmetic as above ----
//
// With given labels the wave first reads the labels of its whole 64 x 16 strip (1 KB: four 4-byte loads per lane) and forms by ballot the
// 16-bit mask of the row segments that hold a non-zero label.  Only those rows are requested, staged and processed; a label-0 pixel never
// contributed, so the sums are the same sums.  The component-filtered label map of CoordLSVotingWeighted(filter_estimates=True) keeps a small
// share of the image.
struct LsStripLabels {
    // lw[k] of lane l holds the four labels of row 4k + (l >> 4), columns 4 (l & 15) .. + 3 (a label outside the image reads as 0)
    unsigned lw[4] = {0u, 0u, 0u, 0u};

    // reads the strip's labels (s decoded, nrows of its rows inside the image); returns the row mask
    __device__ __forceinline__ unsigned load(const uint8_t* __restrict__ labels, const LsStrip& s, int lane, int nrows, int H, int W) {
        const uint8_t* lb = labels + ((size_t)s.img * H + s.y0) * W + s.x0;
        const int lr = lane >> 4, lc = (lane & 15) * 4;
        const bool words = ((W & 3) == 0) && (((uintptr_t)labels & 3) == 0);  // every row segment starts on a 4-byte boundary
        const bool inside = lc < s.ncols;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int ry = 4 * k + lr;
            if (ry < nrows) {
                const uint8_t* p = lb + (size_t)ry * W + lc;
                if (words) {
                    if (inside) lw[k] = *reinterpret_cast<const unsigned*>(p);  // ncols % 4 == 0 here: the word is inside the row
                } else {
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (lc + c < s.ncols) lw[k] |= (unsigned)p[c] << (8 * c);
                }
            }
        }
        unsigned rowmask = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(lw[k] != 0u);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if ((bal >> (16 * j)) & 0xffffull) rowmask |= 1u << (4 * k + j);
        }
        return rowmask;
    }
    // this lane's label in row ry: byte (lane & 3) of the word that lane 16 (ry & 3) + (lane >> 2) holds in lw[ry >> 2]
    __device__ __forceinline__ int at(int ry, int lane) const {
        const int k = ry >> 2;
        const unsigned wsel = (k == 0) ? lw[0] : (k == 1) ? lw[1] : (k == 2) ? lw[2] : lw[3];
        const unsigned wv = (unsigned)__shfl((int)wsel, ((ry & 3) << 4) + (lane >> 2));
        return (int)((wv >> (8 * (lane & 3))) & 0xffu);
    }
};

// Walks the rows of the strip at (x0, y0) whose bit is set in the wave-uniform rowmask and calls body(ry, gap, r) for each: r is the lane's
// record, gap tells that rows were skipped since the row before (every lane's label was 0 there, which ends its run of equal labels).
//   * The next row segment (64 pixels = 9216 contiguous bytes = nine 16-byte loads per lane, nvec of them inside the image) is fetched into
//     registers while the current one is processed -- the generic kernel waits for every row's memory latency (measured 3.1 TB/s with the
//     arithmetic removed).
//   * A lane reads its pixel back from the wave's staging buffer as nine 16-byte LDS reads (144-byte pixel stride: conflict-free) with
//     compile-time channel positions, instead of 27 scalar reads with 4-way bank conflicts.
template <class Body>
__device__ __forceinline__ void ls_walk36(const float* __restrict__ field, int img, int H, int W, int x0, int y0, int nvec, int lane, float4* wstage,
                                          unsigned rowmask, Body body) {
    float4 pre[REC_NV];
    auto issue = [&](int ry) {
        const float4* g = reinterpret_cast<const float4*>(field + (((size_t)img * H + y0 + ry) * W + x0) * REC_LD);
#pragma unroll
        for (int i = 0; i < REC_NV; ++i) {
            const int v = lane + 64 * i;
            pre[i] = (v < nvec) ? g[v] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    unsigned todo = rowmask;
    int ry = -1, prev = -1;
    if (todo) {
        ry = __builtin_ctz(todo);
        todo &= todo - 1;
        issue(ry);
    }
    while (ry >= 0) {
#pragma unroll
        for (int i = 0; i < REC_NV; ++i) wstage[lane + 64 * i] = pre[i];
        int nxt = -1;
        if (todo) {
            nxt = __builtin_ctz(todo);
            todo &= todo - 1;
            issue(nxt);  // in flight while this row is processed
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's LDS writes have landed (the prefetch stays in flight)
        float r[REC_LD];
#pragma unroll
        for (int i = 0; i < REC_NV; ++i) {
            const float4 q = wstage[lane * REC_NV + i];
            r[4 * i] = q.x; r[4 * i + 1] = q.y; r[4 * i + 2] = q.z; r[4 * i + 3] = q.w;
        }
        body(ry, ry != prev + 1, r);
        __builtin_amdgcn_wave_barrier();  // all lanes done reading before the next row overwrites
        prev = ry;
        ry = nxt;
    }
}

// The production record with 8 objects: labels given (LAB) or the arg-max of the nine logits, every row walked then.
template <bool LAB>
__global__ __launch_bounds__(256) void ls_accumulate36_kernel(const float* __restrict__ field, const uint8_t* __restrict__ labels, int B, int H,
                                                              int W, double* __restrict__ sums, int strips_x, int strips_y) {
    constexpr int KP = 9, OBJ = 8;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* acc_lds = reinterpret_cast<double*>(smem_raw);                                // [OBJ][KP][5]
    float4* stage = reinterpret_cast<float4*>(smem_raw + sizeof(double) * OBJ * KP * 5);   // [WAVES][64*REC_NV]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    constexpr int nacc = OBJ * KP * 5;
    ls_table_zero(acc_lds, nacc);

    float4* wstage = stage + (size_t)wave * 64 * REC_NV;
    LsStrip s;
    if (s.find(wave, strips_x, strips_y)) {
        s.decode(lane, strips_x, W);
        const int ncols = s.ncols, y0 = s.y0;
        const int nrows = min(ROWS, H - y0);
        const float cx = s.cx(H);
        LsStripLabels lbl;
        const unsigned rowmask = LAB ? lbl.load(labels, s, lane, nrows, H, W) : (1u << nrows) - 1u;

        LsAcc<KP> acc(acc_lds);
        ls_walk36(field, s.img, H, W, s.x0, y0, ncols * REC_NV, lane, wstage, rowmask, [&](int ry, bool gap, const float (&r)[REC_LD]) {
            int lab = 0;
            if (LAB) {
                lab = lbl.at(ry, lane);
                if (gap) acc.enter(0);
            } else {
                float best = r[0];
#pragma unroll
                for (int k = 1; k <= OBJ; ++k)
                    if (r[k] > best) { best = r[k]; lab = k; }
                if (lane >= ncols) lab = 0;
            }
            acc.enter(lab);
            if (lab > 0) {
                const float cy = ((float)(y0 + ry) + 0.5f) / (float)H;
#pragma unroll
                for (int j = 0; j < KP; ++j) {
                    const float w = softplus_fast(r[REC_CONF + j]);  // softplus (:35)
                    const float2 n = ls_normal_fast(r[REC_DIR + 2 * j], r[REC_DIR + 2 * j + 1]);
                    ls_add_terms(acc.a[j], n.x, n.y, w, cy, cx);
                }
            }
        });
        acc.flush();
    }
    ls_table_commit(acc_lds, nacc, sums + (size_t)s.img * nacc);
}

// ls_accumulate36_kernel<true> keyed by slot: a run-time number of table rows, the LDS table [slots][9][5] in front of the staging buffer, the
// logits not read.  A table of 254 slots is 91 KB, so what a block pays per table entry is kept away from the blocks that have nothing to add:
// the labels are read BEFORE the table is zeroed, and a block whose four strips hold no label ends there (no zeroing, no commit scan).
// LS_REWEIGHTED: a reweighted pass; est is the keypoints buffer of the pass before, fp32 [B][slots][9][2], rscale = H / cutoff.
// LS_MOMENTS: the covariance's pass against the keypoints handed in; rscale = 0 without a cut-off.
template <int MODE>
__global__ __launch_bounds__(256) void ls_accumulate36_slots_kernel(const float* __restrict__ field, const uint8_t* __restrict__ labels, int B, int H,
                                                                    int W, int slots, double* __restrict__ sums, int strips_x, int strips_y,
                                                                    const float* __restrict__ est, float rscale) {
    constexpr int KP = 9;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int nacc = slots * KP * 5;
    double* acc_lds = reinterpret_cast<double*>(smem_raw);                                            // [slots][KP][5]
    float4* stage = reinterpret_cast<float4*>(smem_raw + (sizeof(double) * nacc + 15) / 16 * 16);       // [WAVES][64*REC_NV]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float4* wstage = stage + (size_t)wave * 64 * REC_NV;
    LsStrip s;
    const bool has = s.find(wave, strips_x, strips_y);
    int nvec = 0;
    float cx = 0.f;
    LsStripLabels lbl;
    unsigned rowmask = 0;
    if (has) {
        s.decode(lane, strips_x, W);
        nvec = s.ncols * REC_NV;
        cx = s.cx(H);
        rowmask = lbl.load(labels, s, lane, min(ROWS, H - s.y0), H, W);
    }
    if (!__syncthreads_or(rowmask != 0u)) return;   // block-uniform: nothing labelled in any of its strips
    ls_table_zero(acc_lds, nacc);

    if (rowmask) {   // wave-uniform
        const int img = s.img, y0 = s.y0;
        LsAcc<KP> acc(acc_lds);
        LsEst<MODE, KP> pe;
        ls_walk36(field, img, H, W, s.x0, y0, nvec, lane, wstage, rowmask, [&](int ry, bool gap, const float (&r)[REC_LD]) {
            if (gap) acc.enter(0);
            const int l = lbl.at(ry, lane);
            const int lab = l > slots ? 0 : l;   // a value above `slots` has no table row and is background
            const bool moved = lab != acc.cur;
            acc.enter(lab);
            if (lab > 0) {
                if (MODE != LS_PLAIN && moved) pe.load(est + (size_t)img * slots * KP * 2, lab, H);
                const float cy = ((float)(y0 + ry) + 0.5f) / (float)H;
#pragma unroll
                for (int j = 0; j < KP; ++j) {
                    const float w = softplus_fast(r[REC_CONF + j]);  // softplus (:35)
                    const float2 n = ls_normal_fast(r[REC_DIR + 2 * j], r[REC_DIR + 2 * j + 1]);
                    ls_add_pixel<MODE>(acc.a[j], n, w, cy, cx, pe.p[MODE != LS_PLAIN ? j : 0], rscale);
                }
            }
        });
        acc.flush();
    }
    ls_table_commit(acc_lds, nacc, sums + (size_t)s.img * nacc);
}

// x = [[a,b],[b,c]]^-1 t for a regular symmetric system, det = a c - b^2 (each kernel keeps its own rank test)
__device__ __forceinline__ void solve_sym2x2(double a, double b, double c, double det, double t0, double t1, double& x0, double& x1) {
    x0 = (c * t0 - b * t1) / det;
    x1 = (a * t1 - b * t0) / det;
}

// p = pinv([[S00,S01],[S01,S11]]) [T0,T1]^T * H   (voting_layers_2d.py:116-122);
// tf.linalg.pinv default rcond = 10 * max(m,n) * eps(fp64).
__global__ void ls_solve_kernel(const double* __restrict__ sums, int total, int H, float* __restrict__ out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const double* s = sums + (size_t)i * 5;
    double a = s[0], b = s[1], c = s[2], t0 = s[3], t1 = s[4];
    double half_tr = 0.5 * (a + c), half_df = 0.5 * (a - c);
    double rad = sqrt(half_df * half_df + b * b);
    double l1 = half_tr + rad, l2 = half_tr - rad;  // l1 >= l2 (PSD up to rounding)
    const double rcond = 10.0 * 2.0 * 2.220446049250313e-16;
    double p0 = 0.0, p1 = 0.0;
    double smax = fmax(fabs(l1), fabs(l2));
    if (smax > 0.0) {
        if (fabs(l2) > rcond * smax && fabs(l1) > rcond * smax) {
            solve_sym2x2(a, b, c, a * c - b * b, t0, t1, p0, p1);
        } else {
            // rank one: keep only the dominant eigen-pair
            double lam = (fabs(l1) >= fabs(l2)) ? l1 : l2;
            double vx = b, vy = lam - a;          // (A - a I) v: eigenvector candidates
            double wx = lam - c, wy = b;
            if (wx * wx + wy * wy > vx * vx + vy * vy) { vx = wx; vy = wy; }
            double n2 = vx * vx + vy * vy;
            if (n2 > 0.0) {
                double proj = (vx * t0 + vy * t1) / (n2 * lam);
                p0 = vx * proj;
                p1 = vy * proj;
            }
        }
    }
    out[2 * i] = (float)p0 * (float)H;
    out[2 * i + 1] = (float)p1 * (float)H;
}

// ---------------------------------------------------------------------------------------------
// backward of the voter (the reference differentiates CoordLSVotingWeighted with tf.GradientTape,
// train_casapose.py:555-579,594): with A = sum R, b = sum R c, p = A^-1 b and g = dL/dp,
//   u = A^-1 g,  dL/dR_i = u (c_i - p)^T  for every pixel i of the object, R_i = w_i (I - n_i n_i^T):
//   dL/dw_i = u.e - (u.n)(n.e)                 e = c_i - p
//   dL/dn_i = -w_i (u (e.n) + e (u.n))
//   dL/dd_i = (dL/dn - n (n.dL/dn)) / |d|      n = d/|d|
//   dL/dconf_i = dL/dw_i * sigmoid(conf_i)      w = softplus(conf)
// No reduction: one pass over the pixels given the per-keypoint pair (p, u).
__global__ void ls_bwd_prepare_kernel(const double* __restrict__ sums, const float* __restrict__ dkp, int total, int H, float* __restrict__ pu) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const double* s = sums + (size_t)i * 5;
    const double a = s[0], b = s[1], c = s[2], t0 = s[3], t1 = s[4];
    const double g0 = (double)dkp[2 * i] * H, g1 = (double)dkp[2 * i + 1] * H;  // keypoints = p * H
    const double det = a * c - b * b;
    const double tr = a + c;
    double p0 = 0, p1 = 0, u0 = 0, u1 = 0;
    if (tr > 0.0 && fabs(det) > 1e-12 * tr * tr) {  // regular system; a degenerate one passes no gradient
        solve_sym2x2(a, b, c, det, t0, t1, p0, p1);
        solve_sym2x2(a, b, c, det, g0, g1, u0, u1);
    }
    pu[4 * i] = (float)p0; pu[4 * i + 1] = (float)p1; pu[4 * i + 2] = (float)u0; pu[4 * i + 3] = (float)u1;
}

// One keypoint of one pixel: the gradient of its direction pair and confidence.  The kernels differ only in how values move, so they hand
// in readers: dir() -> (dy, dx) and entry() -> the keypoint's (p0, p1, u0, u1) are read for a labelled pixel only, coef() -> the
// regulariser's coefficient only where it applies (reg).
struct LsGrad { float dy, dx, cf; };
template <class Dir, class Entry, class Coef>
__device__ __forceinline__ LsGrad ls_bwd_keypoint(float cf, int lab, bool reg, float cy, float cx, Dir dir, Entry entry, Coef coef) {
    const float sg = 1.f / (1.f + __expf(-cf));
    float gdy = 0.f, gdx = 0.f, gcf = 0.f;
    if (lab > 0) {
        const float2 d = dir();
        const float dy = d.x, dx = d.y;
        const float w = softplus_fast(cf);
        const float nrm = sqrtf(dy * dy + dx * dx);
        const float4 pu = entry();
        const float p0 = pu.x, p1 = pu.y, u0 = pu.z, u1 = pu.w;
        const float e0 = cy - p0, e1 = cx - p1;
        if (nrm > 0.f) {
            const float inr = 1.f / nrm;
            const float ny = dy * inr, nx = dx * inr;
            const float un = u0 * ny + u1 * nx, en = e0 * ny + e1 * nx, ue = u0 * e0 + u1 * e1;
            gcf = (ue - un * en) * sg;
            const float ln0 = -w * (u0 * en + e0 * un), ln1 = -w * (u1 * en + e1 * un);
            const float nl = ny * ln0 + nx * ln1;
            gdy = (ln0 - ny * nl) * inr;
            gdx = (ln1 - nx * nl) * inr;
        } else {
            gcf = (u0 * e0 + u1 * e1) * sg;  // n = 0: R = w I
        }
    }
    if (reg) gcf += coef() * sg;
    return {gdy, gdx, gcf};
}

template <int KP>
__global__ void ls_bwd_kernel(const float* __restrict__ field, int ld, int dir_off, int conf_off, const uint8_t* __restrict__ labels, int B, int H,
                              int W, int objects, const float* __restrict__ pu, const uint8_t* __restrict__ reg_labels,
                              const float* __restrict__ conf_coef, float* __restrict__ dfield, int dld, int ddir_off, int dconf_off,
                              int accumulate) {
    const long long total = (long long)B * H * W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int lab = labels[i];
        const int rlab = reg_labels ? reg_labels[i] : 0;
        float* g = dfield + i * dld;
        if (lab == 0 && rlab == 0) {
            if (!accumulate) {
                for (int j = 0; j < 2 * KP; ++j) g[ddir_off + j] = 0.f;
                for (int j = 0; j < KP; ++j) g[dconf_off + j] = 0.f;
            }
            continue;
        }
        const int x = (int)(i % W);
        const long long t = i / W;
        const int y = (int)(t % H), b = (int)(t / H);
        const float cy = ((float)y + 0.5f) / (float)H, cx = ((float)x + 0.5f) / (float)H;
        const float* px = field + i * ld;
        const float* tab = pu + ((size_t)b * objects + (lab > 0 ? lab - 1 : 0)) * KP * 4;
        const bool reg = rlab > 0 && conf_coef;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const LsGrad d = ls_bwd_keypoint(px[conf_off + j], lab, reg, cy, cx,
                                             [&] { return make_float2(px[dir_off + 2 * j], px[dir_off + 2 * j + 1]); },
                                             [&] { return make_float4(tab[4 * j], tab[4 * j + 1], tab[4 * j + 2], tab[4 * j + 3]); },
                                             [&] { return conf_coef[b * KP + j]; });
            if (accumulate) {
                g[ddir_off + 2 * j] += d.dy;
                g[ddir_off + 2 * j + 1] += d.dx;
                g[dconf_off + j] += d.cf;
            } else {
                g[ddir_off + 2 * j] = d.dy;
                g[ddir_off + 2 * j + 1] = d.dx;
                g[dconf_off + j] = d.cf;
            }
        }
    }
}

// The production record of ls_bwd_kernel (ld = 36: [9 logits | 18 directions | 9 confidences], gradient rows whose 27 values start on a 16-byte
// boundary with one writable float of padding behind them): a pixel's record and gradient row move as nine / seven 16-byte accesses with
// compile-time channel positions.  The generic kernel's 4-byte accesses at a 144 / 256-byte lane stride took 0.98 ms per training step for a
// quarter of the pixels (the foreground); same arithmetic, same results.
__global__ void ls_bwd36_kernel(const float* __restrict__ field, const uint8_t* __restrict__ labels, int B, int H, int W, int objects,
                                const float* __restrict__ pu, const uint8_t* __restrict__ reg_labels, const float* __restrict__ conf_coef,
                                float* __restrict__ dfield, int dld, int ddir_off, int accumulate) {
    constexpr int KP = 9;
    const long long total = (long long)B * H * W;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int lab = labels[i];
        const int rlab = reg_labels ? reg_labels[i] : 0;
        float4* g4 = reinterpret_cast<float4*>(dfield + i * dld + ddir_off);
        if (lab == 0 && rlab == 0) {
            if (!accumulate) {
#pragma unroll
                for (int q = 0; q < 7; ++q) g4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
            continue;
        }
        const int x = (int)(i % W);
        const long long t = i / W;
        const int y = (int)(t % H), b = (int)(t / H);
        const float cy = ((float)y + 0.5f) / (float)H, cx = ((float)x + 0.5f) / (float)H;
        float rec[REC_LD];
        const float4* r4 = reinterpret_cast<const float4*>(field + i * REC_LD);
#pragma unroll
        for (int q = 0; q < REC_NV; ++q) {
            const float4 v = r4[q];
            rec[4 * q] = v.x; rec[4 * q + 1] = v.y; rec[4 * q + 2] = v.z; rec[4 * q + 3] = v.w;
        }
        float out[28];
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const float4 v = accumulate ? g4[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            out[4 * q] = v.x; out[4 * q + 1] = v.y; out[4 * q + 2] = v.z; out[4 * q + 3] = v.w;
        }
        const float* tab = pu + ((size_t)b * objects + (lab > 0 ? lab - 1 : 0)) * KP * 4;
        const bool reg = rlab > 0 && conf_coef;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const LsGrad d = ls_bwd_keypoint(rec[REC_CONF + j], lab, reg, cy, cx,
                                             [&] { return make_float2(rec[REC_DIR + 2 * j], rec[REC_DIR + 2 * j + 1]); },
                                             [&] { return *reinterpret_cast<const float4*>(tab + 4 * j); },
                                             [&] { return conf_coef[b * KP + j]; });
            out[2 * j] += d.dy;
            out[2 * j + 1] += d.dx;
            out[18 + j] += d.cf;
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) g4[q] = make_float4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
    }
}

// per image: counts of every class in two label maps and, over the foreground of `labels`, the sums of softplus(conf_j)
// (objects_available and the confidence regulariser of keypoint_reprojection_loss, loss_functions.py:236-262)
template <int KP>
__global__ __launch_bounds__(256) void kp_stats_kernel(const float* __restrict__ field, int ld, int conf_off, const uint8_t* __restrict__ labels,
                                                       const uint8_t* __restrict__ labels_est, int pix_per_img, int classes,
                                                       int* __restrict__ counts, double* __restrict__ conf_sums) {
    extern __shared__ int scount[];  // [2][classes]
    __shared__ double ssum[KP];
    const int b = blockIdx.y;
    for (int i = threadIdx.x; i < 2 * classes; i += blockDim.x) scount[i] = 0;
    if (threadIdx.x < KP) ssum[threadIdx.x] = 0.0;
    __syncthreads();
    double cs[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) cs[j] = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < pix_per_img; i += gridDim.x * blockDim.x) {
        const size_t p = (size_t)b * pix_per_img + i;
        const int l = labels[p];
        atomicAdd(&scount[l < classes ? l : 0], 1);
        if (labels_est) {
            const int le = labels_est[p];
            atomicAdd(&scount[classes + (le < classes ? le : 0)], 1);
        }
        if (l > 0) {
            const float* px = field + p * ld + conf_off;
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                const float cf = px[j];
                cs[j] += (double)softplus_fast(cf);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        double v = cs[j];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if ((threadIdx.x & 63) == 0 && v != 0.0) atomicAdd(&ssum[j], v);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * classes; i += blockDim.x)
        if (scount[i]) atomicAdd(&counts[((size_t)(i / classes) * gridDim.y + b) * classes + (i % classes)], scount[i]);
    if (threadIdx.x < KP && ssum[threadIdx.x] != 0.0) atomicAdd(&conf_sums[b * KP + threadIdx.x], ssum[threadIdx.x]);
}

// keypoint_reprojection_loss without BPnP (loss_functions.py:207-344): crop pixels -> original image through the per-image
// affine (transform_points_back_tf_batch, ransac_voting.py:124-158), distance to the projected ground-truth keypoints,
// smooth L1, soft cap at max_err, mean over keypoints, sum over available objects / their number.  One block.
__global__ void kp_reproj_loss_kernel(const float* __restrict__ coords_yx, const float* __restrict__ gt_xy, const float* __restrict__ affine,
                                      const float* __restrict__ avail, int batch, int objects, int kp, float max_err, float weight,
                                      float* __restrict__ g_yx, double* __restrict__ loss_out) {
    __shared__ double red[256];
    __shared__ double navail;
    const int N = batch * objects;
    if (threadIdx.x == 0) {
        double s = 0;
        for (int n = 0; n < N; ++n) s += avail[n];
        navail = s;
    }
    __syncthreads();
    const double na = navail;
    double local = 0.0;
    for (int i = threadIdx.x; i < N * kp; i += blockDim.x) {
        const int n = i / kp;
        const int b = n / objects;
        const float av = avail[n];
        const float* A = affine + b * 6;
        const float y = coords_yx[2 * i], x = coords_yx[2 * i + 1];
        const float X = A[0] * x + A[1] * y + A[2], Y = A[3] * x + A[4] * y + A[5];
        const float dx = (gt_xy[2 * i] - X) * av, dy = (gt_xy[2 * i + 1] - Y) * av;
        const float e = sqrtf(dx * dx + dy * dy);
        float l = e < 1.f ? 0.5f * e * e : e - 0.5f;
        float slope = e < 1.f ? e : 1.f;
        if (l > max_err) { l = max_err + (l - max_err) * 0.01f; slope *= 0.01f; }
        local += (double)(l * av);
        float gx = 0.f, gy = 0.f;
        if (e > 0.f && na > 0.0) {
            const float c = weight * slope * av * av / (e * (float)kp * (float)na);  // d loss / d (X,Y) = -c*(dx,dy)
            const float gX = -c * dx, gY = -c * dy;
            gx = gX * A[0] + gY * A[3];
            gy = gX * A[1] + gY * A[4];
        }
        g_yx[2 * i] = gy;
        g_yx[2 * i + 1] = gx;
    }
    red[threadIdx.x] = local;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss_out = na > 0.0 ? red[0] / ((double)kp * na) : 0.0;
}

// the production record [9 logits | 18 directions | 9 confidences], which has kernels of its own; CP_LS_GENERIC (read on every call)
// sends it to the generic ones
bool is_record36(int ld, int dir_off, int conf_off) { return ld == REC_LD && dir_off == REC_DIR && conf_off == REC_CONF && !getenv("CP_LS_GENERIC"); }

// the solve of a reweighted pass: ls_solve_kernel's value where cp_lsr::solve accepts the reweighted system, otherwise the keypoint is left as
// the pass before wrote it
__global__ void ls_robust_solve_kernel(const double* __restrict__ plain, const double* __restrict__ sums, int total, int H, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    double p0, p1;
    if (cp_lsr::solve(sums + (size_t)i * 5, plain[(size_t)i * 5] + plain[(size_t)i * 5 + 2], p0, p1)) {
        out[2 * i] = (float)p0 * (float)H;
        out[2 * i + 1] = (float)p1 * (float)H;
    }
}

// the finish of the moments pass, one thread per (image, slot, keypoint): cp_lsc::finish of the five sums; the keypoints are only read
__global__ void ls_cov_finish_kernel(const double* __restrict__ sums, const float* __restrict__ keypoints, int total, int H, float* __restrict__ cov,
                                     float* __restrict__ stat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float py = keypoints[2 * i], px = keypoints[2 * i + 1];
    cp_lsc::finish(sums + (size_t)i * 5, isfinite(py) && isfinite(px), H, cov + (size_t)i * 3, stat + (size_t)i * 2);
}

constexpr int LS_MAX_LDS = 160 * 1024;   // per workgroup on gfx950

// what cp_ls_vote_slots_f32 refuses, under the name `fn` of the entry point that was called
int ls_slots_check(const char* fn, const float* field, int ld, int dir_off, int conf_off, const uint8_t* slot_map, int batch, int h, int w, int slots,
                   int kp, const void* sums_ws, const float* keypoints) {
    CP_REQUIRE(field && slot_map && sums_ws && keypoints, "%s: null pointer (the slot map is required)", fn);
    CP_REQUIRE(batch > 0 && h > 0 && w > 0 && slots > 0 && slots < 255, "%s: bad sizes (slots must be in 1..254)", fn);
    CP_REQUIRE(kp == MAXKP, "%s: built for %d keypoints (got %d)", fn, MAXKP, kp);
    CP_REQUIRE(ld % 4 == 0 && ld > 0 && ld <= 64 && ((uintptr_t)field & 15) == 0, "%s: ld must be a multiple of 4 (<= 64) and field 16-byte aligned", fn);
    CP_REQUIRE(dir_off >= 0 && dir_off + 2 * kp <= ld && conf_off >= 0 && conf_off + kp <= ld, "%s: channel offsets outside the pixel record", fn);
    return CP_OK;
}

// launches an accumulate kernel, its LDS limit raised first where the launch needs more than the default 64 KB
template <class... P, class... A>
int ls_launch(const char* fn, void (*kernel)(P...), dim3 grid, size_t lds, hipStream_t st, A... args) {
    if (lds > 64 * 1024)   // (the limit counts the kernel's static LDS too: ask for what this launch needs, not for the whole 160 KB)
        CP_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess,
                   "%s: cannot raise the kernel's LDS limit to %zu bytes", fn, lds);
    CP_LAUNCH(kernel, grid, dim3(256), lds, st, args...);
    return CP_OK;
}

// zeroes `sums` and accumulates one pass over the slot map into it: the plain pass, a reweighted pass or the covariance's moments pass, the two
// latter against the estimates `est` (the keypoints buffer).  The production record has a kernel of its own, every other layout takes the
// generic kernel's walk.
int ls_slots_accumulate(const char* fn, const float* field, int ld, int dir_off, int conf_off, const uint8_t* slot_map, int batch, int h, int w,
                        int slots, int kp, int sigmoid_weights, double* sums, LsMode mode, const float* est, float rscale, hipStream_t st) {
    if (hipMemsetAsync(sums, 0, cp_ls_vote_workspace_bytes(batch, slots, kp), st) != hipSuccess) return cp::check_launch(fn);
    const int strips_x = (w + 63) / 64, strips_y = (h + ROWS - 1) / ROWS;
    const int blocks_per_img = (strips_x * strips_y + WAVES - 1) / WAVES;
    const size_t table = (sizeof(double) * slots * kp * 5 + 15) / 16 * 16;
    const size_t lds = table + sizeof(float) * WAVES * 64 * ld;
    static_assert((sizeof(double) * 254 * MAXKP * 5 + 15) / 16 * 16 + sizeof(float) * WAVES * 64 * 64 <= (size_t)LS_MAX_LDS, "254 slots beside ld = 64 fit");
    const dim3 grid(batch * blocks_per_img);
    int rc;
    if (!sigmoid_weights && is_record36(ld, dir_off, conf_off)) {
        const auto kernel = mode == LS_MOMENTS      ? &ls_accumulate36_slots_kernel<LS_MOMENTS>
                            : mode == LS_REWEIGHTED ? &ls_accumulate36_slots_kernel<LS_REWEIGHTED>
                                                    : &ls_accumulate36_slots_kernel<LS_PLAIN>;
        rc = ls_launch(fn, kernel, grid, lds, st, field, slot_map, batch, h, w, slots, sums, strips_x, strips_y, est, rscale);
    } else {
        // the generic kernel with given labels: its table has `objects` rows, and the logits (seg_off) are read only without labels
        const auto kernel = mode == LS_MOMENTS      ? &ls_accumulate_kernel<MAXKP, LS_MOMENTS>
                            : mode == LS_REWEIGHTED ? &ls_accumulate_kernel<MAXKP, LS_REWEIGHTED>
                                                    : &ls_accumulate_kernel<MAXKP, LS_PLAIN>;
        rc = ls_launch(fn, kernel, grid, lds, st, field, ld, 0, dir_off, conf_off, slot_map, batch, h, w, slots, sums, strips_x, strips_y,
                       sigmoid_weights ? 1 : 0, est, rscale);
    }
    return rc != CP_OK ? rc : cp::check_launch(fn);
}

}  // namespace

extern "C" size_t cp_ls_vote_workspace_bytes(int batch, int objects, int kp) {
    return (size_t)batch * objects * kp * 5 * sizeof(double);
}

extern "C" int cp_ls_vote_f32(const float* field, int ld, int seg_off, int dir_off, int conf_off, const uint8_t* labels,
                              int batch, int h, int w, int objects, int kp, double* sums_ws, float* keypoints,
                              void* stream) {
    return cp_ls_vote_w_f32(field, ld, seg_off, dir_off, conf_off, labels, batch, h, w, objects, kp, 0, sums_ws, keypoints, stream);
}

// the same voter with the pixel weight selectable: sigmoid_weights = 0 softplus(conf) (the configs' choice), 1 sigmoid(conf)
// (CoordLSVotingWeighted(sigmoid_weights=True), voting_layers_2d.py:32-33)
extern "C" int cp_ls_vote_w_f32(const float* field, int ld, int seg_off, int dir_off, int conf_off, const uint8_t* labels, int batch, int h, int w,
                                int objects, int kp, int sigmoid_weights, double* sums_ws, float* keypoints, void* stream) {
    CP_REQUIRE(field && sums_ws && keypoints, "cp_ls_vote_f32: null pointer");
    CP_REQUIRE(batch > 0 && h > 0 && w > 0 && objects > 0 && objects < 255, "cp_ls_vote_f32: bad sizes");
    CP_REQUIRE(kp == MAXKP, "cp_ls_vote_f32: built for %d keypoints (got %d)", MAXKP, kp);
    CP_REQUIRE(ld % 4 == 0 && ld <= 64 && ((uintptr_t)field & 15) == 0, "cp_ls_vote_f32: ld must be a multiple of 4 (<= 64) and field 16-byte aligned");
    CP_REQUIRE(seg_off >= 0 && seg_off + objects + 1 <= ld && dir_off >= 0 && dir_off + 2 * kp <= ld && conf_off >= 0 && conf_off + kp <= ld,
               "cp_ls_vote_f32: channel offsets outside the pixel record");
    hipStream_t st = (hipStream_t)stream;
    size_t nbytes = cp_ls_vote_workspace_bytes(batch, objects, kp);
    if (hipMemsetAsync(sums_ws, 0, nbytes, st) != hipSuccess) return cp::check_launch("cp_ls_vote_f32 memset");
    int strips_x = (w + 63) / 64, strips_y = (h + ROWS - 1) / ROWS;
    int blocks_per_img = (strips_x * strips_y + WAVES - 1) / WAVES;
    size_t lds = sizeof(double) * objects * kp * 5 + sizeof(float) * WAVES * 64 * ld;
    if (!sigmoid_weights && seg_off == 0 && objects == 8 && is_record36(ld, dir_off, conf_off)) {
        if (labels)
            CP_LAUNCH(ls_accumulate36_kernel<true>, dim3(batch * blocks_per_img), dim3(256), lds, st, field, labels, batch, h, w, sums_ws, strips_x, strips_y);
        else
            CP_LAUNCH(ls_accumulate36_kernel<false>, dim3(batch * blocks_per_img), dim3(256), lds, st, field, labels, batch, h, w, sums_ws, strips_x, strips_y);
    } else {
        CP_LAUNCH((ls_accumulate_kernel<MAXKP>), dim3(batch * blocks_per_img), dim3(256), lds, st, field, ld, seg_off,
                  dir_off, conf_off, labels, batch, h, w, objects, sums_ws, strips_x, strips_y, sigmoid_weights ? 1 : 0, (const float*)nullptr, 0.f);
    }
    int total = batch * objects * kp;
    CP_LAUNCH(ls_solve_kernel, dim3((total + 255) / 256), dim3(256), 0, st, sums_ws, total, h, keypoints);
    return cp::check_launch("cp_ls_vote_f32");
}

extern "C" int cp_ls_vote_bwd_f32(const float* field, int ld, int dir_off, int conf_off, const uint8_t* labels, int batch, int h, int w,
                                  int objects, int kp, const double* sums_ws, const float* dkeypoints, float* pu_ws,
                                  const uint8_t* reg_labels, const float* conf_coef, float* dfield, int dld, int ddir_off, int dconf_off,
                                  int accumulate, void* stream) {
    CP_REQUIRE(field && labels && sums_ws && dkeypoints && pu_ws && dfield, "cp_ls_vote_bwd_f32: null pointer");
    CP_REQUIRE(kp == MAXKP, "cp_ls_vote_bwd_f32: built for %d keypoints (got %d)", MAXKP, kp);
    CP_REQUIRE(batch > 0 && h > 0 && w > 0 && objects > 0 && objects < 255, "cp_ls_vote_bwd_f32: bad sizes");
    CP_REQUIRE(dir_off >= 0 && dir_off + 2 * kp <= ld && conf_off >= 0 && conf_off + kp <= ld, "cp_ls_vote_bwd_f32: channel offsets outside the pixel record");
    CP_REQUIRE(ddir_off >= 0 && ddir_off + 2 * kp <= dld && dconf_off >= 0 && dconf_off + kp <= dld, "cp_ls_vote_bwd_f32: gradient offsets outside the row");
    CP_REQUIRE((reg_labels == nullptr) == (conf_coef == nullptr), "cp_ls_vote_bwd_f32: reg_labels and conf_coef come together");
    hipStream_t st = (hipStream_t)stream;
    const int total = batch * objects * kp;
    CP_LAUNCH(ls_bwd_prepare_kernel, dim3((total + 255) / 256), dim3(256), 0, st, sums_ws, dkeypoints, total, h, pu_ws);
    if (cp::check_launch("cp_ls_vote_bwd_f32 prepare") != CP_OK) return CP_ERR_LAUNCH;
    const long long px = (long long)batch * h * w;
    long long blocks = (px + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    const bool rec36 = is_record36(ld, dir_off, conf_off) && dld % 4 == 0 && ddir_off % 4 == 0 && dconf_off == ddir_off + 18 && ddir_off + 28 <= dld &&
                       (((uintptr_t)field | (uintptr_t)dfield | (uintptr_t)pu_ws) & 15) == 0;
    if (rec36)   // in overwrite mode the float behind the 27 gradient values (padding of the row) is zeroed with them
        CP_LAUNCH(ls_bwd36_kernel, dim3((unsigned)blocks), dim3(256), 0, st, field, labels, batch, h, w, objects, pu_ws, reg_labels, conf_coef, dfield, dld,
                  ddir_off, accumulate);
    else
        CP_LAUNCH((ls_bwd_kernel<MAXKP>), dim3((unsigned)blocks), dim3(256), 0, st, field, ld, dir_off, conf_off, labels, batch, h, w, objects, pu_ws, reg_labels,
                  conf_coef, dfield, dld, ddir_off, dconf_off, accumulate);
    return cp::check_launch("cp_ls_vote_bwd_f32");
}

extern "C" int cp_kp_stats_f32(const float* field, int ld, int conf_off, const uint8_t* labels, const uint8_t* labels_est, int batch, int h, int w,
                               int classes, int kp, int32_t* counts, double* conf_sums, void* stream) {
    CP_REQUIRE(field && labels && counts && conf_sums, "cp_kp_stats_f32: null pointer");
    CP_REQUIRE(kp == MAXKP && classes >= 2 && classes <= 256 && conf_off >= 0 && conf_off + kp <= ld, "cp_kp_stats_f32: bad sizes");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(int32_t) * 2 * batch * classes, st) != hipSuccess) return cp::check_launch("cp_kp_stats_f32 memset");
    if (hipMemsetAsync(conf_sums, 0, sizeof(double) * batch * kp, st) != hipSuccess) return cp::check_launch("cp_kp_stats_f32 memset");
    const int ppi = h * w;
    int gx = (ppi + 255) / 256;
    if (gx > 256) gx = 256;
    CP_LAUNCH((kp_stats_kernel<MAXKP>), dim3(gx, batch), dim3(256), sizeof(int) * 2 * classes, st, field, ld, conf_off, labels, labels_est, ppi, classes, counts,
              conf_sums);
    return cp::check_launch("cp_kp_stats_f32");
}

extern "C" int cp_kp_reproj_loss_f32(const float* coords_yx, const float* gt_xy, const float* affine, const float* avail, int batch, int objects,
                                     int kp, float max_pixel_error, float weight, float* g_yx, double* loss_out, void* stream) {
    CP_REQUIRE(coords_yx && gt_xy && affine && avail && g_yx && loss_out && batch > 0 && objects > 0 && kp > 0, "cp_kp_reproj_loss_f32: bad arguments");
    CP_LAUNCH(kp_reproj_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, coords_yx, gt_xy, affine, avail, batch, objects, kp, max_pixel_error, weight,
              g_yx, loss_out);
    return cp::check_launch("cp_kp_reproj_loss_f32");
}

// ---------------------------------------------------------------------------------------------------------------------------------------------
// Voting keyed by (object, instance): cp_ls_vote_slots_f32 takes the slot map of cp_ccl_instance_labels as its label map and keeps one row of
// sums per slot.  The logits are not read.  The per-pixel arithmetic, the accumulators and the solve are the ones above.
extern "C" int cp_ls_vote_slots_f32(const float* field, int ld, int dir_off, int conf_off, const uint8_t* slot_map, int batch, int h, int w,
                                    int slots, int kp, int sigmoid_weights, double* sums_ws, float* keypoints, void* stream) {
    const char* fn = "cp_ls_vote_slots_f32";
    if (ls_slots_check(fn, field, ld, dir_off, conf_off, slot_map, batch, h, w, slots, kp, sums_ws, keypoints) != CP_OK) return CP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int rc = ls_slots_accumulate(fn, field, ld, dir_off, conf_off, slot_map, batch, h, w, slots, kp, sigmoid_weights, sums_ws, LS_PLAIN, nullptr, 0.f, st);
    if (rc != CP_OK) return rc;
    const int total = batch * slots * kp;
    CP_LAUNCH(ls_solve_kernel, dim3((total + 255) / 256), dim3(256), 0, st, sums_ws, total, h, keypoints);
    return cp::check_launch(fn);
}

extern "C" size_t cp_ls_vote_robust_workspace_bytes(int batch, int slots, int kp) { return 2 * cp_ls_vote_workspace_bytes(batch, slots, kp); }

// The robust voter per slot: pass 0 is cp_ls_vote_slots_f32's accumulate and solve into block 0 of the workspace; every further pass zeroes
// block 1, accumulates the sums reweighted against the keypoints of the pass before, and solves by the rule of cp_lsr::solve.
extern "C" int cp_ls_vote_slots_robust_f32(const float* field, int ld, int dir_off, int conf_off, const uint8_t* slot_map, int batch, int h, int w,
                                           int slots, int kp, int sigmoid_weights, float cutoff_px, int passes, void* workspace, float* keypoints,
                                           void* stream) {
    const char* fn = "cp_ls_vote_slots_robust_f32";
    if (ls_slots_check(fn, field, ld, dir_off, conf_off, slot_map, batch, h, w, slots, kp, workspace, keypoints) != CP_OK) return CP_ERR_INVALID;
    CP_REQUIRE(std::isfinite(cutoff_px) && cutoff_px > 0.f, "%s: cutoff_px must be finite and > 0 (got %g)", fn, (double)cutoff_px);
    CP_REQUIRE(passes >= 0 && passes <= cp_lsr::CP_LS_ROBUST_MAX_PASSES, "%s: passes must be in 0..%d (got %d)", fn, cp_lsr::CP_LS_ROBUST_MAX_PASSES, passes);
    CP_REQUIRE((((uintptr_t)workspace | (uintptr_t)keypoints) & 7) == 0, "%s: the workspace and the keypoints must be 8-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    const int total = batch * slots * kp;
    double* plain = static_cast<double*>(workspace);
    double* again = plain + (size_t)total * 5;
    int rc = ls_slots_accumulate(fn, field, ld, dir_off, conf_off, slot_map, batch, h, w, slots, kp, sigmoid_weights, plain, LS_PLAIN, nullptr, 0.f, st);
    if (rc != CP_OK) return rc;
    CP_LAUNCH(ls_solve_kernel, dim3((total + 255) / 256), dim3(256), 0, st, plain, total, h, keypoints);
    if ((rc = cp::check_launch(fn)) != CP_OK) return rc;
    const float rscale = cp_lsr::rho_scale(h, cutoff_px);
    for (int k = 1; k <= passes; ++k) {
        rc = ls_slots_accumulate(fn, field, ld, dir_off, conf_off, slot_map, batch, h, w, slots, kp, sigmoid_weights, again, LS_REWEIGHTED, keypoints, rscale, st);
        if (rc != CP_OK) return rc;
        CP_LAUNCH(ls_robust_solve_kernel, dim3((total + 255) / 256), dim3(256), 0, st, plain, again, total, h, keypoints);
        if ((rc = cp::check_launch(fn)) != CP_OK) return rc;
    }
    return CP_OK;
}

// A covariance per (image, slot, keypoint) for keypoints handed in: one moments pass over the slot map (the reweighted pass's stream) and a
// finish per keypoint; ls_cov_math.h has the definition, include/casapose_hip.h the rule.
extern "C" int cp_ls_slot_covariance_f32(const float* field, int ld, int dir_off, int conf_off, const uint8_t* slot_map, int batch, int h, int w,
                                         int slots, int kp, int sigmoid_weights, float cutoff_px, const float* keypoints, double* sums_ws, float* cov,
                                         float* stat, void* stream) {
    const char* fn = "cp_ls_slot_covariance_f32";
    if (ls_slots_check(fn, field, ld, dir_off, conf_off, slot_map, batch, h, w, slots, kp, sums_ws, keypoints) != CP_OK) return CP_ERR_INVALID;
    CP_REQUIRE(cov && stat, "%s: null pointer (cov and stat are required)", fn);
    CP_REQUIRE(std::isfinite(cutoff_px) && cutoff_px >= 0.f, "%s: cutoff_px must be finite and >= 0, 0 for no reweighting (got %g)", fn, (double)cutoff_px);
    CP_REQUIRE((((uintptr_t)sums_ws | (uintptr_t)keypoints) & 7) == 0, "%s: the workspace and the keypoints must be 8-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    const float rscale = cutoff_px > 0.f ? cp_lsr::rho_scale(h, cutoff_px) : 0.f;
    const int rc = ls_slots_accumulate(fn, field, ld, dir_off, conf_off, slot_map, batch, h, w, slots, kp, sigmoid_weights, sums_ws, LS_MOMENTS, keypoints, rscale, st);
    if (rc != CP_OK) return rc;
    const int total = batch * slots * kp;
    CP_LAUNCH(ls_cov_finish_kernel, dim3((total + 255) / 256), dim3(256), 0, st, sums_ws, keypoints, total, h, cov, stat);
    return cp::check_launch(fn);
}
