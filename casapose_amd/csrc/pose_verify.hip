// Pose verification on the device: per (image, rendered plane, label) job the integers a score is made of -- rendered, hidden, on_label,
// on_background, on_other, label_pixels, pairs, inliers (verify_math.h states the rules).  The planes and records are what cp_render_masks_u8
// left behind; nothing is rewritten but the counts and the workspace.  This file is the schedule.
//
// verify_hist_kernel: grid (images * blocks per image) on x, 256 threads.  A block keeps 256 bins in LDS; a thread takes 16-byte chunks of
//   the image's label bytes (one 16-byte load where the chunk is whole: chunks are cut at absolute 16-byte boundaries, so only the image's first
//   and last chunk can be partial), merges runs of equal labels in registers, keeps its count of label 0 to itself until the end and sends the
//   rest to LDS.  Only non-zero bins go to global memory, with one integer atomic each.  The workspace is zeroed inside the call.
// verify_counts_kernel: grid (jobs * split) on x, 256 threads.  A block owns one job and every split-th step of TILE = 256 pixels of the job's
//   clipped box, pixel s of the box going to row s / bw, column s % bw, so that the lanes of a wave read runs of consecutive words of a row.
//   First the block intersects the job's box with the boxes of the frame's other planes (thread t takes plane t of the frame, from `records`)
//   and lists in LDS the ones that can hide something: with 8 estimates per image that is usually none or one, and only those planes are read.
//   The five pixel predicates are counted with the 64-bit wave ballot and a popcount; the sums are wave-uniform.  An on_label lane reads its
//   pixel's directions (16-byte loads where ld is a multiple of 4 and the field is 16-byte aligned: the production record's directions 9 .. 26
//   come from the five quads 8 .. 27) and counts its pairs and inliers in two registers, which a butterfly sums per wave after the walk.  Each
//   wave adds its integers to LDS, and 8 threads of the block add the non-zero ones to the job's counts with one global integer atomic each.
//   The counts are zeroed inside the call; integer sums do not depend on their order: two calls give the same bytes, whatever split is.
// Every index read from device memory (image, plane, label, the instance count, the box corners) is range-checked before it addresses anything
// (job_setup, hider_box).
#include "common.h"
#include "verify_math.h"

namespace {

using namespace cp_verify;

constexpr int THREADS = TILE, WAVE = 64;
constexpr int HIST_BLOCKS = 64;        // blocks per image at the most
constexpr int MAX_LD = 4096;           // floats of a field record
constexpr int MAX_IMAGES = 1 << 22;    // images * HIST_BLOCKS blocks stay below 2^31

__device__ inline void hist_add(int label, int n, int& zeros, int32_t* s_bins) {
    if (label == 0)
        zeros += n;
    else
        atomicAdd(&s_bins[label], n);
}

__global__ void __launch_bounds__(THREADS) verify_hist_kernel(const uint8_t* __restrict__ labels, size_t hw, int per_image, int32_t* __restrict__ hist) {
    __shared__ int32_t s_bins[BINS];
    const int tid = threadIdx.x;
    const size_t image = blockIdx.x / (unsigned)per_image;
    const int part = (int)(blockIdx.x % (unsigned)per_image);
    s_bins[tid] = 0;
    __syncthreads();
    const uint8_t* __restrict__ base = labels + image * hw;
    size_t head = (size_t)((16 - ((uintptr_t)base & 15)) & 15);   // bytes in front of the first 16-byte boundary
    if (head > hw) head = hw;
    const size_t chunks = 1 + (hw - head + 15) / 16;                // chunk 0: the head (it may be empty)
    int zeros = 0;
    for (size_t c = (size_t)part * THREADS + tid; c < chunks; c += (size_t)per_image * THREADS) {
        const size_t lo = c == 0 ? 0 : head + 16 * (c - 1);
        const size_t hi = c == 0 ? head : (lo + 16 < hw ? lo + 16 : hw);   // lo < hi <= hw, but for an empty head
        int run = 0, count = 0;
        if (hi - lo == 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(base + lo);   // base + lo is 16-byte aligned for every c >= 1
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int l = (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
                if (l != run) {
                    if (count) hist_add(run, count, zeros, s_bins);
                    run = l, count = 0;
                }
                count += 1;
            }
        } else {
            for (size_t at = lo; at < hi; ++at) {
                const int l = base[at];
                if (l != run) {
                    if (count) hist_add(run, count, zeros, s_bins);
                    run = l, count = 0;
                }
                count += 1;
            }
        }
        if (count) hist_add(run, count, zeros, s_bins);
    }
    if (zeros) atomicAdd(&s_bins[0], zeros);
    __syncthreads();
    const int32_t v = s_bins[tid];
    if (v != 0) atomicAdd(hist + image * BINS + tid, v);
}

__global__ void __launch_bounds__(THREADS) verify_counts_kernel(const uint32_t* __restrict__ planes, const int32_t* __restrict__ records, int nplanes, int H,
                                                               int W, const int32_t* __restrict__ inst_counts, int frames, int instances_max,
                                                               const uint8_t* __restrict__ labels, const float* __restrict__ field, int images, int ld,
                                                               int dir_off, int kp, const double* __restrict__ kp2d, const int32_t* __restrict__ jobs,
                                                               double sample, double cos2, int split, int quads, const int32_t* __restrict__ hist,
                                                               int32_t* __restrict__ counts) {
    __shared__ int32_t s_counts[COUNTS];
    __shared__ int s_hiders;
    __shared__ int s_q[MAX_INSTANCES];
    __shared__ Box s_box[MAX_INSTANCES];
    __shared__ double s_kp[2 * MAX_KP];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const size_t job = blockIdx.x / (unsigned)split;
    const int part = (int)(blockIdx.x % (unsigned)split);
    Job j;
    // block-uniform exits: nothing below them has been synchronised yet
    if (!job_setup(jobs + 4 * job, records, nplanes, inst_counts, frames, instances_max, images, H, W, j)) return;
    if (part == 0 && tid == 0) {
        const int32_t v = hist[(size_t)j.image * BINS + j.label];
        if (v != 0) counts[job * COUNTS + C_LABEL_PIXELS] = v;   // the one writer of this word
    }
    if (!j.walks) return;
    const int bw = j.box.x1 - j.box.x0 + 1, bh = j.box.y1 - j.box.y0 + 1;
    const int total = bh * bw;   // <= 2^28
    if (part * TILE >= total) return;
    if (tid < COUNTS) s_counts[tid] = 0;
    if (tid == 0) s_hiders = 0;
    if (tid < 2 * kp) s_kp[tid] = kp2d[job * (size_t)(2 * kp) + tid];
    __syncthreads();
    if (tid < j.hiders) {   // hiders <= instances_max <= THREADS
        Box b;
        if (hider_box(j, j.first + tid, records, H, W, b)) {
            const int k = atomicAdd(&s_hiders, 1);   // the list's order is arbitrary; rule 4 is an OR over it
            s_q[k] = j.first + tid;
            s_box[k] = b;
        }
    }
    __syncthreads();
    const int nh = s_hiders;

    const size_t hw = (size_t)H * (size_t)W;
    const uint32_t* __restrict__ mine = planes + (size_t)j.plane * hw;
    const uint8_t* __restrict__ lab = labels + (size_t)j.image * hw;
    const float* __restrict__ fld = field + (size_t)j.image * hw * (size_t)ld;

    int n_rendered = 0, n_hidden = 0, n_label = 0, n_back = 0, n_other = 0;   // the same in every lane of a wave
    int n_pairs = 0, n_inliers = 0;                                          // per lane
    for (long long first = (long long)part * TILE; first < total; first += (long long)split * TILE) {
        const long long s = first + tid;
        bool rendered = false;
        int i = 0, x = 0;
        size_t at = 0;
        uint32_t w = EMPTY;
        if (s < total) {
            const int di = (int)((unsigned)s / (unsigned)bw);
            i = j.box.y0 + di, x = j.box.x0 + ((int)s - di * bw);   // i < H, x < W (job_setup)
            at = (size_t)i * W + x;
            w = mine[at];
            rendered = w != EMPTY;
        }
        const unsigned long long b_rendered = __ballot(rendered);
        if (b_rendered == 0) continue;   // wave-uniform
        n_rendered += __popcll(b_rendered);
        bool hidden = false;
        if (nh != 0) {   // block-uniform
            if (rendered)
                for (int k = 0; k < nh && !hidden; ++k)
                    if (inside(s_box[k], i, x)) hidden = hides(planes[(size_t)s_q[k] * hw + at], s_q[k], w, j.plane);
            n_hidden += __popcll(__ballot(hidden));
        }
        const bool visible = rendered && !hidden;
        const int L = visible ? (int)lab[at] : -1;
        const bool on_label = L == j.label;
        const unsigned long long b_label = __ballot(on_label);
        n_label += __popcll(b_label);
        n_back += __popcll(__ballot(L == 0));
        n_other += __popcll(__ballot(L > 0 && !on_label));
        if (b_label == 0) continue;
        if (on_label) {
            const float* __restrict__ rec = fld + at * (size_t)ld;
            const double ci = pixel_centre(i, sample), cj = pixel_centre(x, sample);
            if (quads) {
                float dy = 0.f;
                for (int v = dir_off >> 2; v <= (dir_off + 2 * kp - 1) >> 2; ++v) {   // 4 v + 3 < ld: ld is a multiple of 4
                    const float4 f = reinterpret_cast<const float4*>(rec)[v];
                    const float c[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int idx = 4 * v + t - dir_off;
                        if (idx < 0 || idx >= 2 * kp) continue;
                        if ((idx & 1) == 0) {
                            dy = c[t];
                        } else {
                            const int bits = pair_bits(dy, c[t], s_kp[idx - 1], s_kp[idx], ci, cj, cos2);
                            n_pairs += bits & 1, n_inliers += bits >> 1;
                        }
                    }
                }
            } else {
                for (int k = 0; k < kp; ++k) {
                    const int bits = pair_bits(rec[dir_off + 2 * k], rec[dir_off + 2 * k + 1], s_kp[2 * k], s_kp[2 * k + 1], ci, cj, cos2);
                    n_pairs += bits & 1, n_inliers += bits >> 1;
                }
            }
        }
    }
#pragma unroll
    for (int off = WAVE / 2; off >= 1; off >>= 1) {
        n_pairs += __shfl_xor(n_pairs, off);
        n_inliers += __shfl_xor(n_inliers, off);
    }
    if (lane == 0 && n_rendered != 0) {
        atomicAdd(&s_counts[C_RENDERED], n_rendered);
        atomicAdd(&s_counts[C_HIDDEN], n_hidden);
        atomicAdd(&s_counts[C_ON_LABEL], n_label);
        atomicAdd(&s_counts[C_ON_BACKGROUND], n_back);
        atomicAdd(&s_counts[C_ON_OTHER], n_other);
        atomicAdd(&s_counts[C_PAIRS], n_pairs);
        atomicAdd(&s_counts[C_INLIERS], n_inliers);
    }
    __syncthreads();
    if (tid < COUNTS) {
        const int32_t v = s_counts[tid];   // word C_LABEL_PIXELS stays 0 here
        if (v != 0) atomicAdd(counts + job * COUNTS + tid, v);
    }
}

size_t hist_bytes(int images) { return (size_t)images * BINS * sizeof(int32_t); }

int check_verify(const char* fn, const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const int32_t* inst_counts, int frames,
                 int instances_max, const uint8_t* labels, const float* field, int images, int ld, int dir_off, int kp, const double* kp2d,
                 const int32_t* jobs, int njobs, double sample_offset, double cos_min, int split, int32_t* counts, void* workspace,
                 size_t workspace_bytes) {
    CP_REQUIRE(planes && records && inst_counts && labels && field && kp2d && jobs && counts && workspace, "%s: null pointer", fn);
    CP_REQUIRE(kp >= 1 && kp <= MAX_KP, "%s: kp must lie in [1, %d] (got %d)", fn, MAX_KP, kp);
    CP_REQUIRE(nplanes >= 1 && frames >= 1 && images >= 1 && njobs >= 1, "%s: nplanes, frames, images and njobs must be positive (got %d, %d, %d, %d)", fn,
               nplanes, frames, images, njobs);
    CP_REQUIRE(instances_max >= 1 && instances_max <= MAX_INSTANCES, "%s: instances_max must lie in [1, %d] (got %d)", fn, MAX_INSTANCES, instances_max);
    CP_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "%s: H and W must lie in [1, %d] (got %d x %d)", fn, MAX_SIDE, H, W);
    CP_REQUIRE((long long)nplanes < (1ll << 31) / RECORD, "%s: nplanes %d is too large", fn, nplanes);
    CP_REQUIRE(images <= MAX_IMAGES, "%s: images must be at most %d (got %d)", fn, MAX_IMAGES, images);
    CP_REQUIRE(ld >= 2 && ld <= MAX_LD && dir_off >= 0 && (long long)dir_off + 2 * kp <= ld,
               "%s: the field record needs 2 <= ld <= %d and 0 <= dir_off with dir_off + 2 kp <= ld (got ld %d, dir_off %d, kp %d)", fn, MAX_LD, ld, dir_off, kp);
    CP_REQUIRE((long long)H * W * kp <= 0x7fffffffLL, "%s: H x W x kp = %d x %d x %d is above 2^31 - 1: the pair counts would not fit", fn, H, W, kp);
    CP_REQUIRE(sample_offset >= 0.0 && sample_offset <= 1.0, "%s: sample_offset must lie in [0, 1] (got %g)", fn, sample_offset);
    CP_REQUIRE(cos_min >= 0.0 && cos_min <= 1.0, "%s: cos_min must lie in [0, 1] (got %g)", fn, cos_min);
    CP_REQUIRE(split >= 1 && split <= MAX_SPLIT, "%s: split must lie in [1, %d] blocks per job (got %d)", fn, MAX_SPLIT, split);
    CP_REQUIRE((long long)njobs * split <= 0x7fffffffLL, "%s: njobs %d x split %d is above 2^31 - 1 blocks; split the call", fn, njobs, split);
    CP_REQUIRE(workspace_bytes >= hist_bytes(images), "%s: workspace_bytes %zu is below cp_pose_verify_workspace_bytes = %zu", fn, workspace_bytes,
               hist_bytes(images));
    CP_REQUIRE(((uintptr_t)planes & 3) == 0 && ((uintptr_t)records & 3) == 0 && ((uintptr_t)inst_counts & 3) == 0 && ((uintptr_t)field & 3) == 0 &&
                   ((uintptr_t)jobs & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
               "%s: planes, records, inst_counts, field, jobs, counts and workspace must be 4-byte aligned", fn);
    CP_REQUIRE(((uintptr_t)kp2d & 7) == 0, "%s: kp2d must be 8-byte aligned", fn);
    return CP_OK;
}

}  // namespace

extern "C" int cp_pose_verify_tile(void) { return TILE; }

extern "C" size_t cp_pose_verify_workspace_bytes(int images) { return images < 1 || images > MAX_IMAGES ? 0 : hist_bytes(images); }

extern "C" int cp_pose_verify_i32(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const int32_t* inst_counts, int frames,
                                  int instances_max, const uint8_t* labels, const float* field, int images, int ld, int dir_off, int kp,
                                  const double* kp2d, const int32_t* jobs, int njobs, double sample_offset, double cos_min, int split, int32_t* counts,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_verify("cp_pose_verify_i32", planes, records, nplanes, H, W, inst_counts, frames, instances_max, labels, field, images, ld, dir_off, kp,
                              kp2d, jobs, njobs, sample_offset, cos_min, split, counts, workspace, workspace_bytes))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)njobs * COUNTS * sizeof(int32_t), st) != hipSuccess ||
        hipMemsetAsync(workspace, 0, hist_bytes(images), st) != hipSuccess) {
        cp::set_error("cp_pose_verify_i32: clearing the counts and the workspace failed: %s", hipGetErrorString(hipGetLastError()));
        return CP_ERR_LAUNCH;
    }
    const size_t hw = (size_t)H * (size_t)W;
    const size_t chunks = 1 + (hw + 15) / 16;
    const int per_image = (int)((chunks + THREADS - 1) / THREADS < (size_t)HIST_BLOCKS ? (chunks + THREADS - 1) / THREADS : (size_t)HIST_BLOCKS);
    CP_LAUNCH(verify_hist_kernel, dim3((unsigned)((long long)images * per_image)), dim3(THREADS), 0, st, labels, hw, per_image, (int32_t*)workspace);
    if (int rc = cp::check_launch("cp_pose_verify_i32 (histogram)")) return rc;
    const int quads = (ld & 3) == 0 && ((uintptr_t)field & 15) == 0;
    CP_LAUNCH(verify_counts_kernel, dim3((unsigned)((long long)njobs * split)), dim3(THREADS), 0, st, planes, records, nplanes, H, W, inst_counts, frames,
              instances_max, labels, field, images, ld, dir_off, kp, kp2d, jobs, sample_offset, cos_min * cos_min, split, quads, (const int32_t*)workspace,
              counts);
    return cp::check_launch("cp_pose_verify_i32 (counts)");
}

extern "C" int cp_pose_verify_host_i32(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const int32_t* inst_counts, int frames,
                                       int instances_max, const uint8_t* labels, const float* field, int images, int ld, int dir_off, int kp,
                                       const double* kp2d, const int32_t* jobs, int njobs, double sample_offset, double cos_min, int split,
                                       int32_t* counts, void* workspace, size_t workspace_bytes) {
    if (int rc = check_verify("cp_pose_verify_host_i32", planes, records, nplanes, H, W, inst_counts, frames, instances_max, labels, field, images, ld, dir_off,
                              kp, kp2d, jobs, njobs, sample_offset, cos_min, split, counts, workspace, workspace_bytes))
        return rc;
    verify_serial(planes, records, nplanes, H, W, inst_counts, frames, instances_max, labels, field, images, ld, dir_off, kp, kp2d, jobs, njobs, sample_offset,
                  cos_min, counts, (int32_t*)workspace);
    return CP_OK;
}
