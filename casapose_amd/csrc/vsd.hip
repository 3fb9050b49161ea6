// BOP's VSD counts on the device: per (estimate plane, ground-truth plane, image) pair the visible union, the visible intersection and, per
// tau, the intersection pixels whose cost reaches it -- integers from which the host takes the error (vsd_math.h states the rules).  The planes
// and records are what cp_render_masks_u8 left behind; this file is the schedule.
//
// vsd_counts_kernel: grid (pairs * split) on x, 256 threads.  A block owns one pair and every split-th step of TILE = 256 pixels of the union of
//   the pair's two boxes, pixel s of the box going to row s / bw, column s % bw, so that the lanes of a wave read runs of consecutive words of a
//   row of each plane and of the sensor depth.  A pixel neither plane hit costs its three loads and nothing else.  Per step a wave takes one
//   ballot for uni, one for inter and, where any lane has inter, one per tau; lane k keeps tau k's count, the two sums are wave-uniform.  After
//   the walk each wave adds its 2 + ntau integers to LDS, and 2 + ntau threads of the block add the non-zero ones to the pair's counts with one
//   global integer atomic each.  The counts are zeroed inside the call; integer sums do not depend on their order: two calls give the same bytes.
// Every index read from device memory (image, the two planes, the box corners) is range-checked before it addresses anything (pair_setup).
#include "common.h"
#include "vsd_math.h"

namespace {

using namespace cp_vsd;

constexpr int THREADS = TILE, WAVE = 64;

__global__ void __launch_bounds__(THREADS) vsd_counts_kernel(const uint32_t* __restrict__ planes, const int32_t* __restrict__ records, int nplanes,
                                                            int H, int W, const float* __restrict__ depth, const double* __restrict__ cams,
                                                            int images, const int32_t* __restrict__ pairs, const double* __restrict__ diameters,
                                                            double delta, const double* __restrict__ taus, int ntau, int split,
                                                            int32_t* __restrict__ counts) {
    __shared__ int32_t s_counts[2 + MAX_TAUS];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1);
    const size_t pair = blockIdx.x / (unsigned)split;
    const int part = (int)(blockIdx.x % (unsigned)split);
    const double diameter = diameters[pair];
    Pair p;
    // block-uniform exits: nothing below them has been synchronised yet
    if (!pair_setup(pairs + 4 * pair, records, nplanes, images, H, W, diameter, p)) return;
    const int total = p.bh * p.bw;   // <= 2^28
    if (part * TILE >= total) return;
    if (tid < 2 + MAX_TAUS) s_counts[tid] = 0;
    __syncthreads();

    const size_t hw = (size_t)H * (size_t)W;
    const Camera cam = {cams[4 * p.image], cams[4 * p.image + 1], cams[4 * p.image + 2], cams[4 * p.image + 3]};
    const uint32_t* __restrict__ pe = planes + (size_t)p.plane_e * hw;
    const uint32_t* __restrict__ pg = planes + (size_t)p.plane_g * hw;
    const float* __restrict__ pt = depth + (size_t)p.image * hw;

    int n_uni = 0, n_inter = 0, n_tau = 0;   // n_uni, n_inter: the same in every lane of a wave; n_tau: lane k holds tau k's count
    for (long long first = (long long)part * TILE; first < total; first += (long long)split * TILE) {
        const long long s = first + tid;
        Pixel r = {false, false, 0u};
        if (s < total) {
            const int di = (int)((unsigned)s / (unsigned)p.bw), i = p.i0 + di, j = p.j0 + ((int)s - di * p.bw);   // i < H, j < W (pair_setup)
            const size_t at = (size_t)i * W + j;
            r = pixel(pe[at], pg[at], pt[at], i, j, cam, delta, diameter, taus, ntau);
        }
        const unsigned long long b_uni = __ballot(r.uni);
        if (b_uni == 0) continue;   // wave-uniform
        n_uni += __popcll(b_uni);
        const unsigned long long b_inter = __ballot(r.inter);
        if (b_inter == 0) continue;
        n_inter += __popcll(b_inter);
        for (int k = 0; k < ntau; ++k) {
            const int c = __popcll(__ballot((r.reached >> k) & 1u));
            if (lane == k) n_tau += c;
        }
    }
    if (lane == 0 && n_uni != 0) {
        atomicAdd(&s_counts[0], n_uni);
        atomicAdd(&s_counts[1], n_inter);
    }
    if (lane < ntau && n_tau != 0) atomicAdd(&s_counts[2 + lane], n_tau);
    __syncthreads();
    if (tid < 2 + ntau) {
        const int32_t v = s_counts[tid];
        if (v != 0) atomicAdd(counts + pair * (size_t)(2 + ntau) + tid, v);
    }
}

}  // namespace

extern "C" int cp_vsd_tile(void) { return TILE; }

extern "C" int cp_vsd_counts_i32(const uint32_t* planes, const int32_t* records, int nplanes, int H, int W, const float* depth, const double* cams,
                                 int images, const int32_t* pairs, const double* diameters, int npairs, double delta, const double* taus, int ntau,
                                 int split, int32_t* counts, void* stream) {
    CP_REQUIRE(planes && records && depth && cams && pairs && diameters && taus && counts, "cp_vsd_counts_i32: null pointer");
    CP_REQUIRE(ntau >= 1 && ntau <= MAX_TAUS, "cp_vsd_counts_i32: ntau must lie in [1, %d] (got %d)", MAX_TAUS, ntau);
    CP_REQUIRE(nplanes >= 1 && images >= 1 && npairs >= 1, "cp_vsd_counts_i32: nplanes, images and npairs must be positive (got %d, %d, %d)", nplanes,
               images, npairs);
    CP_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "cp_vsd_counts_i32: H and W must lie in [1, %d] (got %d x %d)", MAX_SIDE, H, W);
    CP_REQUIRE((long long)nplanes < (1ll << 31) / RECORD, "cp_vsd_counts_i32: nplanes %d is too large", nplanes);
    CP_REQUIRE(split >= 1 && split <= MAX_SPLIT, "cp_vsd_counts_i32: split must lie in [1, %d] blocks per pair (got %d)", MAX_SPLIT, split);
    CP_REQUIRE((long long)npairs * split <= 0x7fffffffLL, "cp_vsd_counts_i32: npairs %d x split %d is above 2^31 - 1 blocks; split the call", npairs,
               split);
    CP_REQUIRE(delta >= 0.0 && delta <= 1.7976931348623157e308, "cp_vsd_counts_i32: delta must be finite and not negative (got %g)", delta);
    CP_REQUIRE(((uintptr_t)planes & 3) == 0 && ((uintptr_t)records & 3) == 0 && ((uintptr_t)depth & 3) == 0 && ((uintptr_t)pairs & 3) == 0 &&
                   ((uintptr_t)counts & 3) == 0,
               "cp_vsd_counts_i32: planes, records, depth, pairs and counts must be 4-byte aligned");
    CP_REQUIRE(((uintptr_t)cams & 7) == 0 && ((uintptr_t)diameters & 7) == 0 && ((uintptr_t)taus & 7) == 0,
               "cp_vsd_counts_i32: cams, diameters and taus must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)npairs * (size_t)(2 + ntau) * sizeof(int32_t), st) != hipSuccess) {
        cp::set_error("cp_vsd_counts_i32: clearing the counts failed: %s", hipGetErrorString(hipGetLastError()));
        return CP_ERR_LAUNCH;
    }
    CP_LAUNCH(vsd_counts_kernel, dim3((unsigned)((long long)npairs * split)), dim3(THREADS), 0, st, planes, records, nplanes, H, W, depth, cams, images,
              pairs, diameters, delta, taus, ntau, split, counts);
    return cp::check_launch("cp_vsd_counts_i32");
}
