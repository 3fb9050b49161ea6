// Segmentation masks of BOP frames on the device: a z-buffered triangle rasteriser for a batch of frames, and the host twin.  The arithmetic
// is mask_math.h; this file is the schedule.
//
// The caller's workspace holds one uint32 depth plane per (frame, instance), cleared to EMPTY.  Four launches on the caller's stream:
//   clear_records_kernel   one thread per (frame, instance) record.
//   raster_kernel          grid (256-triangle chunks, instances_max, frames), 256 threads.  A lane projects one triangle (mask_math.h
//                          setup_triangle).  When the triangle's clipped bounding box holds at most LANE_SAMPLES samples the lane walks them
//                          itself; the triangles above that are found with a ballot and walked one after the other by all 64 lanes of the wave,
//                          sample s of the box going to lane s % 64, so that a quad filling the frame is 64-way parallel per triangle and never
//                          one lane's loop.  A covered sample is one 32-bit integer atomicMin of the fp32 depth's bit pattern on the
//                          instance's plane.  Dropped triangles are counted in LDS and added to the record once per block.
//   resolve_kernel         grid (256-pixel chunks, frames), a thread per pixel: the arg-min over the frame's planes (strict <, so the lowest
//                          instance index wins a tie), the label byte, and per instance two counts and two boxes reduced in LDS with integer
//                          atomics, then one global integer atomic per block and record word that changed.
//   finish_records_kernel  (xmin, ymin, xmax, ymax) -> (x, y, w, h), or -1 four times.
// Integer minima, maxima and sums do not depend on the order they are applied in: two calls with the same inputs give the same bytes.
// Every index read from device memory (instance count, object index, label, vertex and face counts, face indices) is range-checked before it
// addresses anything.  cp_render_masks_host_u8 runs mask_math.h's serial loop on host pointers and launches nothing.
#include "common.h"
#include "mask_math.h"

namespace {

using namespace cp_mask;

constexpr int THREADS = 256, WAVE = 64;
constexpr int LDS_WORDS = 10;   // per instance in resolve_kernel: the record without its dropped count

__global__ void __launch_bounds__(THREADS) clear_records_kernel(int32_t* __restrict__ records, int count) {
    const int r = blockIdx.x * THREADS + threadIdx.x;
    if (r < count) record_clear(records + (size_t)r * RECORD);
}

__global__ void __launch_bounds__(THREADS) finish_records_kernel(int32_t* __restrict__ records, int count) {
    const int r = blockIdx.x * THREADS + threadIdx.x;
    if (r < count) record_finish(records + (size_t)r * RECORD);
}

__device__ __forceinline__ void walk_samples(const Tri& t, long long first, long long step, int64_t S, double near, double far, int W,
                                             uint32_t* __restrict__ plane) {
    const int bw = t.j1 - t.j0 + 1;
    const long long total = (long long)bw * (t.i1 - t.i0 + 1);
    for (long long s = first; s < total; s += step) {
        const int di = (int)(s / bw), i = t.i0 + di, j = t.j0 + (int)(s - (long long)di * bw);   // i <= i1 < H, j <= j1 < W (setup_triangle)
        uint32_t bits;
        if (sample_depth(t, i, j, S, near, far, bits)) atomicMin(plane + (size_t)i * W + j, bits);
    }
}

__global__ void __launch_bounds__(THREADS) raster_kernel(const float* __restrict__ verts, const int32_t* __restrict__ vert_counts, int Vmax,
                                                        const int32_t* __restrict__ faces, const int32_t* __restrict__ face_counts, int Tmax,
                                                        int objects, const double* __restrict__ cams, const int32_t* __restrict__ inst_counts,
                                                        const int32_t* __restrict__ inst_obj, const int32_t* __restrict__ inst_label,
                                                        const double* __restrict__ poses, int instances_max, int H, int W, double near, double far,
                                                        int64_t S, int32_t* __restrict__ records, uint32_t* __restrict__ planes) {
    __shared__ int s_dropped;
    const int f = blockIdx.z, k = blockIdx.y, tid = threadIdx.x;
    // block-uniform exits: nothing below them has been synchronised yet
    if (k >= clamp_count(inst_counts[f], instances_max)) return;
    const size_t slot = (size_t)f * instances_max + k;
    const int obj = inst_obj[slot];
    if (!instance_valid(obj, inst_label[slot], objects)) return;
    const int vcount = clamp_count(vert_counts[obj], Vmax), tcount = clamp_count(face_counts[obj], Tmax);
    const int first = blockIdx.x * THREADS;
    if (first >= tcount) return;
    if (tid == 0) s_dropped = 0;
    __syncthreads();

    const float* ov = verts + (size_t)obj * Vmax * 3;
    const int32_t* of = faces + (size_t)obj * Tmax * 3;
    const double* P = poses + slot * 12;
    const Camera cam = {cams[4 * f], cams[4 * f + 1], cams[4 * f + 2], cams[4 * f + 3]};
    uint32_t* plane = planes + slot * ((size_t)H * W);

    Tri t;
    const int tri = first + tid;
    const int st = tri < tcount ? setup_triangle(ov, vcount, of + 3 * (size_t)tri, P, cam, near, S, H, W, t) : TRI_EMPTY;
    const long long samples = st == TRI_DRAW ? (long long)(t.j1 - t.j0 + 1) * (t.i1 - t.i0 + 1) : 0;
    if (samples > 0 && samples <= LANE_SAMPLES) walk_samples(t, 0, 1, S, near, far, W, plane);

    // the large triangles of this wave, one after the other, by all of its lanes (`large` is the same in every lane)
    unsigned long long large = __ballot(samples > LANE_SAMPLES);
    const int lane = tid & (WAVE - 1), wave_first = first + (tid - lane);
    while (large) {
        const int src = __ffsll((long long)large) - 1;
        large &= large - 1;
        Tri u;   // lane src's triangle again: it drew, so its indices are in range and every lane gets TRI_DRAW
        if (setup_triangle(ov, vcount, of + 3 * (size_t)(wave_first + src), P, cam, near, S, H, W, u) == TRI_DRAW)
            walk_samples(u, lane, WAVE, S, near, far, W, plane);
    }

    if (st == TRI_DROPPED) atomicAdd(&s_dropped, 1);
    __syncthreads();
    if (tid == 0 && s_dropped != 0) atomicAdd(records + slot * RECORD + R_DROPPED, s_dropped);
}

__global__ void __launch_bounds__(THREADS) resolve_kernel(const int32_t* __restrict__ inst_counts, const int32_t* __restrict__ inst_label,
                                                         int instances_max, int H, int W, const uint32_t* __restrict__ planes,
                                                         uint8_t* __restrict__ label, int32_t* __restrict__ records) {
    extern __shared__ int32_t s_rec[];   // [n][LDS_WORDS]: all, visib, box_obj (min, min, max, max), box_visib
    const int f = blockIdx.y, tid = threadIdx.x, hw = H * W;   // hw <= 2^28
    const int n = clamp_count(inst_counts[f], instances_max);
    for (int w = tid; w < n * LDS_WORDS; w += THREADS) {
        const int e = w % LDS_WORDS;
        s_rec[w] = e < 2 ? 0 : (((e - 2) & 3) < 2 ? BOX_NONE : -1);
    }
    __syncthreads();
    const int p = blockIdx.x * THREADS + tid;
    if (p < hw) {
        const int i = p / W, j = p - i * W;
        const uint32_t* fplanes = planes + (size_t)f * instances_max * (size_t)hw;
        uint32_t best = EMPTY;
        int winner = -1;
        for (int k = 0; k < n; ++k) {
            const uint32_t b = fplanes[(size_t)k * hw + p];
            if (b == EMPTY) continue;
            int32_t* r = s_rec + k * LDS_WORDS;
            atomicAdd(r + 0, 1);
            atomicMin(r + 2, j);
            atomicMin(r + 3, i);
            atomicMax(r + 4, j);
            atomicMax(r + 5, i);
            if (b < best) best = b, winner = k;
        }
        int lab = 0;
        if (winner >= 0) {
            int32_t* r = s_rec + winner * LDS_WORDS;
            atomicAdd(r + 1, 1);
            atomicMin(r + 6, j);
            atomicMin(r + 7, i);
            atomicMax(r + 8, j);
            atomicMax(r + 9, i);
            lab = inst_label[(size_t)f * instances_max + winner] & 255;   // a winner is a valid instance: its label is in [0, 255]
        }
        label[(size_t)f * hw + p] = (uint8_t)lab;
    }
    __syncthreads();
    for (int w = tid; w < n * LDS_WORDS; w += THREADS) {
        const int k = w / LDS_WORDS, e = w - k * LDS_WORDS;
        if (s_rec[k * LDS_WORDS + (e == 1 || e >= 6 ? 1 : 0)] == 0) continue;   // this block added nothing to the word's pixel set
        int32_t* g = records + ((size_t)f * instances_max + k) * RECORD + e;   // record words 0-9 are the LDS words in this order
        const int32_t v = s_rec[w];
        if (e < 2)
            atomicAdd(g, v);
        else if (((e - 2) & 3) < 2)
            atomicMin(g, v);
        else
            atomicMax(g, v);
    }
}

int check_arguments(const char* fn, const void* verts, const void* vert_counts, int Vmax, const void* faces, const void* face_counts, int Tmax,
                    int objects, const void* cams, const void* inst_counts, const void* inst_obj, const void* inst_label, const void* poses,
                    int frames, int instances_max, int H, int W, double near, double far, double sample_offset, const void* label,
                    const void* records, const void* workspace, size_t workspace_bytes) {
    CP_REQUIRE(verts && vert_counts && faces && face_counts && cams && inst_counts && inst_obj && inst_label && poses && label && records && workspace,
               "%s: null pointer", fn);
    CP_REQUIRE(objects >= 1 && Vmax >= 1 && Tmax >= 1, "%s: objects, Vmax and Tmax must be positive (got %d, %d, %d)", fn, objects, Vmax, Tmax);
    CP_REQUIRE((long long)objects * Vmax < (1ll << 31) / 3 && (long long)objects * Tmax < (1ll << 31) / 3,
               "%s: objects * Vmax and objects * Tmax must stay below 2^31 / 3", fn);
    CP_REQUIRE(frames >= 1 && frames <= 65535, "%s: frames must lie in [1, 65535] (got %d)", fn, frames);
    CP_REQUIRE(instances_max >= 1 && instances_max <= MAX_INSTANCES, "%s: instances_max must lie in [1, %d] (got %d)", fn, MAX_INSTANCES, instances_max);
    CP_REQUIRE(H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "%s: H and W must lie in [1, %d] (got %d x %d)", fn, MAX_SIDE, H, W);
    CP_REQUIRE((long long)frames * instances_max < (1ll << 31) / RECORD, "%s: frames * instances_max is too large (%d x %d)", fn, frames, instances_max);
    CP_REQUIRE(near > 0.0 && far >= near, "%s: need 0 < near <= far (got %g, %g): depths are compared as positive bit patterns", fn, near, far);
    CP_REQUIRE(sample_offset >= 0.0 && sample_offset <= 1.0, "%s: sample_offset must lie in [0, 1] (got %g)", fn, sample_offset);
    CP_REQUIRE(workspace_bytes >= cp_mask::workspace_bytes(frames, instances_max, H, W), "%s: the workspace has %zu bytes, %zu are needed", fn,
               workspace_bytes, cp_mask::workspace_bytes(frames, instances_max, H, W));
    CP_REQUIRE(((uintptr_t)verts & 3) == 0 && ((uintptr_t)faces & 3) == 0 && ((uintptr_t)vert_counts & 3) == 0 && ((uintptr_t)face_counts & 3) == 0 &&
                   ((uintptr_t)inst_counts & 3) == 0 && ((uintptr_t)inst_obj & 3) == 0 && ((uintptr_t)inst_label & 3) == 0 &&
                   ((uintptr_t)records & 3) == 0 && ((uintptr_t)workspace & 3) == 0,
               "%s: the fp32 and int32 arrays and the workspace must be 4-byte aligned", fn);
    CP_REQUIRE(((uintptr_t)cams & 7) == 0 && ((uintptr_t)poses & 7) == 0, "%s: cams and poses must be 8-byte aligned", fn);
    return CP_OK;
}

}  // namespace

extern "C" size_t cp_render_masks_workspace_bytes(int frames, int instances_max, int H, int W) {
    if (frames < 1 || frames > 65535 || instances_max < 1 || instances_max > MAX_INSTANCES || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return 0;
    return cp_mask::workspace_bytes(frames, instances_max, H, W);
}

extern "C" int cp_render_masks_u8(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts, int Tmax,
                                  int objects, const double* cams, const int32_t* inst_counts, const int32_t* inst_obj, const int32_t* inst_label,
                                  const double* poses, int frames, int instances_max, int H, int W, double near, double far, double sample_offset,
                                  uint8_t* label, int32_t* records, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_arguments("cp_render_masks_u8", verts, vert_counts, Vmax, faces, face_counts, Tmax, objects, cams, inst_counts, inst_obj,
                                 inst_label, poses, frames, instances_max, H, W, near, far, sample_offset, label, records, workspace, workspace_bytes))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const int slots = frames * instances_max, hw = H * W;
    if (hipMemsetAsync(workspace, 0xff, cp_mask::workspace_bytes(frames, instances_max, H, W), st) != hipSuccess) {
        cp::set_error("cp_render_masks_u8: clearing the depth planes failed: %s", hipGetErrorString(hipGetLastError()));
        return CP_ERR_LAUNCH;
    }
    const dim3 per_slot((unsigned)((slots + THREADS - 1) / THREADS));
    CP_LAUNCH(clear_records_kernel, per_slot, dim3(THREADS), 0, st, records, slots);
    if (int rc = cp::check_launch("cp_render_masks_u8 (records)")) return rc;
    const dim3 rgrid((unsigned)((Tmax + THREADS - 1) / THREADS), (unsigned)instances_max, (unsigned)frames);
    CP_LAUNCH(raster_kernel, rgrid, dim3(THREADS), 0, st, verts, vert_counts, Vmax, faces, face_counts, Tmax, objects, cams, inst_counts, inst_obj,
              inst_label, poses, instances_max, H, W, near, far, sample_origin(sample_offset), records, (uint32_t*)workspace);
    if (int rc = cp::check_launch("cp_render_masks_u8 (raster)")) return rc;
    const dim3 pgrid((unsigned)((hw + THREADS - 1) / THREADS), (unsigned)frames);
    CP_LAUNCH(resolve_kernel, pgrid, dim3(THREADS), (size_t)instances_max * LDS_WORDS * sizeof(int32_t), st, inst_counts, inst_label, instances_max, H,
              W, (const uint32_t*)workspace, label, records);
    if (int rc = cp::check_launch("cp_render_masks_u8 (resolve)")) return rc;
    CP_LAUNCH(finish_records_kernel, per_slot, dim3(THREADS), 0, st, records, slots);
    return cp::check_launch("cp_render_masks_u8 (finish)");
}

extern "C" int cp_render_masks_host_u8(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts,
                                       int Tmax, int objects, const double* cams, const int32_t* inst_counts, const int32_t* inst_obj,
                                       const int32_t* inst_label, const double* poses, int frames, int instances_max, int H, int W, double near,
                                       double far, double sample_offset, uint8_t* label, int32_t* records, void* workspace, size_t workspace_bytes) {
    if (int rc = check_arguments("cp_render_masks_host_u8", verts, vert_counts, Vmax, faces, face_counts, Tmax, objects, cams, inst_counts, inst_obj,
                                 inst_label, poses, frames, instances_max, H, W, near, far, sample_offset, label, records, workspace, workspace_bytes))
        return rc;
    render_serial(verts, vert_counts, Vmax, faces, face_counts, Tmax, objects, cams, inst_counts, inst_obj, inst_label, poses, frames, instances_max,
                  H, W, near, far, sample_offset, label, records, (uint32_t*)workspace);
    return CP_OK;
}
