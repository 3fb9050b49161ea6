// Shaded pictures of meshes on the device: masks.hip's rasteriser with one 64-bit key plane per frame, a shading pass over it, and the host
// twin.  The arithmetic is shade_math.h (on top of mask_math.h and scene_math.h); this file is the schedule.
//
// The caller's workspace holds one uint64 key per pixel and frame, cleared to all ones by the call.  Two launches on the caller's stream:
//   shade_raster_kernel   masks.hip's raster_kernel schedule: grid (256-triangle chunks, instances_max, frames), 256 threads, a lane per
//                         triangle (mask_math.h setup_triangle); a triangle whose clipped bounding box holds more than LANE_SAMPLES samples is
//                         found with a ballot and walked by all 64 lanes of its wave.  A covered sample is one 64-bit integer atomicMin of
//                         depth_bits << 32 | instance << 24 | triangle on the frame's plane.  Dropped triangles are counted in LDS and added
//                         to the frame's count once per block.
//   shade_pixels_kernel   grid (1024-pixel chunks, frames), 256 threads, a thread owns 4 consecutive pixels of one frame.  The frame's record
//                         (light, ambient, diffuse, seed, crop origin) goes to LDS once per block.  Per pixel the thread decodes the key,
//                         re-projects the one winning triangle and applies shade_math.h's rules 3-8.  The four pixels are worked one after the
//                         other and staged in 16 LDS words of the thread's own (word w of thread t at [w][t]: a wave's lanes write
//                         neighbouring banks), so the loop stays rolled and the registers few.
//                         vector path (W % 4 == 0, 16-byte aligned img and depth, 4-byte aligned label; decided on the host): img leaves as
//                         three 16-byte stores per thread, the labels as one dword, the depths as one 16-byte store;
//                         scalar path (any other width or alignment): every pixel is guarded and stored element by element.
// Integer minima and sums do not depend on the order they are applied in: two calls with the same inputs give the same bytes.  Every index
// read from device memory (instance count, object index, label, vertex and face counts, face indices, and what a key decodes to) is
// range-checked before it addresses anything.  cp_render_shaded_host_f32 runs shade_math.h's serial loop on host pointers and launches nothing.
#include "common.h"
#include "shade_math.h"

namespace {

using namespace cp_shade;
using cp_mask::clamp_count;
using cp_mask::LANE_SAMPLES;
using cp_mask::TRI_DRAW;
using cp_mask::TRI_DROPPED;
using cp_mask::TRI_EMPTY;

constexpr int THREADS = 256, WAVE = 64, PER_THREAD = 4, BLOCK_PIXELS = THREADS * PER_THREAD;
constexpr int STAGE = 16;   // LDS words per thread in shade_pixels_kernel: 12 channels and 4 depths

__device__ __forceinline__ void walk_samples(const Tri& t, long long first, long long step, int64_t S, double near, double far, int W, int k, int tri,
                                             unsigned long long* __restrict__ plane) {
    const int bw = t.j1 - t.j0 + 1;
    const long long total = (long long)bw * (t.i1 - t.i0 + 1);
    for (long long s = first; s < total; s += step) {
        const int di = (int)(s / bw), i = t.i0 + di, j = t.j0 + (int)(s - (long long)di * bw);   // i <= i1 < H, j <= j1 < W (setup_triangle)
        uint32_t bits;
        if (cp_mask::sample_depth(t, i, j, S, near, far, bits)) atomicMin(plane + (size_t)i * W + j, (unsigned long long)make_key(bits, k, tri));
    }
}

__global__ void __launch_bounds__(THREADS) shade_raster_kernel(Scene sc, double far, int32_t* __restrict__ dropped,
                                                              unsigned long long* __restrict__ keys) {
    __shared__ int s_dropped;
    const int f = blockIdx.z, k = blockIdx.y, tid = threadIdx.x;
    // block-uniform exits: nothing below them has been synchronised yet
    if (k >= clamp_count(sc.inst_counts[f], sc.instances_max)) return;
    const size_t slot = (size_t)f * sc.instances_max + k;
    const int obj = sc.inst_obj[slot];
    if (!cp_mask::instance_valid(obj, sc.inst_label[slot], sc.objects)) return;
    const int vcount = clamp_count(sc.vert_counts[obj], sc.Vmax), tcount = clamp_count(sc.face_counts[obj], sc.Tmax);
    const int first = blockIdx.x * THREADS;
    if (first >= tcount) return;
    if (tid == 0) s_dropped = 0;
    __syncthreads();

    const float* ov = sc.verts + (size_t)obj * sc.Vmax * 3;
    const int32_t* of = sc.faces + (size_t)obj * sc.Tmax * 3;
    const double* P = sc.poses + slot * 12;
    const Camera cam = {sc.cams[4 * f], sc.cams[4 * f + 1], sc.cams[4 * f + 2], sc.cams[4 * f + 3]};
    unsigned long long* plane = keys + (size_t)f * ((size_t)sc.H * sc.W);

    Tri t;
    const int tri = first + tid;
    const int st = tri < tcount ? cp_mask::setup_triangle(ov, vcount, of + 3 * (size_t)tri, P, cam, sc.near, sc.S, sc.H, sc.W, t) : TRI_EMPTY;
    const long long samples = st == TRI_DRAW ? (long long)(t.j1 - t.j0 + 1) * (t.i1 - t.i0 + 1) : 0;
    if (samples > 0 && samples <= LANE_SAMPLES) walk_samples(t, 0, 1, sc.S, sc.near, far, sc.W, k, tri, plane);

    // the large triangles of this wave, one after the other, by all of its lanes (`large` is the same in every lane)
    unsigned long long large = __ballot(samples > LANE_SAMPLES);
    const int lane = tid & (WAVE - 1), wave_first = first + (tid - lane);
    while (large) {
        const int src = __ffsll((long long)large) - 1;
        large &= large - 1;
        Tri u;   // lane src's triangle again: it drew, so its indices are in range and every lane gets TRI_DRAW
        if (cp_mask::setup_triangle(ov, vcount, of + 3 * (size_t)(wave_first + src), P, cam, sc.near, sc.S, sc.H, sc.W, u) == TRI_DRAW)
            walk_samples(u, lane, WAVE, sc.S, sc.near, far, sc.W, k, wave_first + src, plane);
    }

    if (st == TRI_DROPPED) atomicAdd(&s_dropped, 1);
    __syncthreads();
    if (tid == 0 && s_dropped != 0) atomicAdd(dropped + f, s_dropped);
}

__global__ void __launch_bounds__(THREADS) shade_pixels_kernel(Scene sc, const double* __restrict__ lights, const uint8_t* __restrict__ background,
                                                              int noise, int vec, const unsigned long long* __restrict__ keys,
                                                              float* __restrict__ img, uint8_t* __restrict__ label, float* __restrict__ depth) {
    __shared__ double s_frame[FRAME_WORDS];
    __shared__ float s_stage[THREADS * STAGE];
    const int f = blockIdx.y, tid = threadIdx.x, HW = sc.H * sc.W;   // HW <= 2^28
    if (tid < FRAME_WORDS) s_frame[tid] = lights[(size_t)f * FRAME_WORDS + tid];
    __syncthreads();

    const int p0 = blockIdx.x * BLOCK_PIXELS + tid * PER_THREAD;   // < 2^28 + 1024
    const size_t base = (size_t)f * (size_t)HW;                     // pixels before this frame
    const uint8_t* bg = background ? background + base * 3 : nullptr;
    float* stage = s_stage + tid;   // word w of this thread is stage[w * THREADS]: the lanes of a wave write neighbouring banks
    uint32_t labels = 0;
#pragma unroll 1
    for (int e = 0; e < PER_THREAD; ++e) {
        const int p = p0 + e;
        if (p >= HW) break;
        const int i = p / sc.W, j = p - i * sc.W;
        float rgb[3], d;
        uint8_t lab;
        shade_pixel(sc, s_frame, f, i, j, keys[base + (size_t)p], bg, noise != 0, rgb, lab, d);
        if (vec) {
            stage[(3 * e) * THREADS] = rgb[0], stage[(3 * e + 1) * THREADS] = rgb[1], stage[(3 * e + 2) * THREADS] = rgb[2];
            stage[(12 + e) * THREADS] = d;
            labels |= (uint32_t)lab << (8 * e);
        } else {
            const size_t q = base + (size_t)p;
            img[3 * q] = rgb[0], img[3 * q + 1] = rgb[1], img[3 * q + 2] = rgb[2];
            label[q] = lab;
            if (depth) depth[q] = d;
        }
    }
    if (vec && p0 < HW) {   // HW % 4 == 0: the four pixels of a thread are inside together; the thread reads back its own words
        float w[STAGE];
#pragma unroll
        for (int k = 0; k < STAGE; ++k) w[k] = stage[k * THREADS];
        float4* dst = reinterpret_cast<float4*>(img + (base + (size_t)p0) * 3);
        dst[0] = make_float4(w[0], w[1], w[2], w[3]), dst[1] = make_float4(w[4], w[5], w[6], w[7]), dst[2] = make_float4(w[8], w[9], w[10], w[11]);
        *reinterpret_cast<uint32_t*>(label + base + (size_t)p0) = labels;
        if (depth) *reinterpret_cast<float4*>(depth + base + (size_t)p0) = make_float4(w[12], w[13], w[14], w[15]);
    }
}

int check_arguments(const char* fn, const void* verts, const void* vert_counts, int Vmax, const void* faces, const void* face_counts, int Tmax,
                    int objects, const void* cams, const void* inst_counts, const void* inst_obj, const void* inst_label, const void* poses,
                    int frames, int instances_max, int H, int W, double near, double far, double sample_offset, const void* colors,
                    const void* flat_colors, const void* lights, const void* img, const void* label, const void* depth, const void* dropped,
                    const void* workspace, size_t workspace_bytes) {
    CP_REQUIRE(verts && vert_counts && faces && face_counts && cams && inst_counts && inst_obj && inst_label && poses && flat_colors && lights && img &&
                   label && dropped && workspace,
               "%s: null pointer (only colors, background and depth may be null)", fn);
    CP_REQUIRE(objects >= 1 && Vmax >= 1 && Tmax >= 1, "%s: objects, Vmax and Tmax must be positive (got %d, %d, %d)", fn, objects, Vmax, Tmax);
    CP_REQUIRE(Tmax <= MAX_TRIANGLES, "%s: Tmax must stay at or below 2^24 (got %d): a key holds 24 bits of triangle index", fn, Tmax);
    CP_REQUIRE((long long)objects * Vmax < (1ll << 31) / 3 && (long long)objects * Tmax < (1ll << 31) / 3,
               "%s: objects * Vmax and objects * Tmax must stay below 2^31 / 3", fn);
    CP_REQUIRE(frames >= 1 && frames <= 65535, "%s: frames must lie in [1, 65535] (got %d)", fn, frames);
    CP_REQUIRE(instances_max >= 1 && instances_max <= cp_mask::MAX_INSTANCES, "%s: instances_max must lie in [1, %d] (got %d): a key holds 8 bits of it", fn,
               cp_mask::MAX_INSTANCES, instances_max);
    CP_REQUIRE(H >= 1 && W >= 1 && H <= cp_mask::MAX_SIDE && W <= cp_mask::MAX_SIDE, "%s: H and W must lie in [1, %d] (got %d x %d)", fn, cp_mask::MAX_SIDE, H, W);
    CP_REQUIRE(near > 0.0 && far >= near, "%s: need 0 < near <= far (got %g, %g): depths are compared as positive bit patterns", fn, near, far);
    CP_REQUIRE(sample_offset >= 0.0 && sample_offset <= 1.0, "%s: sample_offset must lie in [0, 1] (got %g)", fn, sample_offset);
    CP_REQUIRE(workspace_bytes >= cp_shade::workspace_bytes(frames, H, W), "%s: the workspace has %zu bytes, %zu are needed", fn, workspace_bytes,
               cp_shade::workspace_bytes(frames, H, W));
    CP_REQUIRE(((uintptr_t)verts & 3) == 0 && ((uintptr_t)faces & 3) == 0 && ((uintptr_t)vert_counts & 3) == 0 && ((uintptr_t)face_counts & 3) == 0 &&
                   ((uintptr_t)inst_counts & 3) == 0 && ((uintptr_t)inst_obj & 3) == 0 && ((uintptr_t)inst_label & 3) == 0 &&
                   ((uintptr_t)flat_colors & 3) == 0 && ((uintptr_t)img & 3) == 0 && ((uintptr_t)depth & 3) == 0 && ((uintptr_t)dropped & 3) == 0,
               "%s: the fp32 and int32 arrays must be 4-byte aligned", fn);
    CP_REQUIRE(((uintptr_t)cams & 7) == 0 && ((uintptr_t)poses & 7) == 0 && ((uintptr_t)lights & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
               "%s: cams, poses, lights and the workspace must be 8-byte aligned", fn);
    return CP_OK;
}

Scene make_scene(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts, int Tmax, int objects,
                 const double* cams, const int32_t* inst_counts, const int32_t* inst_obj, const int32_t* inst_label, const double* poses,
                 int instances_max, int H, int W, double near, double sample_offset, const uint8_t* colors, const float* flat_colors) {
    return Scene{verts, vert_counts, Vmax, faces, face_counts, Tmax, objects, cams, inst_counts, inst_obj, inst_label, poses, instances_max, H, W, near,
                 cp_mask::sample_origin(sample_offset), colors, flat_colors};
}

}  // namespace

extern "C" size_t cp_render_shaded_workspace_bytes(int frames, int H, int W) {
    if (frames < 1 || frames > 65535 || H < 1 || W < 1 || H > cp_mask::MAX_SIDE || W > cp_mask::MAX_SIDE) return 0;
    return cp_shade::workspace_bytes(frames, H, W);
}

extern "C" int cp_render_shaded_f32(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts, int Tmax,
                                    int objects, const double* cams, const int32_t* inst_counts, const int32_t* inst_obj, const int32_t* inst_label,
                                    const double* poses, int frames, int instances_max, int H, int W, double near, double far, double sample_offset,
                                    const uint8_t* colors, const float* flat_colors, const double* lights, const uint8_t* background, int noise,
                                    float* img, uint8_t* label, float* depth, int32_t* dropped, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_arguments("cp_render_shaded_f32", verts, vert_counts, Vmax, faces, face_counts, Tmax, objects, cams, inst_counts, inst_obj,
                                 inst_label, poses, frames, instances_max, H, W, near, far, sample_offset, colors, flat_colors, lights, img, label, depth,
                                 dropped, workspace, workspace_bytes))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0xff, cp_shade::workspace_bytes(frames, H, W), st) != hipSuccess ||
        hipMemsetAsync(dropped, 0, (size_t)frames * sizeof(int32_t), st) != hipSuccess) {
        cp::set_error("cp_render_shaded_f32: clearing the key planes failed: %s", hipGetErrorString(hipGetLastError()));
        return CP_ERR_LAUNCH;
    }
    const Scene sc = make_scene(verts, vert_counts, Vmax, faces, face_counts, Tmax, objects, cams, inst_counts, inst_obj, inst_label, poses, instances_max,
                                H, W, near, sample_offset, colors, flat_colors);
    const dim3 rgrid((unsigned)((Tmax + THREADS - 1) / THREADS), (unsigned)instances_max, (unsigned)frames);
    CP_LAUNCH(shade_raster_kernel, rgrid, dim3(THREADS), 0, st, sc, far, dropped, (unsigned long long*)workspace);
    if (int rc = cp::check_launch("cp_render_shaded_f32 (raster)")) return rc;
    const int vec = W % 4 == 0 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)label & 3) == 0 && ((uintptr_t)depth & 15) == 0;
    const int hw = H * W;
    const dim3 pgrid((unsigned)((hw + BLOCK_PIXELS - 1) / BLOCK_PIXELS), (unsigned)frames);
    CP_LAUNCH(shade_pixels_kernel, pgrid, dim3(THREADS), 0, st, sc, lights, background, noise != 0, vec, (const unsigned long long*)workspace, img, label,
              depth);
    return cp::check_launch("cp_render_shaded_f32 (shade)");
}

extern "C" int cp_render_shaded_host_f32(const float* verts, const int32_t* vert_counts, int Vmax, const int32_t* faces, const int32_t* face_counts,
                                         int Tmax, int objects, const double* cams, const int32_t* inst_counts, const int32_t* inst_obj,
                                         const int32_t* inst_label, const double* poses, int frames, int instances_max, int H, int W, double near,
                                         double far, double sample_offset, const uint8_t* colors, const float* flat_colors, const double* lights,
                                         const uint8_t* background, int noise, float* img, uint8_t* label, float* depth, int32_t* dropped,
                                         void* workspace, size_t workspace_bytes) {
    if (int rc = check_arguments("cp_render_shaded_host_f32", verts, vert_counts, Vmax, faces, face_counts, Tmax, objects, cams, inst_counts, inst_obj,
                                 inst_label, poses, frames, instances_max, H, W, near, far, sample_offset, colors, flat_colors, lights, img, label, depth,
                                 dropped, workspace, workspace_bytes))
        return rc;
    const Scene sc = make_scene(verts, vert_counts, Vmax, faces, face_counts, Tmax, objects, cams, inst_counts, inst_obj, inst_label, poses, instances_max,
                                H, W, near, sample_offset, colors, flat_colors);
    render_shaded_serial(sc, frames, far, lights, background, noise, img, label, depth, dropped, (uint64_t*)workspace);
    return CP_OK;
}
