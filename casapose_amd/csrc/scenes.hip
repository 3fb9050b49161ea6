// The built-in synthetic scenes on the device: per-image records -> img, label map, one-hot target and visible-pixel counts in one launch, and
// the host twin.  The arithmetic is scene_math.h (SyntheticSceneDataset._render restated in fp64); this file is the schedule.
//
// render_scenes_kernel: grid (blocks per image, images), 256 threads, a block works inside one image on 1024 consecutive pixels.
//   1. the image's record goes to LDS once, and one thread per object adds its pixel-independent terms (c, c.c - 1); every later read of the
//      record is the same address in all lanes, a broadcast;
//   2. a thread owns 4 consecutive pixels (horizontally adjacent whenever W % 4 == 0) and walks the objects once for all four;
//   3. vector path (W % 4 == 0 and 16-byte aligned outputs, decided on the host): img leaves as three 16-byte stores per thread, the four
//      labels as one dword, and the one-hot rows of the block's 1024 pixels -- 1024 K contiguous floats -- as 16-byte stores that are
//      contiguous across lanes, rebuilt from the block's labels in LDS;
//      scalar path (any other width or alignment): every pixel is guarded and stored element by element;
//   4. counts: an integer LDS histogram per block, then one integer atomic add per object and block.  Integer addition makes the result
//      independent of the order; there is no floating-point atomic, so two calls with the same records give the same bits.
// cp_render_scenes_host_f32 runs scene_math.h's serial loop on host pointers and launches nothing.
#include "common.h"
#include "scene_math.h"

namespace {

using namespace cp_scene;

constexpr int THREADS = 256, PER_THREAD = 4, BLOCK_PIXELS = THREADS * PER_THREAD;

// dynamic LDS: the record, the derived words, the histogram, the block's labels
__host__ __device__ inline size_t lds_bytes(int oc) {
    return (record_words(oc) + (size_t)DERIVED * oc) * sizeof(double) + (size_t)oc * sizeof(int32_t) + BLOCK_PIXELS;
}

__global__ void __launch_bounds__(THREADS) render_scenes_kernel(const double* __restrict__ records, int oc, int H, int W, int noise, int vec,
                                                               float* __restrict__ img, uint8_t* __restrict__ label,
                                                               float* __restrict__ target_seg, int32_t* __restrict__ counts) {
    extern __shared__ double s_rec[];
    const int words = (int)record_words(oc), K = oc + 1, tid = threadIdx.x, image = blockIdx.y, HW = H * W;
    double* s_der = s_rec + words;
    int32_t* s_hist = (int32_t*)(s_der + DERIVED * oc);
    uint8_t* s_lab = (uint8_t*)(s_hist + oc);
    const double* rec = records + (size_t)image * words;
    for (int i = tid; i < words; i += THREADS) s_rec[i] = rec[i];
    for (int o = tid; o < oc; o += THREADS) s_hist[o] = 0;
    __syncthreads();
    const int n = record_objects(s_rec, oc);
    for (int o = tid; o < n; o += THREADS) object_terms(s_rec + HEADER + OBJECT * o, s_der + DERIVED * o);
    __syncthreads();

    const int first = blockIdx.x * BLOCK_PIXELS;                 // first < HW <= 2^31 - 1 (the host check)
    const long long p0 = (long long)first + tid * PER_THREAD;   // may pass 2^31 in the last block of the largest image
    double xs[PER_THREAD], ys[PER_THREAD], rx[PER_THREAD], ry[PER_THREAD], depth[PER_THREAD], shade[PER_THREAD];
    int lab[PER_THREAD];
    bool valid[PER_THREAD];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        valid[k] = p0 + k < HW;
        const int p = valid[k] ? (int)(p0 + k) : 0;   // a pixel past the end computes pixel 0 and stores nothing
        const int y = p / W;
        pixel_ray(s_rec, y, p - y * W, xs[k], ys[k], rx[k], ry[k]);
        depth[k] = (double)INFINITY;
        shade[k] = 0.0;
        lab[k] = 0;
    }
#pragma unroll 1
    for (int o = 0; o < n; ++o) {
        const double *obj = s_rec + HEADER + OBJECT * o, *der = s_der + DERIVED * o;
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) visit_object(obj, der, o, rx[k], ry[k], depth[k], lab[k], shade[k]);
    }
    const uint64_t seed = record_seed(s_rec);
    float rgb[PER_THREAD][3];
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        float normals[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (noise) pixel_normals(seed, (uint32_t)(valid[k] ? p0 + k : 0), normals);
        shade_pixel(s_rec, lab[k], shade[k], xs[k], ys[k], noise != 0, normals, rgb[k]);
        if (valid[k] && lab[k] > 0) atomicAdd(&s_hist[lab[k] - 1], 1);   // lab <= n <= oc
    }
    const size_t base = (size_t)image * (size_t)HW;   // pixels before this image
    if (vec) {   // block-uniform; HW % 4 == 0, so the four pixels of a thread are valid together
        if (valid[0]) {
            float4* dst = reinterpret_cast<float4*>(img + (base + (size_t)p0) * 3);
            dst[0] = make_float4(rgb[0][0], rgb[0][1], rgb[0][2], rgb[1][0]);
            dst[1] = make_float4(rgb[1][1], rgb[1][2], rgb[2][0], rgb[2][1]);
            dst[2] = make_float4(rgb[2][2], rgb[3][0], rgb[3][1], rgb[3][2]);
            *reinterpret_cast<uint32_t*>(label + base + (size_t)p0) =
                (uint32_t)lab[0] | ((uint32_t)lab[1] << 8) | ((uint32_t)lab[2] << 16) | ((uint32_t)lab[3] << 24);
        }
        *reinterpret_cast<uint32_t*>(s_lab + tid * PER_THREAD) =
            (uint32_t)lab[0] | ((uint32_t)lab[1] << 8) | ((uint32_t)lab[2] << 16) | ((uint32_t)lab[3] << 24);
        __syncthreads();
        // the block's one-hot rows: (pixels in this block) * K floats, a multiple of 4, from float `first * K` of the image
        const int pixels = HW - first < BLOCK_PIXELS ? HW - first : BLOCK_PIXELS;
        const int quads = pixels / 4 * K;   // pixels % 4 == 0
        float4* dst = reinterpret_cast<float4*>(target_seg + (base + (size_t)first) * (size_t)K);
        for (int q = tid; q < quads; q += THREADS) {
            int pix = 4 * q / K, ch = 4 * q - pix * K;   // 4 q < 1024 * 255
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = (int)s_lab[pix] == ch ? 1.f : 0.f;   // pix < pixels: 4 q + e < pixels * K
                if (++ch == K) { ch = 0; ++pix; }
            }
            dst[q] = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER_THREAD; ++k) {
            if (!valid[k]) continue;
            const size_t p = base + (size_t)(p0 + k);
#pragma unroll
            for (int c = 0; c < 3; ++c) img[p * 3 + c] = rgb[k][c];
            label[p] = (uint8_t)lab[k];
            for (int c = 0; c < K; ++c) target_seg[p * (size_t)K + c] = c == lab[k] ? 1.f : 0.f;
        }
        __syncthreads();
    }
    // (both branches end behind a barrier that follows every thread's histogram update)
    for (int o = tid; o < oc; o += THREADS)
        if (s_hist[o] != 0) atomicAdd(&counts[(size_t)image * oc + o], s_hist[o]);
}

int check_arguments(const char* fn, const void* records, int b, int oc, int H, int W, const void* img, const void* label, const void* target_seg,
                    const void* counts) {
    CP_REQUIRE(records && img && label && target_seg && counts, "%s: null pointer", fn);
    CP_REQUIRE(((uintptr_t)records & 7) == 0, "%s: the records must be 8-byte aligned", fn);
    CP_REQUIRE(b >= 1 && b <= 65535, "%s: b must lie in [1, 65535] (got %d)", fn, b);
    CP_REQUIRE(oc >= 1 && oc < 255, "%s: oc must lie in [1, 254] (got %d): labels are uint8", fn, oc);
    CP_REQUIRE(H >= 1 && W >= 1, "%s: H and W must be positive (got %d x %d)", fn, H, W);
    CP_REQUIRE((long long)H * W < (1ll << 31), "%s: H * W must stay below 2^31 (got %d x %d)", fn, H, W);
    return CP_OK;
}

}  // namespace

extern "C" size_t cp_render_scenes_record_words(int oc) { return oc >= 1 && oc <= MAX_OBJECTS ? record_words(oc) : 0; }

extern "C" int cp_render_scenes_f32(const double* records, int b, int oc, int H, int W, int noise, float* img, uint8_t* label, float* target_seg,
                                    int32_t* counts, void* stream) {
    if (int rc = check_arguments("cp_render_scenes_f32", records, b, oc, H, W, img, label, target_seg, counts)) return rc;
    CP_REQUIRE(((uintptr_t)img & 3) == 0 && ((uintptr_t)target_seg & 3) == 0 && ((uintptr_t)counts & 3) == 0,
               "cp_render_scenes_f32: img, target_seg and counts must be 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, (size_t)b * oc * sizeof(int32_t), st) != hipSuccess) {
        cp::set_error("cp_render_scenes_f32: clearing counts failed: %s", hipGetErrorString(hipGetLastError()));
        return CP_ERR_LAUNCH;
    }
    const int vec = W % 4 == 0 && ((uintptr_t)img & 15) == 0 && ((uintptr_t)target_seg & 15) == 0 && ((uintptr_t)label & 3) == 0;
    const long long hw = (long long)H * W;
    const dim3 grid((unsigned)((hw + BLOCK_PIXELS - 1) / BLOCK_PIXELS), (unsigned)b);
    CP_LAUNCH(render_scenes_kernel, grid, dim3(THREADS), lds_bytes(oc), st, records, oc, H, W, noise != 0, vec, img, label, target_seg, counts);
    return cp::check_launch("cp_render_scenes_f32");
}

extern "C" int cp_render_scenes_host_f32(const double* records, int b, int oc, int H, int W, int noise, float* img, uint8_t* label,
                                         float* target_seg, int32_t* counts) {
    if (int rc = check_arguments("cp_render_scenes_host_f32", records, b, oc, H, W, img, label, target_seg, counts)) return rc;
    double der[DERIVED * MAX_OBJECTS];
    const size_t hw = (size_t)H * (size_t)W, words = record_words(oc);
    for (int i = 0; i < b; ++i)
        render_image_serial(records + (size_t)i * words, oc, H, W, noise != 0, der, img + (size_t)i * hw * 3, label + (size_t)i * hw,
                            target_seg + (size_t)i * hw * (size_t)(oc + 1), counts + (size_t)i * oc);
    return CP_OK;
}
