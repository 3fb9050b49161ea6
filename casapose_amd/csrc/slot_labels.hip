// Synthetic scenes with several instances of one object (data_handler/device_scenes.py): cp_render_scenes_f32 casts the rays over
// objects * instances SLOTS, slot (o * I + r) being instance r of object o, and labels every pixel with the 1-based slot of the nearest hit --
// the id convention of pose_estimation/instance_voting.py.  This pass turns that slot map into what a training batch carries:
//   label         uint8 [b][pixels]              the class, (slot - 1) / I + 1, 0 on background
//   instance_seg  uint8 [b][pixels]              the instance, (slot - 1) % I, 0 on background
//   target_seg    fp32  [b][pixels][objects+1]   the one-hot of the class
//   counts        int32 [b][objects]             pixels of each class (pixel_gt_count: summed over the object's instances)
// A slot above objects * I counts as background.  HBM-bound, one pixel per lane; the counts go through per-block LDS counters and integer
// atomics only, so every output is the same bits on every run.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int MAX_OBJECTS = 254;

__global__ __launch_bounds__(THREADS) void slot_labels_kernel(const uint8_t* __restrict__ slots, int objects, int instances, int ppi,
                                                              uint8_t* __restrict__ label, uint8_t* __restrict__ instance_seg,
                                                              float* __restrict__ target_seg, int* __restrict__ counts) {
    __shared__ int scnt[MAX_OBJECTS];
    const int b = blockIdx.y, K = objects + 1;
    for (int i = threadIdx.x; i < objects; i += blockDim.x) scnt[i] = 0;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ppi; i += gridDim.x * blockDim.x) {
        const size_t p = (size_t)b * ppi + i;
        const int s = slots[p];
        const bool on = s > 0 && s <= objects * instances;
        const int cls = on ? (s - 1) / instances + 1 : 0;
        label[p] = (uint8_t)cls;
        instance_seg[p] = (uint8_t)(on ? (s - 1) % instances : 0);
        float* row = target_seg + p * (size_t)K;
        for (int c = 0; c < K; ++c) row[c] = c == cls ? 1.f : 0.f;
        if (on) atomicAdd(&scnt[cls - 1], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < objects; i += blockDim.x)
        if (scnt[i]) atomicAdd(&counts[b * objects + i], scnt[i]);
}

}  // namespace

extern "C" int cp_slot_labels_u8(const uint8_t* slots, int batch, int objects, int instances, long long pixels_per_image, uint8_t* label,
                                 uint8_t* instance_seg, float* target_seg, int32_t* counts, void* stream) {
    CP_REQUIRE(slots && label && instance_seg && target_seg && counts, "cp_slot_labels_u8: null pointer");
    CP_REQUIRE(batch >= 1 && batch <= 65535 && objects >= 1 && instances >= 1 && instances <= 16 && objects * instances <= MAX_OBJECTS,
               "cp_slot_labels_u8: batch in 1..65535, instances in 1..16, objects * instances in 1..254 (got %d, %d, %d)", batch, objects, instances);
    CP_REQUIRE(pixels_per_image >= 1 && pixels_per_image < (1LL << 31), "cp_slot_labels_u8: pixels_per_image must lie in [1, 2^31)");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(int) * (size_t)batch * objects, st) != hipSuccess) return cp::check_launch("cp_slot_labels_u8 memset");
    long long gx = (pixels_per_image + THREADS - 1) / THREADS;
    if (gx > 1024) gx = 1024;
    CP_LAUNCH(slot_labels_kernel, dim3((unsigned)gx, batch), dim3(THREADS), 0, st, slots, objects, instances, (int)pixels_per_image, label, instance_seg,
              target_seg, counts);
    return cp::check_launch("cp_slot_labels_u8");
}
