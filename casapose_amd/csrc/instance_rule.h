// The reference's rule for several instances of one object (compute_vertex_hcoords_batch_v3, utils/image_utils.py:17-63): a pixel takes the
// instance whose centre is nearest.  One copy, shared by the stand-alone target field (loss_functional.hip) and the fused training loss
// (loss_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

// keypoints [b][objects][instances][kp][2] (y,x); kobj points at the object's [instances][kp][2].  Instance in [0, instances) whose centre
// (keypoint 0) is nearest to the pixel centre; first minimum wins (tf.argmin).  A caller with a count per object passes the count: entries
// at and behind it are not read.
__device__ __forceinline__ int nearest_instance(const float* __restrict__ kobj, int instances, int kp, float cy, float cx) {
    int best = 0;
    float bd = 3.4e38f;
    for (int i = 0; i < instances; ++i) {
        const float dy = cy - kobj[(size_t)i * kp * 2], dx = cx - kobj[(size_t)i * kp * 2 + 1];
        const float d = sqrtf(dy * dy + dx * dx);
        if (d < bd) { bd = d; best = i; }
    }
    return best;
}
