// What the mask renderer (masks.hip, mask_math.h) leaves behind for the kernels that read its output (depth_icp.hip, mask_contour.hip, vsd.hip,
// pose_verify.hip): one uint32 depth plane per rendered instance and one int32 record per instance.  Stated once, as __host__ __device__ code.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PLANE_HD __host__ __device__ inline
#else
#define PLANE_HD inline
#endif

namespace cp_plane {

constexpr int RECORD = 11;                // int32 words of an instance's record (mask_math.h rule 8 names them)
constexpr int R_BOX_OBJ = 2;              // bbox_obj: x, y, w, h of the instance's pixels, or a negative w or h for "none"
constexpr uint32_t EMPTY = 0xffffffffu;   // a depth plane's "nothing hit": above the bit pattern of every positive float, +inf included
constexpr int MAX_SIDE = 16384;           // H, W: the renderer's samples stay below 2^22 + 256

struct Camera {
    double fx, fy, cx, cy;
};

struct Box {
    int x0, y0, x1, y1;   // closed, inside the image
};

// the fp32 depth a plane word other than EMPTY holds
PLANE_HD float depth_of(uint32_t bits) {
    float z;
    __builtin_memcpy(&z, &bits, sizeof z);
    return z;
}

// a record's bbox_obj clipped to the image less `margin` pixels on every side: false when nothing is left of it
PLANE_HD bool clipped_box(const int32_t* rec, int H, int W, int margin, Box& b) {
    const int64_t x = rec[R_BOX_OBJ], y = rec[R_BOX_OBJ + 1], w = rec[R_BOX_OBJ + 2], h = rec[R_BOX_OBJ + 3];
    if (w < 0 || h < 0) return false;
    const int64_t lo = margin, xh = W - 1 - margin, yh = H - 1 - margin;
    const int64_t x0 = x < lo ? lo : x, y0 = y < lo ? lo : y;
    const int64_t x1 = x + w > xh ? xh : x + w, y1 = y + h > yh ? yh : y + h;
    if (x0 > x1 || y0 > y1) return false;
    b.x0 = (int)x0, b.y0 = (int)y0, b.x1 = (int)x1, b.y1 = (int)y1;
    return true;
}

}  // namespace cp_plane
