// Network input from decoded uint8 frames: the per-pixel half of ImageOnlyDataset.load_images (casapose/data_handler/image_only_dataset.py
// :36-49 of the reference; casapose_amd/data_handler/image_only_dataset.py here).  One channel is replicated to three, a fourth is dropped,
// and every value becomes ((float)v / 255 - norm0) / norm1 with IEEE fp32 divisions, bit for bit what TF's true division of a uint8 tensor
// and NumPy's float32 formula give.
//
// Pure streaming, no LDS and no MFMA: a bs-16 480 x 640 RGB batch is 14.7 MB read and 59 MB written, so the stores are what must be wide.
// The output is addressed in float4s (lane-contiguous dwordx4 stores); each float4 reads the one or two source words that hold its bytes.
// A frame layout that does not tile into whole float4 rows (odd widths with padded rows, an unaligned pointer) takes a scalar path instead.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr int UNROLL = 4;   // float4s per thread and grid-stride step: four loads in flight before the first store

__device__ __forceinline__ float normalise(uint32_t v, float n0, float n1) { return ((float)v / 255.0f - n0) / n1; }

// Byte offset, inside the row's source bytes, of output element e of the row (pixel e / 3, channel e % 3; one channel is replicated)
template <int C>
__device__ __forceinline__ uint32_t src_byte(uint32_t e) {
    return C == 1 ? e / 3u : (e / 3u) * C + e % 3u;
}

// Vector path.  The frames are `rows` rows of `row_q` output float4s each: the whole batch as one row when the source is dense, else one row
// per image row.  C = 3: output float4 q of a row is source word q.  C = 1 / 4: three float4s are one group of four pixels (4 or 16 source
// bytes); float4 q reads word q / 3 (C = 1) or words 4 (q / 3) + q % 3 and the next (C = 4).
template <int C>
__global__ void __launch_bounds__(THREADS) frames_vec_kernel(const uint8_t* __restrict__ src, uint32_t rows, uint32_t row_q, uint32_t h,
                                                            long long pitch, long long stride, float n0, float n1, float4* __restrict__ out) {
    const uint32_t total = rows * row_q;
    const uint32_t step = gridDim.x * THREADS;
    for (uint32_t q0 = blockIdx.x * THREADS + threadIdx.x; q0 < total; q0 += UNROLL * step) {
        uint64_t win[UNROLL];
        uint32_t shift0[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t q = q0 + u * step;
            win[u] = 0;
            shift0[u] = 0;
            if (q < total) {
                const uint32_t r = rows == 1 ? 0u : q / row_q, ql = q - r * row_q;
                const uint8_t* row = src + (long long)(r / h) * stride + (long long)(r % h) * pitch;
                if (C == 3) {
                    win[u] = *reinterpret_cast<const uint32_t*>(row + 4ull * ql);
                } else {
                    const uint32_t first = src_byte<C>(4u * ql) & ~3u;   // the word holding the float4's first byte
                    const uint32_t* w = reinterpret_cast<const uint32_t*>(row + first);
                    win[u] = (uint64_t)w[0];
                    if (C == 4) win[u] |= (uint64_t)w[1] << 32;          // a float4 spans two pixels: at most 8 bytes from `first` on
                    shift0[u] = first;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const uint32_t q = q0 + u * step;
            if (q >= total) break;
            const uint32_t ql = rows == 1 ? q : q % row_q;
            float4 o;
            if (C == 3) {
                const uint32_t v = (uint32_t)win[u];
                o = make_float4(normalise(v & 255u, n0, n1), normalise((v >> 8) & 255u, n0, n1), normalise((v >> 16) & 255u, n0, n1),
                                normalise(v >> 24, n0, n1));
            } else {
                float f[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) f[j] = normalise((uint32_t)(win[u] >> (8u * (src_byte<C>(4u * ql + j) - shift0[u]))) & 255u, n0, n1);
                o = make_float4(f[0], f[1], f[2], f[3]);
            }
            out[q] = o;
        }
    }
}

// Scalar path: one output value per thread and step (any pitch, stride, width or alignment)
template <int C>
__global__ void __launch_bounds__(THREADS) frames_scalar_kernel(const uint8_t* __restrict__ src, uint32_t hw, uint32_t w, uint32_t total,
                                                               long long pitch, long long stride, float n0, float n1, float* __restrict__ out) {
    for (uint32_t e = blockIdx.x * THREADS + threadIdx.x; e < total; e += gridDim.x * THREADS) {
        const uint32_t p = e / 3u, c = e - 3u * p, b = p / hw, yx = p - b * hw, y = yx / w, x = yx - y * w;
        out[e] = normalise(src[(long long)b * stride + (long long)y * pitch + (long long)x * C + (C == 1 ? 0u : c)], n0, n1);
    }
}

// As many blocks as are resident at once (occupancy x 256 CUs) and no more; fewer when the work does not fill them
template <typename K>
int grid_for(K kernel, int& per_cu, long long blocks) {
    if (per_cu == 0) {
        int n = 0;
        per_cu = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, THREADS, 0) == hipSuccess && n > 0 ? n : 8;
    }
    const long long resident = 256LL * per_cu;
    return (int)(blocks < 1 ? 1 : (blocks > resident ? resident : blocks));
}

template <int C>
int launch(const uint8_t* src, int batch, int h, int w, long long pitch, long long stride, float n0, float n1, float* out, hipStream_t st) {
    const bool dense = pitch == (long long)w * C && stride == (long long)h * pitch;
    // rows of whole float4s (C = 1 / 4: of whole four-pixel groups), every row start 4-byte aligned in the source, 16-byte aligned output
    const long long row_px = dense ? (long long)batch * h * w : w;
    const long long rows = dense ? 1 : (long long)batch * h;
    const bool aligned = ((uintptr_t)src & 3) == 0 && (dense || (pitch % 4 == 0 && stride % 4 == 0)) && ((uintptr_t)out & 15) == 0;
    if (aligned && row_px % 4 == 0) {
        const uint32_t row_q = (uint32_t)(row_px * 3 / 4);
        const long long quads = rows * row_q;
        static int per_cu = 0;   // one per instantiation (benign race: every thread computes the same value)
        auto k = frames_vec_kernel<C>;
        CP_LAUNCH(k, dim3(grid_for(k, per_cu, (quads + THREADS * UNROLL - 1) / (THREADS * UNROLL))), dim3(THREADS), 0, st, src, (uint32_t)rows, row_q,
                  (uint32_t)h, pitch, stride, n0, n1, reinterpret_cast<float4*>(out));
    } else {
        const long long total = (long long)batch * h * w * 3;
        static int per_cu = 0;
        auto k = frames_scalar_kernel<C>;
        CP_LAUNCH(k, dim3(grid_for(k, per_cu, (total + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, src, (uint32_t)h * (uint32_t)w, (uint32_t)w,
                  (uint32_t)total, pitch, stride, n0, n1, out);
    }
    return cp::check_launch("cp_frames_to_input_f32");
}

}  // namespace

extern "C" int cp_frames_to_input_f32(const uint8_t* src, int batch, int h, int w, int channels, long long src_pitch, long long src_stride,
                                      float norm0, float norm1, float* out, void* stream) {
    CP_REQUIRE(src && out, "cp_frames_to_input_f32: null pointer");
    CP_REQUIRE(channels == 1 || channels == 3 || channels == 4, "cp_frames_to_input_f32: channels must be 1, 3 or 4 (got %d)", channels);
    CP_REQUIRE(batch > 0 && h > 0 && w > 0, "cp_frames_to_input_f32: batch, h and w must be positive (got %d, %d, %d)", batch, h, w);
    CP_REQUIRE((long long)batch * h * w <= (1LL << 30), "cp_frames_to_input_f32: more than 2^30 pixels in one call");
    CP_REQUIRE(src_pitch >= (long long)w * channels, "cp_frames_to_input_f32: row pitch %lld is smaller than w * channels = %lld", src_pitch,
               (long long)w * channels);
    CP_REQUIRE(src_stride >= (long long)h * src_pitch, "cp_frames_to_input_f32: image stride %lld is smaller than h * pitch = %lld", src_stride,
               (long long)h * src_pitch);
    hipStream_t st = (hipStream_t)stream;
    if (channels == 1) return launch<1>(src, batch, h, w, src_pitch, src_stride, norm0, norm1, out, st);
    if (channels == 3) return launch<3>(src, batch, h, w, src_pitch, src_stride, norm0, norm1, out, st);
    return launch<4>(src, batch, h, w, src_pitch, src_stride, norm0, norm1, out, st);
}
