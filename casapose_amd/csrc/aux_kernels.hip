// Streaming (HBM-bound) kernels around the convolutions: channel padding, max-pool,
// stand-alone x2 upsamplers, arg-max labels and the label pyramid of decoder 2.
// All of them move 16 B per lane per access and grid-stride over a capped grid.
#include "common.h"

namespace {

constexpr int THREADS = 256;

inline int grid_for(long long work_items) {
    long long b = (work_items + THREADS - 1) / THREADS;
    if (b < 1) b = 1;
    if (b > 256 * 8) b = 256 * 8;
    return (int)b;
}

__global__ void pad3to4_kernel(const float* __restrict__ src, float* __restrict__ dst, long long pixels) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < pixels; i += (long long)gridDim.x * blockDim.x) {
        const float* s = src + i * 3;
        reinterpret_cast<float4*>(dst)[i] = make_float4(s[0], s[1], s[2], 0.f);
    }
}

// one thread = one output pixel x 4 channels
__global__ void maxpool_kernel(const float* __restrict__ src, int B, int H, int W, int C, int Ho, int Wo,
                               const float* __restrict__ scale, const float* __restrict__ shift, int relu,
                               float* __restrict__ dst) {
    const int c4n = C >> 2;
    const long long total = (long long)B * Ho * Wo * c4n;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int c4 = (int)(i % c4n);
        long long pix = i / c4n;
        int ox = (int)(pix % Wo);
        long long t = pix / Wo;
        int oy = (int)(t % Ho);
        int n = (int)(t / Ho);
        // zero padding takes part in the max (resnet.py:253): start from 0 only if a tap is padded
        float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                int iy = oy * 2 - 1 + ky, ix = ox * 2 - 1 + kx;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                    v = *reinterpret_cast<const float4*>(src + (((size_t)n * H + iy) * W + ix) * C + c4 * 4);
                m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
            }
        }
        if (scale) {
            float4 s = *reinterpret_cast<const float4*>(scale + c4 * 4);
            float4 b = *reinterpret_cast<const float4*>(shift + c4 * 4);
            m.x = m.x * s.x + b.x; m.y = m.y * s.y + b.y; m.z = m.z * s.z + b.z; m.w = m.w * s.w + b.w;
        }
        if (relu) { m.x = fmaxf(m.x, 0.f); m.y = fmaxf(m.y, 0.f); m.z = fmaxf(m.z, 0.f); m.w = fmaxf(m.w, 0.f); }
        *reinterpret_cast<float4*>(dst + (size_t)pix * C + c4 * 4) = m;
    }
}

__global__ void bilinear_x2_kernel(const float* __restrict__ src, int B, int H, int W, int C, float* __restrict__ dst) {
    const int c4n = C >> 2, Ho = 2 * H, Wo = 2 * W;
    const long long total = (long long)B * Ho * Wo * c4n;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int c4 = (int)(i % c4n);
        long long pix = i / c4n;
        int ox = (int)(pix % Wo);
        long long t = pix / Wo;
        int oy = (int)(t % Ho);
        int n = (int)(t / Ho);
        int y0 = (oy >> 1) - ((oy & 1) ? 0 : 1), x0 = (ox >> 1) - ((ox & 1) ? 0 : 1);
        float fy = (oy & 1) ? 0.25f : 0.75f, fx = (ox & 1) ? 0.25f : 0.75f;
        int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        y0 = max(y0, 0); x0 = max(x0, 0);
        const float* base = src + (size_t)n * H * W * C + c4 * 4;
        float4 v00 = *reinterpret_cast<const float4*>(base + ((size_t)y0 * W + x0) * C);
        float4 v01 = *reinterpret_cast<const float4*>(base + ((size_t)y0 * W + x1) * C);
        float4 v10 = *reinterpret_cast<const float4*>(base + ((size_t)y1 * W + x0) * C);
        float4 v11 = *reinterpret_cast<const float4*>(base + ((size_t)y1 * W + x1) * C);
        float gx = 1.f - fx, gy = 1.f - fy;
        float4 o;
        o.x = (v00.x * gx + v01.x * fx) * gy + (v10.x * gx + v11.x * fx) * fy;
        o.y = (v00.y * gx + v01.y * fx) * gy + (v10.y * gx + v11.y * fx) * fy;
        o.z = (v00.z * gx + v01.z * fx) * gy + (v10.z * gx + v11.z * fx) * fy;
        o.w = (v00.w * gx + v01.w * fx) * gy + (v10.w * gx + v11.w * fx) * fy;
        *reinterpret_cast<float4*>(dst + (size_t)pix * C + c4 * 4) = o;
    }
}

__global__ void guided_x2_kernel(const float* __restrict__ src, const uint8_t* __restrict__ sel, int B, int H, int W,
                                 int C, float* __restrict__ dst) {
    const int c4n = C >> 2, Ho = 2 * H, Wo = 2 * W;
    const long long total = (long long)B * Ho * Wo * c4n;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int c4 = (int)(i % c4n);
        long long pix = i / c4n;
        int ox = (int)(pix % Wo);
        long long t = pix / Wo;
        int oy = (int)(t % Ho);
        int n = (int)(t / Ho);
        int s = sel[pix];
        int sy = (oy >> 1) + (s >> 1), sx = (ox >> 1) + (s & 1);
        float4 v = *reinterpret_cast<const float4*>(src + (((size_t)n * H + sy) * W + sx) * C + c4 * 4);
        *reinterpret_cast<float4*>(dst + (size_t)pix * C + c4 * 4) = v;
    }
}

__global__ void argmax_kernel(const float* __restrict__ x, int ld, int K, long long pixels, uint8_t* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < pixels; i += (long long)gridDim.x * blockDim.x) {
        const float* p = x + i * ld;
        float best = p[0];
        int bi = 0;
        for (int k = 1; k < K; ++k) {
            float v = p[k];
            if (v > best) { best = v; bi = k; }
        }
        out[i] = (uint8_t)bi;
    }
}

// same result with 16-byte loads: the K (<= 12) logits of a pixel are the first floats of its 16-byte aligned record, so three
// float4 loads replace nine strided scalar loads (the record is touched once either way; this only cuts the request count)
template <int NV>
__global__ void argmax_vec_kernel(const float* __restrict__ x, int ld, int K, long long pixels, uint8_t* __restrict__ out) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < pixels; i += (long long)gridDim.x * blockDim.x) {
        const float4* p = reinterpret_cast<const float4*>(x + i * ld);
        float v[NV * 4];
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            const float4 t = p[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
        float best = v[0];
        int bi = 0;
#pragma unroll
        for (int k = 1; k < NV * 4; ++k)
            if (k < K && v[k] > best) { best = v[k]; bi = k; }
        out[i] = (uint8_t)bi;
    }
}

// The label-derived maps of decoder 2, all levels in one launch.  Level l + 1 is level l [::2, ::2] (HalfSize,
// _normalization_layers.py:294-299), so pixel (y, x) of level l is pixel (y << l, x << l) of the level-0 map and every map of every level is
// read from level 0 alone:
//   labels[l]  the level-l label map (l >= 1)
//   pnorm[l]   9 / #{in-bounds 3x3 neighbours with the centre label} (_normalization_layers.py:344-352)
//   sel[l]     guided-upsampling neighbour selection (_normalization_layers.py:534-551): first of {(y,x),(y,x+1),(y+1,x),(y+1,x+1)} (zero padded
//              bottom/right) in the level-(l+1) map whose label equals the level-l label, else 0
// A thread owns a tile of 2 rows x 4 columns of one level (even row, column a multiple of 4).  Everything the tile needs lies in the 4 x 6
// window of level-l pixels rows y-1 .. y+2, columns x-1 .. x+4: the 3x3 neighbourhoods, and the level-(l+1) pixels (ly + dy, lx + dx), which
// are the level-l pixels (2 ly + 2 dy, 2 lx + 2 dx).  A window pixel outside the level reads as -1, which equals no label.
struct PyramidLevel {
    uint8_t* labels;  // null for level 0 (the input) and for a level without outputs
    float* pnorm;     // may be null
    uint8_t* sel;     // may be null
    int level, h, w, tiles_x, tiles_per_img;
    int first_block;  // blocks [first_block, next level's first_block) work on this level
};
struct PyramidArgs {
    PyramidLevel lv[4];  // the levels with work, in order
    int levels;
};

__global__ __launch_bounds__(256) void label_pyramid_kernel(const uint8_t* __restrict__ lab0, int B, int H0, int W0, PyramidArgs args) {
    int slot = 0;
#pragma unroll
    for (int k = 1; k < 4; ++k)
        if (k < args.levels && (int)blockIdx.x >= args.lv[k].first_block) slot = k;
    const PyramidLevel L = args.lv[slot];
    const int l = L.level;
    const int t = ((int)blockIdx.x - L.first_block) * 256 + (int)threadIdx.x;
    if (t >= B * L.tiles_per_img) return;
    const int n = t / L.tiles_per_img;
    const int r = t - n * L.tiles_per_img;
    const int ty = r / L.tiles_x;
    const int y = 2 * ty, x = 4 * (r - ty * L.tiles_x);
    const int H = L.h, W = L.w;
    const uint8_t* base = lab0 + (size_t)n * H0 * W0;

    int a[4][6];
    const bool words = l == 0 && (W0 & 3) == 0 && ((uintptr_t)lab0 & 3) == 0;  // x + 3 < W and the four labels are one aligned word
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int yy = y - 1 + i;
        const bool yin = (unsigned)yy < (unsigned)H;
        const uint8_t* row = base + (yin ? (yy << l) * W0 : 0);
        if (words) {
            const unsigned wv = yin ? *reinterpret_cast<const unsigned*>(row + x) : 0xffffffffu;
#pragma unroll
            for (int j = 0; j < 4; ++j) a[i][1 + j] = yin ? (int)((wv >> (8 * j)) & 0xffu) : -1;
            a[i][0] = (yin && x > 0) ? (int)row[x - 1] : -1;
            a[i][5] = (yin && x + 4 < W) ? (int)row[x + 4] : -1;
        } else {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const int xx = x - 1 + j;
                a[i][j] = (yin && (unsigned)xx < (unsigned)W) ? (int)row[xx << l] : -1;
            }
        }
    }

#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (y + i >= H) break;
        const int o = (n * H + y + i) * W + x;
        if (L.labels) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x + j < W) L.labels[o + j] = (uint8_t)a[1 + i][1 + j];
        }
        if (L.pnorm) {
            float pn[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = a[1 + i][1 + j];
                int cnt = 0;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) cnt += (a[i + dy][j + dx] == c);
                pn[j] = 9.0f / (float)cnt;  // the centre always matches, cnt >= 1
            }
            if (x + 3 < W && (W & 3) == 0 && ((uintptr_t)L.pnorm & 15) == 0) {
                *reinterpret_cast<float4*>(L.pnorm + o) = make_float4(pn[0], pn[1], pn[2], pn[3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < W) L.pnorm[o + j] = pn[j];
            }
        }
        if (L.sel) {  // H and W are even here, and the window's odd rows / columns are the level-(l+1) pixels
            unsigned sv = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = a[1 + i][1 + j], e = j & ~1;
                int s = 0;
                if (a[1][1 + e] == c) s = 0;
                else if (a[1][3 + e] == c) s = 1;
                else if (a[3][1 + e] == c) s = 2;
                else if (a[3][3 + e] == c) s = 3;
                sv |= (unsigned)s << (8 * j);
            }
            if (x + 3 < W && (W & 3) == 0 && ((uintptr_t)L.sel & 3) == 0) {
                *reinterpret_cast<unsigned*>(L.sel + o) = sv;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x + j < W) L.sel[o + j] = (uint8_t)(sv >> (8 * j));
            }
        }
    }
}

// ransac_voting_layer_all_masks front end (ransac_voting.py:276-301): object masks [b,h,w,oc] (float, > 0.5 = inside) -> uint8 label map
// (the highest such object index + 1, 0 = none) and the per-(image, object) pixel counts the sub-sampling rule needs, in one pass
__global__ __launch_bounds__(256) void mask_to_labels_kernel(const float* __restrict__ mask, int hw, int oc, uint8_t* __restrict__ labels,
                                                             int* __restrict__ counts) {
    __shared__ int cnt[256];
    const int n = blockIdx.y;
    if (threadIdx.x < oc) cnt[threadIdx.x] = 0;
    __syncthreads();
    const float* m = mask + (size_t)n * hw * oc;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += gridDim.x * blockDim.x) {
        int lab = 0;
        for (int k = 0; k < oc; ++k) {
            const bool in = m[(size_t)p * oc + k] > 0.5f;
            const unsigned long long b = __builtin_amdgcn_ballot_w64(in);
            if (in) lab = k + 1;
            if (b && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(b)) atomicAdd(&cnt[k], (int)__popcll(b));
        }
        labels[(size_t)n * hw + p] = (uint8_t)lab;
    }
    __syncthreads();
    if (threadIdx.x < oc && cnt[threadIdx.x]) atomicAdd(&counts[n * oc + threadIdx.x], cnt[threadIdx.x]);
}

}  // namespace

extern "C" int cp_pad_channels_3to4(const float* src, float* dst, long long pixels, void* stream) {
    CP_REQUIRE(src && dst && pixels > 0, "cp_pad_channels_3to4: bad arguments");
    CP_LAUNCH(pad3to4_kernel, dim3(grid_for(pixels)), dim3(THREADS), 0, (hipStream_t)stream, src, dst, pixels);
    return cp::check_launch("cp_pad_channels_3to4");
}

extern "C" int cp_maxpool3x3s2_f32(const float* src, int batch, int h, int w, int channels, const float* scale,
                                   const float* shift, int relu, float* dst, void* stream) {
    CP_REQUIRE(src && dst && batch > 0 && h > 0 && w > 0, "cp_maxpool3x3s2_f32: bad arguments");
    CP_REQUIRE(channels % 4 == 0, "cp_maxpool3x3s2_f32: channels must be a multiple of 4");
    CP_REQUIRE((scale == nullptr) == (shift == nullptr), "cp_maxpool3x3s2_f32: scale/shift come together");
    int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
    long long total = (long long)batch * ho * wo * (channels / 4);
    CP_LAUNCH(maxpool_kernel, dim3(grid_for(total)), dim3(THREADS), 0, (hipStream_t)stream, src, batch, h, w,
                       channels, ho, wo, scale, shift, relu, dst);
    return cp::check_launch("cp_maxpool3x3s2_f32");
}

extern "C" int cp_upsample_bilinear_x2_f32(const float* src, int batch, int h, int w, int channels, float* dst, void* stream) {
    CP_REQUIRE(src && dst && batch > 0 && h > 0 && w > 0 && channels % 4 == 0, "cp_upsample_bilinear_x2_f32: bad arguments");
    long long total = (long long)batch * 4 * h * w * (channels / 4);
    CP_LAUNCH(bilinear_x2_kernel, dim3(grid_for(total)), dim3(THREADS), 0, (hipStream_t)stream, src, batch, h, w, channels, dst);
    return cp::check_launch("cp_upsample_bilinear_x2_f32");
}

extern "C" int cp_guided_upsample_x2_f32(const float* src, const uint8_t* sel, int batch, int h, int w, int channels,
                                         float* dst, void* stream) {
    CP_REQUIRE(src && sel && dst && batch > 0 && h > 0 && w > 0 && channels % 4 == 0, "cp_guided_upsample_x2_f32: bad arguments");
    long long total = (long long)batch * 4 * h * w * (channels / 4);
    CP_LAUNCH(guided_x2_kernel, dim3(grid_for(total)), dim3(THREADS), 0, (hipStream_t)stream, src, sel, batch, h, w, channels, dst);
    return cp::check_launch("cp_guided_upsample_x2_f32");
}

extern "C" int cp_mask_to_labels_f32(const float* mask, int batch, int h, int w, int objects, uint8_t* labels, int32_t* counts, void* stream) {
    CP_REQUIRE(mask && labels && counts && batch > 0 && h > 0 && w > 0 && objects > 0 && objects < 255, "cp_mask_to_labels_f32: bad arguments");
    CP_REQUIRE((long long)h * w < (1LL << 31), "cp_mask_to_labels_f32: image too large");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)batch * objects, st) != hipSuccess) return cp::check_launch("cp_mask_to_labels_f32 memset");
    const int hw = h * w;
    int gx = (hw + 255) / 256;
    if (gx > 512) gx = 512;
    CP_LAUNCH(mask_to_labels_kernel, dim3(gx, batch), dim3(256), 0, st, mask, hw, objects, labels, counts);
    return cp::check_launch("cp_mask_to_labels_f32");
}

extern "C" int cp_argmax_labels(const float* logits, int ld, int classes, long long pixels, uint8_t* labels, void* stream) {
    CP_REQUIRE(logits && labels && pixels > 0, "cp_argmax_labels: bad arguments");
    CP_REQUIRE(classes >= 1 && classes <= 255 && ld >= classes, "cp_argmax_labels: classes must be 1..255 and ld >= classes");
    const int nv = (classes + 3) / 4;
    if (ld % 4 == 0 && ((uintptr_t)logits & 15) == 0 && nv <= 3 && nv * 4 <= ld) {
        if (nv == 1) CP_LAUNCH(argmax_vec_kernel<1>, dim3(grid_for(pixels)), dim3(THREADS), 0, (hipStream_t)stream, logits, ld, classes, pixels, labels);
        else if (nv == 2) CP_LAUNCH(argmax_vec_kernel<2>, dim3(grid_for(pixels)), dim3(THREADS), 0, (hipStream_t)stream, logits, ld, classes, pixels, labels);
        else CP_LAUNCH(argmax_vec_kernel<3>, dim3(grid_for(pixels)), dim3(THREADS), 0, (hipStream_t)stream, logits, ld, classes, pixels, labels);
        return cp::check_launch("cp_argmax_labels");
    }
    CP_LAUNCH(argmax_kernel, dim3(grid_for(pixels)), dim3(THREADS), 0, (hipStream_t)stream, logits, ld, classes, pixels, labels);
    return cp::check_launch("cp_argmax_labels");
}

extern "C" int cp_label_pyramid(const uint8_t* labels0, int batch, int h, int w, uint8_t* const* labels,
                                float* const* pnorm, uint8_t* const* sel, void* stream) {
    CP_REQUIRE(labels0 && batch > 0 && h > 0 && w > 0, "cp_label_pyramid: bad arguments");
    CP_REQUIRE(labels, "cp_label_pyramid: labels[] array required (labels[1..3] receive the half-size maps)");
    CP_REQUIRE((long long)batch * h * w < (1LL << 31), "cp_label_pyramid: batch * h * w must stay below 2^31");
    hipStream_t st = (hipStream_t)stream;
    bool have[4] = {true, false, false, false};  // level l exists: the input, or labels[l] given (and every level before it)
    int hs[4], ws[4];
    hs[0] = h; ws[0] = w;
    for (int l = 1; l < 4; ++l) { hs[l] = hs[l - 1] / 2; ws[l] = ws[l - 1] / 2; }
    for (int l = 1; l < 4; ++l) {
        if (!labels[l]) break;
        CP_REQUIRE(hs[l] > 0 && ws[l] > 0, "cp_label_pyramid: level %d is empty", l);
        have[l] = true;
    }
    PyramidArgs args;
    args.levels = 0;
    int blocks = 0;
    for (int l = 0; l < 4; ++l) {
        PyramidLevel lv;
        lv.labels = (l > 0 && have[l]) ? labels[l] : nullptr;
        lv.pnorm = nullptr;
        lv.sel = nullptr;
        if (pnorm && pnorm[l]) {
            CP_REQUIRE(have[l], "cp_label_pyramid: pnorm[%d] requested without labels[%d]", l, l);
            lv.pnorm = pnorm[l];
        }
        if (l < 3 && sel && sel[l]) {
            CP_REQUIRE(have[l] && have[l + 1], "cp_label_pyramid: sel[%d] needs labels[%d] and labels[%d]", l, l, l + 1);
            CP_REQUIRE(hs[l] == 2 * hs[l + 1] && ws[l] == 2 * ws[l + 1], "cp_label_pyramid: level %d size must be even", l);
            lv.sel = sel[l];
        }
        if (!lv.labels && !lv.pnorm && !lv.sel) continue;
        lv.h = hs[l]; lv.w = ws[l];
        lv.level = l;
        lv.tiles_x = (ws[l] + 3) / 4;
        lv.tiles_per_img = lv.tiles_x * ((hs[l] + 1) / 2);
        lv.first_block = blocks;
        blocks += (int)(((long long)batch * lv.tiles_per_img + THREADS - 1) / THREADS);
        args.lv[args.levels++] = lv;
    }
    if (blocks == 0) return CP_OK;
    CP_LAUNCH(label_pyramid_kernel, dim3(blocks), dim3(THREADS), 0, st, labels0, batch, h, w, args);
    return cp::check_launch("cp_label_pyramid");
}
