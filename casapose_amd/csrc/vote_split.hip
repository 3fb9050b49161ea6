// Splitting touching instances of one object by their centre votes (cp_vote_split_labels; the rule stands in include/casapose_hip.h, its
// arithmetic in vote_split_math.h).  This file is the schedule: four kernels on one stream, integer atomics only.
//
// vs_accumulate_kernel: grid (image, object, band of BAND rows), 1024 threads, one object's whole grid as int32 in dynamic LDS (gh * gw * 4 bytes,
//   76 800 at 480 x 640 with cell 4).  The block first reads the labels of its band's voting pixels; a band without a pixel of its object ends
//   there, before it zeroes anything.  Otherwise a thread takes voting pixels of the band in raster order, reads the two direction floats of a
//   pixel of its object and nothing else of the record, and walks the ray with one LDS integer add per step.  After the walk the block adds its
//   non-zero cells to the global accumulator with one integer atomic each.  Rays of one wave differ in length and nothing is done about it: a
//   wave walks as long as its longest ray (DESIGN 4.21 says what that costs).
// vs_peaks_kernel: one block of 1024 threads per (image, object), the object's grid copied to dynamic LDS so that the window maxima are LDS
//   reads.  Every cell's candidate key (0 for none) goes to the workspace and the LDS copy keeps the candidates' votes only; then R rounds of
//   an LDS atomicMax over the keys below the previous round's winner (the pattern of ccl_instance_select); then thread r writes rank r's row
//   of the table and its fp64 centroid.
// vs_assign_kernel: blocks of 4096 pixels of one image; the image's peaks lie in LDS; a pixel takes its slot, the slot's count is summed per
//   wave by ballot, per block in LDS, and goes to the global counts with one integer add per slot and block.
// vs_write_kernel: empties the slots below min_size in the slot map and fills the tables' first column.
#include "common.h"
#include "vote_split_math.h"

namespace {

using namespace cp_vs;

constexpr int ACC_THREADS = 1024, PEAK_THREADS = 1024, THREADS = 256, ASSIGN_PIXELS = 4096;
constexpr int VS_MAX_LDS = 160 * 1024;   // per workgroup on gfx950
static_assert((size_t)MAX_CELLS * sizeof(int32_t) + 1024 <= (size_t)VS_MAX_LDS, "the largest grid fits beside the kernel's static LDS");
static_assert(MAX_CELLS <= 64 * PEAK_THREADS, "a thread of vs_peaks_kernel keeps one bit per cell it owns");

__global__ __launch_bounds__(ACC_THREADS) void vs_accumulate_kernel(const uint8_t* __restrict__ labels, const float* __restrict__ field, int ld, int dir_at,
                                                                    int h, int w, int objects, int cell, int shift, int vstride, int gh, int gw,
                                                                    int bands, int32_t* __restrict__ acc) {
    extern __shared__ int32_t s_acc[];
    const int tid = threadIdx.x;
    const int band = blockIdx.x % (unsigned)bands, o = (blockIdx.x / (unsigned)bands) % (unsigned)objects;
    const int n = blockIdx.x / ((unsigned)bands * (unsigned)objects);
    const int y0 = band * BAND, y1 = y0 + BAND < h ? y0 + BAND : h;
    const int ly0 = (y0 + vstride - 1) / vstride * vstride;                 // the band's first voting row
    const int rows = ly0 < y1 ? (y1 - ly0 + vstride - 1) / vstride : 0, cols = (w + vstride - 1) / vstride;
    const int total = rows * cols;                                          // <= BAND * MAX_SIDE
    const size_t image = (size_t)n * h * w;
    const int mine = o + 1;

    int any = 0;
    for (int i = tid; i < total; i += ACC_THREADS) {
        const int ry = i / cols, y = ly0 + ry * vstride, x = (i - ry * cols) * vstride;
        any |= labels[image + (size_t)y * w + x] == mine;
    }
    if (!__syncthreads_or(any)) return;   // block-uniform

    const int cells = gh * gw;
    for (int c = tid; c < cells; c += ACC_THREADS) s_acc[c] = 0;
    __syncthreads();
    for (int i = tid; i < total; i += ACC_THREADS) {
        const int ry = i / cols, y = ly0 + ry * vstride, x = (i - ry * cols) * vstride;
        const size_t at = image + (size_t)y * w + x;
        if (labels[at] != mine) continue;
        const float* d = field + at * ld + dir_at;
        Ray r;
        if (!ray_setup(y, x, d[0], d[1], h, w, r)) continue;
        int cy, cx;
        for (int k = 0; ray_cell(r, k, cell, shift, cy, cx); ++k) atomicAdd(&s_acc[cy * gw + cx], 1);   // cy < gh, cx < gw: the ray is inside the image
    }
    __syncthreads();
    int32_t* __restrict__ out = acc + ((size_t)n * objects + o) * cells;
    for (int c = tid; c < cells; c += ACC_THREADS) {
        const int32_t v = s_acc[c];
        if (v != 0) atomicAdd(out + c, v);
    }
}

__global__ __launch_bounds__(PEAK_THREADS) void vs_peaks_kernel(const int32_t* __restrict__ acc, unsigned long long* __restrict__ keys, int gh, int gw,
                                                                int cell, int R, int min_votes, int rel_percent, int nms, int32_t* __restrict__ inst,
                                                                float* __restrict__ peaks) {
    extern __shared__ int32_t s_grid[];   // the object's grid; after the window pass, the candidates' votes and 0 elsewhere
    __shared__ unsigned long long best[MAX_INST];
    const int tid = threadIdx.x, cells = gh * gw;
    const int32_t* __restrict__ a = acc + (size_t)blockIdx.x * cells;
    unsigned long long* __restrict__ k = keys + (size_t)blockIdx.x * cells;
    if (tid < MAX_INST) best[tid] = 0ull;
    for (int c = tid; c < cells; c += PEAK_THREADS) s_grid[c] = a[c];
    __syncthreads();
    unsigned long long mine = 0ull;       // bit i: this thread's i-th cell is a candidate (at most MAX_CELLS / PEAK_THREADS = 36 cells a thread)
    for (int c = tid, i = 0; c < cells; c += PEAK_THREADS, ++i) {
        const int cy = c / gw, cx = c - cy * gw;
        if (is_candidate(s_grid, gh, gw, cy, cx, min_votes, nms)) mine |= 1ull << i;
    }
    __syncthreads();                      // every window has been read
    for (int c = tid, i = 0; c < cells; c += PEAK_THREADS, ++i) {
        const bool cand = (mine >> i) & 1ull;
        const int v = s_grid[c];
        k[c] = cand ? cell_key(v, c) : 0ull;
        if (!cand) s_grid[c] = 0;         // a candidate has votes >= min_votes >= 1: 0 marks "none"
    }
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        const unsigned long long below = r ? best[r - 1] : ~0ull;   // an empty rank r - 1 (0) leaves every later rank empty
        for (int c = tid; c < cells; c += PEAK_THREADS) {
            const int v = s_grid[c];
            if (v == 0) continue;
            const unsigned long long key = cell_key(v, c);
            if (key < below) atomicMax(&best[r], key);
        }
        __syncthreads();
    }
    if (tid < R) {
        const unsigned long long key = best[tid];
        const size_t row = (size_t)blockIdx.x * R + tid;
        const bool ok = key != 0ull && passes_cut(key_votes(key), key_votes(best[0]), rel_percent);
        float py = 0.f, px = 0.f;
        int cy = -1, cx = -1;
        if (ok) {
            const int at = key_index(key);
            cy = at / gw, cx = at - cy * gw;
            peak_position(a, gh, gw, cy, cx, cell, py, px);   // from the accumulator itself: s_grid holds the candidates only
        }
        inst[4 * row] = 0, inst[4 * row + 1] = ok ? key_votes(key) : 0, inst[4 * row + 2] = cy, inst[4 * row + 3] = cx;
        peaks[2 * row] = py, peaks[2 * row + 1] = px;
    }
}

__global__ __launch_bounds__(THREADS) void vs_assign_kernel(const uint8_t* __restrict__ labels, const float* __restrict__ field, int ld, int dir_at, int h,
                                                            int w, int objects, int R, float gate, const int32_t* __restrict__ inst,
                                                            const float* __restrict__ peaks, int blocks_per_image, int32_t* __restrict__ counts,
                                                            uint8_t* __restrict__ slots_out) {
    __shared__ float s_peak[2 * MAX_SLOTS];
    __shared__ int s_np[MAX_SLOTS], s_cnt[MAX_SLOTS];
    const int tid = threadIdx.x, lane = tid & 63, slots = objects * R;
    const int n = blockIdx.x / (unsigned)blocks_per_image, part = blockIdx.x % (unsigned)blocks_per_image;
    for (int s = tid; s < slots; s += THREADS) {
        s_peak[2 * s] = peaks[2 * ((size_t)n * slots + s)];
        s_peak[2 * s + 1] = peaks[2 * ((size_t)n * slots + s) + 1];
        s_cnt[s] = 0;
    }
    for (int o = tid; o < objects; o += THREADS) {
        int np = 0;
        for (int r = 0; r < R; ++r) np += inst[4 * ((size_t)n * slots + o * R + r) + 2] >= 0;   // the surviving ranks are the first ones
        s_np[o] = np;
    }
    __syncthreads();
    const int hw = h * w;
    const size_t image = (size_t)n * hw;
    for (int it = 0; it < ASSIGN_PIXELS / THREADS; ++it) {   // wave-uniform trip count: the ballots below need every lane
        const int p = part * ASSIGN_PIXELS + it * THREADS + tid;
        int slot = 0;
        if (p < hw) {
            const int l = labels[image + p];
            if (l >= 1 && l <= objects && s_np[l - 1] > 0) {
                const int y = p / w, x = p - y * w;
                const float* d = field + (image + p) * ld + dir_at;
                const int r = assign_rank(y, x, d[0], d[1], s_peak + 2 * (l - 1) * R, s_np[l - 1], gate);
                if (r >= 0) slot = (l - 1) * R + r + 1;
            }
            slots_out[image + p] = (uint8_t)slot;
        }
        int pending = slot;
        for (;;) {
            const unsigned long long left = __ballot(pending != 0);
            if (left == 0ull) break;
            const int leader = __ffsll((long long)left) - 1;
            const int s = __shfl(pending, leader);
            const unsigned long long same = __ballot(pending == s);
            if (lane == leader) atomicAdd(&s_cnt[s - 1], __popcll(same));
            if (pending == s) pending = 0;
        }
    }
    __syncthreads();
    for (int s = tid; s < slots; s += THREADS) {
        const int c = s_cnt[s];
        if (c != 0) atomicAdd(counts + (size_t)n * slots + s, c);
    }
}

__global__ __launch_bounds__(THREADS) void vs_write_kernel(const int32_t* __restrict__ counts, int slots, int hw, long long pixels, long long rows,
                                                           int min_size, uint8_t* __restrict__ slots_out, int32_t* __restrict__ inst) {
    const long long most = pixels > rows ? pixels : rows;
    for (long long i = blockIdx.x * (long long)THREADS + threadIdx.x; i < most; i += (long long)gridDim.x * THREADS) {
        if (i < pixels) {
            const int s = slots_out[i];
            if (s != 0 && counts[(i / hw) * slots + (s - 1)] < min_size) slots_out[i] = 0;
        }
        if (i < rows) {
            const int c = counts[i];
            inst[4 * i] = c >= min_size ? c : 0;
        }
    }
}

// THE carve of the workspace: acc int32 [n][objects][gh][gw], the slots' pixel counts int32 [n][objects * R] (both zeroed by one memset), then
// the candidate keys uint64 [n][objects][gh][gw] on the next multiple of 16 bytes.
struct VsWs {
    size_t acc, counts, keys, bytes;
};
inline VsWs vs_carve(int batch, int h, int w, int objects, int R, int cell) {
    const size_t cells = (size_t)((h + cell - 1) / cell) * (size_t)((w + cell - 1) / cell) * objects * batch;
    VsWs ws;
    ws.acc = 0;
    ws.counts = cells * sizeof(int32_t);
    ws.keys = (ws.counts + (size_t)batch * objects * R * sizeof(int32_t) + 15) / 16 * 16;
    ws.bytes = ws.keys + cells * sizeof(unsigned long long);
    return ws;
}

// the limits of the sizes, by name: nullptr when they hold
inline const char* vs_sizes_refused(int batch, int h, int w, int objects, int R, int cell) {
    if (R < 1 || R > MAX_INST) return "max_instances must be in 1..16";
    if (batch < 1 || h < 1 || w < 1 || objects < 1) return "batch, h, w and objects must be positive";
    if (objects > MAX_SLOTS || objects * R > MAX_SLOTS) return "objects * max_instances must be at most 254: slot ids are bytes";
    if (cell != 2 && cell != 4 && cell != 8) return "cell must be 2, 4 or 8";
    if (h > MAX_SIDE || w > MAX_SIDE) return "h and w must be at most 16384";
    const long long cells = (long long)((h + cell - 1) / cell) * ((w + cell - 1) / cell);
    if (cells > MAX_CELLS) return "the grid of one object, ceil(h / cell) * ceil(w / cell) cells, must be at most 36864 (it lies in LDS); use a larger cell";
    if ((long long)batch * h * w >= (1LL << 31) || cells * objects * batch >= (1LL << 31)) return "too many pixels or cells for 32-bit indices";
    if ((long long)batch * objects * ((h + BAND - 1) / BAND) >= (1LL << 31)) return "too many blocks";
    return nullptr;
}

}  // namespace

extern "C" size_t cp_vote_split_workspace_bytes(int batch, int h, int w, int objects, int max_instances, int cell) {
    if (vs_sizes_refused(batch, h, w, objects, max_instances, cell)) return 0;
    return vs_carve(batch, h, w, objects, max_instances, cell).bytes;
}

extern "C" int cp_vote_split_workspace_layout(int batch, int h, int w, int objects, int max_instances, int cell, size_t* offsets) {
    CP_REQUIRE(offsets, "cp_vote_split_workspace_layout: null pointer");
    const char* why = vs_sizes_refused(batch, h, w, objects, max_instances, cell);
    CP_REQUIRE(!why, "cp_vote_split_workspace_layout: %s (got batch %d, %d x %d, %d objects, max_instances %d, cell %d)", why, batch, h, w, objects,
               max_instances, cell);
    const VsWs lay = vs_carve(batch, h, w, objects, max_instances, cell);
    offsets[0] = lay.acc, offsets[1] = lay.keys, offsets[2] = lay.counts;
    return CP_OK;
}

extern "C" int cp_vote_split_labels(const uint8_t* labels, const float* field, int ld, int dir_off, int kp_index, int batch, int h, int w, int objects,
                                    int max_instances, int cell, int vote_stride, int min_votes, int rel_percent, int nms_radius, float gate,
                                    int min_size, void* ws, uint8_t* slots_out, int32_t* inst_out, float* peaks_out, void* stream) {
    CP_REQUIRE(labels && field && ws && slots_out && inst_out && peaks_out, "cp_vote_split_labels: null pointer");
    const char* why = vs_sizes_refused(batch, h, w, objects, max_instances, cell);
    CP_REQUIRE(!why, "cp_vote_split_labels: %s (got batch %d, %d x %d, %d objects, max_instances %d, cell %d)", why, batch, h, w, objects,
               max_instances, cell);
    CP_REQUIRE(ld >= 2 && ld <= 4096 && dir_off >= 0 && kp_index >= 0 && kp_index <= 2048 && dir_off <= 4096 && dir_off + 2 * kp_index + 2 <= ld,
               "cp_vote_split_labels: the direction at dir_off + 2 * kp_index lies outside the pixel record (ld %d, dir_off %d, kp_index %d)", ld,
               dir_off, kp_index);
    CP_REQUIRE(vote_stride >= 1 && vote_stride <= MAX_STRIDE, "cp_vote_split_labels: vote_stride must be in 1..%d (got %d)", MAX_STRIDE, vote_stride);
    CP_REQUIRE(min_votes >= 1, "cp_vote_split_labels: min_votes must be at least 1 (got %d)", min_votes);
    CP_REQUIRE(rel_percent >= 0 && rel_percent <= 100, "cp_vote_split_labels: rel_percent must be in 0..100 (got %d)", rel_percent);
    CP_REQUIRE(nms_radius >= 1 && nms_radius <= MAX_NMS, "cp_vote_split_labels: nms_radius must be in 1..%d cells (got %d)", MAX_NMS, nms_radius);
    CP_REQUIRE(gate > 0.f && finite32(gate), "cp_vote_split_labels: gate must be positive and finite (got %g)", (double)gate);
    CP_REQUIRE(min_size >= 1, "cp_vote_split_labels: min_size must be at least 1 (got %d)", min_size);
    CP_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)field & 3) == 0 && ((uintptr_t)inst_out & 3) == 0 && ((uintptr_t)peaks_out & 3) == 0,
               "cp_vote_split_labels: ws must be 16-byte aligned, field, inst_out and peaks_out 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const VsWs lay = vs_carve(batch, h, w, objects, max_instances, cell);
    char* base = static_cast<char*>(ws);
    int32_t* acc = reinterpret_cast<int32_t*>(base + lay.acc);
    int32_t* counts = reinterpret_cast<int32_t*>(base + lay.counts);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + lay.keys);
    const int gh = (h + cell - 1) / cell, gw = (w + cell - 1) / cell, bands = (h + BAND - 1) / BAND, slots = objects * max_instances;
    const int dir_at = dir_off + 2 * kp_index;
    const size_t lds = (size_t)gh * gw * sizeof(int32_t);
    if (hipMemsetAsync(acc, 0, lay.counts + (size_t)batch * slots * sizeof(int32_t), st) != hipSuccess) return cp::check_launch("cp_vote_split_labels memset");
    if (lds > 64 * 1024)   // (the limit counts the kernel's static LDS too: ask for what this launch needs, not for the whole 160 KB)
        CP_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&vs_accumulate_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==
                       hipSuccess, "cp_vote_split_labels: cannot raise the kernel's LDS limit to %zu bytes", lds);
    CP_LAUNCH(vs_accumulate_kernel, dim3((unsigned)(batch * objects * bands)), dim3(ACC_THREADS), lds, st, labels, field, ld, dir_at, h, w, objects, cell,
              cell_shift(cell), vote_stride, gh, gw, bands, acc);
    if (lds > 64 * 1024)
        CP_REQUIRE(hipFuncSetAttribute(reinterpret_cast<const void*>(&vs_peaks_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess,
                   "cp_vote_split_labels: cannot raise the kernel's LDS limit to %zu bytes", lds);
    CP_LAUNCH(vs_peaks_kernel, dim3((unsigned)(batch * objects)), dim3(PEAK_THREADS), lds, st, acc, keys, gh, gw, cell, max_instances, min_votes, rel_percent,
              nms_radius, inst_out, peaks_out);
    const int blocks_per_image = (int)(((long long)h * w + ASSIGN_PIXELS - 1) / ASSIGN_PIXELS);
    CP_LAUNCH(vs_assign_kernel, dim3((unsigned)(batch * blocks_per_image)), dim3(THREADS), 0, st, labels, field, ld, dir_at, h, w, objects, max_instances,
              gate, inst_out, peaks_out, blocks_per_image, counts, slots_out);
    const long long total = (long long)batch * h * w, rows = (long long)batch * slots;
    const long long need = total > rows ? total : rows;
    const long long g = (need + THREADS - 1) / THREADS;
    CP_LAUNCH(vs_write_kernel, dim3((unsigned)(g > 4096 ? 4096 : g)), dim3(THREADS), 0, st, counts, slots, h * w, total, rows, min_size, slots_out, inst_out);
    return cp::check_launch("cp_vote_split_labels");
}
