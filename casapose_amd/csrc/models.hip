// Keypoints and models_info of a folder of meshes on the device: box, diameter and farthest-point keypoints of every object in one call, and the
// host twin.  The arithmetic is model_math.h; this file is the schedule.
//
// The vertices of all objects lie back to back in one fp32 array; offsets / counts say where each object's are.  Three launches on the caller's
// stream, none of them per object from the host, no host round trip in between:
//   setup_kernel     one block.  Validates every object's vertex range, writes the prefix sums of the objects' tile-pair counts (64-bit) into
//                    the workspace and clears the squared diameters.
//   fps_kernel       one 1024-thread block per object.  Box (min / max reduced through wave shuffles and LDS), centre, m_i = d2(P_i, centre), then
//                    K - 1 rounds of: block arg-max of m (largest value, lowest index), emit the vertex, m_i = min(m_i, d2(P_i, pick)) fused with
//                    the next round's arg-max.  m lives in the workspace.  Writes box, keypoints, indices and the status word.
//   diameter_kernel  a persistent grid over the flattened list of upper-triangle TILE x TILE tile pairs of all objects (grid stride; a block's
//                    pairs come in object order).  Per pair a thread holds one vertex of tile A in registers as fp64 and runs over tile B, which
//                    the block staged in LDS as fp64: every lane reads the same LDS address, a broadcast.  Nine fp64 vector operations per
//                    pair (three differences, three products, two sums, one compare-select), no FMA.  A lane past the object's last vertex holds
//                    a copy of the last vertex, tile B's loop stops at the object's last vertex: padding is never a point.  Each thread keeps an fp64
//                    running maximum; when the block leaves an object it reduces once and issues one 64-bit unsigned atomicMax on the bit pattern
//                    (non-negative doubles order like their bit patterns), a vector atomic on plain global memory.
// A maximum and the lowest-index arg-max do not depend on the order they are taken in: two calls with the same inputs give the same bits, and
// the same bits as model_math.h's serial loop (cp_model_prep_host_f32, which launches nothing).
#include "common.h"
#include "model_math.h"

namespace {

using namespace cp_model;

constexpr int FPS_THREADS = 1024, DIAM_THREADS = TILE, SETUP_THREADS = 256, WAVE = 64;
constexpr int DIAM_BLOCKS = 1024;   // four 256-thread blocks per CU

__global__ void __launch_bounds__(SETUP_THREADS) setup_kernel(long long total, const long long* __restrict__ offsets,
                                                             const int32_t* __restrict__ counts, int objects, int64_t* __restrict__ prefix,
                                                             double* __restrict__ diameter_sq) {
    __shared__ int64_t s_pairs[MAX_OBJECTS];
    for (int o = threadIdx.x; o < objects; o += SETUP_THREADS) {   // objects <= MAX_OBJECTS (checked before the launch)
        s_pairs[o] = object_valid(offsets[o], counts[o], total) ? tile_pairs(counts[o]) : 0;
        diameter_sq[o] = 0.0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t sum = 0;
        for (int o = 0; o < objects; ++o) {
            prefix[o] = sum;
            sum += s_pairs[o];
        }
        prefix[objects] = sum;
    }
}

// block-wide (value, index) arg-max under model_math.h's `better`; every thread of the block calls it and gets the result
__device__ __forceinline__ void block_argmax(double& v, int& i, double* s_v, int* s_i) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(v, m);
        const int oi = __shfl_xor(i, m);
        if (better(ov, oi, v, i)) v = ov, i = oi;
    }
    const int wave = threadIdx.x / WAVE;
    __syncthreads();   // the previous round's readers are done with s_v / s_i
    if ((threadIdx.x & (WAVE - 1)) == 0) s_v[wave] = v, s_i[wave] = i;
    __syncthreads();
    v = s_v[0], i = s_i[0];
    for (int w = 1; w < FPS_THREADS / WAVE; ++w)
        if (better(s_v[w], s_i[w], v, i)) v = s_v[w], i = s_i[w];
}

__global__ void __launch_bounds__(FPS_THREADS) fps_kernel(const float* __restrict__ verts, long long total, const long long* __restrict__ offsets,
                                                         const int32_t* __restrict__ counts, int K, float* __restrict__ box,
                                                         float* __restrict__ keypoints, int32_t* __restrict__ indices, int32_t* __restrict__ status,
                                                         double* __restrict__ m_all) {
    __shared__ float s_box[FPS_THREADS / WAVE][6];
    __shared__ double s_v[FPS_THREADS / WAVE];
    __shared__ int s_i[FPS_THREADS / WAVE];
    const int o = blockIdx.x, tid = threadIdx.x;
    const int n = counts[o];
    const long long off = offsets[o];
    float* obox = box + 6 * (size_t)o;
    float* okp = keypoints + 3 * (size_t)K * o;
    int32_t* oidx = indices + (size_t)(K - 1) * o;
    if (!object_valid(off, n, total)) {   // block-uniform: nothing has been synchronised yet
        if (tid < 6) obox[tid] = 0.f;
        if (tid < 3 * K) okp[tid] = 0.f;
        if (tid < K - 1) oidx[tid] = 0;
        if (tid == 0) status[o] = ST_BAD_COUNT;
        return;
    }
    const float* P = verts + 3 * (size_t)off;   // [n][3], inside [0, total)
    double* m = m_all + off;

    // rule 1
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < n; i += FPS_THREADS) box_add(mn, mx, P + 3 * (size_t)i);
#pragma unroll
    for (int s = WAVE / 2; s >= 1; s >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = __shfl_xor(mn[a], s), hi = __shfl_xor(mx[a], s);
            if (below(lo, mn[a])) mn[a] = lo;
            if (below(mx[a], hi)) mx[a] = hi;
        }
    if ((tid & (WAVE - 1)) == 0)
        for (int a = 0; a < 3; ++a) s_box[tid / WAVE][a] = mn[a], s_box[tid / WAVE][3 + a] = mx[a];
    __syncthreads();
    for (int w = 0; w < FPS_THREADS / WAVE; ++w)
        for (int a = 0; a < 3; ++a) {
            if (below(s_box[w][a], mn[a])) mn[a] = s_box[w][a];
            if (below(mx[a], s_box[w][3 + a])) mx[a] = s_box[w][3 + a];
        }
    // rule 2
    const double cx = centre(mn[0], mx[0]), cy = centre(mn[1], mx[1]), cz = centre(mn[2], mx[2]);
    if (tid == 0) {
        for (int a = 0; a < 3; ++a) obox[a] = mn[a], obox[3 + a] = mx[a];
        okp[0] = (float)cx, okp[1] = (float)cy, okp[2] = (float)cz;
    }
    // rule 5
    double bv = -1.0;
    int bi = 0x7fffffff;
    for (int i = tid; i < n; i += FPS_THREADS) {
        const double d = dist2((double)P[3 * (size_t)i], (double)P[3 * (size_t)i + 1], (double)P[3 * (size_t)i + 2], cx, cy, cz);
        m[i] = d;
        if (better(d, i, bv, bi)) bv = d, bi = i;
    }
    int st = ST_OK;
    for (int k = 1; k < K; ++k) {
        block_argmax(bv, bi, s_v, s_i);   // block-uniform from here
        if (!(bv > 0.0)) {
            st = ST_TOO_FEW;
            if (tid == 0) zero_picks(okp, oidx, K, k);
            break;
        }
        const int j = bi;   // a vertex of this object: only indices below n enter the arg-max with a value above -1
        const float qx = P[3 * (size_t)j], qy = P[3 * (size_t)j + 1], qz = P[3 * (size_t)j + 2];
        if (tid == 0) okp[3 * k] = qx, okp[3 * k + 1] = qy, okp[3 * k + 2] = qz, oidx[k - 1] = j;
        if (k == K - 1) break;
        bv = -1.0, bi = 0x7fffffff;
        for (int i = tid; i < n; i += FPS_THREADS) {   // a thread reads back only the m it wrote itself
            const double d = dist2((double)P[3 * (size_t)i], (double)P[3 * (size_t)i + 1], (double)P[3 * (size_t)i + 2], (double)qx, (double)qy, (double)qz);
            double mi = m[i];
            if (d < mi) m[i] = mi = d;
            if (better(mi, i, bv, bi)) bv = mi, bi = i;
        }
    }
    if (tid == 0) status[o] = st;
}

// the object whose tile pairs include p: the largest o with prefix[o] <= p (objects with no pairs are skipped by the strict upper bound)
__device__ __forceinline__ int object_of_pair(const int64_t* __restrict__ prefix, int objects, int64_t p) {
    int lo = 0, hi = objects - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= p) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// every thread of the block calls it: the block's maximum into the object's squared diameter
__device__ __forceinline__ void flush_maximum(double best, double* s_red, double* diameter_sq) {
#pragma unroll
    for (int m = WAVE / 2; m >= 1; m >>= 1) {
        const double ob = __shfl_xor(best, m);
        if (ob > best) best = ob;
    }
    __syncthreads();
    if ((threadIdx.x & (WAVE - 1)) == 0) s_red[threadIdx.x / WAVE] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < DIAM_THREADS / WAVE; ++w)
            if (s_red[w] > best) best = s_red[w];
        if (best > 0.0) atomicMax(reinterpret_cast<unsigned long long*>(diameter_sq), (unsigned long long)__double_as_longlong(best));
    }
}

__global__ void __launch_bounds__(DIAM_THREADS) diameter_kernel(const float* __restrict__ verts, const long long* __restrict__ offsets,
                                                               const int32_t* __restrict__ counts, int objects, const int64_t* __restrict__ prefix,
                                                               double* __restrict__ diameter_sq) {
    __shared__ double s_b[TILE * 3];
    __shared__ double s_red[DIAM_THREADS / WAVE];
    const int tid = threadIdx.x;
    const int64_t all = prefix[objects];
    int obj = -1, n = 0;
    int64_t first = 0, end = 0;   // the current object's pairs are [first, end)
    const float* P = nullptr;
    double best = 0.0;
    for (int64_t p = blockIdx.x; p < all; p += gridDim.x) {   // block-uniform
        if (p >= end) {
            if (obj >= 0) flush_maximum(best, s_red, diameter_sq + obj);
            best = 0.0;
            obj = object_of_pair(prefix, objects, p);   // prefix[obj] <= p < prefix[obj + 1]: the object has pairs, so setup_kernel found it valid
            first = prefix[obj], end = prefix[obj + 1];
            n = counts[obj];
            P = verts + 3 * (size_t)offsets[obj];
        }
        int ta, tb;
        tile_of_pair(p - first, ta, tb);   // ta <= tb < tiles(n)
        const int ia = min(ta * TILE + tid, n - 1);   // past the last vertex: the last vertex once more
        const double ax = (double)P[3 * (size_t)ia], ay = (double)P[3 * (size_t)ia + 1], az = (double)P[3 * (size_t)ia + 2];
        const int cb = min(TILE, n - tb * TILE);   // >= 1
        __syncthreads();   // the previous pair's readers are done with s_b
        if (tid < cb) {
            const float* Q = P + 3 * (size_t)(tb * TILE + tid);
            s_b[3 * tid] = (double)Q[0], s_b[3 * tid + 1] = (double)Q[1], s_b[3 * tid + 2] = (double)Q[2];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cb; ++j) {
            const double d = dist2(ax, ay, az, s_b[3 * j], s_b[3 * j + 1], s_b[3 * j + 2]);
            if (d > best) best = d;
        }
    }
    if (obj >= 0) flush_maximum(best, s_red, diameter_sq + obj);
}

int check_arguments(const char* fn, const void* verts, long long total, const void* offsets, const void* counts, int objects, int no_points,
                    const void* diameter_sq, const void* box, const void* keypoints, const void* indices, const void* status, const void* workspace,
                    size_t workspace_bytes) {
    CP_REQUIRE(verts && offsets && counts && diameter_sq && box && keypoints && indices && status && workspace, "%s: null pointer", fn);
    CP_REQUIRE(objects >= 1 && objects <= MAX_OBJECTS, "%s: objects must lie in [1, %d] (got %d)", fn, MAX_OBJECTS, objects);
    CP_REQUIRE(no_points >= MIN_POINTS && no_points <= MAX_POINTS, "%s: no_points counts the centre and must lie in [%d, %d] (got %d)", fn, MIN_POINTS,
               MAX_POINTS, no_points);
    CP_REQUIRE(total >= 0 && total <= (long long)MAX_OBJECTS * MAX_VERTICES, "%s: total must lie in [0, %lld] (got %lld)", fn,
               (long long)MAX_OBJECTS * MAX_VERTICES, total);
    CP_REQUIRE(workspace_bytes >= cp_model::workspace_bytes(objects, total), "%s: the workspace has %zu bytes, %zu are needed", fn, workspace_bytes,
               cp_model::workspace_bytes(objects, total));
    CP_REQUIRE(((uintptr_t)verts & 3) == 0 && ((uintptr_t)counts & 3) == 0 && ((uintptr_t)box & 3) == 0 && ((uintptr_t)keypoints & 3) == 0 &&
                   ((uintptr_t)indices & 3) == 0 && ((uintptr_t)status & 3) == 0,
               "%s: the fp32 and int32 arrays must be 4-byte aligned", fn);
    CP_REQUIRE(((uintptr_t)offsets & 7) == 0 && ((uintptr_t)diameter_sq & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
               "%s: offsets, diameter_sq and the workspace must be 8-byte aligned", fn);
    return CP_OK;
}

}  // namespace

namespace cp {

size_t model_prep_workspace_bytes(int objects, long long total) {
    if (objects < 1 || objects > MAX_OBJECTS || total < 0 || total > (long long)MAX_OBJECTS * MAX_VERTICES) return 0;
    return cp_model::workspace_bytes(objects, total);
}

int model_prep_device(const float* verts, long long total, const long long* offsets, const int32_t* counts, int objects, int no_points,
                      double* diameter_sq, float* box, float* keypoints, int32_t* indices, int32_t* status, void* workspace, size_t workspace_bytes,
                      hipStream_t st) {
    if (int rc = check_arguments("cp_model_prep_f32", verts, total, offsets, counts, objects, no_points, diameter_sq, box, keypoints, indices, status,
                                 workspace, workspace_bytes))
        return rc;
    int64_t* prefix = (int64_t*)workspace;
    double* m_all = (double*)(prefix + objects + 1);
    CP_LAUNCH(setup_kernel, dim3(1), dim3(SETUP_THREADS), 0, st, total, offsets, counts, objects, prefix, diameter_sq);
    if (int rc = cp::check_launch("cp_model_prep_f32 (setup)")) return rc;
    CP_LAUNCH(fps_kernel, dim3((unsigned)objects), dim3(FPS_THREADS), 0, st, verts, total, offsets, counts, no_points, box, keypoints, indices, status,
              m_all);
    if (int rc = cp::check_launch("cp_model_prep_f32 (keypoints)")) return rc;
    CP_LAUNCH(diameter_kernel, dim3(DIAM_BLOCKS), dim3(DIAM_THREADS), 0, st, verts, offsets, counts, objects, (const int64_t*)prefix, diameter_sq);
    return cp::check_launch("cp_model_prep_f32 (diameter)");
}

int model_prep_host(const float* verts, long long total, const long long* offsets, const int32_t* counts, int objects, int no_points,
                    double* diameter_sq, float* box, float* keypoints, int32_t* indices, int32_t* status, void* workspace, size_t workspace_bytes) {
    if (int rc = check_arguments("cp_model_prep_host_f32", verts, total, offsets, counts, objects, no_points, diameter_sq, box, keypoints, indices,
                                 status, workspace, workspace_bytes))
        return rc;
    prep_serial(verts, total, offsets, counts, objects, no_points, diameter_sq, box, keypoints, indices, status, workspace);
    return CP_OK;
}

}  // namespace cp
