// Operand arithmetic and small helpers shared by the matrix-pipe kernels: vector types, the LDS hand-over barrier, static_for, the exact three-way
// bf16 split, the bf16 roundings and the transposed LDS fragment read.  (The fp16 two-way split "f16x2" and its contract: split_f16.h.)
//
// The exact bf16 split.  Every fp32 operand x is split into three bf16 terms of 8 + 8 + 8 significand bits:
//     hi = trunc_bf16(x),   mid = trunc_bf16(x - hi),   lo = x - hi - mid
// (trunc_bf16 = the top 16 bits of the fp32 pattern).  Both subtractions are exact in fp32, and the last remainder has at most 8 significant bits,
// so taking its top half is exact too: hi + mid + lo == x for every finite x whose low terms stay normal fp32 numbers.  A product of two bf16
// numbers is exact in the fp32 accumulator of v_mfma_f32_32x32x16_bf16, so the six products
//     lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi          (weight / A plane first; issued in THIS order: smallest terms first)
// accumulate to the fp32 product; the three dropped ones (mid*lo, lo*mid, lo*lo) are <= 2^-24 of the full product -- the rounding an fp32 multiply
// makes anyway.  This is the "fp32-equivalent" mode (planes = 3) whose kernels are gated at the fp32 kernels' tolerance; six bf16 MFMAs of K = 16
// take 6 x 32 cycles where the fp32 MFMA needs 8 x 64.  Two planes (hi, mid: the last three products) and one plane (operands rounded to nearest
// even, round4 / round8 below) are the bf16 modes and NOT fp32-equivalent.
#pragma once
#include "split_f16.h"

#include <type_traits>

namespace cp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));   // (also the container of a 16-byte fp16 fragment)
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// LDS hand-over between the waves of a block: this wave's LDS accesses have retired, then the barrier (global loads stay in flight across it)
#define CP_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// f(integral_constant<int, I>) for I in [I, N): a loop whose index is a compile-time constant in the body
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// [hi16(a_lo), hi16(b_hi)] in one v_perm_b32.  perm(src0, src1, sel): byte k of the result = byte sel[k] of {src0 (bytes 4-7), src1 (bytes 0-3)}
__device__ __forceinline__ unsigned pack_hi16(unsigned a_lo, unsigned b_hi) { return __builtin_amdgcn_perm(b_hi, a_lo, 0x07060302u); }

// the exact three-way split of N floats: fp32 bit patterns whose top halves are the bf16 terms
template <int N>
__device__ __forceinline__ void split_bits(const float (&x)[N], unsigned (&h)[N], unsigned (&m)[N], unsigned (&l)[N]) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
        h[e] = __builtin_bit_cast(unsigned, x[e]);
        const float r1 = x[e] - __builtin_bit_cast(float, h[e] & 0xffff0000u);
        m[e] = __builtin_bit_cast(unsigned, r1);
        const float r2 = r1 - __builtin_bit_cast(float, m[e] & 0xffff0000u);
        l[e] = __builtin_bit_cast(unsigned, r2);
    }
}
// round-to-nearest-even bf16 in integer arithmetic: the result is the top half (finite inputs; NaN payloads are not preserved bit for bit, which no
// caller needs)
template <int N>
__device__ __forceinline__ void round_bits(const float (&x)[N], unsigned (&r)[N]) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const unsigned u = __builtin_bit_cast(unsigned, x[e]);
        r[e] = u + 0x7fffu + ((u >> 16) & 1u);
    }
}
__device__ __forceinline__ uint2 pack4(const unsigned (&b)[4]) { return make_uint2(pack_hi16(b[0], b[1]), pack_hi16(b[2], b[3])); }
__device__ __forceinline__ uint4 pack8(const unsigned (&b)[8]) {
    return make_uint4(pack_hi16(b[0], b[1]), pack_hi16(b[2], b[3]), pack_hi16(b[4], b[5]), pack_hi16(b[6], b[7]));
}

// four / eight floats -> packed bf16 planes
__device__ __forceinline__ void split4(const float4 v, uint2& hi, uint2& mid, uint2& lo) {
    const float x[4] = {v.x, v.y, v.z, v.w};
    unsigned h[4], m[4], l[4];
    split_bits(x, h, m, l);
    hi = pack4(h);
    mid = pack4(m);
    lo = pack4(l);
}
__device__ __forceinline__ void split8(const float4 v0, const float4 v1, uint4& hi, uint4& mid, uint4& lo) {
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    unsigned h[8], m[8], l[8];
    split_bits(x, h, m, l);
    hi = pack8(h);
    mid = pack8(m);
    lo = pack8(l);
}
__device__ __forceinline__ uint2 round4(const float4 v) {
    const float x[4] = {v.x, v.y, v.z, v.w};
    unsigned r[4];
    round_bits(x, r);
    return pack4(r);
}
__device__ __forceinline__ uint4 round8(const float4 v0, const float4 v1) {
    const float x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    unsigned r[8];
    round_bits(x, r);
    return pack8(r);
}
// the same rounding by the hardware convert (two v_cvt_pk_bf16_f32, gfx950): another instruction stream (conv_bf16d.hip), kept apart from round4
__device__ __forceinline__ uint2 round4_cvt(const float4 v) {
    const f32x2 a = {v.x, v.y}, b = {v.z, v.w};
    return make_uint2(__builtin_bit_cast(unsigned, __builtin_convertvector(a, bf16x2)), __builtin_bit_cast(unsigned, __builtin_convertvector(b, bf16x2)));
}

// An MFMA operand fragment out of a pixel-major LDS image ([row][32 channels] = 64-byte rows of bf16 / fp16): 8 consecutive rows (the MFMA's k) of
// this lane's channel, two transpose reads (ds_read_b64_tr_b16) of 4 rows each
__device__ __forceinline__ bf16x8 frag_tr(const unsigned char* a) {
    typedef s16x4 __attribute__((address_space(3))) * lds_p;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(a + 4 * 64));
    const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, v);
}

}  // namespace cp
