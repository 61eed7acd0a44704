// attention_device.h -- what the kernels of the fused attention share (device side): the view of the row walk and the column, dot,
// axpy and slot-reduction helpers of attention_kernels.hip (flex_attention) and attention_backward_kernels.hip (flex_attention_backward).
#pragma once
#include <cstdint>

#include "internal.h"

namespace flex {
namespace attention {

struct View {
    const uint32_t *rowptr;  // the plan's rows, entries as hostA numbers them
    const uint32_t *src;     // K / V row of entry e at src[e - e0]
    const uint4 *item;
    const uint32_t *grp;
    uint32_t e0;
    uint32_t n_groups, n_wave_items, n_block_rows;
    uint32_t xcd_remap;
    int32_t k, ldb, ldc;
};

constexpr int U = static_cast<int>(kAtPass);
static_assert(U == 4, "the slot reduction below hands four scores to every lane");

// columns c .. c + 3 of a row; a column at or past k is not read and reads as 0
template <bool VEC>
__device__ __forceinline__ float4 load_cols(const float *__restrict__ row, int c, int k) {
    if constexpr (VEC) {
        if (c < k) return *reinterpret_cast<const float4 *>(row + c);
        return make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < k) r.x = row[c];
        if (c + 1 < k) r.y = row[c + 1];
        if (c + 2 < k) r.z = row[c + 2];
        if (c + 3 < k) r.w = row[c + 3];
        return r;
    }
}

template <bool VEC>
__device__ __forceinline__ void store_cols(float *__restrict__ row, int c, int k, const float4 &x) {
    if constexpr (VEC) {
        if (c < k) *reinterpret_cast<float4 *>(row + c) = x;
    } else {
        if (c < k) row[c] = x.x;
        if (c + 1 < k) row[c + 1] = x.y;
        if (c + 2 < k) row[c + 2] = x.z;
        if (c + 3 < k) row[c + 3] = x.w;
    }
}

// sum over the lane's columns of q * b; columns at or past k add nothing (not even 0 x b)
template <bool VEC>
__device__ __forceinline__ float dot_cols(float acc, const float4 &q, const float4 &b, int c, int k) {
    if (c < k) acc = __builtin_fmaf(q.x, b.x, acc);
    if (VEC ? c < k : c + 1 < k) acc = __builtin_fmaf(q.y, b.y, acc);  // VEC: k % 4 == 0, the four columns stand or fall together
    if (VEC ? c < k : c + 2 < k) acc = __builtin_fmaf(q.z, b.z, acc);
    if (VEC ? c < k : c + 3 < k) acc = __builtin_fmaf(q.w, b.w, acc);
    return acc;
}

// acc += t * v on the lane's columns; columns at or past k hold v = 0 and stay 0
__device__ __forceinline__ void axpy(float4 &acc, float t, const float4 &v) {
    acc.x = __builtin_fmaf(t, v.x, acc.x);
    acc.y = __builtin_fmaf(t, v.y, acc.y);
    acc.z = __builtin_fmaf(t, v.z, acc.z);
    acc.w = __builtin_fmaf(t, v.w, acc.w);
}
__device__ __forceinline__ float4 scaled(const float4 &a, float f) { return make_float4(a.x * f, a.y * f, a.z * f, a.w * f); }
__device__ __forceinline__ float4 shfl_xor4(const float4 &a, int off) {
    return make_float4(__shfl_xor(a.x, off), __shfl_xor(a.y, off), __shfl_xor(a.z, off), __shfl_xor(a.w, off));
}

// The four totals of the four per-lane partial sums over the W lanes of a slot, on every lane: the SDDMM's transposed reduction (two
// exchange steps leave each lane one record), a butterfly over the rest, and two exchange steps back.  Every addition has the same two
// operands on both lanes of its pair, so all lanes of the slot hold the same bits.
template <int W>
__device__ __forceinline__ void slot_totals(const float (&pr)[U], uint32_t li, float (&s)[U]) {
    const bool hi2 = (li & (W / 2)) != 0, hi4 = (li & (W / 4)) != 0;
    const float a0 = (hi2 ? pr[2] : pr[0]) + __shfl_xor(hi2 ? pr[0] : pr[2], W / 2);
    const float a1 = (hi2 ? pr[3] : pr[1]) + __shfl_xor(hi2 ? pr[1] : pr[3], W / 2);
    float t = (hi4 ? a1 : a0) + __shfl_xor(hi4 ? a0 : a1, W / 4);  // record 2 hi2 + hi4
#pragma unroll
    for (int o = W / 8; o >= 1; o >>= 1) t += __shfl_xor(t, o);
    const float x = __shfl_xor(t, W / 4);  // record 2 hi2 + !hi4
    const float even = hi4 ? x : t, odd = hi4 ? t : x;
    const float oe = __shfl_xor(even, W / 2), oo = __shfl_xor(odd, W / 2);
    s[0] = hi2 ? oe : even;
    s[1] = hi2 ? oo : odd;
    s[2] = hi2 ? even : oe;
    s[3] = hi2 ? odd : oo;
}

}  // namespace attention
}  // namespace flex
