// axw_bf16_dw_device.h -- the loader that the two bf16 dW kernels share (axw_dw_bf16_kernel in axw_bf16_backward_kernels.hip: 4 waves, two
// operands, static LDS; axw_dw_bf16_root_kernel in axw_bf16_root_backward_kernels.hip: 6 waves, three operands, a db sum, dynamic LDS), and
// the slice-order sum of their reduce kernels.  The data path is described at the top of axw_bf16_backward_kernels.hip.
// The block load, the transposing store and the walk over a tile's rows are MACROS, as FLEX_AXW_BF16_STORE_PANEL is: as functions (by
// reference, or taking a callable) each of them moved the register allocation and the schedule of both dW kernels (36 -> 46 SGPRs and
// 86 -> 100 VGPRs in axw_dw_bf16_kernel), and this header was to change no instruction of either (profiles/axw_bf16_refactor_isa.txt).
#pragma once
#include "axw_bf16_device.h"  // the vector types, and the launchers' host side

namespace flex_axw_bf16_dw {

using namespace flex_axw_bf16;

constexpr int kStage = 64;  // rows of a stage: four k-steps of 16

// slot of the fragment (k-step s, tile t of `tiles`, row half h, column i of the tile) in an operand's stage.  The eight fragments of a
// loader thread are neighbours in LDS, so the slot of column i is i ^ swz, swz = bit 4 of i | 2 t: 16 lanes write 16 bank groups
__device__ __forceinline__ int frag_slot(int s, int t, int h, int i, int tiles) {
    return ((s * tiles + t) * 2 + h) * 32 + (i ^ (((i >> 4) & 1) | (t << 1)));
}

// a loader thread's 8 x 8 block into u32x4 v[8]: rows r0 .. r0 + 7 of the eight columns at src (rows ld elements apart), one 16-byte load
// a row; a row from r_end on, or the whole block where !ok, is a zero operand and is not loaded
#define FLEX_AXW_DW_LOAD_BLOCK(v, src, ld, r0, r_end, ok)                                                                                  \
    _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                                        \
        const int r = r0 + e;                                                                                                              \
        v[e] = ok && r < r_end ? *reinterpret_cast<const u32x4 *>(src + static_cast<size_t>(r) * ld) : u32x4{0u, 0u, 0u, 0u};              \
    }

// the block of row group rg and column group q of a stage, transposed in registers into eight fragments of an operand of `tiles` tiles at
// dst: v[e][d] holds columns 2 d (low half) and 2 d + 1 of row e; fragment cc is column cc of the eight rows, rows 2 p and 2 p + 1 in word p
#define FLEX_AXW_DW_STORE_BLOCK(v, dst, rg, q, tiles)                                                                                      \
    _Pragma("unroll") for (int cc = 0; cc < 8; ++cc) {                                                                                     \
        u32x4 f;                                                                                                                           \
        _Pragma("unroll") for (int p = 0; p < 4; ++p) {                                                                                    \
            const uint32_t lo = v[2 * p][cc >> 1], hi = v[2 * p + 1][cc >> 1];                                                             \
            f[p] = (cc & 1) ? (lo >> 16) | (hi & 0xFFFF0000u) : (lo & 0xFFFFu) | (hi << 16);                                               \
        }                                                                                                                                  \
        dst[frag_slot(rg >> 1, q >> 2, rg & 1, 8 * (q & 3) + cc, tiles)] = f;                                                              \
    }

// the head of a loop over the 16 entries k of an accumulator tile whose row ii = i0 + 8 (k >> 2) + 4 h + (k & 3) lies below dim
#define FLEX_AXW_DW_FOR_TILE_ROWS(k, ii, i0, h, dim)                                                                                       \
    _Pragma("unroll") for (int k = 0; k < 16; ++k)                                                                                         \
        if (const int ii = i0 + (k & 3) + 8 * (k >> 2) + 4 * (h); ii < dim)

// part[0][e] + part[1][e] + ... + part[slices - 1][e], left to right in fp32, the loads 16 at a time; slices are `count` floats apart
__device__ __forceinline__ float slice_sum(const float *__restrict__ part, int e, int count, int slices) {
    constexpr int kBatch = 16;
    float s = part[e];
    int k = 1;
    for (; k + kBatch <= slices; k += kBatch) {
        float v[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) v[j] = part[static_cast<size_t>(k + j) * count + e];
#pragma unroll
        for (int j = 0; j < kBatch; ++j) s += v[j];
    }
    for (; k < slices; ++k) s += part[static_cast<size_t>(k) * count + e];
    return s;
}

}  // namespace flex_axw_bf16_dw
