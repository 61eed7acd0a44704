// axw_bf16_device.h -- the device code that axw_bf16_kernels.hip (dim <= 256) and axw_bf16_wide_kernels.hip (dim > 256) share: the
// fragment staging of W, the persistent panel loop and the permlane store of a panel's accumulators.  The data path is described at the
// top of axw_bf16_kernels.hip.  The instantiations with kWindow = false compile to the instructions they had in axw_bf16_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "attention_device.h"  // flex_bf16, bf16_bits: the project's one fp32 -> bf16 rounding

namespace flex_axw_bf16 {

using flex::attention::bf16_bits;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kRows = 32;   // rows of a panel: the MFMA's N
constexpr int kWaves = 8;
constexpr int kUnit = 8;    // k-steps (of 16) whose L fragments a wave holds: 256 bytes of each row

// Wp[dim x 32 NT], rows ldw elements apart -> LDS fragments, once per workgroup.  Fragment-lane f = (k-octet kq, column col) gathers
// Wp[8 kq .. 8 kq + 7][col] (eight 2-byte loads, a wave's 64 on 128 contiguous bytes) and writes them as ONE 16-byte LDS store to the slot
// of (s = kq >> 1, t = col >> 5, lane = 32 (kq & 1) + (col & 31)); 16 fragment-lanes in flight a thread.
template <int NT>
__device__ __forceinline__ void stage_w(const flex_bf16 *__restrict__ Wp, u32x4 *sW, int dim, int ldw) {
    constexpr int cp = 32 * NT;
    constexpr int kBatch = 4;
    const int total = (dim >> 3) * cp;
    for (int f0 = threadIdx.x; f0 < total; f0 += kBatch * 64 * kWaves) {
        uint32_t v[kBatch][8];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int f = min(f0 + b * 64 * kWaves, total - 1);  // a slot past the end re-reads the last one and is not written
            const flex_bf16 *src = Wp + static_cast<size_t>(f / cp) * 8 * ldw + f % cp;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[b][e] = src[e * ldw];
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int f = f0 + b * 64 * kWaves;
            if (f < total) {
                const int kq = f / cp, col = f % cp;
                const u32x4 w = {v[b][0] | (v[b][1] << 16), v[b][2] | (v[b][3] << 16), v[b][4] | (v[b][5] << 16), v[b][6] | (v[b][7] << 16)};
                sW[((kq >> 1) * NT + (col >> 5)) * 64 + 32 * (kq & 1) + (col & 31)] = w;
            }
        }
    }
}

// A panel's accumulators acc[NT], rounded to bf16, to the 64 NT bytes at dst = &Out[row of this lane][16 h], h = lane >> 5:
// acc[t][reg] = Out[r0 + j][32 t + 8 (reg >> 2) + 4 h + (reg & 3)]
// A tile that holds padding (a wave-uniform test) masks the rounded bits of its columns >= c to +0: the mask is the sign of
// column - c, integer arithmetic on one register (a compare per element kept 2 SGPRs each alive across the panel loop:
// 192 spilled at NT = 8); the empty asm keeps the 16 masks from being hoisted out of the loop into registers of their own.
// The 8-byte chunks of a row's 64 bytes of a tile alternate between lanes j (h = 0: chunks 0 2 4 6) and j + 32 (1 3 5 7);
// v_permlane32_swap trades chunk 2g + 1 of the lower half for chunk 2g + 4 of the upper, so that h = 0 ends with chunks 0..3 and
// h = 1 with 4..7: 32 contiguous bytes a lane, two 16-byte stores.  Plain stores, not nontemporal ones: a line arrives in
// pieces, which the L2 has to merge before it writes the line back (measured with 8-byte nontemporal stores: the reddit
// shape's 60 MB of Out took 138 us, the time of a read-modify-write of every piece -- DESIGN.md 3.26).
// A macro, not a function: as a function taking acc by reference it changed the register allocation of axw_gemm_bf16_kernel's
// instantiations, whose code the wide kernels' arrival was to leave as it is.
#define FLEX_AXW_BF16_STORE_PANEL(NT, acc, dst, c, h)                                                                             \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) {                                                                              \
        const bool pad = 32 * t + 32 > c;                                                                                         \
        int lim = 32 * t + 4 * h - c; /* column of reg 0, minus c */                                                              \
        asm volatile("" : "+v"(lim));                                                                                             \
        auto bits = [&](int reg) {                                                                                                \
            const uint32_t b = bf16_bits(acc[t][reg]);                                                                            \
            return pad ? b & static_cast<uint32_t>((lim + 8 * (reg >> 2) + (reg & 3)) >> 31) : b;                                 \
        };                                                                                                                        \
        uint32_t w[8]; /* w[2 g], w[2 g + 1]: the lane's chunk g */                                                               \
        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                                           \
            w[2 * g] = bits(4 * g) | (bits(4 * g + 1) << 16);                                                                     \
            w[2 * g + 1] = bits(4 * g + 2) | (bits(4 * g + 3) << 16);                                                             \
        }                                                                                                                         \
        _Pragma("unroll") for (int p = 0; p < 2; ++p) { /* chunk p against chunk p + 2 */                                         \
            const auto lo = __builtin_amdgcn_permlane32_swap(w[2 * p], w[2 * p + 4], false, false);                               \
            const auto hi = __builtin_amdgcn_permlane32_swap(w[2 * p + 1], w[2 * p + 5], false, false);                           \
            const u32x4 v = {lo[0], hi[0], lo[1], hi[1]};                                                                         \
            *reinterpret_cast<u32x4 *>(dst + 32 * t + 8 * p) = v;                                                                 \
        }                                                                                                                         \
    }

// Out[n x 32 NT] = L[n x dim] Wp[dim x 32 NT], the whole Wp in LDS for the life of the workgroup (axw_bf16_kernels.hip).  kWindow (the wide
// dX kernel): Wp and Out are the 32 NT columns from 256 blockIdx.y on of arrays whose rows are ld elements apart.
template <int NT, bool kWindow = false>  // 32-column tiles of Out: cp = 32 NT
__global__ __launch_bounds__(64 * kWaves) void axw_gemm_bf16_kernel(const flex_bf16 *__restrict__ L, const flex_bf16 *__restrict__ Wp,
                                                                    flex_bf16 *__restrict__ Out, int n, int dim, int c, int ld) {
    extern __shared__ u32x4 sW[];  // [dim / 16][NT][64] fragments of 8 bf16
    const int ldw = kWindow ? ld : 32 * NT, ldo = ldw;
    if constexpr (kWindow) {
        Wp += 256 * blockIdx.y;
        Out += 256 * blockIdx.y;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int steps = dim >> 4;
    const int n_panels = (n + kRows - 1) / kRows;
    auto panel_row = [&](int pnl) { return min(min(pnl, n_panels - 1) * kRows, n - kRows); };  // past the end: the last panel again
    const int first_panel = wave < 4 ? blockIdx.x * 4 + wave : gridDim.x * 4 + blockIdx.x * 4 + (wave - 4);
    const int panel_step = gridDim.x * kWaves;
    // this lane's 16 bytes of k-step s of a panel
    auto lfrag = [&](int pnl, int s) {
        return *reinterpret_cast<const bf16x8 *>(L + static_cast<size_t>(panel_row(pnl) + j) * dim + 16 * s + 8 * h);
    };

    bf16x8 pre[kUnit] = {};  // the L fragments of the unit about to be multiplied
#pragma unroll
    for (int q = 0; q < kUnit; ++q)
        if (q < steps) pre[q] = lfrag(first_panel, q);
    stage_w<NT>(Wp, sW, dim, ldw);
    __syncthreads();  // the only barrier

    const bf16x8 *wf = reinterpret_cast<const bf16x8 *>(sW) + lane;
    for (int panel = first_panel; panel < n_panels; panel += panel_step) {
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
        for (int s0 = 0; s0 < steps; s0 += kUnit) {
            const bool last = s0 + kUnit >= steps;  // wave-uniform, like everything that guards a load or an MFMA below
            const int np = last ? panel + panel_step : panel, ns0 = last ? 0 : s0 + kUnit;
            const int n_cur = min(kUnit, steps - s0), n_next = min(kUnit, steps - ns0);
#pragma unroll
            for (int q = 0; q < kUnit; ++q) {
                const bf16x8 b = pre[q];
                if (q < n_next) pre[q] = lfrag(np, ns0 + q);
                if (q < n_cur) {
                    const bf16x8 *w = wf + (s0 + q) * (NT * 64);
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t * 64], b, acc[t], 0, 0, 0);
                }
            }
        }
        flex_bf16 *dst = Out + static_cast<size_t>(panel_row(panel) + j) * ldo + 16 * h;
        FLEX_AXW_BF16_STORE_PANEL(NT, acc, dst, c, h)
    }
}

}  // namespace flex_axw_bf16
