// axw_bf16_kernels.hip -- the dense half of the bf16 A*X*W layer (libflex_axw.so, FLEX_AXW_BF16):
//   Out[n x cp] = L[n x dim] * Wp[dim x cp], row-major flex_bf16, fp32 sums on the bf16 MFMA, one rounding to bf16 at the store;
//   n tall (10^5..10^6), dim <= 256 (a multiple of 16), cp <= 256 (a multiple of 64).
// At bf16 the matrix unit is far ahead of what streaming (n dim + n cp) 2 bytes can feed (v_mfma_f32_32x32x16_bf16: 32 K FLOP in 32
// cycles; a 32-row panel at dim = cp = 128 is 32 of them, 256 cycles a CU over four SIMDs, against 16 KiB of HBM traffic), so
// nothing of the fp32 kernel's data path (axw_kernels.hip) is kept:
//   * L is never staged.  The operands are swapped: Wp^T is the MFMA's A operand and L its B operand, D[i][j] = Out[row j][col i].
//     The B operand of lane l at k-step s is L[r0 + (l & 31)][16 s + 8 (l >> 5) .. + 7]: 16 contiguous bytes, ONE global load.  The
//     k-steps run in ascending order, so four consecutive load instructions of a wave cover one whole 128-byte line of each of the
//     panel's 32 rows (the L1 merges the four quarter-line requests, which leave back to back, into one miss).
//     32x32x16 against 16x16x32: a 16x16x32 load covers 64 bytes of 16 rows, a 32x32x16 load 32 bytes of 32 rows -- the same 1 KiB an
//     instruction and the same whole lines every four (two) instructions; 32x32x16 is taken because it halves the MFMA and LDS-read
//     instructions per FLOP (one W fragment feeds 32 rows without a second register copy), which is what keeps the LDS (W is re-read
//     for every panel: as many cycles as the MFMAs themselves) off the critical path.  The alternative was not measured.
//   * Wp sits in LDS for the whole launch as ready-made fragments: [k-step s][32-column tile t][lane l][8 k values], so the A operand
//     of lane l is one 16-byte LDS read and a wave's 64 reads are 1 KiB in a row: no bank conflict.  The whole cp <= 256 is ONE pass
//     (128 KiB of LDS at 256 x 256; 8 tiles x 16 accumulator registers).
//   * C/D layout: lane l holds D column j = l & 31 -- ONE row of Out -- and D rows i = 8 (reg >> 2) + 4 (l >> 5) + (reg & 3): runs of
//     four consecutive columns, rounded and packed into 8-byte chunks; lanes j and j + 32 trade chunks (v_permlane32_swap) so that each
//     stores 32 contiguous bytes as two 16-byte stores.
//   * one workgroup of 8 waves per CU, persistent over full 32-row panels; the last panel starts at n - 32 and overlaps its predecessor
//     (both write the same bits), so no load or store carries a row guard.  Panels are dealt as in axw_kernels.hip: waves w and w + 4
//     share a SIMD, and the second wave of a SIMD gets a panel only after every SIMD of every workgroup has one.
//   * the L fragments of the NEXT unit (8 k-steps: two lines of each row; the next panel's first unit after a panel's last) are loaded
//     into the registers of the current one as its MFMAs consume them: 8 KiB in flight a wave, 64 KiB a CU, through the MFMAs and
//     the stores.
//   * columns c .. cp-1 of Out are +0 bits whatever L holds (a zero column of Wp times an inf or NaN of L would be NaN), cleared in the
//     accumulators of the tiles that hold padding only (a wave-uniform test).
//   * k order of every dot product: k-step by k-step into one fp32 accumulator; inside a step the unit's own sum of 16 products
//     (DESIGN.md 3.26 for what was measured of it).
#include <hip/hip_runtime.h>

#include <algorithm>
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

// Wp[dim x cp] -> LDS fragments, once per workgroup.  Fragment-lane f = (k-octet kq, column col) gathers Wp[8 kq .. 8 kq + 7][col]
// (eight 2-byte loads, a wave's 64 on 128 contiguous bytes) and writes them as ONE 16-byte LDS store to the slot of
// (s = kq >> 1, t = col >> 5, lane = 32 (kq & 1) + (col & 31)); 16 fragment-lanes in flight a thread.
template <int NT>
__device__ __forceinline__ void stage_w(const flex_bf16 *__restrict__ Wp, u32x4 *sW, int dim) {
    constexpr int cp = 32 * NT;
    constexpr int kBatch = 4;
    const int total = (dim >> 3) * cp;
    for (int f0 = threadIdx.x; f0 < total; f0 += kBatch * 64 * kWaves) {
        uint32_t v[kBatch][8];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int f = min(f0 + b * 64 * kWaves, total - 1);  // a slot past the end re-reads the last one and is not written
            const flex_bf16 *src = Wp + static_cast<size_t>(f / cp) * 8 * cp + f % cp;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[b][e] = src[e * cp];
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

template <int NT>  // 32-column tiles of Out: cp = 32 NT
__global__ __launch_bounds__(64 * kWaves) void axw_gemm_bf16_kernel(const flex_bf16 *__restrict__ L, const flex_bf16 *__restrict__ Wp,
                                                                    flex_bf16 *__restrict__ Out, int n, int dim, int c) {
    extern __shared__ u32x4 sW[];  // [dim / 16][NT][64] fragments of 8 bf16
    constexpr int cp = 32 * NT;
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
    stage_w<NT>(Wp, sW, dim);
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
        // acc[t][reg] = Out[r0 + j][32 t + 8 (reg >> 2) + 4 h + (reg & 3)]
        // A tile that holds padding (a wave-uniform test) masks the rounded bits of its columns >= c to +0: the mask is the sign of
        // column - c, integer arithmetic on one register (a compare per element kept 2 SGPRs each alive across the panel loop:
        // 192 spilled at NT = 8); the empty asm keeps the 16 masks from being hoisted out of the loop into registers of their own.
        // The 8-byte chunks of a row's 64 bytes of a tile alternate between lanes j (h = 0: chunks 0 2 4 6) and j + 32 (1 3 5 7);
        // v_permlane32_swap trades chunk 2g + 1 of the lower half for chunk 2g + 4 of the upper, so that h = 0 ends with chunks 0..3 and
        // h = 1 with 4..7: 32 contiguous bytes a lane, two 16-byte stores.  Plain stores, not nontemporal ones: a line arrives in
        // pieces, which the L2 has to merge before it writes the line back (measured with 8-byte nontemporal stores: the reddit
        // shape's 60 MB of Out took 138 us, the time of a read-modify-write of every piece -- DESIGN.md 3.26).
        flex_bf16 *dst = Out + static_cast<size_t>(panel_row(panel) + j) * cp + 16 * h;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const bool pad = 32 * t + 32 > c;
            int lim = 32 * t + 4 * h - c;  // column of reg 0, minus c
            asm volatile("" : "+v"(lim));
            auto bits = [&](int reg) {
                const uint32_t b = bf16_bits(acc[t][reg]);
                return pad ? b & static_cast<uint32_t>((lim + 8 * (reg >> 2) + (reg & 3)) >> 31) : b;
            };
            uint32_t w[8];  // w[2 g], w[2 g + 1]: the lane's chunk g
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                w[2 * g] = bits(4 * g) | (bits(4 * g + 1) << 16);
                w[2 * g + 1] = bits(4 * g + 2) | (bits(4 * g + 3) << 16);
            }
#pragma unroll
            for (int p = 0; p < 2; ++p) {  // chunk p against chunk p + 2
                const auto lo = __builtin_amdgcn_permlane32_swap(w[2 * p], w[2 * p + 4], false, false);
                const auto hi = __builtin_amdgcn_permlane32_swap(w[2 * p + 1], w[2 * p + 5], false, false);
                const u32x4 v = {lo[0], hi[0], lo[1], hi[1]};
                *reinterpret_cast<u32x4 *>(dst + 32 * t + 8 * p) = v;
            }
        }
    }
}

// columns c .. cp-1 of an n x cp array := +0 bits (after the SpMM of order A_XW on a non-finite A).  One thread per (row, padding
// column); a kernel, not a 2-D memset, so that a captured graph replays it like any other launch
__global__ __launch_bounds__(256) void axw_bf16_clear_padding_kernel(flex_bf16 *__restrict__ Out, int n, int c, int cp) {
    const int w = cp - c;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (e < static_cast<int64_t>(n) * w) Out[(e / w) * cp + c + e % w] = 0;
}

// Wt[k][i] = W[i][k] for i < dim, k < c (W: dim x c, Wt: dim elements a row); Wt's other rows are left as they are: the twin of
// axw_transpose_kernel, for the dX product of flex_axw_backward_bf16
__global__ __launch_bounds__(256) void axw_bf16_transpose_kernel(const flex_bf16 *__restrict__ W, flex_bf16 *__restrict__ Wt, int dim, int c) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= dim * c) return;
    const int k = e / dim, i = e % dim;
    Wt[static_cast<size_t>(k) * dim + i] = W[static_cast<size_t>(i) * c + k];
}

}  // namespace flex_axw_bf16

// Out[n x cp] = L[n x dim] * Wp[dim x cp] on flex_bf16, columns c .. cp-1 of Out written as +0.  Takes n >= 32, dim % 16 == 0,
// 0 < dim <= 256, cp % 64 == 0, 0 < c <= cp <= 256, n_cus > 0 and 16-byte aligned L, Wp and Out; anything else returns
// hipErrorInvalidValue before a launch.  Returns hipSuccess or the launch error.
extern "C" hipError_t flex_axw_gemm_bf16_launch(const flex_bf16 *L, const flex_bf16 *Wp, flex_bf16 *Out, int n, int dim, int c, int cp,
                                                int n_cus, hipStream_t s) {
    using namespace flex_axw_bf16;
    const auto misaligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    if (!L || !Wp || !Out || n < kRows || dim <= 0 || dim % 16 != 0 || dim > 256 || cp <= 0 || cp % 64 != 0 || cp > 256 || c <= 0 || c > cp ||
        n_cus <= 0 || misaligned(L) || misaligned(Wp) || misaligned(Out))
        return hipErrorInvalidValue;
    const int n_panels = (n + kRows - 1) / kRows;
    const size_t lds = static_cast<size_t>(dim) * cp * sizeof(flex_bf16);
    const dim3 grid(static_cast<unsigned>(std::min(n_cus, (n_panels + 3) / 4))), block(64 * kWaves);  // no workgroup without a panel
    hipError_t e = hipSuccess;
    auto go = [&](auto kernel) {  // more than 64 KiB of dynamic LDS has to be asked for
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return;
        hipLaunchKernelGGL(kernel, grid, block, lds, s, L, Wp, Out, n, dim, c);
        e = hipGetLastError();
    };
    switch (cp / 32) {
        case 2: go(axw_gemm_bf16_kernel<2>); break;
        case 4: go(axw_gemm_bf16_kernel<4>); break;
        case 6: go(axw_gemm_bf16_kernel<6>); break;
        default: go(axw_gemm_bf16_kernel<8>); break;
    }
    return e;
}

// The dX product of flex_axw_backward_bf16: dX[n x dim] = G[n x cp] * Wt[cp x dim] on flex_bf16 -- the kernel above with the contraction
// over cp and NT = dim / 32 output tiles, odd counts included; dim is dX's row stride, so there is no padding to mask (c == cp == dim in
// the kernel's terms).  Takes n >= 32, cp % 64 == 0, 0 < cp <= 256, dim % 32 == 0, 0 < dim <= 256, n_cus > 0 and 16-byte aligned G, Wt and
// dX; anything else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_dx_bf16_launch(const flex_bf16 *G, const flex_bf16 *Wt, flex_bf16 *dX, int n, int cp, int dim, int n_cus,
                                              hipStream_t s) {
    using namespace flex_axw_bf16;
    const auto misaligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; };
    if (!G || !Wt || !dX || n < kRows || cp <= 0 || cp % 64 != 0 || cp > 256 || dim <= 0 || dim % 32 != 0 || dim > 256 || n_cus <= 0 ||
        misaligned(G) || misaligned(Wt) || misaligned(dX))
        return hipErrorInvalidValue;
    const int n_panels = (n + kRows - 1) / kRows;
    const size_t lds = static_cast<size_t>(cp) * dim * sizeof(flex_bf16);
    const dim3 grid(static_cast<unsigned>(std::min(n_cus, (n_panels + 3) / 4))), block(64 * kWaves);
    hipError_t e = hipSuccess;
    auto go = [&](auto kernel) {
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return;
        hipLaunchKernelGGL(kernel, grid, block, lds, s, G, Wt, dX, n, cp, dim);
        e = hipGetLastError();
    };
    switch (dim / 32) {
        case 1: go(axw_gemm_bf16_kernel<1>); break;
        case 2: go(axw_gemm_bf16_kernel<2>); break;
        case 3: go(axw_gemm_bf16_kernel<3>); break;
        case 4: go(axw_gemm_bf16_kernel<4>); break;
        case 5: go(axw_gemm_bf16_kernel<5>); break;
        case 6: go(axw_gemm_bf16_kernel<6>); break;
        case 7: go(axw_gemm_bf16_kernel<7>); break;
        default: go(axw_gemm_bf16_kernel<8>); break;
    }
    return e;
}

// Wt[c x dim] := W[dim x c]^T (rows c .. of Wt are not written)
extern "C" hipError_t flex_axw_bf16_transpose_launch(const flex_bf16 *W, flex_bf16 *Wt, int dim, int c, hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!W || !Wt || dim <= 0 || c <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(axw_bf16_transpose_kernel, dim3(static_cast<unsigned>((dim * c + 255) / 256)), dim3(256), 0, s, W, Wt, dim, c);
    return hipGetLastError();
}

// columns c .. cp-1 of Out[n x cp] := +0 bits; c == cp: nothing to do
extern "C" hipError_t flex_axw_bf16_clear_padding_launch(flex_bf16 *Out, int n, int c, int cp, hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!Out || n <= 0 || c <= 0 || c > cp) return hipErrorInvalidValue;
    if (c == cp) return hipSuccess;
    const int64_t count = static_cast<int64_t>(n) * (cp - c);
    hipLaunchKernelGGL(axw_bf16_clear_padding_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, s, Out, n, c, cp);
    return hipGetLastError();
}
