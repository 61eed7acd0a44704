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

#include "axw_bf16_device.h"  // axw_gemm_bf16_kernel, stage_w, the panel store and the launch helpers: shared with the wide and root files

namespace flex_axw_bf16 {

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
    if (!L || !Wp || !Out || n < kRows || dim <= 0 || dim % 16 != 0 || dim > 256 || cp <= 0 || cp % 64 != 0 || cp > 256 || c <= 0 || c > cp ||
        n_cus <= 0 || misaligned(L) || misaligned(Wp) || misaligned(Out))
        return hipErrorInvalidValue;
    return dispatch_tiles<2, 4, 6, 8>(cp / 32, [&](auto tiles) {
        return launch(axw_gemm_bf16_kernel<decltype(tiles)::value>, dim3(panel_groups(n, 4, n_cus)), 64 * kWaves,
                      static_cast<size_t>(dim) * cp * sizeof(flex_bf16), s, L, Wp, Out, n, dim, c, 0);
    });
}

// The dX product of flex_axw_backward_bf16: dX[n x dim] = G[n x cp] * Wt[cp x dim] on flex_bf16 -- the kernel above with the contraction
// over cp and NT = dim / 32 output tiles, odd counts included; dim is dX's row stride, so there is no padding to mask (c == cp == dim in
// the kernel's terms).  Takes n >= 32, cp % 64 == 0, 0 < cp <= 256, dim % 32 == 0, 0 < dim <= 256, n_cus > 0 and 16-byte aligned G, Wt and
// dX; anything else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_dx_bf16_launch(const flex_bf16 *G, const flex_bf16 *Wt, flex_bf16 *dX, int n, int cp, int dim, int n_cus,
                                              hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!G || !Wt || !dX || n < kRows || cp <= 0 || cp % 64 != 0 || cp > 256 || dim <= 0 || dim % 32 != 0 || dim > 256 || n_cus <= 0 ||
        misaligned(G) || misaligned(Wt) || misaligned(dX))
        return hipErrorInvalidValue;
    return dispatch_tiles<1, 2, 3, 4, 5, 6, 7, 8>(dim / 32, [&](auto tiles) {
        return launch(axw_gemm_bf16_kernel<decltype(tiles)::value>, dim3(panel_groups(n, 4, n_cus)), 64 * kWaves,
                      static_cast<size_t>(cp) * dim * sizeof(flex_bf16), s, G, Wt, dX, n, cp, dim, 0);
    });
}

// Wt[c x dim] := W[dim x c]^T (rows c .. of Wt are not written)
extern "C" hipError_t flex_axw_bf16_transpose_launch(const flex_bf16 *W, flex_bf16 *Wt, int dim, int c, hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!W || !Wt || dim <= 0 || c <= 0) return hipErrorInvalidValue;
    return launch(axw_bf16_transpose_kernel, dim3(static_cast<unsigned>((dim * c + 255) / 256)), 256, 0, s, W, Wt, dim, c);
}

// columns c .. cp-1 of Out[n x cp] := +0 bits; c == cp: nothing to do
extern "C" hipError_t flex_axw_bf16_clear_padding_launch(flex_bf16 *Out, int n, int c, int cp, hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!Out || n <= 0 || c <= 0 || c > cp) return hipErrorInvalidValue;
    if (c == cp) return hipSuccess;
    const int64_t count = static_cast<int64_t>(n) * (cp - c);
    return launch(axw_bf16_clear_padding_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), 256, 0, s, Out, n, c, cp);
}
