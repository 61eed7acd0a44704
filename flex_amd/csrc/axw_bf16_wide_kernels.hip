// axw_bf16_wide_kernels.hip -- the dense half of the bf16 A*X*W layer at input-layer widths, 256 < dim <= 4096 (libflex_axw.so,
// FLEX_AXW_BF16; axw_bf16_kernels.hip and axw_bf16_backward_kernels.hip serve dim <= 256):
//   forward  Out[n x cp] = L[n x dim] W[dim x c]   a long contraction: W no longer fits the LDS (dim x cp x 2 bytes: 256 KiB at 512 x 256)
//   dX       dX[n x dim] = G[n x cp] Wt[cp x dim]  a wide output: more accumulator tiles than a wave has registers for
//   dW       dW[dim x c] = X[n x dim]^T G[n x cp]  the 128 x 128-block kernel as it is, under a slice rule that bounds its fp32 partials
// Forward.  The L side is that of axw_bf16_kernels.hip: operands swapped (Wp^T the MFMA's A operand, L its B operand, 16 bytes of one row
// a lane straight from global memory), v_mfma_f32_32x32x16_bf16, the k-steps in ascending order into ONE fp32 accumulator per entry (no
// split of the contraction across waves or workgroups), the permlane store, the overlapping last panel, padding columns masked to +0.
// The kernel is axw_gemm_bf16_stream_kernel<NT, P, Stream::kWide> (axw_bf16_device.h): the body that the root forward and the root dX of
// axw_bf16_root_kernels.hip instantiate with two sources.  Its W side:
//   * pack once: axw_bf16_pack_kernel (axw_bf16_root_kernels.hip, d2 = 0) turns W[dim x c] into the fragment order [k-step s][32-column tile t][lane][8 k values] in global
//     memory, zero padding columns included (dim x cp x 2 bytes, once per call: the eight 2-byte loads per fragment of stage_w are
//     paid once, not once per round of panels).  A slab of kSlab = 8 k-steps (128 values of k, 256 bytes of each L row -- the unit whose
//     L fragments a wave holds) is then 8 NT KiB of CONTIGUOUS memory in exactly the order the LDS wants.
//   * stream after: the slabs pass through two LDS buffers of 8 NT KiB each (128 KiB at cp = 256).  A round is the workgroup's 8 waves
//     times P panels; the waves keep their panels' accumulators across all slabs of dim.  While the MFMAs of k-step q of the current
//     slab run, every thread loads 16 bytes of k-step q of the NEXT slab (one global_load_dwordx4: a wave's 64 are 1 KiB in a row) and
//     writes the 16 bytes it loaded two k-steps earlier into the other buffer (one ds_write_b128, the same 1 KiB in a row: no bank
//     conflict): three loads in flight a thread, 12 registers.  ONE barrier per slab: the buffer written during slab i was last read
//     during slab i - 1, before the barrier that opened slab i.  The slab after a round's last is the next round's first, so the
//     stream never drains between rounds.
//   * rows per pass: P = 2 panels a wave at cp = 64 (NT = 2), else 1.  At NT = 4 two panels are 128 accumulator registers and 64 of L
//     fragments, and with the staging registers the compiler spilled 114 VGPRs; one panel it is.  Every round re-reads W from the L2:
//     W-to-L bytes = cp / (256 P): 1/8 at cp = 64, 1/2 at 128, 3/4 at 192, 1 at 256 -- at most as much again as L, from the L2 (W is at most
//     2 MiB), not from HBM.  With P = 2 one W fragment read from LDS feeds both panels.
// dX.  Output-column passes of 256 columns (8 tiles) and one narrower last pass: each is axw_gemm_bf16_kernel itself (axw_bf16_device.h,
// kWindow) on a cp x 256 window of W^T, held in LDS as fragments for the life of the workgroup (at most 128 KiB), writing its columns of
// dX at row stride dim.  The full passes are a grid dimension, the narrower last pass a launch of its own: it is another instantiation
// (fewer tiles), and as a grid dimension the passes need no barrier or restaging inside the persistent loop -- a CU whose workgroup of
// pass p has ended takes one of pass p + 1.  G is read once per pass: cp / 256 <= 1 of the bytes of dX that the pass writes.
// dW.  flex_axw_dw_bf16_rows_launch (axw_bf16_backward_kernels.hip) with rows from dw_wide_rows below.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "axw_bf16_device.h"

extern "C" hipError_t flex_axw_dw_bf16_rows_launch(const flex_bf16 *X, const flex_bf16 *G, flex_bf16 *dW, float *part, int n, int dim, int c,
                                                   int cp, int rows, hipStream_t s);  // axw_bf16_backward_kernels.hip

namespace flex_axw_bf16 {

// rows of an n-slice of the wide dW: ceil(n / S0) rounded up to a whole number of stages, S0 the smallest of
//   ceil(n / 256)                      about 256 rows a slice, as the narrow rule,
//   ceil(2 n_cus / blocks)             two workgroups a CU (64 KiB of LDS each) over the blocks = ceil(dim / 128) ceil(c / 128) of dW,
//   floor(n / (2 c))                   slices x dim x c x 4 bytes of partials <= n x dim x 2 bytes, the bytes of X,
// and at least 1.  slices = ceil(n / rows) <= S0, and no slice is empty.
inline int dw_wide_rows(int n, int dim, int c, int n_cus) {
    const int blocks = ((dim + 127) / 128) * ((c + 127) / 128);
    const int s0 = std::max(1, std::min({(n + 255) / 256, (2 * n_cus + blocks - 1) / blocks, n / (2 * c)}));
    return ((n + s0 - 1) / s0 + 63) / 64 * 64;
}

inline bool wide_dim(int dim, int multiple) { return dim > 256 && dim <= 4096 && dim % multiple == 0; }

}  // namespace flex_axw_bf16

// Out[n x cp] = L[n x dim] * W[dim x c] on flex_bf16, columns c .. cp-1 of Out written as +0, through Wf (dim x cp elements of scratch:
// W in fragment order).  Takes n >= 32, 256 < dim <= 4096, dim % 16 == 0, cp % 64 == 0, 0 < c <= cp <= 256, n_cus > 0 and 16-byte aligned
// L, Wf and Out (W: any flex_bf16 pointer); anything else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_gemm_bf16_wide_launch(const flex_bf16 *L, const flex_bf16 *W, flex_bf16 *Wf, flex_bf16 *Out, int n, int dim, int c,
                                                     int cp, int n_cus, hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!L || !W || !Wf || !Out || n < kRows || !wide_dim(dim, 16) || cp <= 0 || cp % 64 != 0 || cp > 256 || c <= 0 || c > cp || n_cus <= 0 ||
        misaligned(L) || misaligned(Wf) || misaligned(Out))
        return hipErrorInvalidValue;
    u32x4 *wf = reinterpret_cast<u32x4 *>(Wf);
    const hipError_t e = pack_launch(W, nullptr, wf, dim, 0, c, cp / 32, s);
    if (e != hipSuccess) return e;
    return dispatch_tiles<2, 4, 6, 8>(cp / 32, [&](auto tiles) {
        constexpr int NT = decltype(tiles)::value, P = stream_panels(NT);
        return launch(axw_gemm_bf16_stream_kernel<NT, P, Stream::kWide>, dim3(panel_groups(n, kWaves * P, n_cus)), 64 * kWaves, stream_lds(NT), s, L,
                      dim, nullptr, 0, wf, nullptr, nullptr, Out, n, c);
    });
}

// dX[n x dim] = G[n x cp] * Wt[cp x dim] on flex_bf16.  Takes n >= 32, cp % 64 == 0, 0 < cp <= 256, 256 < dim <= 4096, dim % 32 == 0,
// n_cus > 0 and 16-byte aligned G, Wt and dX; anything else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_dx_bf16_wide_launch(const flex_bf16 *G, const flex_bf16 *Wt, flex_bf16 *dX, int n, int cp, int dim, int n_cus,
                                                   hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!G || !Wt || !dX || n < kRows || cp <= 0 || cp % 64 != 0 || cp > 256 || !wide_dim(dim, 32) || n_cus <= 0 || misaligned(G) ||
        misaligned(Wt) || misaligned(dX))
        return hipErrorInvalidValue;
    const int full = dim / 256, tail = dim % 256;
    auto windows = [&](auto tiles, int passes, int col0) {  // `passes` windows of 32 NT columns of dX from column col0 on
        constexpr int NT = decltype(tiles)::value;
        return launch(axw_gemm_bf16_kernel<NT, true>, dim3(panel_groups(n, 4, n_cus), static_cast<unsigned>(passes)), 64 * kWaves,
                      static_cast<size_t>(cp) * 32 * NT * sizeof(flex_bf16), s, G, Wt + col0, dX + col0, n, cp, 32 * NT, dim);
    };
    const hipError_t e = windows(std::integral_constant<int, 8>(), full, 0);
    if (e != hipSuccess || tail == 0) return e;
    return dispatch_tiles<1, 2, 3, 4, 5, 6, 7>(tail / 32, [&](auto tiles) { return windows(tiles, 1, 256 * full); });
}

// n-slices of the wide bf16 dW: ceil(n / rows), rows = dw_wide_rows above; 0 for arguments the launcher refuses
extern "C" int flex_axw_dw_bf16_wide_slices(int n, int dim, int c, int n_cus) {
    if (n <= 0 || dim <= 0 || c <= 0 || n_cus <= 0) return 0;
    const int rows = flex_axw_bf16::dw_wide_rows(n, dim, c, n_cus);
    return (n + rows - 1) / rows;
}

// dW[dim x c] = rn_bf16(X[n x dim]^T G[n x cp]) through `part` (flex_axw_dw_bf16_wide_slices(n, dim, c, n_cus) * dim * c floats).  Takes
// n >= 32, 256 < dim <= 4096, dim % 32 == 0, 0 < c <= cp <= 256, cp % 32 == 0, n_cus > 0 and 16-byte aligned X and G; anything else returns
// hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_dw_bf16_wide_launch(const flex_bf16 *X, const flex_bf16 *G, flex_bf16 *dW, float *part, int n, int dim, int c,
                                                   int cp, int n_cus, hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!X || !G || !dW || !part || n < 32 || !wide_dim(dim, 32) || c <= 0 || c > cp || cp > 256 || cp % 32 != 0 || n_cus <= 0 || misaligned(X) ||
        misaligned(G))
        return hipErrorInvalidValue;
    return flex_axw_dw_bf16_rows_launch(X, G, dW, part, n, dim, c, cp, dw_wide_rows(n, dim, c, n_cus), s);
}
