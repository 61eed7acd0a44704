// axw_bf16_wide_kernels.hip -- the dense half of the bf16 A*X*W layer at input-layer widths, 256 < dim <= 4096 (libflex_axw.so,
// FLEX_AXW_BF16; axw_bf16_kernels.hip and axw_bf16_backward_kernels.hip serve dim <= 256):
//   forward  Out[n x cp] = L[n x dim] W[dim x c]   a long contraction: W no longer fits the LDS (dim x cp x 2 bytes: 256 KiB at 512 x 256)
//   dX       dX[n x dim] = G[n x cp] Wt[cp x dim]  a wide output: more accumulator tiles than a wave has registers for
//   dW       dW[dim x c] = X[n x dim]^T G[n x cp]  the 128 x 128-block kernel as it is, under a slice rule that bounds its fp32 partials
// Forward.  The L side is that of axw_bf16_kernels.hip: operands swapped (Wp^T the MFMA's A operand, L its B operand, 16 bytes of one row
// a lane straight from global memory), v_mfma_f32_32x32x16_bf16, the k-steps in ascending order into ONE fp32 accumulator per entry (no
// split of the contraction across waves or workgroups), the permlane store, the overlapping last panel, padding columns masked to +0.
// The W side is new:
//   * pack once: axw_bf16_pack_w_kernel turns W[dim x c] into the fragment order [k-step s][32-column tile t][lane][8 k values] in global
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

constexpr int kSlab = kUnit;  // k-steps of a slab of W

// Wf[(s NT + t) 64 + lane] = the eight values W[16 s + 8 (lane >> 5) .. + 7][32 t + (lane & 31)], zero from column c on; one thread a fragment
__global__ __launch_bounds__(256) void axw_bf16_pack_w_kernel(const flex_bf16 *__restrict__ W, u32x4 *__restrict__ Wf, int dim, int c, int nt) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= (dim >> 4) * nt * 64) return;
    const int lane = f & 63, t = (f >> 6) % nt, s = (f >> 6) / nt;
    const int col = 32 * t + (lane & 31), k0 = 16 * s + 8 * (lane >> 5);
    uint32_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = col < c ? W[static_cast<size_t>(k0 + e) * c + col] : 0u;
    Wf[f] = u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
}

template <int NT, int P>  // 32-column tiles of Out, panels a wave
__global__ __launch_bounds__(64 * kWaves) void axw_gemm_bf16_wide_kernel(const flex_bf16 *__restrict__ L, const u32x4 *__restrict__ Wf,
                                                                         flex_bf16 *__restrict__ Out, int n, int dim, int c) {
    extern __shared__ u32x4 sW[];  // [2 buffers][kSlab][NT][64] fragments of 8 bf16
    constexpr int cp = 32 * NT, kStepFrags = NT * 64, kSlabFrags = kSlab * kStepFrags;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int steps = dim >> 4, slabs = (steps + kSlab - 1) / kSlab;
    const int n_panels = (n + kRows - 1) / kRows;
    const int n_rounds = (n_panels + kWaves * P - 1) / (kWaves * P);  // gridDim.x <= n_rounds: every workgroup has a round
    auto panel_of = [&](int round, int p) { return (round * P + p) * kWaves + wave; };
    auto panel_row = [&](int pnl) { return min(min(pnl, n_panels - 1) * kRows, n - kRows); };  // past the end: the last panel again
    auto lfrag = [&](int pnl, int s) {
        return *reinterpret_cast<const bf16x8 *>(L + static_cast<size_t>(panel_row(pnl) + j) * dim + 16 * s + 8 * h);
    };
    const bool stager = tid < kStepFrags;  // a k-step of W is NT KiB: one 16-byte fragment a thread of the first NT waves

    bf16x8 pre[P][kSlab] = {};  // the L fragments of the slab about to be multiplied
#pragma unroll
    for (int q = 0; q < kSlab; ++q) {  // dim > 256: the first slab is a full one
#pragma unroll
        for (int p = 0; p < P; ++p) pre[p][q] = lfrag(panel_of(blockIdx.x, p), q);
        if (stager) sW[q * kStepFrags + tid] = Wf[q * kStepFrags + tid];
    }

    int buf = 0;
    const bf16x8 *wf = reinterpret_cast<const bf16x8 *>(sW) + lane;
    for (int round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        f32x16 acc[P][NT];
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
            for (int t = 0; t < NT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[p][t][i] = 0.f;
        for (int sl = 0; sl < slabs; ++sl, buf ^= 1) {
            // slab sl is whole in buffer buf (every store into it came before this barrier), and buffer buf ^ 1 was last read before it
            __syncthreads();
            const bool last = sl + 1 == slabs;  // workgroup-uniform, like everything that guards a load, a store or an MFMA below
            const int nr = last ? round + gridDim.x : round, ns0 = last ? 0 : (sl + 1) * kSlab;
            const int n_cur = min(kSlab, steps - sl * kSlab), n_next = nr < n_rounds ? min(kSlab, steps - ns0) : 0;
            const u32x4 *src = Wf + static_cast<size_t>(ns0) * kStepFrags + tid;
            u32x4 *dst = sW + (buf ^ 1) * kSlabFrags + tid;
            const bf16x8 *w = wf + buf * kSlabFrags;
            u32x4 stage[kSlab];
#pragma unroll
            for (int q = 0; q < kSlab; ++q) {
                if (q >= 2 && q - 2 < n_next && stager) dst[(q - 2) * kStepFrags] = stage[q - 2];
                bf16x8 b[P];
#pragma unroll
                for (int p = 0; p < P; ++p) b[p] = pre[p][q];
                if (q < n_next) {
#pragma unroll
                    for (int p = 0; p < P; ++p) pre[p][q] = lfrag(panel_of(nr, p), ns0 + q);
                    if (stager) stage[q] = src[q * kStepFrags];
                }
                if (q < n_cur) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const bf16x8 a = w[(q * NT + t) * 64];
#pragma unroll
                        for (int p = 0; p < P; ++p) acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[p], acc[p][t], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int q = kSlab - 2; q < kSlab; ++q)
                if (q < n_next && stager) dst[q * kStepFrags] = stage[q];
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int panel = panel_of(round, p);
            if (panel >= n_panels) continue;  // wave-uniform: the round's panels past the end were multiplied as copies of the last
            flex_bf16 *dst = Out + static_cast<size_t>(panel_row(panel) + j) * cp + 16 * h;
            const f32x16(&panel_acc)[NT] = acc[p];  // the macro has a loop variable p of its own
            FLEX_AXW_BF16_STORE_PANEL(NT, panel_acc, dst, c, h)
        }
    }
}

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

inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
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
    const int nt = cp / 32, frags = (dim / 16) * nt * 64;
    u32x4 *wf = reinterpret_cast<u32x4 *>(Wf);
    hipLaunchKernelGGL(axw_bf16_pack_w_kernel, dim3(static_cast<unsigned>((frags + 255) / 256)), dim3(256), 0, s, W, wf, dim, c, nt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int n_panels = (n + kRows - 1) / kRows;
    const size_t lds = static_cast<size_t>(2) * kSlab * nt * 64 * sizeof(u32x4);
    auto go = [&](auto kernel, int panels_a_round) {  // more than 64 KiB of dynamic LDS has to be asked for
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return;
        const int n_rounds = (n_panels + panels_a_round - 1) / panels_a_round;
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(std::min(n_cus, n_rounds))), dim3(64 * kWaves), lds, s, L, wf, Out, n, dim, c);
        e = hipGetLastError();
    };
    switch (nt) {
        case 2: go(axw_gemm_bf16_wide_kernel<2, 2>, 2 * kWaves); break;
        case 4: go(axw_gemm_bf16_wide_kernel<4, 1>, kWaves); break;
        case 6: go(axw_gemm_bf16_wide_kernel<6, 1>, kWaves); break;
        default: go(axw_gemm_bf16_wide_kernel<8, 1>, kWaves); break;
    }
    return e;
}

// dX[n x dim] = G[n x cp] * Wt[cp x dim] on flex_bf16.  Takes n >= 32, cp % 64 == 0, 0 < cp <= 256, 256 < dim <= 4096, dim % 32 == 0,
// n_cus > 0 and 16-byte aligned G, Wt and dX; anything else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_dx_bf16_wide_launch(const flex_bf16 *G, const flex_bf16 *Wt, flex_bf16 *dX, int n, int cp, int dim, int n_cus,
                                                   hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!G || !Wt || !dX || n < kRows || cp <= 0 || cp % 64 != 0 || cp > 256 || !wide_dim(dim, 32) || n_cus <= 0 || misaligned(G) ||
        misaligned(Wt) || misaligned(dX))
        return hipErrorInvalidValue;
    const int n_panels = (n + kRows - 1) / kRows, groups = std::min(n_cus, (n_panels + 3) / 4);
    const int full = dim / 256, tail = dim % 256;
    hipError_t e = hipSuccess;
    auto go = [&](auto kernel, int passes, int col0, int width) {
        const size_t lds = static_cast<size_t>(cp) * width * sizeof(flex_bf16);
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return;
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(groups), static_cast<unsigned>(passes)), dim3(64 * kWaves), lds, s, G, Wt + col0,
                           dX + col0, n, cp, width, dim);
        e = hipGetLastError();
    };
    go(axw_gemm_bf16_kernel<8, true>, full, 0, 256);
    if (e != hipSuccess || tail == 0) return e;
    switch (tail / 32) {
        case 1: go(axw_gemm_bf16_kernel<1, true>, 1, 256 * full, tail); break;
        case 2: go(axw_gemm_bf16_kernel<2, true>, 1, 256 * full, tail); break;
        case 3: go(axw_gemm_bf16_kernel<3, true>, 1, 256 * full, tail); break;
        case 4: go(axw_gemm_bf16_kernel<4, true>, 1, 256 * full, tail); break;
        case 5: go(axw_gemm_bf16_kernel<5, true>, 1, 256 * full, tail); break;
        case 6: go(axw_gemm_bf16_kernel<6, true>, 1, 256 * full, tail); break;
        default: go(axw_gemm_bf16_kernel<7, true>, 1, 256 * full, tail); break;
    }
    return e;
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
