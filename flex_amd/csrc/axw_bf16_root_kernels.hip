// axw_bf16_root_kernels.hip -- the dense stage of the bf16 layer with a root-weight term, Out = A X W + X R + b (libflex_axw.so,
// FLEX_AXW_ROOT; flex_axw_run_root_bf16):
//   Out[n x cp] = rn_bf16( L1[n x d1] W1[d1 x c] + L2[n x d2] W2[d2 x c] + Cin[n x cp] + bias[c] )
// two dense products into ONE fp32 accumulator chain, an addend and a bias, one rounding at the store.  L2 / W2 (d2 = 0), Cin and bias may
// each be absent.  The kernel is axw_gemm_bf16_stream_kernel (axw_bf16_device.h), the body it shares with the wide forward, whose L side
// and W streaming are described at the top of axw_bf16_wide_kernels.hip; this file holds its kRoot and kWindow instantiations, the two
// pack kernels and the launchers.  What kRoot adds to the wide forward:
//   * one fragment stream for both weights: axw_bf16_pack_kernel writes [W1; W2] as (d1 + d2) / 16 k-steps of fragments into Wf
//     ((d1 + d2) x cp elements, once per call), so the LDS side sees one contraction of length d1 + d2 <= 8192 and knows of no seam.  With
//     d2 = 0 it is the pack of the wide forward (pack_launch).
//   * the L fragment of k-step s comes from L1 (row stride d1) for s < d1 / 16 and from L2 (row stride d2, k-step s - d1 / 16) after
//     that: a wave-uniform select between two row pointers that a wave computes once per slab and panel.  d1 is a multiple of 16, not
//     of 128: the seam falls anywhere inside a slab.
//   * the chain: acc = fp32(Cin) + bias (ACCUMULATOR INITIALISATION: one fp32 addition, exact where either is absent, since the absent one
//     is +0), then the k-steps in ascending order, all of L1 W1 before all of L2 W2, into that one accumulator per entry; the contraction
//     is split neither across waves nor across workgroups.  d1 + d2 + 1 additions and the products exact: gamma(d1 + d2 + 2) covers it.
//     With Cin and bias absent the chain starts from +0 as kWide's does, and zero products change no accumulator.
//   * Cin is read in the C/D layout the lane stores in: acc[t][4 g + e] = Out[r0 + j][32 t + 8 g + 4 h + e], so four 8-byte loads a tile
//     from the lane's own row, issued at the head of a round (behind the barrier that every wave waits at anyway).  Its columns >= c meet
//     the store's mask and never reach Out.  bias is staged once per workgroup into cp floats of LDS behind the W buffers (zero from
//     column c on, all zero without a bias) and read back four floats a ds_read_b128 in the same layout.
//   * any d1 + d2 >= 16: the first slab may be a partial one (the prologue stages min(8, steps) k-steps), and with a single slab the two
//     LDS buffers alternate between rounds instead of between slabs.
//   * Cin must not overlap Out: the overlapping last panel is computed twice over the rows it shares with its predecessor, and an
//     in-place Cin would be added twice there.  The launcher refuses the overlap.
// Panels a wave: P = 2 at cp = 64 (NT = 2), else 1 (the compiler's report is in DESIGN.md 3.29: no scratch anywhere).
// kWindow is the dX of the layer's backward (flex_axw_backward_root_bf16; flex_axw_dx_bf16_root_launch at the end of this file, DESIGN.md
// 3.30): dX = rn_bf16(G W^T + dOut R^T) in 256-column passes over a transposing pack of [W^T; R^T].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "axw_bf16_device.h"

namespace flex_axw_bf16 {

// Wf[(s NT + t) 64 + lane] = the eight values Wcat[16 s + 8 (lane >> 5) .. + 7][32 t + (lane & 31)], Wcat = [W1; W2], zero from column c on; one
// thread a fragment.  d1 % 16 == 0: a fragment lies in one of the two.
__global__ __launch_bounds__(256) void axw_bf16_pack_kernel(const flex_bf16 *__restrict__ W1, const flex_bf16 *__restrict__ W2,
                                                            u32x4 *__restrict__ Wf, int d1, int d2, int c, int nt) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= ((d1 + d2) >> 4) * nt * 64) return;
    const int lane = f & 63, t = (f >> 6) % nt, s = (f >> 6) / nt;
    const int col = 32 * t + (lane & 31), k0 = 16 * s + 8 * (lane >> 5);
    const flex_bf16 *src = k0 < d1 ? W1 + static_cast<size_t>(k0) * c : W2 + static_cast<size_t>(k0 - d1) * c;
    uint32_t v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = col < c ? src[static_cast<size_t>(e) * c + col] : 0u;
    Wf[f] = u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
}

hipError_t pack_launch(const flex_bf16 *W1, const flex_bf16 *W2, u32x4 *wf, int d1, int d2, int c, int nt, hipStream_t s) {
    const int frags = ((d1 + d2) / 16) * nt * 64;
    return launch(axw_bf16_pack_kernel, dim3(static_cast<unsigned>((frags + 255) / 256)), 256, 0, s, W1, W2, wf, d1, d2, c, nt);
}

// The transposing pack of the dual-source dX: the stream [W^T; R^T] (2 cp / 16 k-steps, rows c .. cp-1 of either zero) of every 256-column
// pass of dX, pass after pass, into Wf (2 dim x cp elements in all).  Fragment (pass p, k-step s, tile t, lane) holds
// Wsrc[256 p + 32 t + (lane & 31)][k .. k + 7], k = 16 s + 8 (lane >> 5) in W for k < cp and in R, set back by cp, after that: eight
// consecutive elements of one row -- one 16-byte load where c % 8 == 0 and both pointers are 16-byte aligned (`vec`: k + 8 <= c or k >= c,
// a fragment is whole or zero), eight 2-byte loads otherwise.  A narrower last pass has dim / 32 % 8 tiles; its fragments are fewer than
// a full pass's, so f / (fragments of a full pass) names the pass of every fragment.  One thread a fragment.
__global__ __launch_bounds__(256) void axw_bf16_root_pack_t_kernel(const flex_bf16 *__restrict__ W, const flex_bf16 *__restrict__ R,
                                                                   u32x4 *__restrict__ Wf, int c, int cp, int dim, bool vec) {
    const int f = blockIdx.x * 256 + threadIdx.x, steps = cp >> 3, pass_frags = steps * 8 * 64;
    if (f >= steps * (dim >> 5) * 64) return;
    const int p = f / pass_frags, rem = f - p * pass_frags, nt = min(8, (dim >> 5) - 8 * p);
    const int lane = rem & 63, t = (rem >> 6) % nt, s = (rem >> 6) / nt;
    const int row = 256 * p + 32 * t + (lane & 31), kk = 16 * s + 8 * (lane >> 5), k = kk < cp ? kk : kk - cp;
    const flex_bf16 *src = (kk < cp ? W : R) + static_cast<size_t>(row) * c + k;
    u32x4 v = {0u, 0u, 0u, 0u};
    if (vec) {
        if (k < c) v = *reinterpret_cast<const u32x4 *>(src);
    } else {
        uint32_t e[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) e[i] = k + i < c ? src[i] : 0u;
        v = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
    }
    Wf[f] = v;
}

inline bool width(int d, int least) { return d >= least && d <= 4096 && d % 16 == 0; }

}  // namespace flex_axw_bf16

// Out[n x cp] = rn_bf16(L1[n x d1] W1[d1 x c] + L2[n x d2] W2[d2 x c] + Cin[n x cp] + bias[c]) on flex_bf16 (bias: fp32), columns c .. cp-1
// of Out written as +0 bits, through Wf ((d1 + d2) x cp elements of scratch: [W1; W2] in fragment order).  L2 and W2 NULL with d2 = 0, Cin
// NULL and bias NULL each drop their term.  Takes n >= 32, 16 <= d1 <= 4096, d2 = 0 or 16 <= d2 <= 4096, both multiples of 16, cp % 64 == 0,
// 0 < c <= cp <= 256, n_cus > 0, 16-byte aligned L1, L2, Cin, Wf and Out (W1, W2: any flex_bf16 pointer; bias: any float pointer) and a Cin
// whose n x cp elements do not overlap Out's; anything else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_gemm_bf16_root_launch(const flex_bf16 *L1, const flex_bf16 *W1, int d1, const flex_bf16 *L2, const flex_bf16 *W2,
                                                     int d2, const flex_bf16 *Cin, const float *bias, flex_bf16 *Wf, flex_bf16 *Out, int n, int c,
                                                     int cp, int n_cus, hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!L1 || !W1 || !Wf || !Out || n < kRows || !width(d1, 16) || !width(d2, 0) || (d2 > 0) != (L2 != nullptr) || (d2 > 0) != (W2 != nullptr) ||
        cp <= 0 || cp % 64 != 0 || cp > 256 || c <= 0 || c > cp || n_cus <= 0 || misaligned(L1) || misaligned(L2) || misaligned(Cin) ||
        misaligned(Wf) || misaligned(Out))
        return hipErrorInvalidValue;
    const uintptr_t bytes = static_cast<uintptr_t>(n) * cp * sizeof(flex_bf16), ci = reinterpret_cast<uintptr_t>(Cin),
                    oi = reinterpret_cast<uintptr_t>(Out);
    if (Cin && ci < oi + bytes && oi < ci + bytes) return hipErrorInvalidValue;
    u32x4 *wf = reinterpret_cast<u32x4 *>(Wf);
    const hipError_t e = pack_launch(W1, W2, wf, d1, d2, c, cp / 32, s);
    if (e != hipSuccess) return e;
    return dispatch_tiles<2, 4, 6, 8>(cp / 32, [&](auto tiles) {
        constexpr int NT = decltype(tiles)::value, P = stream_panels(NT);
        return launch(axw_gemm_bf16_stream_kernel<NT, P, Stream::kRoot>, dim3(panel_groups(n, kWaves * P, n_cus)), 64 * kWaves,
                      stream_lds(NT) + cp * sizeof(float), s, L1, d1, d2 ? L2 : L1, d2, wf, Cin, bias, Out, n, c);
    });
}

// dX[n x dim] = rn_bf16(G[n x cp] W^T + dOut[n x cp] R^T), W and R [dim x c], on flex_bf16: the dX of flex_axw_backward_root_bf16.  One fp32
// chain per entry: +0, all of G W^T in ascending k, then all of dOut R^T, one rounding; columns c .. cp-1 of G and of dOut are read (they
// meet zero rows and must be finite).  dim / 256 passes of 256 columns are the grid's y dimension and a narrower last pass a launch of
// its own (another instantiation: NT = 1 .. 7), through Wf (2 dim x cp elements of scratch: every pass's [W^T; R^T] stream).  Takes
// n >= 32, cp % 64 == 0, 0 < c <= cp <= 256, 0 < dim <= 4096, dim % 32 == 0, n_cus > 0 and 16-byte aligned G, dOut, Wf and dX (W, R: any
// flex_bf16 pointer); anything else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_dx_bf16_root_launch(const flex_bf16 *G, const flex_bf16 *W, const flex_bf16 *dOut, const flex_bf16 *R,
                                                   flex_bf16 *Wf, flex_bf16 *dX, int n, int c, int cp, int dim, int n_cus, hipStream_t s) {
    using namespace flex_axw_bf16;
    if (!G || !W || !dOut || !R || !Wf || !dX || n < kRows || cp <= 0 || cp % 64 != 0 || cp > 256 || c <= 0 || c > cp || dim <= 0 || dim > 4096 ||
        dim % 32 != 0 || n_cus <= 0 || misaligned(G) || misaligned(dOut) || misaligned(Wf) || misaligned(dX))
        return hipErrorInvalidValue;
    u32x4 *wf = reinterpret_cast<u32x4 *>(Wf);
    const int frags = (cp / 8) * (dim / 32) * 64, full = dim / 256, tail = dim % 256;
    const bool vec = c % 8 == 0 && !misaligned(W) && !misaligned(R);
    hipError_t e = launch(axw_bf16_root_pack_t_kernel, dim3(static_cast<unsigned>((frags + 255) / 256)), 256, 0, s, W, R, wf, c, cp, dim, vec);
    // `passes` windows of 32 NT columns of dX from pass `first` on, and their streams
    auto windows = [&](auto tiles, int passes, int first) {
        constexpr int NT = decltype(tiles)::value, P = stream_panels(NT);
        return launch(axw_gemm_bf16_stream_kernel<NT, P, Stream::kWindow>, dim3(panel_groups(n, kWaves * P, n_cus), static_cast<unsigned>(passes)),
                      64 * kWaves, stream_lds(NT), s, G, cp, dOut, cp, wf + static_cast<size_t>(first) * (cp / 8) * 8 * 64, nullptr, nullptr,
                      dX + 256 * first, n, dim);
    };
    if (e == hipSuccess && full > 0) e = windows(std::integral_constant<int, 8>(), full, 0);
    if (e != hipSuccess || tail == 0) return e;
    return dispatch_tiles<1, 2, 3, 4, 5, 6, 7>(tail / 32, [&](auto tiles) { return windows(tiles, 1, full); });
}
