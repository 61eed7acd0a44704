// axw_bf16_root_kernels.hip -- the dense stage of the bf16 layer with a root-weight term, Out = A X W + X R + b (libflex_axw.so,
// FLEX_AXW_ROOT; flex_axw_run_root_bf16):
//   Out[n x cp] = rn_bf16( L1[n x d1] W1[d1 x c] + L2[n x d2] W2[d2 x c] + Cin[n x cp] + bias[c] )
// two dense products into ONE fp32 accumulator chain, an addend and a bias, one rounding at the store.  L2 / W2 (d2 = 0), Cin and bias may
// each be absent.  A namespace of its own: nothing in flex_axw_bf16 (axw_bf16_kernels.hip, axw_bf16_wide_kernels.hip) moves.
// The L side and the W streaming are those of axw_gemm_bf16_wide_kernel: operands swapped (W^T fragments the MFMA's A operand from LDS, 16
// bytes of one L row a lane straight from global memory its B operand), v_mfma_f32_32x32x16_bf16, persistent workgroups of 8 waves, W as
// ready-made fragments streamed through two LDS buffers in slabs of 8 k-steps with one barrier a slab, the permlane store, the
// overlapping last panel, padding columns masked to +0 bits.  What differs:
//   * one fragment stream for both weights: axw_bf16_root_pack_kernel writes [W1; W2] as (d1 + d2) / 16 k-steps of fragments into Wf
//     ((d1 + d2) x cp elements, once per call), so the LDS side sees one contraction of length d1 + d2 <= 8192 and knows of no seam.
//   * the L fragment of k-step s comes from L1 (row stride d1) for s < d1 / 16 and from L2 (row stride d2, k-step s - d1 / 16) after
//     that: a wave-uniform select between two row pointers that a wave computes once per slab and panel.  d1 is a multiple of 16, not
//     of 128: the seam falls anywhere inside a slab.
//   * the chain: acc = fp32(Cin) + bias (ACCUMULATOR INITIALISATION: one fp32 addition, exact where either is absent, since the absent one
//     is +0), then the k-steps in ascending order, all of L1 W1 before all of L2 W2, into that one accumulator per entry; the contraction
//     is split neither across waves nor across workgroups.  d1 + d2 + 1 additions and the products exact: gamma(d1 + d2 + 2) covers it.
//     With Cin and bias absent the chain starts from +0 as axw_gemm_bf16_wide_kernel's does, and zero products change no accumulator.
//   * Cin is read in the C/D layout the lane stores in: acc[t][4 g + e] = Out[r0 + j][32 t + 8 g + 4 h + e], so four 8-byte loads a tile
//     from the lane's own row, issued at the head of a round (behind the barrier that every wave waits at anyway).  Its columns >= c meet
//     the store's mask and never reach Out.  bias is staged once per workgroup into cp floats of LDS behind the W buffers (zero from
//     column c on, all zero without a bias) and read back four floats a ds_read_b128 in the same layout.
//   * any d1 + d2 >= 16: the first slab may be a partial one (the prologue stages min(8, steps) k-steps), and with a single slab the two
//     LDS buffers alternate between rounds instead of between slabs.
//   * Cin must not overlap Out: the overlapping last panel is computed twice over the rows it shares with its predecessor, and an
//     in-place Cin would be added twice there.  The launcher refuses the overlap.
// Panels a wave: P = 2 at cp = 64 (NT = 2), else 1, as the wide kernel (the compiler's report is in DESIGN.md 3.29: no scratch anywhere).
// The same kernel, instantiated with kWindow, is the dX of the layer's backward (flex_axw_backward_root_bf16; flex_axw_dx_bf16_root_launch at
// the end of this file): dX = rn_bf16(G W^T + dOut R^T) in 256-column passes over a transposing pack of [W^T; R^T].
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "axw_bf16_device.h"

namespace flex_axw_bf16_root {

using flex_axw_bf16::bf16_bits;
using flex_axw_bf16::bf16x8;
using flex_axw_bf16::f32x16;
using flex_axw_bf16::kRows;
using flex_axw_bf16::kWaves;
using flex_axw_bf16::u32x2;
using flex_axw_bf16::u32x4;

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kSlab = flex_axw_bf16::kUnit;  // k-steps of a slab of [W1; W2]

// Wf[(s NT + t) 64 + lane] = the eight values Wcat[16 s + 8 (lane >> 5) .. + 7][32 t + (lane & 31)], Wcat = [W1; W2], zero from column c on; one
// thread a fragment.  d1 % 16 == 0: a fragment lies in one of the two.
__global__ __launch_bounds__(256) void axw_bf16_root_pack_kernel(const flex_bf16 *__restrict__ W1, const flex_bf16 *__restrict__ W2,
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

// kWindow (the dual-source dX of flex_axw_backward_root_bf16, below): Out is a window of 32 NT whole columns, from 256 blockIdx.y on, of an
// array whose rows are `c` elements apart (the parameter carries the row stride: a window has no padding to mask), Wf holds one
// fragment stream of (d1 + d2) / 16 k-steps per 256-column pass, and there is neither a Cin nor a bias: the chain starts from +0.  The
// instantiations with kWindow = false compile to the instructions they had before the switch existed.
template <int NT, int P, bool kWindow = false>  // 32-column tiles of Out, panels a wave
__global__ __launch_bounds__(64 * kWaves) void axw_gemm_bf16_root_kernel(const flex_bf16 *__restrict__ L1, int d1, const flex_bf16 *__restrict__ L2,
                                                                         int d2, const u32x4 *__restrict__ Wf, const flex_bf16 *__restrict__ Cin,
                                                                         const float *__restrict__ bias, flex_bf16 *__restrict__ Out, int n,
                                                                         int c) {
    extern __shared__ u32x4 sW[];  // [2 buffers][kSlab][NT][64] fragments of 8 bf16, then cp floats of bias
    constexpr int cp = 32 * NT, kStepFrags = NT * 64, kSlabFrags = kSlab * kStepFrags;
    float *sBias = reinterpret_cast<float *>(sW + 2 * kSlabFrags);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // in an SGPR, and so is every panel's row
    const int j = lane & 31, h = lane >> 5;
    const int s1 = d1 >> 4, steps = (d1 + d2) >> 4, slabs = (steps + kSlab - 1) / kSlab;
    if constexpr (kWindow) {
        Wf += static_cast<size_t>(blockIdx.y) * steps * (8 * 64);  // a full pass is 8 tiles wide
        Out += 256 * blockIdx.y;
    }
    const int n_panels = (n + kRows - 1) / kRows;
    const int n_rounds = (n_panels + kWaves * P - 1) / (kWaves * P);  // gridDim.x <= n_rounds: every workgroup has a round
    auto panel_of = [&](int round, int p) { return (round * P + p) * kWaves + wave; };
    auto panel_row = [&](int pnl) { return min(min(pnl, n_panels - 1) * kRows, n - kRows); };  // past the end: the last panel again
    // A fragment's address is a wave-uniform 64-bit base (the panel's first row in L1 or in L2, the latter set back by d1 / 16 k-steps, so
    // that k-step s of the WHOLE contraction is 32 s bytes on in either) plus this lane's 32-bit byte offset inside a panel (at most 32 rows
    // of 8 KiB), which no round changes: one register a source instead of a pointer a source and panel.  The launcher passes L2 = L1 when
    // d2 = 0, and no k-step then selects it.
    const uint32_t lane1 = (static_cast<uint32_t>(j) * d1 + 8 * h) * 2, lane2 = (static_cast<uint32_t>(j) * d2 + 8 * h) * 2;
    struct Rows {
        const char *a, *b;
    };
    auto rows_of = [&](int pnl) {
        const size_t r = static_cast<size_t>(panel_row(pnl));
        return Rows{reinterpret_cast<const char *>(L1 + r * d1), reinterpret_cast<const char *>(L2 + r * d2) - 32 * static_cast<ptrdiff_t>(s1)};
    };
    auto lfrag = [&](const Rows &r, int s) {  // a wave-uniform choice of base and stride
        return *reinterpret_cast<const bf16x8 *>(s < s1 ? r.a + 32 * s + lane1 : r.b + 32 * s + lane2);
    };
    const bool stager = tid < kStepFrags;  // a k-step of W is NT KiB: one 16-byte fragment a thread of the first NT waves

    bf16x8 pre[P][kSlab] = {};  // the L fragments of the slab about to be multiplied
    {
        Rows r[P];
#pragma unroll
        for (int p = 0; p < P; ++p) r[p] = rows_of(panel_of(blockIdx.x, p));
#pragma unroll
        for (int q = 0; q < kSlab; ++q) {
            if (q < steps) {  // the first slab may be the only one, and a partial one
#pragma unroll
                for (int p = 0; p < P; ++p) pre[p][q] = lfrag(r[p], q);
                if (stager) sW[q * kStepFrags + tid] = Wf[q * kStepFrags + tid];
            }
        }
    }
    if constexpr (!kWindow)
        if (tid < cp) sBias[tid] = bias && tid < c ? bias[tid] : 0.f;
    __syncthreads();  // sBias is read before a round's first slab barrier

    int buf = 0;
    const bf16x8 *wf = reinterpret_cast<const bf16x8 *>(sW) + lane;
    for (int round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        f32x16 acc[P][NT];
#pragma unroll
        for (int p = 0; p < P; ++p) {  // acc = Cin + bias, in the layout of the store: four columns from 32 t + 8 g + 4 h on
            auto init = [&](int t, int g, u32x2 v) {
                const f32x4 b = *reinterpret_cast<const f32x4 *>(sBias + 32 * t + 8 * g + 4 * h);
                acc[p][t][4 * g] = __uint_as_float(v[0] << 16) + b[0];
                acc[p][t][4 * g + 1] = __uint_as_float(v[0] & 0xFFFF0000u) + b[1];
                acc[p][t][4 * g + 2] = __uint_as_float(v[1] << 16) + b[2];
                acc[p][t][4 * g + 3] = __uint_as_float(v[1] & 0xFFFF0000u) + b[3];
            };
            if constexpr (kWindow) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[p][t][i] = 0.f;
            } else if (Cin) {  // workgroup-uniform
                const flex_bf16 *crow = Cin + static_cast<size_t>(panel_row(panel_of(round, p))) * cp + (j * cp + 4 * h);
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) init(t, g, *reinterpret_cast<const u32x2 *>(crow + 32 * t + 8 * g));
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) init(t, g, u32x2{0u, 0u});  // +0 without a Cin
            }
        }
        for (int sl = 0; sl < slabs; ++sl, buf ^= 1) {
            // slab sl is whole in buffer buf (every store into it came before this barrier), and buffer buf ^ 1 was last read before it
            __syncthreads();
            const bool last = sl + 1 == slabs;  // workgroup-uniform, like everything that guards a load, a store or an MFMA below
            const int nr = last ? round + gridDim.x : round, ns0 = last ? 0 : (sl + 1) * kSlab;
            const int n_cur = min(kSlab, steps - sl * kSlab), n_next = nr < n_rounds ? min(kSlab, steps - ns0) : 0;
            const u32x4 *src = Wf + static_cast<size_t>(ns0) * kStepFrags + tid;
            u32x4 *dst = sW + (buf ^ 1) * kSlabFrags + tid;
            const bf16x8 *w = wf + buf * kSlabFrags;
            Rows r[P];
#pragma unroll
            for (int p = 0; p < P; ++p) r[p] = rows_of(panel_of(nr, p));
            u32x4 stage[kSlab];
#pragma unroll
            for (int q = 0; q < kSlab; ++q) {
                if (q >= 2 && q - 2 < n_next && stager) dst[(q - 2) * kStepFrags] = stage[q - 2];
                bf16x8 b[P];
#pragma unroll
                for (int p = 0; p < P; ++p) b[p] = pre[p][q];
                if (q < n_next) {
#pragma unroll
                    for (int p = 0; p < P; ++p) pre[p][q] = lfrag(r[p], ns0 + q);
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
            const f32x16(&panel_acc)[NT] = acc[p];  // the macro has a loop variable p of its own
            if constexpr (kWindow) {
                flex_bf16 *dst = Out + static_cast<size_t>(panel_row(panel) + j) * c + 16 * h;
                FLEX_AXW_BF16_STORE_PANEL(NT, panel_acc, dst, cp, h)
            } else {
                flex_bf16 *dst = Out + static_cast<size_t>(panel_row(panel) + j) * cp + 16 * h;
                FLEX_AXW_BF16_STORE_PANEL(NT, panel_acc, dst, c, h)
            }
        }
    }
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

inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool width(int d, int least) { return d >= least && d <= 4096 && d % 16 == 0; }

// one launch of the window kernel: `passes` windows of 32 NT columns of dX from column col0 on, their streams from wf on
template <int NT>
hipError_t launch_window(const flex_bf16 *G, const flex_bf16 *dOut, const u32x4 *wf, flex_bf16 *dX, int n, int cp, int dim, int passes, int n_cus,
                         hipStream_t s) {
    constexpr int P = NT <= 2 ? 2 : 1;  // panels a wave, as the forward: two while the accumulators are 64 registers or fewer
    const auto kernel = axw_gemm_bf16_root_kernel<NT, P, true>;
    const size_t lds = static_cast<size_t>(2) * kSlab * NT * 64 * sizeof(u32x4);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
    if (e != hipSuccess) return e;
    const int n_panels = (n + kRows - 1) / kRows, n_rounds = (n_panels + kWaves * P - 1) / (kWaves * P);
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(std::min(n_cus, n_rounds)), static_cast<unsigned>(passes)), dim3(64 * kWaves), lds, s, G,
                       cp, dOut, cp, wf, static_cast<const flex_bf16 *>(nullptr), static_cast<const float *>(nullptr), dX, n, dim);
    return hipGetLastError();
}

}  // namespace flex_axw_bf16_root

// Out[n x cp] = rn_bf16(L1[n x d1] W1[d1 x c] + L2[n x d2] W2[d2 x c] + Cin[n x cp] + bias[c]) on flex_bf16 (bias: fp32), columns c .. cp-1
// of Out written as +0 bits, through Wf ((d1 + d2) x cp elements of scratch: [W1; W2] in fragment order).  L2 and W2 NULL with d2 = 0, Cin
// NULL and bias NULL each drop their term.  Takes n >= 32, 16 <= d1 <= 4096, d2 = 0 or 16 <= d2 <= 4096, both multiples of 16, cp % 64 == 0,
// 0 < c <= cp <= 256, n_cus > 0, 16-byte aligned L1, L2, Cin, Wf and Out (W1, W2: any flex_bf16 pointer; bias: any float pointer) and a Cin
// whose n x cp elements do not overlap Out's; anything else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_gemm_bf16_root_launch(const flex_bf16 *L1, const flex_bf16 *W1, int d1, const flex_bf16 *L2, const flex_bf16 *W2,
                                                     int d2, const flex_bf16 *Cin, const float *bias, flex_bf16 *Wf, flex_bf16 *Out, int n, int c,
                                                     int cp, int n_cus, hipStream_t s) {
    using namespace flex_axw_bf16_root;
    if (!L1 || !W1 || !Wf || !Out || n < kRows || !width(d1, 16) || !width(d2, 0) || (d2 > 0) != (L2 != nullptr) || (d2 > 0) != (W2 != nullptr) ||
        cp <= 0 || cp % 64 != 0 || cp > 256 || c <= 0 || c > cp || n_cus <= 0 || misaligned(L1) || misaligned(L2) || misaligned(Cin) ||
        misaligned(Wf) || misaligned(Out))
        return hipErrorInvalidValue;
    const uintptr_t bytes = static_cast<uintptr_t>(n) * cp * sizeof(flex_bf16), ci = reinterpret_cast<uintptr_t>(Cin),
                    oi = reinterpret_cast<uintptr_t>(Out);
    if (Cin && ci < oi + bytes && oi < ci + bytes) return hipErrorInvalidValue;
    const int nt = cp / 32, frags = ((d1 + d2) / 16) * nt * 64;
    u32x4 *wf = reinterpret_cast<u32x4 *>(Wf);
    hipLaunchKernelGGL(axw_bf16_root_pack_kernel, dim3(static_cast<unsigned>((frags + 255) / 256)), dim3(256), 0, s, W1, W2, wf, d1, d2, c, nt);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int n_panels = (n + kRows - 1) / kRows;
    const size_t lds = static_cast<size_t>(2) * kSlab * nt * 64 * sizeof(u32x4) + static_cast<size_t>(cp) * sizeof(float);
    auto go = [&](auto kernel, int panels_a_round) {  // more than 64 KiB of dynamic LDS has to be asked for
        e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return;
        const int n_rounds = (n_panels + panels_a_round - 1) / panels_a_round;
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(std::min(n_cus, n_rounds))), dim3(64 * kWaves), lds, s, L1, d1, d2 ? L2 : L1, d2, wf,
                           Cin, bias, Out, n, c);
        e = hipGetLastError();
    };
    switch (nt) {
        case 2: go(axw_gemm_bf16_root_kernel<2, 2>, 2 * kWaves); break;
        case 4: go(axw_gemm_bf16_root_kernel<4, 1>, kWaves); break;
        case 6: go(axw_gemm_bf16_root_kernel<6, 1>, kWaves); break;
        default: go(axw_gemm_bf16_root_kernel<8, 1>, kWaves); break;
    }
    return e;
}

// dX[n x dim] = rn_bf16(G[n x cp] W^T + dOut[n x cp] R^T), W and R [dim x c], on flex_bf16: the dX of flex_axw_backward_root_bf16.  One fp32
// chain per entry: +0, all of G W^T in ascending k, then all of dOut R^T, one rounding; columns c .. cp-1 of G and of dOut are read (they
// meet zero rows and must be finite).  dim / 256 passes of 256 columns are the grid's y dimension and a narrower last pass a launch of
// its own (another instantiation: NT = 1 .. 7), through Wf (2 dim x cp elements of scratch: every pass's [W^T; R^T] stream).  Takes
// n >= 32, cp % 64 == 0, 0 < c <= cp <= 256, 0 < dim <= 4096, dim % 32 == 0, n_cus > 0 and 16-byte aligned G, dOut, Wf and dX (W, R: any
// flex_bf16 pointer); anything else returns hipErrorInvalidValue before a launch.
extern "C" hipError_t flex_axw_dx_bf16_root_launch(const flex_bf16 *G, const flex_bf16 *W, const flex_bf16 *dOut, const flex_bf16 *R,
                                                   flex_bf16 *Wf, flex_bf16 *dX, int n, int c, int cp, int dim, int n_cus, hipStream_t s) {
    using namespace flex_axw_bf16_root;
    if (!G || !W || !dOut || !R || !Wf || !dX || n < kRows || cp <= 0 || cp % 64 != 0 || cp > 256 || c <= 0 || c > cp || dim <= 0 || dim > 4096 ||
        dim % 32 != 0 || n_cus <= 0 || misaligned(G) || misaligned(dOut) || misaligned(Wf) || misaligned(dX))
        return hipErrorInvalidValue;
    u32x4 *wf = reinterpret_cast<u32x4 *>(Wf);
    const int frags = (cp / 8) * (dim / 32) * 64, full = dim / 256, tail = dim % 256;
    const bool vec = c % 8 == 0 && !misaligned(W) && !misaligned(R);
    hipLaunchKernelGGL(axw_bf16_root_pack_t_kernel, dim3(static_cast<unsigned>((frags + 255) / 256)), dim3(256), 0, s, W, R, wf, c, cp, dim, vec);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && full > 0) e = launch_window<8>(G, dOut, wf, dX, n, cp, dim, full, n_cus, s);
    if (e != hipSuccess || tail == 0) return e;
    const u32x4 *twf = wf + static_cast<size_t>(full) * (cp / 8) * 8 * 64;
    flex_bf16 *tdx = dX + 256 * full;
    switch (tail / 32) {
        case 1: return launch_window<1>(G, dOut, twf, tdx, n, cp, dim, 1, n_cus, s);
        case 2: return launch_window<2>(G, dOut, twf, tdx, n, cp, dim, 1, n_cus, s);
        case 3: return launch_window<3>(G, dOut, twf, tdx, n, cp, dim, 1, n_cus, s);
        case 4: return launch_window<4>(G, dOut, twf, tdx, n, cp, dim, 1, n_cus, s);
        case 5: return launch_window<5>(G, dOut, twf, tdx, n, cp, dim, 1, n_cus, s);
        case 6: return launch_window<6>(G, dOut, twf, tdx, n, cp, dim, 1, n_cus, s);
        default: return launch_window<7>(G, dOut, twf, tdx, n, cp, dim, 1, n_cus, s);
    }
}
