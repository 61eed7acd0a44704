// axw_bf16_backward_kernels.hip -- dW of the bf16 A*X*W layer (libflex_axw.so, flex_axw_backward_bf16):
//   dW[dim x c] = X[n x dim]^T G[n x cp], row-major flex_bf16, fp32 sums on the bf16 MFMA, ONE rounding to bf16 after the last addition;
//   n tall (10^5..10^6), dim <= 256 (a multiple of 8), cp <= 256 (a multiple of 32).
// v_mfma_f32_32x32x16_bf16 with its k = the ROW index r: the A operand of lane (i, h) is X[r0 + 8 h .. r0 + 8 h + 7][i0 + i], the B operand
// of lane (j, h) is G[r0 + 8 h .. + 7][j0 + j] -- eight values a row stride apart, where memory has eight values along a row.  Nothing of
// the fp32 kernel's data path (axw_dw_kernel: 4-byte operands straight from global) carries over; its work split does:
//   * a workgroup of 4 waves owns one n-slice and one 128 x 128 block of dW: wave w the 32 rows i0 = 128 gi + 32 w and the four column
//     tiles j0 = 128 gj + 32 t.  Each (slice, block) writes one fp32 partial; axw_dw_bf16_reduce_kernel adds the partials in slice order
//     and rounds once.  No atomics: the same bits on every run.
//   * X and G go through LDS as ready-made MFMA fragments ([k-step s][tile t][half h][column i][8 rows], what stage_w of
//     axw_bf16_kernels.hip builds of W), so that every operand is one ds_read_b128.  A stage is 64 rows (four k-steps) of the block's 128
//     columns of X and of G: 16 KiB each, two stages, 64 KiB -- two workgroups a CU.
//   * the transposition happens in REGISTERS, once per element on the way in (candidate (b) of DESIGN.md 3.27, with 16-byte LDS stores
//     where the plain form has 2-byte ones): a thread loads an 8 row x 8 column block -- eight 16-byte loads, one per row, 16 lanes side by
//     side on the 256 bytes of a row's window, so every load instruction fetches whole lines -- turns it into eight fragments (32
//     two-halfword merges) and writes them with eight 16-byte LDS stores.  Waves 0 and 1 carry X's 128 blocks of a stage, waves 2 and 3
//     G's.  The eight fragments of a thread are neighbours in LDS (128 bytes), so 16 lanes of one store instruction would sit 128 bytes
//     apart, on 2 of the 16 bank groups; the slot of column i is therefore i ^ swz, swz = bit 4 of i | 2 t: the 16 lanes of a row of
//     blocks then write 16 different bank groups, and a read (t fixed, 8 consecutive lanes on the same 128 bytes, permuted) is as
//     conflict-free as without it.
//   * double buffer, one barrier a stage: the loads of stage k + 1 are issued right after the barrier of stage k and land in registers
//     while the 16 MFMAs of stage k run; they are transposed and stored into the other buffer at the top of the next iteration.
//   * rows past the slice end or past n, columns i >= dim of X and columns >= cp of G are zero OPERANDS selected in registers: never
//     loaded (a load past n is out of bounds), and a k-step of 16 rows wholly past the end is not multiplied.  Rows i >= dim are not
//     stored; G's padding columns c .. cp-1 are computed and dropped.
//   * order of every sum: k-step by k-step (16 rows, ascending) into one fp32 accumulator, the unit's own sum of 16 products inside a
//     step; then the partials in slice order.  include/flex_axw.h bounds it by L = rows per slice + slices roundings.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "axw_bf16_dw_device.h"  // frag_slot, the block load and store, slice_sum: shared with axw_bf16_root_backward_kernels.hip

namespace flex_axw_bf16_dw {

constexpr int kFrags = 4 * 4 * 64;    // fragments of one operand of a stage: [4 k-steps][4 tiles][64 lanes]

__global__ __launch_bounds__(256) void axw_dw_bf16_kernel(const flex_bf16 *__restrict__ X, const flex_bf16 *__restrict__ G,
                                                          float *__restrict__ part, int n, int dim, int c, int cp, int rows_per_slice) {
    __shared__ u32x4 sF[2 * 2 * kFrags];  // [buffer][X, G][fragment]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int slice = blockIdx.x;
    const int gi = blockIdx.y % ((dim + 127) / 128), gj = blockIdx.y / ((dim + 127) / 128);
    const int i0 = gi * 128 + wave * 32, j0 = gj * 128;
    const bool active = i0 < dim;  // wave-uniform; an inactive wave still loads, stores and meets the barriers
    const int nt = min(4, (cp - j0) / 32);
    const int r_beg = slice * rows_per_slice, r_end = min(n, r_beg + rows_per_slice);

    // the loader's block: operand op, rows 8 rg .. 8 rg + 7 of the stage, columns 8 q .. 8 q + 7 of the operand's 128-column window
    const int op = wave >> 1, q = threadIdx.x & 15, rg = (threadIdx.x & 127) >> 4;
    const int ld = op ? cp : dim, col = (op ? j0 : gi * 128) + 8 * q;
    const bool col_ok = col < ld;  // dim % 8 == 0 and cp % 8 == 0: a block's eight columns stand or fall together
    const flex_bf16 *src = (op ? G : X) + col;
    u32x4 v[8];
    auto load = [&](int r0) { FLEX_AXW_DW_LOAD_BLOCK(v, src, ld, r0 + 8 * rg, r_end, col_ok) };
    auto store = [&](int buf) {
        u32x4 *dst = sF + (buf * 2 + op) * kFrags;
        FLEX_AXW_DW_STORE_BLOCK(v, dst, rg, q, 4)
    };

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[t][k] = 0.f;

    load(r_beg);
    int buf = 0;
    for (int r0 = r_beg; r0 < r_end; r0 += kStage, buf ^= 1) {  // the same trip count for every wave of the workgroup
        store(buf);
        __syncthreads();  // the other buffer was last read before this barrier: the next store into it needs no barrier of its own
        if (r0 + kStage < r_end) load(r0 + kStage);
        if (active) {
            const u32x4 *fx = sF + buf * 2 * kFrags, *fg = fx + kFrags;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (r0 + 16 * s >= r_end) break;  // wave-uniform
                const bf16x8 a = __builtin_bit_cast(bf16x8, fx[frag_slot(s, wave, lane >> 5, lane & 31, 4)]);
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt)
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, fg[frag_slot(s, t, lane >> 5, lane & 31, 4)]),
                                                                         acc[t], 0, 0, 0);
            }
        }
    }
    if (!active) return;
    // acc[t][k] = dW[i0 + 8 (k >> 2) + 4 (lane >> 5) + (k & 3)][j0 + 32 t + (lane & 31)]
    float *dst = part + static_cast<size_t>(slice) * dim * c;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int j = j0 + 32 * t + (lane & 31);
        if (t >= nt || j >= c) continue;
        FLEX_AXW_DW_FOR_TILE_ROWS(k, ii, i0, lane >> 5, dim) dst[static_cast<size_t>(ii) * c + j] = acc[t][k];
    }
}

// dW[e] = rn_bf16(part[0][e] + part[1][e] + ... + part[S-1][e]), left to right in fp32, the loads 16 at a time (axw_dw_reduce_kernel)
__global__ __launch_bounds__(256) void axw_dw_bf16_reduce_kernel(const float *__restrict__ part, flex_bf16 *__restrict__ dW, int count,
                                                                 int slices) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    dW[e] = static_cast<flex_bf16>(bf16_bits(slice_sum(part, e, count, slices)));
}

// rows of an n-slice: about 256, at most n_cus slices, a whole number of stages
inline int dw_rows(int n, int n_cus) {
    const int s0 = std::max(1, std::min(n_cus, (n + 255) / 256));
    return ((n + s0 - 1) / s0 + kStage - 1) / kStage * kStage;
}

}  // namespace flex_axw_bf16_dw

extern "C" hipError_t flex_axw_dw_bf16_rows_launch(const flex_bf16 *X, const flex_bf16 *G, flex_bf16 *dW, float *part, int n, int dim, int c,
                                                   int cp, int rows, hipStream_t s);

// n-slices of the bf16 dW kernel: ceil(n / rows), rows = ceil(n / min(n_cus, ceil(n / 256))) rounded up to a multiple of 64; no slice is empty
extern "C" int flex_axw_dw_bf16_slices(int n, int n_cus) {
    if (n <= 0 || n_cus <= 0) return 0;
    const int rows = flex_axw_bf16_dw::dw_rows(n, n_cus);
    return (n + rows - 1) / rows;
}

// dW[dim x c] = rn_bf16(X[n x dim]^T G[n x cp]) through `part` (flex_axw_dw_bf16_slices(n, n_cus) * dim * c floats).  Takes n >= 32,
// 0 < dim <= 256, dim % 8 == 0, 0 < c <= cp <= 256, cp % 32 == 0, n_cus > 0 and 16-byte aligned X and G; anything else returns
// hipErrorInvalidValue before a launch.  Returns hipSuccess or the launch error.
extern "C" hipError_t flex_axw_dw_bf16_launch(const flex_bf16 *X, const flex_bf16 *G, flex_bf16 *dW, float *part, int n, int dim, int c, int cp,
                                              int n_cus, hipStream_t s) {
    using namespace flex_axw_bf16_dw;
    if (!X || !G || !dW || !part || n < 32 || dim <= 0 || dim > 256 || dim % 8 != 0 || c <= 0 || c > cp || cp > 256 || cp % 32 != 0 || n_cus <= 0 ||
        misaligned(X) || misaligned(G))
        return hipErrorInvalidValue;
    return flex_axw_dw_bf16_rows_launch(X, G, dW, part, n, dim, c, cp, dw_rows(n, n_cus), s);
}

// The two launches behind flex_axw_dw_bf16_launch and flex_axw_dw_bf16_wide_launch (axw_bf16_wide_kernels.hip), which check their
// arguments and choose `rows`, a multiple of 64: n-slices of `rows` rows, `part` holds ceil(n / rows) * dim * c floats.  Not checked
// here: any dim % 8 == 0 is served by the grid of 128 x 128 blocks.
extern "C" hipError_t flex_axw_dw_bf16_rows_launch(const flex_bf16 *X, const flex_bf16 *G, flex_bf16 *dW, float *part, int n, int dim, int c,
                                                   int cp, int rows, hipStream_t s) {
    using namespace flex_axw_bf16_dw;
    const int slices = (n + rows - 1) / rows;
    const dim3 grid(static_cast<unsigned>(slices), static_cast<unsigned>(((dim + 127) / 128) * ((cp + 127) / 128)));
    const hipError_t e = launch(axw_dw_bf16_kernel, grid, 256, 0, s, X, G, part, n, dim, c, cp, rows);
    if (e != hipSuccess) return e;
    const int count = dim * c;
    return launch(axw_dw_bf16_reduce_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), 256, 0, s, part, dW, count, slices);
}
