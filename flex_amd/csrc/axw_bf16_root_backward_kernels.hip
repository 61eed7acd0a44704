// axw_bf16_root_backward_kernels.hip -- dW, dR and db of the bf16 layer with a root-weight term in ONE pass over X (libflex_axw.so,
// flex_axw_backward_root_bf16):
//   dW[dim x c] = rn_bf16(X[n x dim]^T G[n x cp])    dR[dim x c] = rn_bf16(X^T dOut[n x cp])    db[c] = 1^T dOut  (fp32)
// axw_dw_bf16_kernel (axw_bf16_backward_kernels.hip) run twice would read and transpose X, the largest array of the layer, twice.  This
// kernel stages X's fragments once per stage and multiplies them against both right operands.  From that kernel: v_mfma_f32_32x32x16_bf16
// with k = the row index, n-slices by 128-row blocks of dW, X and the right operands transposed in registers (8 x 8 blocks, eight 16-byte
// loads and eight 16-byte LDS stores a thread, the frag_slot swizzle), stages of 64 rows in two LDS buffers with one barrier a stage,
// one fp32 partial per (slice, block) and a reduce kernel that adds the partials in slice order and rounds once.  What differs:
//   * the work split: a workgroup owns one n-slice, one 128-row block gi of dW and dR, and one column window gj of min(128, cp - 128 gj)
//     columns.  Its tiles are the window's nt <= NT tiles of G and the same nt tiles of dOut: 2 nt accumulator tiles a wave, 4 at cp = 64
//     (64 registers, as axw_dw_bf16_kernel) and 8 from cp = 128 on (128 registers).  NT = min(4, cp / 32) is the instantiation.
//   * LDS: a stage is X's 16 KiB and 4 NT KiB of fragments of each right operand ([k-step][NT tiles][half][32 columns]); two stages are
//     64 KiB at NT = 2 (two workgroups a CU) and 96 KiB at NT = 4 (one), dynamic and asked for with hipFuncSetAttribute.
//   * the loaders: THREE operands of 128 blocks each a stage do not divide over four waves, so the workgroup has SIX: waves 0 and 1 carry
//     X's blocks, 2 and 3 G's, 4 and 5 dOut's -- every loader thread one 8 x 8 block a stage, as in axw_dw_bf16_kernel.  Waves 0 .. 3
//     multiply (wave w the rows 128 gi + 32 w of dW and dR); waves 4 and 5 only load, and sum db.  The other ways to split it -- 1.5
//     blocks a thread of four waves (half blocks of 4 rows: 8-byte LDS stores and twice the merges) or G and dOut both on waves 2 and 3
//     (64 load registers there and a loader twice as slow as its partner) -- cost more than two waves that do not multiply: six waves are
//     two on two of the four SIMDs, and the compiler's budget of 256 registers a wave holds the 128 accumulators.
//   * db: the threads of waves 4 and 5 have dOut's raw rows in registers and add them, row by row in ascending order, into 8 fp32
//     column sums each; after the slice's last stage the 8 row groups of a column are added in row-group order through LDS, and the
//     workgroups with gi == 0 write c floats a slice.  A sum passes rows / 8 + 8 + slices roundings: fewer than rows per slice + slices.
//   * X == NULL (db alone): only the window workgroups of gi = 0 are launched, nothing of X or G is loaded and nothing is multiplied.
//   * rows past the slice end or past n, columns >= dim of X and >= cp of G and dOut are zero OPERANDS selected in registers, never
//     loaded; a k-step of 16 rows wholly past the end is not multiplied; a wave whose rows lie past dim still stages and meets the
//     barriers; the padding columns c .. cp-1 are computed and dropped.
//   * order of every sum of dW and dR: that of axw_dw_bf16_kernel -- k-step by k-step (16 rows, ascending) into one fp32 accumulator per
//     entry, then the partials in slice order: L = rows per slice + slices roundings (include/flex_axw.h).  No atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "axw_bf16_dw_device.h"  // frag_slot, the block load and store, slice_sum: shared with axw_bf16_backward_kernels.hip

namespace flex_axw_bf16_dw {

constexpr int kThreads = 6 * 64;     // three loader pairs, of which the first two multiply
constexpr int kXFrags = 4 * 4 * 64;  // X's fragments of a stage: [4 k-steps][4 waves' row tiles][64 lanes]

template <int NT>  // tiles of a column window of G and of dOut: min(4, cp / 32)
__global__ __launch_bounds__(kThreads) void axw_dw_bf16_root_kernel(const flex_bf16 *__restrict__ X, const flex_bf16 *__restrict__ G,
                                                                    const flex_bf16 *__restrict__ dOut, float *__restrict__ part, int n, int dim,
                                                                    int c, int cp, int rows_per_slice) {
    extern __shared__ u32x4 sF[];  // [buffer][X: kXFrags | G: kOpFrags | dOut: kOpFrags]
    constexpr int kOpFrags = 4 * NT * 64, kBufFrags = kXFrags + 2 * kOpFrags;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool want_w = X != nullptr;  // workgroup-uniform
    const int slice = blockIdx.x, blocks_i = want_w ? (dim + 127) / 128 : 1;
    const int gi = blockIdx.y % blocks_i, gj = blockIdx.y / blocks_i;
    const int i0 = gi * 128 + wave * 32, j0 = gj * 128;
    const bool active = want_w && wave < 4 && i0 < dim;  // wave-uniform; every wave loads, stores and meets the barriers
    const int nt = min(NT, (cp - j0) / 32);
    const int r_beg = slice * rows_per_slice, r_end = min(n, r_beg + rows_per_slice);
    const size_t count = static_cast<size_t>(2) * dim * c + c;  // floats of a slice's partial: [dW | dR | db]

    // the loader's block: operand op (0 X, 1 G, 2 dOut), rows 8 rg .. 8 rg + 7 of the stage, columns 8 q .. 8 q + 7 of the operand's window
    const int op = wave >> 1, q = tid & 15, rg = (tid & 127) >> 4;
    const int ld = op ? cp : dim, col = (op ? j0 : gi * 128) + 8 * q;
    // dim % 8 == 0 and cp % 8 == 0: a block's eight columns stand or fall together.  A right operand's block lies in tile q >> 2 < NT
    const bool col_ok = col < ld && (op == 2 || want_w) && (op == 0 || (q >> 2) < NT);
    const bool stores = want_w && (op == 0 || (q >> 2) < NT);
    const bool sums = op == 2 && gi == 0;  // wave-uniform
    const flex_bf16 *src = (op == 0 ? X : op == 1 ? G : dOut) + col;
    u32x4 v[8];  // v[e][d]: columns 2 d (low half) and 2 d + 1 of row e of the block
    auto load = [&](int r0) { FLEX_AXW_DW_LOAD_BLOCK(v, src, ld, r0 + 8 * rg, r_end, col_ok) };
    auto store = [&](int buf) {
        u32x4 *dst = sF + buf * kBufFrags + (op == 0 ? 0 : op == 1 ? kXFrags : kXFrags + kOpFrags);
        FLEX_AXW_DW_STORE_BLOCK(v, dst, rg, q, op ? NT : 4)
    };
    float colsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // db: columns col .. col + 7 over this thread's rows, in ascending order
    auto sum_rows = [&]() {
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                colsum[2 * d] += __uint_as_float(v[e][d] << 16);
                colsum[2 * d + 1] += __uint_as_float(v[e][d] & 0xFFFF0000u);
            }
    };

    f32x16 acc[2 * NT];  // [G's tiles | dOut's tiles]
#pragma unroll
    for (int t = 0; t < 2 * NT; ++t)
#pragma unroll
        for (int k = 0; k < 16; ++k) acc[t][k] = 0.f;

    load(r_beg);
    int buf = 0;
    for (int r0 = r_beg; r0 < r_end; r0 += kStage, buf ^= 1) {  // the same trip count for every wave of the workgroup
        if (stores) store(buf);
        if (sums) sum_rows();
        __syncthreads();  // the other buffer was last read before this barrier: the next store into it needs no barrier of its own
        if (r0 + kStage < r_end) load(r0 + kStage);
        if (active) {
            const u32x4 *fx = sF + buf * kBufFrags, *fg = fx + kXFrags, *fo = fg + kOpFrags;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                if (r0 + 16 * s >= r_end) break;  // wave-uniform
                const bf16x8 a = __builtin_bit_cast(bf16x8, fx[frag_slot(s, wave, lane >> 5, lane & 31, 4)]);
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    if (t < nt) {
                        const int slot = frag_slot(s, t, lane >> 5, lane & 31, NT);
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, fg[slot]), acc[t], 0, 0, 0);
                        acc[NT + t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, __builtin_bit_cast(bf16x8, fo[slot]), acc[NT + t], 0, 0, 0);
                    }
            }
        }
    }
    float *dst = part + static_cast<size_t>(slice) * count;
    if (gi == 0) {  // workgroup-uniform: db of this window's columns, the 8 row groups of a column added in row-group order
        float *sDb = reinterpret_cast<float *>(sF);  // [8 row groups][128 columns]
        __syncthreads();                             // every wave has read its last stage
        if (op == 2) {
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) sDb[rg * 128 + 8 * q + cc] = colsum[cc];
        }
        __syncthreads();
        if (tid < 32 * nt && j0 + tid < c) {
            float s = sDb[tid];
#pragma unroll
            for (int g = 1; g < 8; ++g) s += sDb[g * 128 + tid];
            dst[static_cast<size_t>(2) * dim * c + j0 + tid] = s;
        }
    }
    if (!active) return;
    // acc[t][k] = dW[i0 + 8 (k >> 2) + 4 (lane >> 5) + (k & 3)][j0 + 32 t + (lane & 31)], acc[NT + t][k] the same entry of dR
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = j0 + 32 * t + (lane & 31);
        if (t >= nt || j >= c) continue;
        FLEX_AXW_DW_FOR_TILE_ROWS(k, ii, i0, lane >> 5, dim) {
            dst[static_cast<size_t>(ii) * c + j] = acc[t][k];
            dst[static_cast<size_t>(dim + ii) * c + j] = acc[NT + t][k];
        }
    }
}

// out[e] = part[0][e] + part[1][e] + ... + part[S-1][e], left to right in fp32, the loads 16 at a time (axw_dw_bf16_reduce_kernel), for the
// elements from `first` on of a partial of [dW: dc | dR: dc | db: c] floats; dW and dR are rounded once to bf16, db stays fp32.  An
// output that is NULL is neither summed nor written.
__global__ __launch_bounds__(256) void axw_dw_bf16_root_reduce_kernel(const float *__restrict__ part, flex_bf16 *__restrict__ dW,
                                                                      flex_bf16 *__restrict__ dR, float *__restrict__ db, int first, int dc, int c,
                                                                      int slices) {
    const int e = first + blockIdx.x * 256 + threadIdx.x, count = 2 * dc + c;
    if (e >= count || (e < dc ? !dW : e < 2 * dc ? !dR : !db)) return;
    const float s = slice_sum(part, e, count, slices);
    if (e < dc)
        dW[e] = static_cast<flex_bf16>(bf16_bits(s));
    else if (e < 2 * dc)
        dR[e - dc] = static_cast<flex_bf16>(bf16_bits(s));
    else
        db[e - 2 * dc] = s;
}

// rows of an n-slice: ceil(n / S0) rounded up to a whole number of stages, S0 the smallest of
//   ceil(n / 256)                      about 256 rows a slice, as the other dW rules,
//   floor(wgs n_cus / blocks)          wgs workgroups a CU -- 2 while c <= 64 (64 KiB of LDS each), else 1 (96 KiB) -- over the
//                                      blocks = ceil(dim / 128) ceil(c / 128) of dW; rounded DOWN, so that slices x blocks workgroups
//                                      are resident at once: a few workgroups more than fit would run alone after all the others,
//   floor(n / (4 c))                   slices x 2 dim c x 4 bytes of dW and dR partials <= n x dim x 2 bytes, the bytes of X (db adds c
//                                      floats a slice),
// and at least 1.  slices = ceil(n / rows) <= S0, and no slice is empty.
inline int dw_root_rows(int n, int dim, int c, int n_cus) {
    const int blocks = ((dim + 127) / 128) * ((c + 127) / 128), wgs = c <= 64 ? 2 : 1;
    const int s0 = std::max(1, std::min({(n + 255) / 256, wgs * n_cus / blocks, n / (4 * c)}));
    return ((n + s0 - 1) / s0 + kStage - 1) / kStage * kStage;
}

}  // namespace flex_axw_bf16_dw

// n-slices of the dual dW kernel: ceil(n / rows), rows = dw_root_rows above; 0 for arguments the launcher refuses
extern "C" int flex_axw_dw_bf16_root_slices(int n, int dim, int c, int n_cus) {
    if (n <= 0 || dim <= 0 || c <= 0 || n_cus <= 0) return 0;
    const int rows = flex_axw_bf16_dw::dw_root_rows(n, dim, c, n_cus);
    return (n + rows - 1) / rows;
}

// dW[dim x c] = rn_bf16(X[n x dim]^T G[n x cp]), dR[dim x c] = rn_bf16(X^T dOut[n x cp]) and db[c] = 1^T dOut (fp32) through `part`
// (flex_axw_dw_bf16_root_slices(n, dim, c, n_cus) * (2 dim c + c) floats).  An output that is NULL is not written; X may be NULL when
// dW and dR both are.  Takes n >= 32, 0 < dim <= 4096, dim % 8 == 0, 0 < c <= cp <= 256, cp % 32 == 0, n_cus > 0 and 16-byte aligned X, G
// and dOut; anything else returns hipErrorInvalidValue before a launch.  Returns hipSuccess or the launch error.
extern "C" hipError_t flex_axw_dw_bf16_root_launch(const flex_bf16 *X, const flex_bf16 *G, const flex_bf16 *dOut, flex_bf16 *dW, flex_bf16 *dR,
                                                   float *db, float *part, int n, int dim, int c, int cp, int n_cus, hipStream_t s) {
    using namespace flex_axw_bf16_dw;
    const bool want_w = dW || dR;
    if ((want_w && !X) || !G || !dOut || !part || n < 32 || dim <= 0 || dim > 4096 || dim % 8 != 0 || c <= 0 || c > cp || cp > 256 || cp % 32 != 0 ||
        n_cus <= 0 || misaligned(X) || misaligned(G) || misaligned(dOut))
        return hipErrorInvalidValue;
    if (!want_w && !db) return hipSuccess;
    const int rows = dw_root_rows(n, dim, c, n_cus), slices = (n + rows - 1) / rows;
    const flex_bf16 *x = want_w ? X : nullptr;
    const dim3 grid(static_cast<unsigned>(slices), static_cast<unsigned>((x ? (dim + 127) / 128 : 1) * ((cp + 127) / 128)));
    const hipError_t e = dispatch_tiles<1, 2, 3, 4>(cp / 32, [&](auto tiles) {
        constexpr int NT = decltype(tiles)::value;
        return launch(axw_dw_bf16_root_kernel<NT>, grid, kThreads, static_cast<size_t>(2) * (kXFrags + 2 * 4 * NT * 64) * sizeof(u32x4), s, x, G, dOut,
                      part, n, dim, c, cp, rows);
    });
    if (e != hipSuccess) return e;
    const int dc = dim * c, first = want_w ? 0 : 2 * dc, todo = 2 * dc + c - first;
    return launch(axw_dw_bf16_root_reduce_kernel, dim3(static_cast<unsigned>((todo + 255) / 256)), 256, 0, s, part, dW, dR, db, first, dc, c, slices);
}
