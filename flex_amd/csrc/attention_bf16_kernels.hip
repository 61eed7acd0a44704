// attention_bf16_kernels.hip -- the multi-head fused attention on bf16 row operands (include/flex_spmm.h: flex_attention_bf16,
// flex_attention_bf16_backward): Q, K, V, Out, g, gQ, gK and gV are flex_bf16, the edge arrays dP and dWork stay fp32, and everything
// between a row's load and a row's store is the fp32 code of flex_attention_heads and flex_attention_heads_backward.
// tests/test_gpu_attention_bf16.py covers it; its (k, H) table is tests/attention_forms.py's, and tests/test_attention_routes.py holds
// every instantiation to a case that launches it.
//
// The sweeps are attention_heads_device.h's with the element type flex_bf16: the same walk, head split, slot placement, merges and LDS
// meeting places (fp32) as attention_heads_kernels.hip, one forward launch and two backward launches on the same plans.  A row load is
// one 8-byte load of four bf16 widened by shifts (exact), a row store narrows four fp32 to bf16 (round to nearest even, the one rounding
// of an output element) and is one 8-byte store (attention_device.h: load_cols, store_cols).  With the same source expressions under
// -ffp-contract=on, the fp32 value that is rounded at the store -- and every element of dP and dWork -- has the bits that
// flex_attention_heads and flex_attention_heads_backward give on the widened operands.  heads = 1 runs here as well (there is no
// generic form to forward to), so d = k is then a power of two.  Only the 8-byte form is built (the host refuses the rest).
// This file holds the kernels and their three launchers (internal.h, launch_heads_* on flex_bf16 rows); the entry points, with the argument
// checks, the alignment rule (internal.h, pick_rows) and the head split (head_split_lg), are attention_entry.h's.
#include <cmath>
#include <cstdint>

#include "attention_heads_device.h"

namespace flex {
namespace attention {

template <int W, int NS>
__global__ __launch_bounds__(256) void attention_bf16_rows(View v, HeadSplit hs, const flex_bf16 *__restrict__ Q, const flex_bf16 *__restrict__ K,
                                                            const flex_bf16 *__restrict__ V, float scale, flex_bf16 *__restrict__ Out,
                                                            float *__restrict__ P) {
    __shared__ HeadsShared<W, NS> sh;
    walk_rows_heads<W, NS>(v, hs, Q, K, V, scale, Out, P, sh);
}

template <int W, int NS>
__global__ __launch_bounds__(256) void attention_bf16_rows_backward(View v, HeadSplit hs, const flex_bf16 *__restrict__ K, const flex_bf16 *__restrict__ V,
                                                                     const float *__restrict__ P, const flex_bf16 *__restrict__ G, float scale,
                                                                     flex_bf16 *__restrict__ GQ, float *__restrict__ Work) {
    __shared__ HeadsRowShared<W, NS> sh;
    walk_rows_heads_backward<W, NS>(v, hs, K, V, P, G, scale, GQ, Work, sh);
}

template <int W, int NS>
__global__ __launch_bounds__(256) void attention_bf16_columns_backward(ColumnView v, HeadSplit hs, const flex_bf16 *__restrict__ Q,
                                                                        const flex_bf16 *__restrict__ G, const float *__restrict__ P,
                                                                        const float *__restrict__ DS, flex_bf16 *__restrict__ GK,
                                                                        flex_bf16 *__restrict__ GV) {
    __shared__ HeadsColumnShared<W, NS> sh;
    walk_columns_heads_backward<W, NS>(v, hs, Q, G, P, DS, GK, GV, sh);
}

// ---- launches

int launch_heads_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const flex_bf16 *Q, const flex_bf16 *G, const float *P,
                                  const float *DS, flex_bf16 *GK, flex_bf16 *GV, hipStream_t s) {
    const ColumnView cv = column_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 cgrid = launch_grid(cv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention_bf16_columns_backward<W(), NS()>), cgrid, block, 0, s, cv, hs, Q, G, P, DS, GK, GV);
    });
    return FLEX_OK;
}

int launch_heads_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const flex_bf16 *Q, const flex_bf16 *K, const flex_bf16 *V, float scale,
                      flex_bf16 *Out, float *P, hipStream_t s) {
    const View v = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 grid = launch_grid(v), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) { hipLaunchKernelGGL((attention_bf16_rows<W(), NS()>), grid, block, 0, s, v, hs, Q, K, V, scale, Out, P); });
    return FLEX_OK;
}

int launch_heads_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const flex_bf16 *K, const flex_bf16 *V, const float *P,
                               const flex_bf16 *G, float scale, flex_bf16 *GQ, float *Work, hipStream_t s) {
    const View rv = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 rgrid = launch_grid(rv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention_bf16_rows_backward<W(), NS()>), rgrid, block, 0, s, rv, hs, K, V, P, G, scale, GQ, Work);
    });
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex
