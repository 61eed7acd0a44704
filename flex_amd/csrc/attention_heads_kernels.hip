// attention_heads_kernels.hip -- the multi-head forms of the fused attention (include/flex_spmm.h: flex_attention_heads,
// flex_attention_heads_backward): H heads of d = k / H columns each in the one forward launch and the two backward launches of
// flex_attention and flex_attention_backward, on the same plans.  tests/test_gpu_multihead_attention.py covers it; its (k, H) table is
// tests/attention_forms.py's, and tests/test_attention_routes.py holds every instantiation to a case that launches it.
//
// The sweeps are attention_heads_device.h's with the element type float (attention_bf16_kernels.hip instantiates the same sweeps with
// flex_bf16); the kernels below declare the LDS and call them.
//
// The walk, the head split and the layout of the edge arrays are described there.  Only the 16-byte form is built (the host refuses
// the rest).  This file holds the kernels and their three launchers (internal.h, launch_heads_* on float rows); the entry points, with
// the argument checks and the head split (internal.h, head_split_lg), are attention_entry.h's, and the biased entry points launch the
// column kernel of this file through launch_heads_columns_backward.
#include <cmath>
#include <cstdint>

#include "attention_heads_device.h"

namespace flex {
namespace attention {

template <int W, int NS>
__global__ __launch_bounds__(256) void attention_heads_rows(View v, HeadSplit hs, const float *__restrict__ Q, const float *__restrict__ K,
                                                             const float *__restrict__ V, float scale, float *__restrict__ Out, float *__restrict__ P) {
    __shared__ HeadsShared<W, NS> sh;
    walk_rows_heads<W, NS>(v, hs, Q, K, V, scale, Out, P, sh);
}

template <int W, int NS>
__global__ __launch_bounds__(256) void attention_heads_rows_backward(View v, HeadSplit hs, const float *__restrict__ K, const float *__restrict__ V,
                                                                      const float *__restrict__ P, const float *__restrict__ G, float scale,
                                                                      float *__restrict__ GQ, float *__restrict__ Work) {
    __shared__ HeadsRowShared<W, NS> sh;
    walk_rows_heads_backward<W, NS>(v, hs, K, V, P, G, scale, GQ, Work, sh);
}

template <int W, int NS>
__global__ __launch_bounds__(256) void attention_heads_columns_backward(ColumnView v, HeadSplit hs, const float *__restrict__ Q, const float *__restrict__ G,
                                                                         const float *__restrict__ P, const float *__restrict__ DS, float *__restrict__ GK,
                                                                         float *__restrict__ GV) {
    __shared__ HeadsColumnShared<W, NS> sh;
    walk_columns_heads_backward<W, NS>(v, hs, Q, G, P, DS, GK, GV, sh);
}

// ---- launches

int launch_heads_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Q, const float *G, const float *P,
                                  const float *DS, float *GK, float *GV, hipStream_t s) {
    const ColumnView cv = column_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 cgrid = launch_grid(cv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention_heads_columns_backward<W(), NS()>), cgrid, block, 0, s, cv, hs, Q, G, P, DS, GK, GV);
    });
    return FLEX_OK;
}

int launch_heads_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Q, const float *K, const float *V, float scale,
                      float *Out, float *P, hipStream_t s) {
    const View v = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 grid = launch_grid(v), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) { hipLaunchKernelGGL((attention_heads_rows<W(), NS()>), grid, block, 0, s, v, hs, Q, K, V, scale, Out, P); });
    return FLEX_OK;
}

int launch_heads_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *K, const float *V, const float *P,
                               const float *G, float scale, float *GQ, float *Work, hipStream_t s) {
    const View rv = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 rgrid = launch_grid(rv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention_heads_rows_backward<W(), NS()>), rgrid, block, 0, s, rv, hs, K, V, P, G, scale, GQ, Work);
    });
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex
