// attention_bias_kernels.hip -- the multi-head fused attention with a per-edge, per-head additive bias in the score
// (include/flex_spmm.h: flex_attention_bias, flex_attention_bias_backward on fp32 rows, flex_attention_bf16_bias,
// flex_attention_bf16_bias_backward on bf16 rows): alpha = the softmax over the row of t = fma(scale, <q, k>, bias[e, h]), a bias of
// -inf masking an entry for a head.  tests/test_gpu_attention_bias.py covers it; its (k, H) table is tests/attention_forms.py's, and
// tests/test_attention_routes.py holds every instantiation to a case that launches it.
//
// The sweeps are attention_heads_device.h's under their compile-time BIAS switch, for both element types: the same walk, head split, slot
// placement, merges and LDS meeting places as attention_heads_kernels.hip and attention_bf16_kernels.hip.  Forward: every lane of a head
// loads its head's bias element of a valid entry (one address for the HW lanes of a head), the score takes it in one fma, and everything
// after the score runs with scale 1, as the GAT kernels run it; the first dP sweep stores t.  Row backward: sweep 2 stores
// gBias = p (da - delta) beside ds, on the same lane.  The column backward does not see the bias: it is attention_heads_device.h's
// walk_columns_heads_backward, instantiated where it always was (attention_heads_kernels.hip, attention_bf16_kernels.hip) and launched
// by the entry points through launch_heads_columns_backward.  heads = 1 runs here as well.  Only the vector form is built (the host
// refuses the rest).  This file holds the two row kernels and their launchers for both element types (internal.h, launch_bias_rows,
// launch_bias_rows_backward); the entry points -- the per-head template pair with its bias flag set -- are attention_entry.h's.
#include <cmath>
#include <cstdint>

#include "attention_heads_device.h"

namespace flex {
namespace attention {

template <int W, int NS, class E>
__global__ __launch_bounds__(256) void attention_bias_rows(View v, HeadSplit hs, const E *__restrict__ Q, const E *__restrict__ K, const E *__restrict__ V,
                                                            const float *__restrict__ Bias, float scale, E *__restrict__ Out, float *__restrict__ P) {
    __shared__ HeadsShared<W, NS> sh;
    walk_rows_heads<W, NS, true>(v, hs, Q, K, V, scale, Out, P, sh, Bias);
}

template <int W, int NS, class E>
__global__ __launch_bounds__(256) void attention_bias_rows_backward(View v, HeadSplit hs, const E *__restrict__ K, const E *__restrict__ V,
                                                                     const float *__restrict__ P, const E *__restrict__ G, float scale,
                                                                     E *__restrict__ GQ, float *__restrict__ GB, float *__restrict__ Work) {
    __shared__ HeadsRowShared<W, NS> sh;
    walk_rows_heads_backward<W, NS, true>(v, hs, K, V, P, G, scale, GQ, Work, sh, GB);
}

// ---- launches

template <class E>
int launch_bias_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *Q, const E *K, const E *V, const float *Bias, float scale,
                     E *Out, float *P, hipStream_t s) {
    const View v = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 grid = launch_grid(v), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention_bias_rows<W(), NS(), E>), grid, block, 0, s, v, hs, Q, K, V, Bias, scale, Out, P);
    });
    return FLEX_OK;
}

template <class E>
int launch_bias_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *K, const E *V, const float *P, const E *G,
                              float scale, E *GQ, float *GB, float *Work, hipStream_t s) {
    const View rv = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 rgrid = launch_grid(rv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention_bias_rows_backward<W(), NS(), E>), rgrid, block, 0, s, rv, hs, K, V, P, G, scale, GQ, GB, Work);
    });
    return FLEX_OK;
}

// both element types; float first and the forward before the backward, the order in which the object has always held its kernels
template int launch_bias_rows<float>(const flex_plan *, const AttentionPick &, int, int, const float *, const float *, const float *, const float *, float,
                                     float *, float *, hipStream_t);
template int launch_bias_rows_backward<float>(const flex_plan *, const AttentionPick &, int, int, const float *, const float *, const float *,
                                              const float *, float, float *, float *, float *, hipStream_t);
template int launch_bias_rows<flex_bf16>(const flex_plan *, const AttentionPick &, int, int, const flex_bf16 *, const flex_bf16 *, const flex_bf16 *,
                                         const float *, float, flex_bf16 *, float *, hipStream_t);
template int launch_bias_rows_backward<flex_bf16>(const flex_plan *, const AttentionPick &, int, int, const flex_bf16 *, const flex_bf16 *, const float *,
                                                  const flex_bf16 *, float, flex_bf16 *, float *, float *, hipStream_t);

}  // namespace attention
}  // namespace flex
