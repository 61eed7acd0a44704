// attention_dropout_kernels.hip -- the multi-head fused attention with dropout of the probabilities after the softmax
// (include/flex_spmm.h: flex_attention_dropout, flex_attention_dropout_backward on fp32 rows, flex_attention_bf16_dropout,
// flex_attention_bf16_dropout_backward on bf16 rows; each with or without the per-edge bias): Out = sum_e alpha_e w_e V[col e] with
// w_e = keep(seed, e H + h) ? 1 / (1 - p) : 0, in the one forward launch and the two backward launches of the undropped calls, on the same
// plans.  tests/test_gpu_attention_dropout.py covers it, and tests/test_attention_dropout_host.py holds every instantiation to a case
// that launches it.
//
// The sweeps are attention_heads_device.h's under their compile-time DROP switch, for both element types and both settings of BIAS: the
// same walk, head split, slot placement, merges and LDS meeting places as the undropped kernels.  The mask is not stored: element (e, h)
// of the edge arrays is kept iff dropout_bits(seed, e H + h) < thr (internal.h, DropMask -- the definition flex_dropout_mask evaluates
// on the host), and every lane recomputes the bit of its head from the entry index it already holds, in all three launches: four 32-bit
// multiplies per (entry, head).  All lanes of a head compute the same bit; one lane computing and broadcasting it would trade the
// multiplies for a cross-lane move per bit and was not measured against this.  seed, thr and c are kernel arguments, the same for every
// lane.  The score, the bias, the maximum, the sum and P are the undropped kernels'; a kept entry enters Out, da and gV with the factor
// c, a dropped one is selected out and its V row (forward, row backward) or g row (gV) is not gathered.  The column launch needs the
// mask for gV alone: ds in dWork already holds it through da.
//
// This file holds the three kernels (namespace flex::dropout: 7 forms x (rows and rows backward x {float, bf16} x {no bias, bias} +
// columns backward x {float, bf16}) = 70 instantiations) and their launchers for both element types (internal.h, launch_dropout_*: a
// NULL Bias / GB launches the kernels without the bias); the entry points -- the per-head template pair with its drop flag set -- are
// attention_entry.h's.
#include <cmath>
#include <cstdint>

#include "attention_heads_device.h"

namespace flex {
namespace dropout {

using namespace flex::attention;

template <int W, int NS, bool BIAS, class E>
__global__ __launch_bounds__(256) void attention_dropout_rows(View v, HeadSplit hs, const E *__restrict__ Q, const E *__restrict__ K,
                                                               const E *__restrict__ V, const float *__restrict__ Bias, float scale, DropMask dm,
                                                               E *__restrict__ Out, float *__restrict__ P) {
    __shared__ HeadsShared<W, NS> sh;
    walk_rows_heads<W, NS, BIAS, true>(v, hs, Q, K, V, scale, Out, P, sh, Bias, dm);
}

template <int W, int NS, bool BIAS, class E>
__global__ __launch_bounds__(256) void attention_dropout_rows_backward(View v, HeadSplit hs, const E *__restrict__ K, const E *__restrict__ V,
                                                                        const float *__restrict__ P, const E *__restrict__ G, float scale, DropMask dm,
                                                                        E *__restrict__ GQ, float *__restrict__ GB, float *__restrict__ Work) {
    __shared__ HeadsRowShared<W, NS> sh;
    walk_rows_heads_backward<W, NS, BIAS, true>(v, hs, K, V, P, G, scale, GQ, Work, sh, GB, dm);
}

template <int W, int NS, class E>
__global__ __launch_bounds__(256) void attention_dropout_columns_backward(ColumnView v, HeadSplit hs, const E *__restrict__ Q, const E *__restrict__ G,
                                                                           const float *__restrict__ P, const float *__restrict__ DS, DropMask dm,
                                                                           E *__restrict__ GK, E *__restrict__ GV) {
    __shared__ HeadsColumnShared<W, NS> sh;
    walk_columns_heads_backward<W, NS, true>(v, hs, Q, G, P, DS, GK, GV, sh, dm);
}

}  // namespace dropout

// ---- launches

namespace attention {

template <class E>
int launch_dropout_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *Q, const E *K, const E *V, const float *Bias,
                        float scale, const DropMask &dm, E *Out, float *P, hipStream_t s) {
    const View v = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 grid = launch_grid(v), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        if (Bias)
            hipLaunchKernelGGL((dropout::attention_dropout_rows<W(), NS(), true, E>), grid, block, 0, s, v, hs, Q, K, V, Bias, scale, dm, Out, P);
        else
            hipLaunchKernelGGL((dropout::attention_dropout_rows<W(), NS(), false, E>), grid, block, 0, s, v, hs, Q, K, V, Bias, scale, dm, Out, P);
    });
    return FLEX_OK;
}

template <class E>
int launch_dropout_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *K, const E *V, const float *P,
                                 const E *G, float scale, const DropMask &dm, E *GQ, float *GB, float *Work, hipStream_t s) {
    const View rv = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 rgrid = launch_grid(rv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        if (GB)
            hipLaunchKernelGGL((dropout::attention_dropout_rows_backward<W(), NS(), true, E>), rgrid, block, 0, s, rv, hs, K, V, P, G, scale, dm, GQ, GB,
                               Work);
        else
            hipLaunchKernelGGL((dropout::attention_dropout_rows_backward<W(), NS(), false, E>), rgrid, block, 0, s, rv, hs, K, V, P, G, scale, dm, GQ,
                               GB, Work);
    });
    return FLEX_OK;
}

template <class E>
int launch_dropout_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *Q, const E *G, const float *P,
                                    const float *DS, const DropMask &dm, E *GK, E *GV, hipStream_t s) {
    const ColumnView cv = column_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 cgrid = launch_grid(cv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((dropout::attention_dropout_columns_backward<W(), NS(), E>), cgrid, block, 0, s, cv, hs, Q, G, P, DS, dm, GK, GV);
    });
    return FLEX_OK;
}

template int launch_dropout_rows<float>(const flex_plan *, const AttentionPick &, int, int, const float *, const float *, const float *, const float *,
                                        float, const DropMask &, float *, float *, hipStream_t);
template int launch_dropout_rows_backward<float>(const flex_plan *, const AttentionPick &, int, int, const float *, const float *, const float *,
                                                 const float *, float, const DropMask &, float *, float *, float *, hipStream_t);
template int launch_dropout_columns_backward<float>(const flex_plan *, const AttentionPick &, int, int, const float *, const float *, const float *,
                                                    const float *, const DropMask &, float *, float *, hipStream_t);
template int launch_dropout_rows<flex_bf16>(const flex_plan *, const AttentionPick &, int, int, const flex_bf16 *, const flex_bf16 *, const flex_bf16 *,
                                            const float *, float, const DropMask &, flex_bf16 *, float *, hipStream_t);
template int launch_dropout_rows_backward<flex_bf16>(const flex_plan *, const AttentionPick &, int, int, const flex_bf16 *, const flex_bf16 *,
                                                     const float *, const flex_bf16 *, float, const DropMask &, flex_bf16 *, float *, float *,
                                                     hipStream_t);
template int launch_dropout_columns_backward<flex_bf16>(const flex_plan *, const AttentionPick &, int, int, const flex_bf16 *, const flex_bf16 *,
                                                        const float *, const float *, const DropMask &, flex_bf16 *, flex_bf16 *, hipStream_t);

}  // namespace attention
}  // namespace flex
