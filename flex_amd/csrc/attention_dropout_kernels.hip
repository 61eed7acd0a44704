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
// columns backward x {float, bf16}) = 70 instantiations), their launchers (internal.h, launch_dropout_*) and the four entry points: the
// per-head template pair of attention_entry.h with the drop_p check beside the scale check.  They are here and not in attention_entry.h
// because the host simulator includes that header and has no stand-ins for these launchers.
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

// ---- the entry points: heads_forward / heads_backward of attention_entry.h, refusal for refusal, with the drop_p check beside the
// scale check.  drop_p == 0: once nothing is refused, `plain` -- the undropped entry point on the same operands -- runs instead, so the
// bits are its own (its checks repeat these and pass).  A NULL dBias / dGradBias selects the kernels without the bias.

template <class E, class F>
static int dropout_forward(const flex_plan *p, int heads, const E *dQ, const E *dK, const E *dV, const float *dBias, float scale, float drop_p,
                           uint64_t seed, E *dOut, float *dP, flex_stream_t stream, F &&plain) {
    if (!p || !p->at_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!(std::isfinite(scale) && scale > 0.f) || !drop_p_ok(drop_p)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<E>(p->k, p->ldb, p->ldc, {dQ, dK, dV, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (drop_p == 0.f) return plain();
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    if (const int rc = launch_dropout_rows(p, pick, heads, lg, dQ, dK, dV, dBias, scale, drop_mask(drop_p, seed), dOut, dP,
                                           reinterpret_cast<hipStream_t>(stream)))
        return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

template <class E, class F>
static int dropout_backward(const flex_plan *p, int heads, const E *dQ, const E *dK, const E *dV, const float *dP, const E *dGradOut, float scale,
                            float drop_p, uint64_t seed, E *dGradQ, E *dGradK, E *dGradV, float *dGradBias, float *dWork, flex_stream_t stream,
                            F &&plain) {
    if (!p || !p->ab_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!(std::isfinite(scale) && scale > 0.f) || !drop_p_ok(drop_p)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dP || !dGradOut || !dWork || dWork == dP) return FLEX_ERR_INVALID;
    if (dGradBias && (dGradBias == dP || dGradBias == dWork)) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<E>(p->k, p->ldb, p->ldc, {dQ, dK, dV, dGradOut, dGradQ, dGradK, dGradV});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradQ && !dGradK && !dGradV && !dGradBias) return FLEX_OK;
    if (drop_p == 0.f) return plain();
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const DropMask dm = drop_mask(drop_p, seed);
    if (dGradQ || dGradK || dGradBias) {
        if (const int rc = launch_dropout_rows_backward(p, pick, heads, lg, dK, dV, dP, dGradOut, scale, dm, dGradQ, dGradBias, dWork, s)) return rc;
    }
    if (dGradK || dGradV) {
        if (const int rc = launch_dropout_columns_backward(p, pick, heads, lg, dQ, dGradOut, dP, dWork, dm, dGradK, dGradV, s)) return rc;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex

extern "C" {

int flex_attention_dropout(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dBias, float scale, float drop_p,
                           uint64_t seed, float *dOut, float *dP, flex_stream_t stream) {
    return flex::attention::dropout_forward<float>(p, heads, dQ, dK, dV, dBias, scale, drop_p, seed, dOut, dP, stream, [&] {
        return dBias ? flex_attention_bias(p, heads, dQ, dK, dV, dBias, scale, dOut, dP, stream)
                     : flex_attention_heads(p, heads, dQ, dK, dV, scale, dOut, dP, stream);
    });
}

int flex_attention_dropout_backward(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                    const float *dGradOut, float scale, float drop_p, uint64_t seed, float *dGradQ, float *dGradK, float *dGradV,
                                    float *dGradBias, float *dWork, flex_stream_t stream) {
    return flex::attention::dropout_backward<float>(p, heads, dQ, dK, dV, dP, dGradOut, scale, drop_p, seed, dGradQ, dGradK, dGradV, dGradBias, dWork,
                                                    stream, [&] {
        return dGradBias ? flex_attention_bias_backward(p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dGradBias, dWork, stream)
                         : flex_attention_heads_backward(p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dWork, stream);
    });
}

int flex_attention_bf16_dropout(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dBias,
                                float scale, float drop_p, uint64_t seed, flex_bf16 *dOut, float *dP, flex_stream_t stream) {
    return flex::attention::dropout_forward<flex_bf16>(p, heads, dQ, dK, dV, dBias, scale, drop_p, seed, dOut, dP, stream, [&] {
        return dBias ? flex_attention_bf16_bias(p, heads, dQ, dK, dV, dBias, scale, dOut, dP, stream)
                     : flex_attention_bf16(p, heads, dQ, dK, dV, scale, dOut, dP, stream);
    });
}

int flex_attention_bf16_dropout_backward(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dP,
                                         const flex_bf16 *dGradOut, float scale, float drop_p, uint64_t seed, flex_bf16 *dGradQ, flex_bf16 *dGradK,
                                         flex_bf16 *dGradV, float *dGradBias, float *dWork, flex_stream_t stream) {
    return flex::attention::dropout_backward<flex_bf16>(p, heads, dQ, dK, dV, dP, dGradOut, scale, drop_p, seed, dGradQ, dGradK, dGradV, dGradBias,
                                                        dWork, stream, [&] {
        return dGradBias ? flex_attention_bf16_bias_backward(p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dGradBias, dWork, stream)
                         : flex_attention_bf16_backward(p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dWork, stream);
    });
}

}  // extern "C"
