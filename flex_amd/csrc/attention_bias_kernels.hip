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
// from here through launch_columns_backward.  heads = 1 runs here as well.  Only the vector form is built (the host refuses the rest).
#include <cmath>
#include <cstdint>
#include <initializer_list>

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

// the vector form of either element type: k and both strides multiples of four elements, every row operand aligned to four elements
// (16 bytes of float, 8 of flex_bf16; a NULL output is aligned)
template <class E>
inline AttentionPick pick_rows(const flex_plan *p, std::initializer_list<const void *> rows) {
    AttentionPick pick = attention_pick(p->k, p->ldb, p->ldc, nullptr, nullptr, nullptr, nullptr);
    for (const void *r : rows) pick.vec4 = pick.vec4 && reinterpret_cast<uintptr_t>(r) % (4 * sizeof(E)) == 0;
    return pick;
}

template <class E>
struct BiasOperands {
    const E *Q, *K, *V;
    const float *P;
    const E *G;
    float scale;
    E *GQ, *GK, *GV;
    float *GB, *Work;
};

template <class E>
int bias_forward(const flex_plan *p, int heads, const E *dQ, const E *dK, const E *dV, const float *dBias, float scale, E *dOut, float *dP,
                 flex_stream_t stream) {
    if (!p || !p->at_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!std::isfinite(scale) || !(scale > 0.f)) return FLEX_ERR_INVALID;
    HeadSplit hs;
    if (const int rc = split_of(p->k, heads, &hs)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dBias || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<E>(p, {dQ, dK, dV, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const View v = row_view(p);
    const dim3 grid = launch_grid(v), block(64 * kWavesPerBlock);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention_bias_rows<W(), NS(), E>), grid, block, 0, s, v, hs, dQ, dK, dV, dBias, scale, dOut, dP);
    });
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

template <class E>
int bias_backward(const flex_plan *p, int heads, const E *dQ, const E *dK, const E *dV, const float *dP, const E *dGradOut, float scale, E *dGradQ,
                  E *dGradK, E *dGradV, float *dGradBias, float *dWork, flex_stream_t stream) {
    if (!p || !p->ab_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!std::isfinite(scale) || !(scale > 0.f)) return FLEX_ERR_INVALID;
    HeadSplit hs;
    if (const int rc = split_of(p->k, heads, &hs)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dP || !dGradOut || !dWork || dWork == dP) return FLEX_ERR_INVALID;
    if (dGradBias && (dGradBias == dP || dGradBias == dWork)) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<E>(p, {dQ, dK, dV, dGradOut, dGradQ, dGradK, dGradV});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradQ && !dGradK && !dGradV && !dGradBias) return FLEX_OK;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const View rv = row_view(p);
    const dim3 rgrid = launch_grid(rv), block(64 * kWavesPerBlock);
    const BiasOperands<E> o{dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dGradBias, dWork};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (o.GQ || o.GK || o.GB) {
        dispatch(pick, [&](auto W, auto NS) {
            hipLaunchKernelGGL((attention_bias_rows_backward<W(), NS(), E>), rgrid, block, 0, s, rv, hs, o.K, o.V, o.P, o.G, o.scale, o.GQ, o.GB, o.Work);
        });
    }
    if (o.GK || o.GV) launch_columns_backward(p, pick, hs, o.Q, o.G, o.P, o.Work, o.GK, o.GV, s);
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex

using namespace flex;

extern "C" {

int flex_attention_bias(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dBias, float scale, float *dOut,
                        float *dP, flex_stream_t stream) {
    return attention::bias_forward<float>(p, heads, dQ, dK, dV, dBias, scale, dOut, dP, stream);
}

int flex_attention_bias_backward(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                 const float *dGradOut, float scale, float *dGradQ, float *dGradK, float *dGradV, float *dGradBias, float *dWork,
                                 flex_stream_t stream) {
    return attention::bias_backward<float>(p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dGradBias, dWork, stream);
}

int flex_attention_bf16_bias(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dBias,
                             float scale, flex_bf16 *dOut, float *dP, flex_stream_t stream) {
    return attention::bias_forward<flex_bf16>(p, heads, dQ, dK, dV, dBias, scale, dOut, dP, stream);
}

int flex_attention_bf16_bias_backward(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dP,
                                      const flex_bf16 *dGradOut, float scale, flex_bf16 *dGradQ, flex_bf16 *dGradK, flex_bf16 *dGradV,
                                      float *dGradBias, float *dWork, flex_stream_t stream) {
    return attention::bias_backward<flex_bf16>(p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dGradBias, dWork, stream);
}

}  // extern "C"
