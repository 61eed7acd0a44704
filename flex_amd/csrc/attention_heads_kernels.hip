// attention_heads_kernels.hip -- the multi-head forms of the fused attention (include/flex_spmm.h: flex_attention_heads,
// flex_attention_heads_backward): H heads of d = k / H columns each in the one forward launch and the two backward launches of
// flex_attention and flex_attention_backward, on the same plans.  tests/test_gpu_multihead_attention.py covers it; its (k, H) table is
// tests/attention_forms.py's, and tests/test_attention_routes.py holds every instantiation to a case that launches it.
//
// The sweeps are attention_heads_device.h's with the element type float (attention_bf16_kernels.hip instantiates the same sweeps with
// flex_bf16); the kernels below declare the LDS and call them.
//
// The walk, the head split and the layout of the edge arrays are described there.  Only the 16-byte form is built (the host refuses
// the rest).
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

struct HeadsOperands {
    const float *Q, *K, *V, *P, *G;
    float scale;
    float *GQ, *GK, *GV, *Work;
};

void launch_columns_backward(const flex_plan *p, const AttentionPick &pick, const HeadSplit &hs, const float *Q, const float *G, const float *P,
                             const float *DS, float *GK, float *GV, hipStream_t s) {
    const ColumnView cv = column_view(p);
    const dim3 cgrid = launch_grid(cv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention_heads_columns_backward<W(), NS()>), cgrid, block, 0, s, cv, hs, Q, G, P, DS, GK, GV);
    });
}

}  // namespace attention
}  // namespace flex

using namespace flex;

extern "C" {

int flex_attention_heads(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, float scale, float *dOut, float *dP,
                         flex_stream_t stream) {
    if (!p || !p->at_ok || heads < 1) return FLEX_ERR_INVALID;
    if (heads == 1) return flex_attention(p, dQ, dK, dV, scale, dOut, dP, stream);
    if (!std::isfinite(scale) || !(scale > 0.f)) return FLEX_ERR_INVALID;
    attention::HeadSplit hs;
    if (const int rc = attention::split_of(p->k, heads, &hs)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = attention_pick(p->k, p->ldb, p->ldc, dQ, dK, dV, dOut);
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const attention::View v = attention::row_view(p);
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    attention::dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((attention::attention_heads_rows<W(), NS()>), grid, block, 0, s, v, hs, dQ, dK, dV, scale, dOut, dP);
    });
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int flex_attention_heads_backward(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                  const float *dGradOut, float scale, float *dGradQ, float *dGradK, float *dGradV, float *dWork, flex_stream_t stream) {
    if (!p || !p->ab_ok || heads < 1) return FLEX_ERR_INVALID;
    if (heads == 1) return flex_attention_backward(p, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dWork, stream);
    if (!std::isfinite(scale) || !(scale > 0.f)) return FLEX_ERR_INVALID;
    attention::HeadSplit hs;
    if (const int rc = attention::split_of(p->k, heads, &hs)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dP || !dGradOut || !dWork || dWork == dP) return FLEX_ERR_INVALID;
    // the forward's rule over every row operand of the two launches (a NULL output is aligned)
    const AttentionPick pick = attention_pick(p->k, p->ldb, p->ldc, dQ, dK, dV, dGradOut);
    if (!pick.vec4 || !attention_pick(p->k, p->ldb, p->ldc, dGradQ, dGradK, dGradV, nullptr).vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradQ && !dGradK && !dGradV) return FLEX_OK;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const attention::View rv = attention::row_view(p);
    const attention::ColumnView cv = attention::column_view(p);
    const dim3 rgrid = attention::launch_grid(rv), cgrid = attention::launch_grid(cv), block(64 * kWavesPerBlock);
    const attention::HeadsOperands o{dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dWork};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    attention::dispatch(pick, [&](auto W, auto NS) {
        using namespace attention;
        if (o.GQ || o.GK) hipLaunchKernelGGL((attention_heads_rows_backward<W(), NS()>), rgrid, block, 0, s, rv, hs, o.K, o.V, o.P, o.G, o.scale, o.GQ, o.Work);
        if (o.GK || o.GV) hipLaunchKernelGGL((attention_heads_columns_backward<W(), NS()>), cgrid, block, 0, s, cv, hs, o.Q, o.G, o.P, o.Work, o.GK, o.GV);
    });
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // extern "C"
