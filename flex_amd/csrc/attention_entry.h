// attention_entry.h -- the twelve entry points of the fused attention (include/flex_spmm.h): the argument checks, the pick of the
// (W, NS) form and which launch happens for which outputs.  Host code only, and ordinary (non-inline) definitions: this file is included
// by exactly ONE translation unit per build -- attention_kernels.hip in the GPU library, tests/hostsim/shim.cpp in the host simulator --
// so both builds run the same entry points, as both run plan.cpp's flex_spmm.  What differs between them is the launchers alone
// (internal.h, flex::attention::launch_*): in the library the view, the grid and the kernel of the attention_*_kernels.hip files, in the
// simulator a stand-in that logs the instantiation's name.  An entry point decides which launchers run, holds the plan's device around
// them and returns the first launcher code that is not FLEX_OK.
//
// The single-head pair, the GAT pair and the per-head family each keep their own order of refusals: the single-head pair runs the
// generic form on misaligned operands and looks at the outputs before the pick; the per-head family (heads, bf16 and the two bias
// forms: one template pair over the element type) refuses misaligned operands, and does so before "no output wanted".
#pragma once
#include <cmath>

#include "internal.h"
#include "plan.h"

namespace flex {
namespace attention {

static bool scale_ok(float scale) { return std::isfinite(scale) && scale > 0.f; }
static bool slope_ok(float slope) { return std::isfinite(slope) && slope > 0.f && slope <= 1.f; }

// flex_attention_heads (heads > 1), flex_attention_bf16, and with `bias` flex_attention_bias and flex_attention_bf16_bias.  heads = 1
// runs here as well: d = k is then a power of two.
template <class E>
static int heads_forward(bool bias, const flex_plan *p, int heads, const E *dQ, const E *dK, const E *dV, const float *dBias, float scale, E *dOut,
                         float *dP, flex_stream_t stream) {
    if (!p || !p->at_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!scale_ok(scale)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || (bias && !dBias) || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<E>(p->k, p->ldb, p->ldc, {dQ, dK, dV, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = bias ? launch_bias_rows(p, pick, heads, lg, dQ, dK, dV, dBias, scale, dOut, dP, s)
                            : launch_heads_rows(p, pick, heads, lg, dQ, dK, dV, scale, dOut, dP, s))
        return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

// the backward of the same four; dGradBias is NULL without `bias`.  The column launch does not see the bias.
template <class E>
static int heads_backward(bool bias, const flex_plan *p, int heads, const E *dQ, const E *dK, const E *dV, const float *dP, const E *dGradOut, float scale,
                          E *dGradQ, E *dGradK, E *dGradV, float *dGradBias, float *dWork, flex_stream_t stream) {
    if (!p || !p->ab_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!scale_ok(scale)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dP || !dGradOut || !dWork || dWork == dP) return FLEX_ERR_INVALID;
    if (dGradBias && (dGradBias == dP || dGradBias == dWork)) return FLEX_ERR_INVALID;
    // one rule over every row operand of the two launches
    const AttentionPick pick = pick_rows<E>(p->k, p->ldb, p->ldc, {dQ, dK, dV, dGradOut, dGradQ, dGradK, dGradV});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradQ && !dGradK && !dGradV && !dGradBias) return FLEX_OK;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dGradQ || dGradK || dGradBias) {
        if (const int rc = bias ? launch_bias_rows_backward(p, pick, heads, lg, dK, dV, dP, dGradOut, scale, dGradQ, dGradBias, dWork, s)
                                : launch_heads_rows_backward(p, pick, heads, lg, dK, dV, dP, dGradOut, scale, dGradQ, dWork, s))
            return rc;
    }
    if (dGradK || dGradV) {
        if (const int rc = launch_heads_columns_backward(p, pick, heads, lg, dQ, dGradOut, dP, dWork, dGradK, dGradV, s)) return rc;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex

extern "C" {

int flex_attention(const flex_plan *p, const float *dQ, const float *dK, const float *dV, float scale, float *dOut, float *dP, flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->at_ok) return FLEX_ERR_INVALID;
    if (!attention::scale_ok(scale)) return FLEX_ERR_INVALID;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = attention_pick(p->k, p->ldb, p->ldc, dQ, dK, dV, dOut);
    if (p->k > 4 * 64 * kAtMaxSlabs) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    if (const int rc = attention::launch_rows(p, pick, dQ, dK, dV, scale, dOut, dP, reinterpret_cast<hipStream_t>(stream))) return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int flex_attention_backward(const flex_plan *p, const float *dQ, const float *dK, const float *dV, const float *dP, const float *dGradOut, float scale,
                            float *dGradQ, float *dGradK, float *dGradV, float *dWork, flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->ab_ok) return FLEX_ERR_INVALID;
    if (!attention::scale_ok(scale)) return FLEX_ERR_INVALID;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || !dP || !dGradOut || !dWork || dWork == dP) return FLEX_ERR_INVALID;
    if (p->k > 4 * 64 * kAtMaxSlabs) return FLEX_ERR_UNSUPPORTED;
    if (!dGradQ && !dGradK && !dGradV) return FLEX_OK;
    // the forward's rule over every row operand of the two launches (a NULL output is aligned)
    AttentionPick pick = attention_pick(p->k, p->ldb, p->ldc, dQ, dK, dV, dGradOut);
    pick.vec4 = pick.vec4 && attention_pick(p->k, p->ldb, p->ldc, dGradQ, dGradK, dGradV, nullptr).vec4;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dGradQ || dGradK) {
        if (const int rc = attention::launch_rows_backward(p, pick, dK, dV, dP, dGradOut, scale, dGradQ, dWork, s)) return rc;
    }
    if (dGradK || dGradV) {
        if (const int rc = attention::launch_columns_backward(p, pick, dQ, dGradOut, dP, dWork, dGradK, dGradV, s)) return rc;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int flex_attention_heads(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, float scale, float *dOut, float *dP,
                         flex_stream_t stream) {
    if (!p || !p->at_ok || heads < 1) return FLEX_ERR_INVALID;
    if (heads == 1) return flex_attention(p, dQ, dK, dV, scale, dOut, dP, stream);  // the single-head kernels: they have a generic form
    return flex::attention::heads_forward<float>(false, p, heads, dQ, dK, dV, nullptr, scale, dOut, dP, stream);
}

int flex_attention_heads_backward(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                  const float *dGradOut, float scale, float *dGradQ, float *dGradK, float *dGradV, float *dWork, flex_stream_t stream) {
    if (!p || !p->ab_ok || heads < 1) return FLEX_ERR_INVALID;
    if (heads == 1) return flex_attention_backward(p, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dWork, stream);
    return flex::attention::heads_backward<float>(false, p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, nullptr, dWork, stream);
}

int flex_attention_bf16(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, float scale, flex_bf16 *dOut,
                        float *dP, flex_stream_t stream) {
    return flex::attention::heads_forward<flex_bf16>(false, p, heads, dQ, dK, dV, nullptr, scale, dOut, dP, stream);
}

int flex_attention_bf16_backward(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dP,
                                 const flex_bf16 *dGradOut, float scale, flex_bf16 *dGradQ, flex_bf16 *dGradK, flex_bf16 *dGradV, float *dWork,
                                 flex_stream_t stream) {
    return flex::attention::heads_backward<flex_bf16>(false, p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, nullptr, dWork, stream);
}

int flex_attention_bias(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dBias, float scale, float *dOut,
                        float *dP, flex_stream_t stream) {
    return flex::attention::heads_forward<float>(true, p, heads, dQ, dK, dV, dBias, scale, dOut, dP, stream);
}

int flex_attention_bias_backward(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                 const float *dGradOut, float scale, float *dGradQ, float *dGradK, float *dGradV, float *dGradBias, float *dWork,
                                 flex_stream_t stream) {
    return flex::attention::heads_backward<float>(true, p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dGradBias, dWork, stream);
}

int flex_attention_bf16_bias(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dBias,
                             float scale, flex_bf16 *dOut, float *dP, flex_stream_t stream) {
    return flex::attention::heads_forward<flex_bf16>(true, p, heads, dQ, dK, dV, dBias, scale, dOut, dP, stream);
}

int flex_attention_bf16_bias_backward(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dP,
                                      const flex_bf16 *dGradOut, float scale, flex_bf16 *dGradQ, flex_bf16 *dGradK, flex_bf16 *dGradV,
                                      float *dGradBias, float *dWork, flex_stream_t stream) {
    return flex::attention::heads_backward<flex_bf16>(true, p, heads, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dGradBias, dWork, stream);
}

int flex_gat_attention(const flex_plan *p, int heads, const float *dEl, const float *dEr, const float *dV, float slope, float *dOut, float *dP,
                       flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->at_ok || heads < 1 || !attention::slope_ok(slope)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dEl || !dEr || !dV || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = attention_pick(p->k, p->ldb, p->ldc, dV, dOut, nullptr, nullptr);
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    if (const int rc = attention::launch_gat_rows(p, pick, heads, lg, dEl, dEr, dV, slope, dOut, dP, reinterpret_cast<hipStream_t>(stream))) return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int flex_gat_attention_backward(const flex_plan *p, int heads, const float *dEl, const float *dEr, const float *dV, const float *dP,
                                const float *dGradOut, float slope, float *dGradEl, float *dGradEr, float *dGradV, float *dWork, flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->ab_ok || heads < 1 || !attention::slope_ok(slope)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dEl || !dEr || !dV || !dP || !dGradOut || !dWork || dWork == dP) return FLEX_ERR_INVALID;
    // the forward's rule over every row operand of the two launches (a NULL output is aligned)
    const AttentionPick pick = attention_pick(p->k, p->ldb, p->ldc, dV, dGradOut, dGradV, nullptr);
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradEl && !dGradEr && !dGradV) return FLEX_OK;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dGradEl || dGradEr) {
        if (const int rc = attention::launch_gat_rows_backward(p, pick, heads, lg, dEl, dEr, dV, dP, dGradOut, slope, dGradEl, dWork, s)) return rc;
    }
    if (dGradEr || dGradV) {
        if (const int rc = attention::launch_gat_columns_backward(p, pick, heads, lg, dGradOut, dP, dWork, dGradEr, dGradV, s)) return rc;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // extern "C"
