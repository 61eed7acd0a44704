// attention_entry.h -- all 22 entry points of the fused attention (include/flex_spmm.h): the argument checks, the pick of the
// (W, NS) form and which launch happens for which outputs.  Host code only, and ordinary (non-inline) definitions: this file is included
// by exactly ONE translation unit per build -- attention_kernels.hip in the GPU library, tests/hostsim/shim.cpp in the host simulator --
// so both builds run the same entry points, as both run plan.cpp's flex_spmm.  What differs between them is the launchers alone
// (internal.h, flex::attention::launch_*): in the library the view, the grid and the kernel of the attention_*_kernels.hip files, in the
// simulator a stand-in that logs the instantiation's name.  An entry point decides which launchers run, holds the plan's device around
// them and returns the first launcher code that is not FLEX_OK.
//
// The single-head pair, the GAT family and the per-head family each keep their own order of refusals: the single-head pair runs the
// generic form on misaligned operands and looks at the outputs before the pick; the per-head family (heads, bf16, the two bias forms
// and the four dropout calls: one template pair over the element type, with a bias flag and a drop flag) refuses misaligned operands,
// and does so before "no output wanted".  Per-head: plan, flag and heads; scale and drop_p; head split; empty plan (OK); NULL operands
// and dWork == dP; the gBias aliases; alignment; no output wanted (OK).  GAT (six calls, one template pair over the element type of the V
// rows, with a drop flag): the slope and drop_p stand in the first check, beside the plan and the heads; the rest is the per-head order.
// drop_p == 0 is no refusal: it launches the undropped kernels of the same operands, after every check.
// The GATv2 calls (flex_gatv2_attention, flex_gatv2_attention_backward, flex_gatv2_attention_work_size) are not among the 22: their entry
// points live in attention_gatv2_entry.h, which attention_gatv2_kernels.hip alone includes, on launchers of namespace flex::gatv2.
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "internal.h"
#include "plan.h"

namespace flex {
namespace attention {

static bool scale_ok(float scale) { return std::isfinite(scale) && scale > 0.f; }
static bool slope_ok(float slope) { return std::isfinite(slope) && slope > 0.f && slope <= 1.f; }

// flex_attention_heads (heads > 1), flex_attention_bf16, with `bias` flex_attention_bias and flex_attention_bf16_bias, and with `drop` the
// two dropout calls, whose bias is optional: their `bias` says whether dBias is there.  heads = 1 runs here as well: d = k is then a
// power of two.  drop_p == 0 launches what the undropped call launches on the same operands, once nothing is refused.
template <class E>
static int heads_forward(bool bias, bool drop, const flex_plan *p, int heads, const E *dQ, const E *dK, const E *dV, const float *dBias, float scale,
                         float drop_p, uint64_t seed, E *dOut, float *dP, flex_stream_t stream) {
    if (!p || !p->at_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!scale_ok(scale) || (drop && !drop_p_ok(drop_p))) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dQ || !dK || !dV || (bias && !dBias) || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<E>(p->k, p->ldb, p->ldc, {dQ, dK, dV, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const auto rows = [&]() -> int {
        if (drop && drop_p != 0.f) return launch_dropout_rows(p, pick, heads, lg, dQ, dK, dV, dBias, scale, drop_mask(drop_p, seed), dOut, dP, s);
        if (bias) return launch_bias_rows(p, pick, heads, lg, dQ, dK, dV, dBias, scale, dOut, dP, s);
        if constexpr (std::is_same_v<E, float>)  // drop_p == 0: what flex_attention_heads runs for one head, in the 16-byte form
            if (drop && heads == 1) return launch_rows(p, pick, dQ, dK, dV, scale, dOut, dP, s);
        return launch_heads_rows(p, pick, heads, lg, dQ, dK, dV, scale, dOut, dP, s);
    };
    if (const int rc = rows()) return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

// the backward of the same; dGradBias is NULL without `bias`, and optional with `drop`.  The undropped column launch does not see the bias.
template <class E>
static int heads_backward(bool bias, bool drop, const flex_plan *p, int heads, const E *dQ, const E *dK, const E *dV, const float *dP, const E *dGradOut,
                          float scale, float drop_p, uint64_t seed, E *dGradQ, E *dGradK, E *dGradV, float *dGradBias, float *dWork,
                          flex_stream_t stream) {
    if (!p || !p->ab_ok || heads < 1) return FLEX_ERR_INVALID;
    if (!scale_ok(scale) || (drop && !drop_p_ok(drop_p))) return FLEX_ERR_INVALID;
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
    const bool masked = drop && drop_p != 0.f;
    const DropMask dm = masked ? drop_mask(drop_p, seed) : DropMask{};
    const auto rows = [&]() -> int {
        if (masked) return launch_dropout_rows_backward(p, pick, heads, lg, dK, dV, dP, dGradOut, scale, dm, dGradQ, dGradBias, dWork, s);
        if (bias) return launch_bias_rows_backward(p, pick, heads, lg, dK, dV, dP, dGradOut, scale, dGradQ, dGradBias, dWork, s);
        if constexpr (std::is_same_v<E, float>)  // as in heads_forward
            if (drop && heads == 1) return launch_rows_backward(p, pick, dK, dV, dP, dGradOut, scale, dGradQ, dWork, s);
        return launch_heads_rows_backward(p, pick, heads, lg, dK, dV, dP, dGradOut, scale, dGradQ, dWork, s);
    };
    const auto columns = [&]() -> int {
        if (masked) return launch_dropout_columns_backward(p, pick, heads, lg, dQ, dGradOut, dP, dWork, dm, dGradK, dGradV, s);
        if constexpr (std::is_same_v<E, float>)
            if (drop && !bias && heads == 1) return launch_columns_backward(p, pick, dQ, dGradOut, dP, dWork, dGradK, dGradV, s);
        return launch_heads_columns_backward(p, pick, heads, lg, dQ, dGradOut, dP, dWork, dGradK, dGradV, s);
    };
    if (dGradQ || dGradK || dGradBias) {
        if (const int rc = rows()) return rc;
    }
    if (dGradK || dGradV) {
        if (const int rc = columns()) return rc;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

// The six GAT calls, E the element type of the V, Out, g and gV rows (el, er, their gradients, dP and dWork are floats); `drop`: the
// call has drop_p and seed.  On float rows pick_rows is attention_pick over the same operands (internal.h).
template <class E>
static int gat_forward(bool drop, const flex_plan *p, int heads, const float *dEl, const float *dEr, const E *dV, float slope, float drop_p,
                       uint64_t seed, E *dOut, float *dP, flex_stream_t stream) {
    if (!p || !p->at_ok || heads < 1 || !slope_ok(slope) || (drop && !drop_p_ok(drop_p))) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dEl || !dEr || !dV || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<E>(p->k, p->ldb, p->ldc, {dV, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const bool masked = drop && drop_p != 0.f;
    const DropMask dm = masked ? drop_mask(drop_p, seed) : DropMask{};
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const auto rows = [&]() -> int {
        if constexpr (std::is_same_v<E, float>)
            return masked ? launch_gat_dropout_rows(p, pick, heads, lg, dEl, dEr, dV, slope, dm, dOut, dP, s)
                          : launch_gat_rows(p, pick, heads, lg, dEl, dEr, dV, slope, dOut, dP, s);
        else
            return launch_gat_bf16_rows(p, pick, heads, lg, dEl, dEr, dV, slope, masked ? &dm : nullptr, dOut, dP, s);
    };
    if (const int rc = rows()) return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

template <class E>
static int gat_backward(bool drop, const flex_plan *p, int heads, const float *dEl, const float *dEr, const E *dV, const float *dP, const E *dGradOut,
                        float slope, float drop_p, uint64_t seed, float *dGradEl, float *dGradEr, E *dGradV, float *dWork, flex_stream_t stream) {
    if (!p || !p->ab_ok || heads < 1 || !slope_ok(slope) || (drop && !drop_p_ok(drop_p))) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dEl || !dEr || !dV || !dP || !dGradOut || !dWork || dWork == dP) return FLEX_ERR_INVALID;
    // the forward's rule over every row operand of the two launches (a NULL output is aligned)
    const AttentionPick pick = pick_rows<E>(p->k, p->ldb, p->ldc, {dV, dGradOut, dGradV});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradEl && !dGradEr && !dGradV) return FLEX_OK;
    const bool masked = drop && drop_p != 0.f;
    const DropMask dm = masked ? drop_mask(drop_p, seed) : DropMask{};
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const auto rows = [&]() -> int {
        if constexpr (std::is_same_v<E, float>)
            return masked ? launch_gat_dropout_rows_backward(p, pick, heads, lg, dEl, dEr, dV, dP, dGradOut, slope, dm, dGradEl, dWork, s)
                          : launch_gat_rows_backward(p, pick, heads, lg, dEl, dEr, dV, dP, dGradOut, slope, dGradEl, dWork, s);
        else
            return launch_gat_bf16_rows_backward(p, pick, heads, lg, dEl, dEr, dV, dP, dGradOut, slope, masked ? &dm : nullptr, dGradEl, dWork, s);
    };
    const auto columns = [&]() -> int {
        if constexpr (std::is_same_v<E, float>)
            return masked ? launch_gat_dropout_columns_backward(p, pick, heads, lg, dGradOut, dP, dWork, dm, dGradEr, dGradV, s)
                          : launch_gat_columns_backward(p, pick, heads, lg, dGradOut, dP, dWork, dGradEr, dGradV, s);
        else
            return launch_gat_bf16_columns_backward(p, pick, heads, lg, dGradOut, dP, dWork, masked ? &dm : nullptr, dGradEr, dGradV, s);
    };
    if (dGradEl || dGradEr) {
        if (const int rc = rows()) return rc;
    }
    if (dGradEr || dGradV) {
        if (const int rc = columns()) return rc;
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
    return flex::attention::heads_forward<float>(false, false, p, heads, dQ, dK, dV, nullptr, scale, 0.f, 0, dOut, dP, stream);
}

int flex_attention_heads_backward(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                  const float *dGradOut, float scale, float *dGradQ, float *dGradK, float *dGradV, float *dWork, flex_stream_t stream) {
    if (!p || !p->ab_ok || heads < 1) return FLEX_ERR_INVALID;
    if (heads == 1) return flex_attention_backward(p, dQ, dK, dV, dP, dGradOut, scale, dGradQ, dGradK, dGradV, dWork, stream);
    return flex::attention::heads_backward<float>(false, false, p, heads, dQ, dK, dV, dP, dGradOut, scale, 0.f, 0, dGradQ, dGradK, dGradV, nullptr, dWork, stream);
}

int flex_attention_bf16(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, float scale, flex_bf16 *dOut,
                        float *dP, flex_stream_t stream) {
    return flex::attention::heads_forward<flex_bf16>(false, false, p, heads, dQ, dK, dV, nullptr, scale, 0.f, 0, dOut, dP, stream);
}

int flex_attention_bf16_backward(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dP,
                                 const flex_bf16 *dGradOut, float scale, flex_bf16 *dGradQ, flex_bf16 *dGradK, flex_bf16 *dGradV, float *dWork,
                                 flex_stream_t stream) {
    return flex::attention::heads_backward<flex_bf16>(false, false, p, heads, dQ, dK, dV, dP, dGradOut, scale, 0.f, 0, dGradQ, dGradK, dGradV, nullptr, dWork, stream);
}

int flex_attention_bias(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dBias, float scale, float *dOut,
                        float *dP, flex_stream_t stream) {
    return flex::attention::heads_forward<float>(true, false, p, heads, dQ, dK, dV, dBias, scale, 0.f, 0, dOut, dP, stream);
}

int flex_attention_bias_backward(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                 const float *dGradOut, float scale, float *dGradQ, float *dGradK, float *dGradV, float *dGradBias, float *dWork,
                                 flex_stream_t stream) {
    return flex::attention::heads_backward<float>(true, false, p, heads, dQ, dK, dV, dP, dGradOut, scale, 0.f, 0, dGradQ, dGradK, dGradV, dGradBias, dWork, stream);
}

int flex_attention_bf16_bias(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dBias,
                             float scale, flex_bf16 *dOut, float *dP, flex_stream_t stream) {
    return flex::attention::heads_forward<flex_bf16>(true, false, p, heads, dQ, dK, dV, dBias, scale, 0.f, 0, dOut, dP, stream);
}

int flex_attention_bf16_bias_backward(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dP,
                                      const flex_bf16 *dGradOut, float scale, flex_bf16 *dGradQ, flex_bf16 *dGradK, flex_bf16 *dGradV,
                                      float *dGradBias, float *dWork, flex_stream_t stream) {
    return flex::attention::heads_backward<flex_bf16>(true, false, p, heads, dQ, dK, dV, dP, dGradOut, scale, 0.f, 0, dGradQ, dGradK, dGradV, dGradBias, dWork, stream);
}

int flex_attention_dropout(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dBias, float scale, float drop_p,
                           uint64_t seed, float *dOut, float *dP, flex_stream_t stream) {
    return flex::attention::heads_forward<float>(dBias != nullptr, true, p, heads, dQ, dK, dV, dBias, scale, drop_p, seed, dOut, dP, stream);
}

int flex_attention_dropout_backward(const flex_plan *p, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                    const float *dGradOut, float scale, float drop_p, uint64_t seed, float *dGradQ, float *dGradK, float *dGradV,
                                    float *dGradBias, float *dWork, flex_stream_t stream) {
    return flex::attention::heads_backward<float>(dGradBias != nullptr, true, p, heads, dQ, dK, dV, dP, dGradOut, scale, drop_p, seed, dGradQ, dGradK,
                                                  dGradV, dGradBias, dWork, stream);
}

int flex_attention_bf16_dropout(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dBias,
                                float scale, float drop_p, uint64_t seed, flex_bf16 *dOut, float *dP, flex_stream_t stream) {
    return flex::attention::heads_forward<flex_bf16>(dBias != nullptr, true, p, heads, dQ, dK, dV, dBias, scale, drop_p, seed, dOut, dP, stream);
}

int flex_attention_bf16_dropout_backward(const flex_plan *p, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dP,
                                         const flex_bf16 *dGradOut, float scale, float drop_p, uint64_t seed, flex_bf16 *dGradQ, flex_bf16 *dGradK,
                                         flex_bf16 *dGradV, float *dGradBias, float *dWork, flex_stream_t stream) {
    return flex::attention::heads_backward<flex_bf16>(dGradBias != nullptr, true, p, heads, dQ, dK, dV, dP, dGradOut, scale, drop_p, seed, dGradQ,
                                                      dGradK, dGradV, dGradBias, dWork, stream);
}

int flex_gat_attention(const flex_plan *p, int heads, const float *dEl, const float *dEr, const float *dV, float slope, float *dOut, float *dP,
                       flex_stream_t stream) {
    return flex::attention::gat_forward<float>(false, p, heads, dEl, dEr, dV, slope, 0.f, 0, dOut, dP, stream);
}

int flex_gat_attention_backward(const flex_plan *p, int heads, const float *dEl, const float *dEr, const float *dV, const float *dP,
                                const float *dGradOut, float slope, float *dGradEl, float *dGradEr, float *dGradV, float *dWork, flex_stream_t stream) {
    return flex::attention::gat_backward<float>(false, p, heads, dEl, dEr, dV, dP, dGradOut, slope, 0.f, 0, dGradEl, dGradEr, dGradV, dWork, stream);
}

int flex_gat_attention_dropout(const flex_plan *p, int heads, const float *dEl, const float *dEr, const float *dV, float slope, float drop_p,
                               uint64_t seed, float *dOut, float *dP, flex_stream_t stream) {
    return flex::attention::gat_forward<float>(true, p, heads, dEl, dEr, dV, slope, drop_p, seed, dOut, dP, stream);
}

int flex_gat_attention_dropout_backward(const flex_plan *p, int heads, const float *dEl, const float *dEr, const float *dV, const float *dP,
                                        const float *dGradOut, float slope, float drop_p, uint64_t seed, float *dGradEl, float *dGradEr,
                                        float *dGradV, float *dWork, flex_stream_t stream) {
    return flex::attention::gat_backward<float>(true, p, heads, dEl, dEr, dV, dP, dGradOut, slope, drop_p, seed, dGradEl, dGradEr, dGradV, dWork, stream);
}

int flex_gat_attention_bf16(const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, float slope, flex_bf16 *dOut,
                            float *dP, flex_stream_t stream) {
    return flex::attention::gat_forward<flex_bf16>(false, p, heads, dEl, dEr, dV, slope, 0.f, 0, dOut, dP, stream);
}

int flex_gat_attention_bf16_backward(const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, const float *dP,
                                     const flex_bf16 *dGradOut, float slope, float *dGradEl, float *dGradEr, flex_bf16 *dGradV, float *dWork,
                                     flex_stream_t stream) {
    return flex::attention::gat_backward<flex_bf16>(false, p, heads, dEl, dEr, dV, dP, dGradOut, slope, 0.f, 0, dGradEl, dGradEr, dGradV, dWork, stream);
}

int flex_gat_attention_bf16_dropout(const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, float slope, float drop_p,
                                    uint64_t seed, flex_bf16 *dOut, float *dP, flex_stream_t stream) {
    return flex::attention::gat_forward<flex_bf16>(true, p, heads, dEl, dEr, dV, slope, drop_p, seed, dOut, dP, stream);
}

int flex_gat_attention_bf16_dropout_backward(const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, const float *dP,
                                             const flex_bf16 *dGradOut, float slope, float drop_p, uint64_t seed, float *dGradEl, float *dGradEr,
                                             flex_bf16 *dGradV, float *dWork, flex_stream_t stream) {
    return flex::attention::gat_backward<flex_bf16>(true, p, heads, dEl, dEr, dV, dP, dGradOut, slope, drop_p, seed, dGradEl, dGradEr, dGradV, dWork,
                                                    stream);
}

}  // extern "C"
