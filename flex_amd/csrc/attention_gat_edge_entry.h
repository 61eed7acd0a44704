// attention_gat_edge_entry.h -- the two entry points of the fused GAT attention with a per-edge score term (include/flex_spmm.h:
// flex_edge_gat_attention, flex_edge_gat_attention_backward): the argument checks, the pick of the (W, NS) form and which launch happens
// for which outputs.  Host code only, and ordinary (non-inline) definitions, as attention_gatv2_dropout_entry.h: this file is included
// by exactly ONE translation unit per build -- attention_gat_edge_kernels.hip in the GPU library, tests/hostsim_gat_edge/launchers.cpp
// in the host-simulator build of tests/test_gat_edge_entry_host.py -- on row launchers of their own (flex::gat_edge::launch_*, declared
// here).  The column launch is the GAT family's (internal.h: launch_gat_columns_backward, launch_gat_dropout_columns_backward): that
// kernel reads P, dx and g alone, and never sees the edge term.
//
// Every refusal is gat_forward's / gat_backward's of attention_entry.h, code for code and in their order: dEe joins the required
// operands, drop_p is checked beside the slope.  One pair serves both modes: drop_p == 0 launches the DROP-off kernels after the
// refusals.  The backward's work array is dGradEe when it is given, else dWork; on return it holds dx, which is gEe.
#pragma once
#include <cmath>
#include <cstdint>

#include "internal.h"
#include "plan.h"

namespace flex {
namespace gat_edge {

// dm NULL: no dropout
int launch_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *Ee, const float *V,
                float slope, const DropMask *dm, float *Out, float *P, hipStream_t s);
int launch_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *Ee,
                         const float *V, const float *P, const float *G, float slope, const DropMask *dm, float *GEl, float *Work, hipStream_t s);

static bool slope_ok(float slope) { return std::isfinite(slope) && slope > 0.f && slope <= 1.f; }

}  // namespace gat_edge
}  // namespace flex

extern "C" {

int flex_edge_gat_attention(const flex_plan *p, int heads, const float *dEl, const float *dEr, const float *dEe, const float *dV, float slope,
                            float drop_p, uint64_t seed, float *dOut, float *dP, flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->at_ok || heads < 1 || !gat_edge::slope_ok(slope) || !drop_p_ok(drop_p)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dEl || !dEr || !dEe || !dV || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<float>(p->k, p->ldb, p->ldc, {dV, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const bool masked = drop_p != 0.f;
    const DropMask dm = masked ? drop_mask(drop_p, seed) : DropMask{};
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = gat_edge::launch_rows(p, pick, heads, lg, dEl, dEr, dEe, dV, slope, masked ? &dm : nullptr, dOut, dP, s)) return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int flex_edge_gat_attention_backward(const flex_plan *p, int heads, const float *dEl, const float *dEr, const float *dEe, const float *dV,
                                     const float *dP, const float *dGradOut, float slope, float drop_p, uint64_t seed, float *dGradEl, float *dGradEr,
                                     float *dGradEe, float *dGradV, float *dWork, flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->ab_ok || heads < 1 || !gat_edge::slope_ok(slope) || !drop_p_ok(drop_p)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    float *work = dGradEe ? dGradEe : dWork;  // dx: gEe itself where it is wanted
    if (!dEl || !dEr || !dEe || !dV || !dP || !dGradOut || !work || work == dP) return FLEX_ERR_INVALID;
    // the forward's rule over every row operand of the two launches (a NULL output is aligned)
    const AttentionPick pick = pick_rows<float>(p->k, p->ldb, p->ldc, {dV, dGradOut, dGradV});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradEl && !dGradEr && !dGradEe && !dGradV) return FLEX_OK;
    const bool masked = drop_p != 0.f;
    const DropMask dm = masked ? drop_mask(drop_p, seed) : DropMask{};
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dGradEl || dGradEr || dGradEe) {
        if (const int rc = gat_edge::launch_rows_backward(p, pick, heads, lg, dEl, dEr, dEe, dV, dP, dGradOut, slope, masked ? &dm : nullptr, dGradEl,
                                                          work, s))
            return rc;
    }
    if (dGradEr || dGradV) {
        if (const int rc = masked ? attention::launch_gat_dropout_columns_backward(p, pick, heads, lg, dGradOut, dP, work, dm, dGradEr, dGradV, s)
                                  : attention::launch_gat_columns_backward(p, pick, heads, lg, dGradOut, dP, work, dGradEr, dGradV, s))
            return rc;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // extern "C"
