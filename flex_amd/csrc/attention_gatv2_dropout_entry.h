// attention_gatv2_dropout_entry.h -- the two entry points of the fused GATv2 attention with dropout after the softmax
// (include/flex_spmm.h: flex_dropout_gatv2_attention, flex_dropout_gatv2_attention_backward): the argument checks, the pick of the
// (W, NS) form and which launch happens for which outputs.  Host code only, and ordinary (non-inline) definitions, as
// attention_gatv2_entry.h: this file is included by exactly ONE translation unit per build -- attention_gatv2_dropout_kernels.hip in
// the GPU library, tests/hostsim_gatv2_dropout/launchers.cpp in the host-simulator build of tests/test_gatv2_dropout_entry_host.py --
// on launchers of their own (flex::gatv2_dropout::launch_*, declared here).
//
// Every refusal is the undropped call's, code for code and in its order; drop_p is checked beside the slope.  drop_p == 0 launches the
// undropped kernels (flex::gatv2::launch_*) after the refusals.  The reduction of gAtt is the undropped one either way.
#pragma once
#include "attention_gatv2_common.h"

namespace flex {
namespace gatv2_dropout {

int launch_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att, float slope,
                const DropMask &dm, float *Out, float *P, hipStream_t s);
int launch_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att,
                         const float *P, const float *G, float slope, const DropMask &dm, float *GXt, float *Work, float *AttWork, hipStream_t s);
int launch_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att,
                            const float *G, const float *P, const float *DZ, float slope, const DropMask &dm, float *GXs, hipStream_t s);

}  // namespace gatv2_dropout
}  // namespace flex

extern "C" {

int flex_dropout_gatv2_attention(const flex_plan *p, int heads, const float *dXt, const float *dXs, const float *dAtt, float slope, float drop_p,
                                 uint64_t seed, float *dOut, float *dP, flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->at_ok || heads < 1 || !gatv2::slope_ok(slope) || !drop_p_ok(drop_p)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dXt || !dXs || !dAtt || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<float>(p->k, p->ldb, p->ldc, {dXt, dXs, dAtt, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int rc = drop_p == 0.f ? gatv2::launch_rows(p, pick, heads, lg, dXt, dXs, dAtt, slope, dOut, dP, s)
                                 : gatv2_dropout::launch_rows(p, pick, heads, lg, dXt, dXs, dAtt, slope, drop_mask(drop_p, seed), dOut, dP, s);
    if (rc) return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int flex_dropout_gatv2_attention_backward(const flex_plan *p, int heads, const float *dXt, const float *dXs, const float *dAtt, const float *dP,
                                          const float *dGradOut, float slope, float drop_p, uint64_t seed, float *dGradXt, float *dGradXs,
                                          float *dGradAtt, float *dWork, float *dAttWork, flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->ab_ok || heads < 1 || !gatv2::slope_ok(slope) || !drop_p_ok(drop_p)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dXt || !dXs || !dAtt || !dP || !dGradOut || !dWork || dWork == dP || (dGradAtt && !dAttWork)) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<float>(p->k, p->ldb, p->ldc, {dXt, dXs, dAtt, dGradOut, dGradXt, dGradXs, dGradAtt ? dAttWork : nullptr});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradXt && !dGradXs && !dGradAtt) return FLEX_OK;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool masked = drop_p != 0.f;
    const DropMask dm = masked ? drop_mask(drop_p, seed) : DropMask{};
    float *aw = dGradAtt ? dAttWork : nullptr;
    if (const int rc = masked ? gatv2_dropout::launch_rows_backward(p, pick, heads, lg, dXt, dXs, dAtt, dP, dGradOut, slope, dm, dGradXt, dWork, aw, s)
                              : gatv2::launch_rows_backward(p, pick, heads, lg, dXt, dXs, dAtt, dP, dGradOut, slope, dGradXt, dWork, aw, s))
        return rc;
    if (dGradXs) {
        if (const int rc = masked ? gatv2_dropout::launch_columns_backward(p, pick, heads, lg, dXt, dXs, dAtt, dGradOut, dP, dWork, slope, dm, dGradXs, s)
                                  : gatv2::launch_columns_backward(p, pick, heads, lg, dXt, dXs, dAtt, dGradOut, dP, dWork, slope, dGradXs, s))
            return rc;
    }
    if (dGradAtt) {
        if (const int rc = gatv2::launch_att_reduce(p, dAttWork, dGradAtt, s)) return rc;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // extern "C"
