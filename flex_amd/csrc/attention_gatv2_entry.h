// attention_gatv2_entry.h -- the three entry points of the fused GATv2 attention (include/flex_spmm.h: flex_gatv2_attention,
// flex_gatv2_attention_backward, flex_gatv2_attention_work_size): the argument checks, the pick of the (W, NS) form and which launch
// happens for which outputs.  Host code only, and ordinary (non-inline) definitions, as attention_entry.h: this file is included by
// exactly ONE translation unit per build -- attention_gatv2_kernels.hip in the GPU library, tests/hostsim_gatv2/launchers.cpp in the
// host-simulator build of tests/test_gatv2_entry_host.py -- so both builds run the same entry points on launchers of their own
// (flex::gatv2::launch_*, declared in attention_gatv2_common.h: the view, the grid and the kernel in the library, a stand-in that logs the instantiation's
// name in the simulator).
//
// The order of refusals is the GAT calls' (attention_entry.h): plan, flag, heads and slope; head split; empty plan (OK); NULL operands
// and dWork == dP; alignment; no output wanted (OK).  The backward launches the rows whenever a gradient is wanted (each needs dz), the
// columns for gXs alone and the reduction for gAtt alone.
#pragma once
#include "attention_gatv2_common.h"

extern "C" {

int flex_gatv2_attention(const flex_plan *p, int heads, const float *dXt, const float *dXs, const float *dAtt, float slope, float *dOut, float *dP,
                         flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->at_ok || heads < 1 || !gatv2::slope_ok(slope)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dXt || !dXs || !dAtt || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<float>(p->k, p->ldb, p->ldc, {dXt, dXs, dAtt, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    if (const int rc = gatv2::launch_rows(p, pick, heads, lg, dXt, dXs, dAtt, slope, dOut, dP, reinterpret_cast<hipStream_t>(stream))) return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int flex_gatv2_attention_backward(const flex_plan *p, int heads, const float *dXt, const float *dXs, const float *dAtt, const float *dP,
                                  const float *dGradOut, float slope, float *dGradXt, float *dGradXs, float *dGradAtt, float *dWork, float *dAttWork,
                                  flex_stream_t stream) {
    using namespace flex;
    if (!p || !p->ab_ok || heads < 1 || !gatv2::slope_ok(slope)) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dXt || !dXs || !dAtt || !dP || !dGradOut || !dWork || dWork == dP || (dGradAtt && !dAttWork)) return FLEX_ERR_INVALID;
    // the forward's rule over every row operand of the launches (a NULL output is aligned); dAttWork holds k-rows that are stored whole
    const AttentionPick pick = pick_rows<float>(p->k, p->ldb, p->ldc, {dXt, dXs, dAtt, dGradOut, dGradXt, dGradXs, dGradAtt ? dAttWork : nullptr});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradXt && !dGradXs && !dGradAtt) return FLEX_OK;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (const int rc = gatv2::launch_rows_backward(p, pick, heads, lg, dXt, dXs, dAtt, dP, dGradOut, slope, dGradXt, dWork, dGradAtt ? dAttWork : nullptr, s))
        return rc;
    if (dGradXs) {
        if (const int rc = gatv2::launch_columns_backward(p, pick, heads, lg, dXt, dXs, dAtt, dGradOut, dP, dWork, slope, dGradXs, s)) return rc;
    }
    if (dGradAtt) {
        if (const int rc = gatv2::launch_att_reduce(p, dAttWork, dGradAtt, s)) return rc;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int flex_gatv2_attention_work_size(const flex_plan *p, uint64_t *floats) {
    using namespace flex;
    if (!p || !p->at_ok || !floats) return FLEX_ERR_INVALID;
    *floats = p->at_entries == 0 ? 0 : static_cast<uint64_t>(gatv2::att_work_rows(p)) * static_cast<uint64_t>(p->k);
    return FLEX_OK;
}

}  // extern "C"
