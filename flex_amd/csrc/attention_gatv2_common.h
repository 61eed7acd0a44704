// attention_gatv2_common.h -- what the two GATv2 entry headers share on the host: the launchers of the undropped kernels
// (attention_gatv2_kernels.hip, or a simulator's stand-ins), the slope rule and the row count of dAttWork.  attention_gatv2_entry.h
// (flex_gatv2_attention*) and attention_gatv2_dropout_entry.h (flex_dropout_gatv2_attention*) include it; it defines no entry point
// and references no launcher, so a simulator that defines the four launchers below alone still links against the former.
#pragma once
#include <cmath>
#include <cstdint>

#include "internal.h"
#include "plan.h"

namespace flex {
namespace gatv2 {

int launch_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att, float slope,
                float *Out, float *P, hipStream_t s);
// AttWork NULL: no gAtt partials; GXt NULL: no gXt; dz is written over da in Work either way
int launch_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att,
                         const float *P, const float *G, float slope, float *GXt, float *Work, float *AttWork, hipStream_t s);
int launch_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att,
                            const float *G, const float *P, const float *DZ, float slope, float *GXs, hipStream_t s);
int launch_att_reduce(const flex_plan *p, const float *AttWork, float *GAtt, hipStream_t s);

inline bool slope_ok(float slope) { return std::isfinite(slope) && slope > 0.f && slope <= 1.f; }

// The k-rows of dAttWork: one per workgroup of the row launch, which is attention_host.h's launch_grid of the row walk -- one
// workgroup per block row, then one per kWavesPerBlock groups, under the remap a multiple of kXcds of the latter.
inline uint32_t att_work_rows(const flex_plan *p) {
    uint32_t wgs = (p->n_at_groups + kWavesPerBlock - 1) / kWavesPerBlock;
    if (p->xcd_remap) wgs = (wgs + kXcds - 1) / kXcds * kXcds;
    return p->n_at_block_rows + wgs;
}

}  // namespace gatv2
}  // namespace flex
