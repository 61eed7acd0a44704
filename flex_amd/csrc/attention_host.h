// attention_host.h -- what the launchers of the fused attention (internal.h, flex::attention::launch_*; one body each in the
// attention_*_kernels.hip files) share on the host: the two views of a plan, the launch grid of a walk and the one list of the (W, NS)
// forms that are built.  The entry points, their argument checks and the head split are host code of their own (attention_entry.h).
#pragma once
#include <type_traits>

#include "attention_device.h"
#include "plan.h"

namespace flex {
namespace attention {

inline View row_view(const flex_plan *p) {
    return View{p->d_at_rowptr.get(), p->d_at_src.get(), p->d_at_item.get(), p->d_at_grp.get(), p->at_first_entry,
                p->n_at_groups, p->n_at_wave_items, p->n_at_block_rows, p->xcd_remap ? 1u : 0u, p->k, p->ldb, p->ldc};
}

inline ColumnView column_view(const flex_plan *p) {
    return ColumnView{p->d_ab_colptr.get(), p->d_ab_ent.get(), p->d_ab_item.get(), p->d_ab_grp.get(),
                      p->n_ab_groups, p->n_ab_wave_items, p->n_ab_block_cols, p->xcd_remap ? 1u : 0u, p->k, p->ldb, p->ldc};
}

// one workgroup per block line, then one per kWavesPerBlock groups; under the remap a multiple of kXcds of the latter
inline dim3 launch_grid(uint32_t groups, uint32_t block_lines, uint32_t remap) {
    uint32_t wgs = (groups + kWavesPerBlock - 1) / kWavesPerBlock;
    if (remap) wgs = (wgs + kXcds - 1) / kXcds * kXcds;
    return dim3(block_lines + wgs);
}
inline dim3 launch_grid(const View &v) { return launch_grid(v.n_groups, v.n_block_rows, v.xcd_remap); }
inline dim3 launch_grid(const ColumnView &v) { return launch_grid(v.n_groups, v.n_block_cols, v.xcd_remap); }

// f(W, NS) as integral constants for the pick of attention_pick (internal.h): the seven forms every kernel here is built in
template <class F>
inline void dispatch(const AttentionPick &pick, F &&f) {
    using std::integral_constant;
    switch (pick.W * 8 + pick.NS) {
        case 4 * 8 + 1: f(integral_constant<int, 4>{}, integral_constant<int, 1>{}); break;
        case 8 * 8 + 1: f(integral_constant<int, 8>{}, integral_constant<int, 1>{}); break;
        case 16 * 8 + 1: f(integral_constant<int, 16>{}, integral_constant<int, 1>{}); break;
        case 32 * 8 + 1: f(integral_constant<int, 32>{}, integral_constant<int, 1>{}); break;
        case 64 * 8 + 1: f(integral_constant<int, 64>{}, integral_constant<int, 1>{}); break;
        case 64 * 8 + 2: f(integral_constant<int, 64>{}, integral_constant<int, 2>{}); break;
        default: f(integral_constant<int, 64>{}, integral_constant<int, 4>{}); break;
    }
}

}  // namespace attention
}  // namespace flex
