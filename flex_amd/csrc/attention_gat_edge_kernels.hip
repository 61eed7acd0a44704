// attention_gat_edge_kernels.hip -- the fused GAT attention with a per-edge term inside the LeakyReLU (include/flex_spmm.h:
// flex_edge_gat_attention, flex_edge_gat_attention_backward): x = (el[r] + er[src e]) + ee[e] per head, the score of the edge-feature GAT
// (alpha_dst + alpha_src + alpha_edge), with and without dropout of the probabilities, in the one forward launch and the row launch of
// the backward of the GAT calls, on the same plans, walk and grid.  tests/test_gpu_gat_edge.py covers it, and tests/test_gat_edge_host.py
// holds every instantiation to a case that launches it.
// tests/test_gpu_gat_edge_walks.py runs both kernels' own loop over a group's items, class pick and remap above the floor group budget.
//
// The sweeps are attention_gat_device.h's under their compile-time EDGE switch, with DROP off and on: the forward loads ee[e, head]
// with the pass's er loads and V gathers (the lanes of a head share the address; a dropped entry's term is read all the same, it stays
// in the softmax), sweep 2 of the row backward forms the same x from the same two additions, and the dx it writes is gEe: the caller's
// work array is the gradient.  The column launch has no edge form: it reads P, dx and g alone, and the entry points launch the GAT
// family's column kernels.
//
// This file holds the two kernels (namespace flex::gat_edge: 7 forms x 2 x DROP off / on = 28 instantiations), their launchers and,
// through attention_gat_edge_entry.h, which no other file of the library includes, the two entry points.
#include <cmath>
#include <cstdint>

#include "attention_gat_device.h"
#include "attention_gat_edge_entry.h"

namespace flex {
namespace gat_edge {

// Grid: as attention::gat::gat_rows.
template <int W, int NS, bool DROP>
__global__ __launch_bounds__(256) void gat_edge_rows(attention::View v, attention::HeadSplit hs, const float *__restrict__ El,
                                                      const float *__restrict__ Er, const float *__restrict__ Ee, const float *__restrict__ V,
                                                      float slope, DropMask dm, float *__restrict__ Out, float *__restrict__ P) {
    using namespace attention;
    __shared__ HeadsShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        gat::run_item<W, NS, DROP, true>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, slope, dm, Out, P, lane, w, sh, Ee);
        return;
    }
    uint32_t wg = blockIdx.x - v.n_block_rows;
    if (v.xcd_remap) {
        const uint32_t per = (gridDim.x - v.n_block_rows) / kXcds;
        wg = (wg % kXcds) * per + wg / kXcds;
    }
    const uint32_t grp = wg * kWavesPerBlock + w;
    if (grp >= v.n_groups) return;
    const uint32_t i1 = v.grp[grp + 1];
    for (uint32_t i = v.grp[grp]; i < i1; ++i) {
        const uint4 it = v.item[i];
        const int kind = (it.w > 1 || it.y <= kAtSlotRow) ? kSlotLine : kWaveLine;  // internal.h, attention_row_class
        gat::run_item<W, NS, DROP, true>(v, hs, it, kind, El, Er, V, slope, dm, Out, P, lane, w, sh, Ee);
    }
}

// Grid: as attention::gat::gat_rows_backward.  Work receives da in sweep 1 and dx = gEe in sweep 2.
template <int W, int NS, bool DROP>
__global__ __launch_bounds__(256) void gat_edge_rows_backward(attention::View v, attention::HeadSplit hs, const float *__restrict__ El,
                                                               const float *__restrict__ Er, const float *__restrict__ Ee,
                                                               const float *__restrict__ V, const float *__restrict__ P, const float *__restrict__ G,
                                                               float slope, DropMask dm, float *__restrict__ GEl, float *__restrict__ Work) {
    using namespace attention;
    __shared__ gat::RowShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        gat::run_row<W, NS, DROP, true>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, P, G, slope, dm, GEl, Work, lane, w, sh, Ee);
        return;
    }
    uint32_t wg = blockIdx.x - v.n_block_rows;
    if (v.xcd_remap) {
        const uint32_t per = (gridDim.x - v.n_block_rows) / kXcds;
        wg = (wg % kXcds) * per + wg / kXcds;
    }
    const uint32_t grp = wg * kWavesPerBlock + w;
    if (grp >= v.n_groups) return;
    const uint32_t i1 = v.grp[grp + 1];
    for (uint32_t i = v.grp[grp]; i < i1; ++i) {
        const uint4 it = v.item[i];
        const int kind = (it.w > 1 || it.y <= kAtSlotRow) ? kSlotLine : kWaveLine;
        gat::run_row<W, NS, DROP, true>(v, hs, it, kind, El, Er, V, P, G, slope, dm, GEl, Work, lane, w, sh, Ee);
    }
}

// ---- launches

int launch_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *Ee, const float *V,
                float slope, const DropMask *dm, float *Out, float *P, hipStream_t s) {
    const attention::View v = attention::row_view(p);
    const attention::HeadSplit hs{heads, lg};
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    attention::dispatch(pick, [&](auto W, auto NS) {
        if (dm)
            hipLaunchKernelGGL((gat_edge_rows<W(), NS(), true>), grid, block, 0, s, v, hs, El, Er, Ee, V, slope, *dm, Out, P);
        else
            hipLaunchKernelGGL((gat_edge_rows<W(), NS(), false>), grid, block, 0, s, v, hs, El, Er, Ee, V, slope, DropMask{}, Out, P);
    });
    return FLEX_OK;
}

int launch_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *Ee,
                         const float *V, const float *P, const float *G, float slope, const DropMask *dm, float *GEl, float *Work, hipStream_t s) {
    const attention::View v = attention::row_view(p);
    const attention::HeadSplit hs{heads, lg};
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    attention::dispatch(pick, [&](auto W, auto NS) {
        if (dm)
            hipLaunchKernelGGL((gat_edge_rows_backward<W(), NS(), true>), grid, block, 0, s, v, hs, El, Er, Ee, V, P, G, slope, *dm, GEl, Work);
        else
            hipLaunchKernelGGL((gat_edge_rows_backward<W(), NS(), false>), grid, block, 0, s, v, hs, El, Er, Ee, V, P, G, slope, DropMask{}, GEl, Work);
    });
    return FLEX_OK;
}

}  // namespace gat_edge
}  // namespace flex
