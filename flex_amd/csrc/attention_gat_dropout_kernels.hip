// attention_gat_dropout_kernels.hip -- the fused GAT attention with dropout of the probabilities after the softmax
// (include/flex_spmm.h: flex_gat_attention_dropout, flex_gat_attention_dropout_backward): Out = sum_e alpha_e w_e V[src e] with
// w_e = keep(seed, e H + h) ? 1 / (1 - p) : 0, in the one forward launch and the two backward launches of the undropped GAT calls, on
// the same plans.  tests/test_gpu_gat_dropout.py covers it, and tests/test_gat_dropout_host.py holds every instantiation to a case that
// launches it.
//
// The sweeps are attention_gat_device.h's under their compile-time DROP switch: the same walk (in the kernel bodies, as in
// attention_gat_kernels.hip), head split, slot placement, merges and LDS meeting places as the undropped kernels.  The mask is not stored: element (e, h) of the edge arrays is kept iff
// dropout_bits(seed, e H + h) < thr (internal.h, DropMask -- the definition flex_dropout_mask evaluates on the host), and every lane
// recomputes the bit of its head from the entry index it already holds, in all three launches.  The score x = el + er, the LeakyReLU,
// the maximum, the sum and P are the undropped kernels'; a kept entry enters Out, da and gV with the factor c, a dropped one is selected
// out and its V row (forward, row backward) or g row (gV) is not gathered.  The column launch needs the mask for gV alone: dx in dWork
// already holds it through da, and so do gEl and gEr.
//
// This file holds the three kernels (namespace flex::gat_dropout: 7 forms x 3 = 21 instantiations) and their launchers (internal.h,
// launch_gat_dropout_*); the entry points -- the GAT template pair on float rows with its drop flag set -- are attention_entry.h's.
#include <cmath>
#include <cstdint>

#include "attention_gat_device.h"

namespace flex {
namespace gat_dropout {

using namespace flex::attention;

template <int W, int NS>
__global__ __launch_bounds__(256) void gat_dropout_rows(View v, HeadSplit hs, const float *__restrict__ El, const float *__restrict__ Er,
                                                         const float *__restrict__ V, float slope, DropMask dm, float *__restrict__ Out,
                                                         float *__restrict__ P) {
    __shared__ HeadsShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        gat::run_item<W, NS, true>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, slope, dm, Out, P, lane, w, sh);
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
        gat::run_item<W, NS, true>(v, hs, it, kind, El, Er, V, slope, dm, Out, P, lane, w, sh);
    }
}

template <int W, int NS>
__global__ __launch_bounds__(256) void gat_dropout_rows_backward(View v, HeadSplit hs, const float *__restrict__ El, const float *__restrict__ Er,
                                                                  const float *__restrict__ V, const float *__restrict__ P,
                                                                  const float *__restrict__ G, float slope, DropMask dm, float *__restrict__ GEl,
                                                                  float *__restrict__ Work) {
    __shared__ gat::RowShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        gat::run_row<W, NS, true>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, P, G, slope, dm, GEl, Work, lane, w, sh);
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
        gat::run_row<W, NS, true>(v, hs, it, kind, El, Er, V, P, G, slope, dm, GEl, Work, lane, w, sh);
    }
}

template <int W, int NS>
__global__ __launch_bounds__(256) void gat_dropout_columns_backward(ColumnView v, HeadSplit hs, const float *__restrict__ G,
                                                                     const float *__restrict__ P, const float *__restrict__ DX, DropMask dm,
                                                                     float *__restrict__ GEr, float *__restrict__ GV) {
    __shared__ gat::ColumnShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_cols) {
        gat::run_column<W, NS, true>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, G, P, DX, dm, GEr, GV, lane, w, sh);
        return;
    }
    uint32_t wg = blockIdx.x - v.n_block_cols;
    if (v.xcd_remap) {
        const uint32_t per = (gridDim.x - v.n_block_cols) / kXcds;
        wg = (wg % kXcds) * per + wg / kXcds;
    }
    const uint32_t grp = wg * kWavesPerBlock + w;
    if (grp >= v.n_groups) return;
    const uint32_t i1 = v.grp[grp + 1];
    for (uint32_t i = v.grp[grp]; i < i1; ++i) {
        const uint4 it = v.item[i];
        const int kind = (it.w > 1 || it.y <= kAtSlotRow) ? kSlotLine : kWaveLine;
        gat::run_column<W, NS, true>(v, hs, it, kind, G, P, DX, dm, GEr, GV, lane, w, sh);
    }
}

}  // namespace gat_dropout

// ---- launches

namespace attention {

int launch_gat_dropout_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *V,
                            float slope, const DropMask &dm, float *Out, float *P, hipStream_t s) {
    const View v = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 grid = launch_grid(v), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((gat_dropout::gat_dropout_rows<W(), NS()>), grid, block, 0, s, v, hs, El, Er, V, slope, dm, Out, P);
    });
    return FLEX_OK;
}

int launch_gat_dropout_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er,
                                     const float *V, const float *P, const float *G, float slope, const DropMask &dm, float *GEl, float *Work,
                                     hipStream_t s) {
    const View rv = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 rgrid = launch_grid(rv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((gat_dropout::gat_dropout_rows_backward<W(), NS()>), rgrid, block, 0, s, rv, hs, El, Er, V, P, G, slope, dm, GEl, Work);
    });
    return FLEX_OK;
}

int launch_gat_dropout_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *G, const float *P,
                                        const float *DX, const DropMask &dm, float *GEr, float *GV, hipStream_t s) {
    const ColumnView cv = column_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 cgrid = launch_grid(cv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((gat_dropout::gat_dropout_columns_backward<W(), NS()>), cgrid, block, 0, s, cv, hs, G, P, DX, dm, GEr, GV);
    });
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex
