// attention_gatv2_dropout_kernels.hip -- the fused GATv2 attention with dropout of the probabilities after the softmax
// (include/flex_spmm.h: flex_dropout_gatv2_attention, flex_dropout_gatv2_attention_backward): Out = sum_e alpha_e w_e Xs[src e] with
// w_e = keep(seed, e H + h) ? 1 / (1 - p) : 0, in the one forward launch and the row and column launches of the undropped GATv2 calls,
// on the same plans and the same walk and grid.  tests/test_gpu_gatv2_dropout.py covers it, and tests/test_gatv2_dropout_host.py holds
// every instantiation to a case that launches it.
//
// The sweeps are attention_gatv2_device.h's under their compile-time DROP switch.  The mask is not stored: element (e, h) of the edge
// arrays is kept iff dropout_bits(seed, e H + h) < thr (internal.h, DropMask -- the definition flex_dropout_mask evaluates on the
// host), and a lane computes the bits of a pass from the entry index it already holds -- in the two row kernels packed into one
// register by a rolled loop (unrolled, the hashes cost a wave), in the column kernel where it uses them.  In GATv2 the gathered row Xs[c] is score
// operand and value, so a dropped entry is gathered all the same and stays in the softmax: the score, the maximum, the sum and P are
// the undropped kernels'.  The bit enters in three places only: the value term of Out (forward), da in sweep 1 of the row launch, and
// the p g term of gXs in the column launch -- there a dropped entry is selected out, and its g row is not gathered.  The score term of
// gXs, gXt and the gAtt partials carry the mask through dz alone.  gAtt's reduction is gatv2::gatt_reduce, through launch_att_reduce.
//
// This file holds the three kernels (namespace flex::gatv2_dropout: 7 forms x 3 = 21 instantiations), their launchers and, through
// attention_gatv2_dropout_entry.h, which no other file of the library includes, the two entry points.
#include <cmath>
#include <cstdint>

#include "attention_gatv2_device.h"
#include "attention_gatv2_dropout_entry.h"

namespace flex {
namespace gatv2_dropout {

// Grid: as gatv2::rows.
template <int W, int NS>
__global__ __launch_bounds__(256) void rows(attention::View v, attention::HeadSplit hs, const float *__restrict__ Xt, const float *__restrict__ Xs,
                                             const float *__restrict__ Att, float slope, DropMask dm, float *__restrict__ Out,
                                             float *__restrict__ P) {
    using namespace attention;
    __shared__ HeadsShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        gatv2::run_item<W, NS, true>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Xt, Xs, Att, slope, Out, P, lane, w, sh, dm);
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
        gatv2::run_item<W, NS, true>(v, hs, it, kind, Xt, Xs, Att, slope, Out, P, lane, w, sh, dm);
    }
}

// Grid: as gatv2::rows_backward.  AttWork NULL: gAtt is not wanted.  No wave leaves early: the workgroup meets in store_att_partial.
template <int W, int NS>
__global__ __launch_bounds__(256) void rows_backward(attention::View v, attention::HeadSplit hs, const float *__restrict__ Xt, const float *__restrict__ Xs,
                                                      const float *__restrict__ Att, const float *__restrict__ P, const float *__restrict__ G,
                                                      float slope, DropMask dm, float *__restrict__ GXt, float *__restrict__ Work,
                                                      float *__restrict__ AttWork) {
    using namespace attention;
    __shared__ HeadsRowShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const bool want_att = AttWork != nullptr;
    float4 ga[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) ga[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blockIdx.x < v.n_block_rows) {
        gatv2::run_row<W, NS, true>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Xt, Xs, Att, P, G, slope, GXt, want_att, Work, ga, lane, w, sh,
                                    dm);
    } else {
        uint32_t wg = blockIdx.x - v.n_block_rows;
        if (v.xcd_remap) {
            const uint32_t per = (gridDim.x - v.n_block_rows) / kXcds;
            wg = (wg % kXcds) * per + wg / kXcds;
        }
        const uint32_t grp = wg * kWavesPerBlock + w;
        if (grp < v.n_groups) {
            const uint32_t i1 = v.grp[grp + 1];
            for (uint32_t i = v.grp[grp]; i < i1; ++i) {
                const uint4 it = v.item[i];
                const int kind = (it.w > 1 || it.y <= kAtSlotRow) ? kSlotLine : kWaveLine;
                gatv2::run_row<W, NS, true>(v, hs, it, kind, Xt, Xs, Att, P, G, slope, GXt, want_att, Work, ga, lane, w, sh, dm);
            }
        }
    }
    if (want_att) gatv2::store_att_partial<W, NS>(ga, v.k, AttWork, lane, w, sh);
}

template <int W, int NS>
__global__ __launch_bounds__(256) void columns_backward(attention::ColumnView v, attention::HeadSplit hs, const float *__restrict__ Xt,
                                                         const float *__restrict__ Xs, const float *__restrict__ Att, const float *__restrict__ G,
                                                         const float *__restrict__ P, const float *__restrict__ DZ, float slope, DropMask dm,
                                                         float *__restrict__ GXs) {
    using namespace attention;
    __shared__ gatv2::ColumnShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_cols) {
        gatv2::run_column<W, NS, true>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Xt, Xs, Att, G, P, DZ, slope, GXs, lane, w, sh, dm);
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
        gatv2::run_column<W, NS, true>(v, hs, it, kind, Xt, Xs, Att, G, P, DZ, slope, GXs, lane, w, sh, dm);
    }
}

// ---- launches

int launch_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att, float slope,
                const DropMask &dm, float *Out, float *P, hipStream_t s) {
    const attention::View v = attention::row_view(p);
    const attention::HeadSplit hs{heads, lg};
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    attention::dispatch(pick, [&](auto W, auto NS) { hipLaunchKernelGGL((rows<W(), NS()>), grid, block, 0, s, v, hs, Xt, Xs, Att, slope, dm, Out, P); });
    return FLEX_OK;
}

int launch_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att,
                         const float *P, const float *G, float slope, const DropMask &dm, float *GXt, float *Work, float *AttWork, hipStream_t s) {
    const attention::View v = attention::row_view(p);
    const attention::HeadSplit hs{heads, lg};
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    if (AttWork && grid.x != gatv2::att_work_rows(p)) return FLEX_ERR_INVALID;  // the rows flex_gatv2_attention_work_size reported
    attention::dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((rows_backward<W(), NS()>), grid, block, 0, s, v, hs, Xt, Xs, Att, P, G, slope, dm, GXt, Work, AttWork);
    });
    return FLEX_OK;
}

int launch_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att,
                            const float *G, const float *P, const float *DZ, float slope, const DropMask &dm, float *GXs, hipStream_t s) {
    const attention::ColumnView v = attention::column_view(p);
    const attention::HeadSplit hs{heads, lg};
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    attention::dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((columns_backward<W(), NS()>), grid, block, 0, s, v, hs, Xt, Xs, Att, G, P, DZ, slope, dm, GXs);
    });
    return FLEX_OK;
}

}  // namespace gatv2_dropout
}  // namespace flex
