// attention_gat_kernels.hip -- the fused GAT attention (include/flex_spmm.h: flex_gat_attention, flex_gat_attention_backward): the
// additive score s = LeakyReLU(el[r] + er[src]) per head in place of the dot product <Q[r], K[src]>, in the ONE forward launch and the
// TWO backward launches of the multi-head fused attention, on the same plans.  tests/test_gpu_gat_attention.py covers it; its (k, H)
// table is tests/attention_forms.py's, and tests/test_attention_routes.py holds every instantiation to a case that launches it.
//
// The walk is attention_heads_kernels.hip's (attention_device.h): the same view, items, groups, slot / wave / block ownership by
// place_of, W = sddmm_lanes(k) lanes per slot, four entries per pass, four columns per lane and slab, the XCD remap, State<1> per lane
// and slab, merge, write_row, the mask and poison logic, ColumnView for the second backward launch.  A head is HW = d / 4 whole lanes
// of one slab; HW is a launch argument (its log2), so there is one instantiation per (W, NS).  The head split (HeadSplit, HeadLane,
// LaneHeads, head_total, merge_slots_heads, HeadsShared, sum_slot_scalars) is attention_device.h's, its rule internal.h's head_split_lg;
// namespace gat holds what is GAT's alone, and the entry points are attention_entry.h's.  What differs from the dot-product heads:
//   forward        no K gather and no reduction across lanes for a score: per row a lane loads el[r, head] once, per entry
//                  er[src, head] -- one float, the lanes of a head reading the same address, the H heads of an entry one contiguous run --
//                  together with the four V gathers of the pass; scale = 1
//   row backward   sweep 1 is the heads kernel's (da by head_total, delta by fma); sweep 2 gathers nothing: the owning lane recomputes
//                  x = el + er, writes dx = (x > 0 ? 1 : slope) p (da - delta) over da and adds it into a per-head scalar gEl
//   column backward one accumulator row (gV) and one scalar per head and lane (gEr: all lanes of a head hold the same bits)
// Edge arrays (dP, dWork) are entry-major, (entry e, head h) at e H + h, written and read back by the lane HeadLane::writes names.
// Fixed order everywhere, no atomics.  Only the 16-byte form is built (the host refuses the rest).
// The sweeps live in attention_gat_device.h, behind the compile-time DROP switch that attention_gat_dropout_kernels.hip turns on; the
// kernels here instantiate it off, which leaves them what they were.  The walk over the items stays in the kernel bodies of both files:
// behind a shared inline wrapper the SGPR spill counts of gat_rows_backward<64, 2> and <64, 4> moved (14 -> 15, 28 -> 24).
#include <cmath>
#include <cstdint>

#include "attention_gat_device.h"

namespace flex {
namespace attention {
namespace gat {

// Grid: as attention_rows.
template <int W, int NS>
__global__ __launch_bounds__(256) void gat_rows(View v, HeadSplit hs, const float *__restrict__ El, const float *__restrict__ Er, const float *__restrict__ V,
                                                 float slope, float *__restrict__ Out, float *__restrict__ P) {
    __shared__ HeadsShared<W, NS> sh;
    const DropMask dm{};  // not read with DROP off
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        run_item<W, NS, false>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, slope, dm, Out, P, lane, w, sh);
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
        run_item<W, NS, false>(v, hs, it, kind, El, Er, V, slope, dm, Out, P, lane, w, sh);
    }
}

template <int W, int NS>
__global__ __launch_bounds__(256) void gat_rows_backward(View v, HeadSplit hs, const float *__restrict__ El, const float *__restrict__ Er,
                                                          const float *__restrict__ V, const float *__restrict__ P, const float *__restrict__ G,
                                                          float slope, float *__restrict__ GEl, float *__restrict__ Work) {
    __shared__ RowShared<W, NS> sh;
    const DropMask dm{};
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        run_row<W, NS, false>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, P, G, slope, dm, GEl, Work, lane, w, sh);
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
        run_row<W, NS, false>(v, hs, it, kind, El, Er, V, P, G, slope, dm, GEl, Work, lane, w, sh);
    }
}

template <int W, int NS>
__global__ __launch_bounds__(256) void gat_columns_backward(ColumnView v, HeadSplit hs, const float *__restrict__ G, const float *__restrict__ P,
                                                             const float *__restrict__ DX, float *__restrict__ GEr, float *__restrict__ GV) {
    __shared__ ColumnShared<W, NS> sh;
    const DropMask dm{};
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_cols) {
        run_column<W, NS, false>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, G, P, DX, dm, GEr, GV, lane, w, sh);
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
        run_column<W, NS, false>(v, hs, it, kind, G, P, DX, dm, GEr, GV, lane, w, sh);
    }
}

}  // namespace gat

// ---- launches

int launch_gat_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *V, float slope,
                    float *Out, float *P, hipStream_t s) {
    const View v = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 grid = launch_grid(v), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) { hipLaunchKernelGGL((gat::gat_rows<W(), NS()>), grid, block, 0, s, v, hs, El, Er, V, slope, Out, P); });
    return FLEX_OK;
}

int launch_gat_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *V,
                             const float *P, const float *G, float slope, float *GEl, float *Work, hipStream_t s) {
    const View rv = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 rgrid = launch_grid(rv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((gat::gat_rows_backward<W(), NS()>), rgrid, block, 0, s, rv, hs, El, Er, V, P, G, slope, GEl, Work);
    });
    return FLEX_OK;
}

int launch_gat_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *G, const float *P, const float *DX,
                                float *GEr, float *GV, hipStream_t s) {
    const ColumnView cv = column_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 cgrid = launch_grid(cv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) { hipLaunchKernelGGL((gat::gat_columns_backward<W(), NS()>), cgrid, block, 0, s, cv, hs, G, P, DX, GEr, GV); });
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex
