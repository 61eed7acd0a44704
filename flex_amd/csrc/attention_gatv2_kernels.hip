// attention_gatv2_kernels.hip -- the fused GATv2 attention (include/flex_spmm.h: flex_gatv2_attention, flex_gatv2_attention_backward,
// flex_gatv2_attention_work_size): the score s = a_h . LeakyReLU(Xt[r] + Xs[src]) per head, in ONE forward launch and up to THREE
// backward launches (rows: dz, gXt and the gAtt partials; columns: gXs; a small reduction: gAtt) on the plans of the multi-head fused
// attention.  tests/test_gpu_gatv2_attention.py covers it, and holds every kernel handle of namespace gatv2 to a case that launches it;
// tests/test_gpu_gatv2_walks.py runs it above the floor group budget, without the XCD remap, and holds gAtt by the rows of dAttWork.
//
// The walk is attention_heads_kernels.hip's (attention_device.h): the same view, items, groups, slot / wave / block ownership by
// place_of, W = sddmm_lanes(k) lanes per slot, four entries per pass, four columns per lane and slab, the XCD remap.  A head is
// HW = d / 4 whole lanes of one slab; HW is a launch argument (its log2), so there is one instantiation per (W, NS), and the template
// arguments are ints alone.  The sweeps are attention_gatv2_device.h's; the entry points are attention_gatv2_entry.h's, included at
// the end of this file and by no other file of the library.
//
// gAtt is a sum over every entry of the graph.  A lane of the row launch keeps its four columns per slab of it across all the rows its
// wave walks; the workgroup's slots and waves meet once, in a fixed order, and wave 0 stores one k-row per workgroup into dAttWork
// (row blockIdx.x; a workgroup whose waves have no group stores zeros).  gatt_reduce then sums the rows of a column in an order that
// depends on their count alone: wave w of a workgroup takes rows w, w + 4, ... in a chain, the four chains meet in LDS in wave order.
#include <cmath>
#include <cstdint>

#include "attention_gatv2_device.h"
#include "attention_gatv2_entry.h"

namespace flex {
namespace gatv2 {

// Grid: as attention_rows.
template <int W, int NS>
__global__ __launch_bounds__(256) void rows(attention::View v, attention::HeadSplit hs, const float *__restrict__ Xt, const float *__restrict__ Xs,
                                             const float *__restrict__ Att, float slope, float *__restrict__ Out, float *__restrict__ P) {
    using namespace attention;
    __shared__ HeadsShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        run_item<W, NS>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Xt, Xs, Att, slope, Out, P, lane, w, sh);
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
        run_item<W, NS>(v, hs, it, kind, Xt, Xs, Att, slope, Out, P, lane, w, sh);
    }
}

// Grid: as attention_rows.  AttWork NULL: gAtt is not wanted.  No wave leaves early: the workgroup meets in store_att_partial.
template <int W, int NS>
__global__ __launch_bounds__(256) void rows_backward(attention::View v, attention::HeadSplit hs, const float *__restrict__ Xt, const float *__restrict__ Xs,
                                                      const float *__restrict__ Att, const float *__restrict__ P, const float *__restrict__ G,
                                                      float slope, float *__restrict__ GXt, float *__restrict__ Work, float *__restrict__ AttWork) {
    using namespace attention;
    __shared__ HeadsRowShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const bool want_att = AttWork != nullptr;
    float4 ga[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) ga[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (blockIdx.x < v.n_block_rows) {
        run_row<W, NS>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Xt, Xs, Att, P, G, slope, GXt, want_att, Work, ga, lane, w, sh);
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
                run_row<W, NS>(v, hs, it, kind, Xt, Xs, Att, P, G, slope, GXt, want_att, Work, ga, lane, w, sh);
            }
        }
    }
    if (want_att) store_att_partial<W, NS>(ga, v.k, AttWork, lane, w, sh);
}

template <int W, int NS>
__global__ __launch_bounds__(256) void columns_backward(attention::ColumnView v, attention::HeadSplit hs, const float *__restrict__ Xt,
                                                         const float *__restrict__ Xs, const float *__restrict__ Att, const float *__restrict__ G,
                                                         const float *__restrict__ P, const float *__restrict__ DZ, float slope, float *__restrict__ GXs) {
    using namespace attention;
    __shared__ ColumnShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_cols) {
        run_column<W, NS>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Xt, Xs, Att, G, P, DZ, slope, GXs, lane, w, sh);
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
        run_column<W, NS>(v, hs, it, kind, Xt, Xs, Att, G, P, DZ, slope, GXs, lane, w, sh);
    }
}

// GAtt[c] = the sum of column c over the n_part rows of AttWork.  Grid: one workgroup of 256 threads per 64 columns.
__global__ __launch_bounds__(256) void gatt_reduce(const float *__restrict__ AttWork, uint32_t n_part, int k, float *__restrict__ GAtt) {
    __shared__ float sh[kWavesPerBlock][64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const int c = static_cast<int>(blockIdx.x * 64u + lane);
    float acc = 0.f;
    if (c < k) {
        for (uint32_t r = w; r < n_part; r += kWavesPerBlock) acc += AttWork[static_cast<size_t>(r) * static_cast<size_t>(k) + static_cast<size_t>(c)];
    }
    sh[w][lane] = acc;
    __syncthreads();
    if (w == 0 && c < k) {
        float tot = sh[0][lane];
#pragma unroll
        for (int i = 1; i < kWavesPerBlock; ++i) tot += sh[i][lane];
        GAtt[c] = tot;
    }
}

// ---- launches

int launch_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att, float slope,
                float *Out, float *P, hipStream_t s) {
    const attention::View v = attention::row_view(p);
    const attention::HeadSplit hs{heads, lg};
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    attention::dispatch(pick, [&](auto W, auto NS) { hipLaunchKernelGGL((rows<W(), NS()>), grid, block, 0, s, v, hs, Xt, Xs, Att, slope, Out, P); });
    return FLEX_OK;
}

int launch_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att,
                         const float *P, const float *G, float slope, float *GXt, float *Work, float *AttWork, hipStream_t s) {
    const attention::View v = attention::row_view(p);
    const attention::HeadSplit hs{heads, lg};
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    if (AttWork && grid.x != att_work_rows(p)) return FLEX_ERR_INVALID;  // the rows flex_gatv2_attention_work_size reported
    attention::dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((rows_backward<W(), NS()>), grid, block, 0, s, v, hs, Xt, Xs, Att, P, G, slope, GXt, Work, AttWork);
    });
    return FLEX_OK;
}

int launch_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Xt, const float *Xs, const float *Att,
                            const float *G, const float *P, const float *DZ, float slope, float *GXs, hipStream_t s) {
    const attention::ColumnView v = attention::column_view(p);
    const attention::HeadSplit hs{heads, lg};
    const dim3 grid = attention::launch_grid(v), block(64 * kWavesPerBlock);
    attention::dispatch(pick, [&](auto W, auto NS) {
        hipLaunchKernelGGL((columns_backward<W(), NS()>), grid, block, 0, s, v, hs, Xt, Xs, Att, G, P, DZ, slope, GXs);
    });
    return FLEX_OK;
}

int launch_att_reduce(const flex_plan *p, const float *AttWork, float *GAtt, hipStream_t s) {
    const dim3 grid((static_cast<uint32_t>(p->k) + 63u) / 64u), block(64 * kWavesPerBlock);
    hipLaunchKernelGGL(gatt_reduce, grid, block, 0, s, AttWork, att_work_rows(p), p->k, GAtt);
    return FLEX_OK;
}

}  // namespace gatv2
}  // namespace flex
