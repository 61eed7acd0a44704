// attention_gat_bf16_kernels.hip -- the fused GAT attention on bf16 V rows, with and without dropout of the probabilities after the
// softmax (include/flex_spmm.h: flex_gat_attention_bf16, flex_gat_attention_bf16_backward, flex_gat_attention_bf16_dropout,
// flex_gat_attention_bf16_dropout_backward): V, Out, g and gV are flex_bf16, half the bytes of the one row a nonzero gathers; el, er,
// gEl, gEr, dP and dWork stay fp32.  The one forward launch and the two backward launches of the fp32 GAT calls, on the same plans.
// tests/test_gpu_gat_bf16.py covers it, and tests/test_gat_bf16_host.py holds every instantiation to a case that launches it.
//
// The sweeps are attention_gat_device.h's under their deduced element type E = flex_bf16 and their compile-time DROP switch: the same
// walk (in the kernel bodies, as in attention_gat_kernels.hip), head split, slot placement, merges and LDS meeting places as the fp32
// kernels, and the same source expressions, so dP, dWork, gEl and gEr have the fp32 kernels' bits on the widened operands.  A row is
// reached through attention_device.h's load_cols / store_cols / write_row for flex_bf16 alone: one 8-byte load per lane and slab,
// widened by shifts (exact), every sum in fp32, and one rounding to nearest even at the single 8-byte store of an element of Out or gV.
// No 2-byte access, no atomics, fixed order everywhere.
//
// This file holds the three kernels (namespace flex::gat_bf16: 7 forms x 3 x DROP off / on = 42 instantiations) and their launchers
// (internal.h, launch_gat_bf16_*: a NULL mask launches DROP off); the entry points -- the GAT template pair on flex_bf16 rows, with
// pick_rows<flex_bf16> as the alignment rule -- are attention_entry.h's.
#include <cmath>
#include <cstdint>

#include "attention_gat_device.h"

namespace flex {
namespace gat_bf16 {

using namespace flex::attention;

// Grid: as attention_rows.  dm is not read with DROP off.
template <int W, int NS, bool DROP>
__global__ __launch_bounds__(256) void gat_bf16_rows(View v, HeadSplit hs, const float *__restrict__ El, const float *__restrict__ Er,
                                                      const flex_bf16 *__restrict__ V, float slope, DropMask dm, flex_bf16 *__restrict__ Out,
                                                      float *__restrict__ P) {
    __shared__ HeadsShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        gat::run_item<W, NS, DROP>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, slope, dm, Out, P, lane, w, sh);
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
        gat::run_item<W, NS, DROP>(v, hs, it, kind, El, Er, V, slope, dm, Out, P, lane, w, sh);
    }
}

template <int W, int NS, bool DROP>
__global__ __launch_bounds__(256) void gat_bf16_rows_backward(View v, HeadSplit hs, const float *__restrict__ El, const float *__restrict__ Er,
                                                               const flex_bf16 *__restrict__ V, const float *__restrict__ P,
                                                               const flex_bf16 *__restrict__ G, float slope, DropMask dm, float *__restrict__ GEl,
                                                               float *__restrict__ Work) {
    __shared__ gat::RowShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        gat::run_row<W, NS, DROP>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, P, G, slope, dm, GEl, Work, lane, w, sh);
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
        gat::run_row<W, NS, DROP>(v, hs, it, kind, El, Er, V, P, G, slope, dm, GEl, Work, lane, w, sh);
    }
}

template <int W, int NS, bool DROP>
__global__ __launch_bounds__(256) void gat_bf16_columns_backward(ColumnView v, HeadSplit hs, const flex_bf16 *__restrict__ G,
                                                                  const float *__restrict__ P, const float *__restrict__ DX, DropMask dm,
                                                                  float *__restrict__ GEr, flex_bf16 *__restrict__ GV) {
    __shared__ gat::ColumnShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_cols) {
        gat::run_column<W, NS, DROP>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, G, P, DX, dm, GEr, GV, lane, w, sh);
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
        gat::run_column<W, NS, DROP>(v, hs, it, kind, G, P, DX, dm, GEr, GV, lane, w, sh);
    }
}

}  // namespace gat_bf16

// ---- launches: dm == NULL launches the DROP-off instantiation

namespace attention {

int launch_gat_bf16_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const flex_bf16 *V,
                         float slope, const DropMask *dm, flex_bf16 *Out, float *P, hipStream_t s) {
    const View v = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 grid = launch_grid(v), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        if (dm) {
            hipLaunchKernelGGL((gat_bf16::gat_bf16_rows<W(), NS(), true>), grid, block, 0, s, v, hs, El, Er, V, slope, *dm, Out, P);
        } else {
            hipLaunchKernelGGL((gat_bf16::gat_bf16_rows<W(), NS(), false>), grid, block, 0, s, v, hs, El, Er, V, slope, DropMask{}, Out, P);
        }
    });
    return FLEX_OK;
}

int launch_gat_bf16_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er,
                                  const flex_bf16 *V, const float *P, const flex_bf16 *G, float slope, const DropMask *dm, float *GEl, float *Work,
                                  hipStream_t s) {
    const View rv = row_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 rgrid = launch_grid(rv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        if (dm) {
            hipLaunchKernelGGL((gat_bf16::gat_bf16_rows_backward<W(), NS(), true>), rgrid, block, 0, s, rv, hs, El, Er, V, P, G, slope, *dm, GEl, Work);
        } else {
            hipLaunchKernelGGL((gat_bf16::gat_bf16_rows_backward<W(), NS(), false>), rgrid, block, 0, s, rv, hs, El, Er, V, P, G, slope, DropMask{}, GEl,
                               Work);
        }
    });
    return FLEX_OK;
}

int launch_gat_bf16_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const flex_bf16 *G, const float *P,
                                     const float *DX, const DropMask *dm, float *GEr, flex_bf16 *GV, hipStream_t s) {
    const ColumnView cv = column_view(p);
    const HeadSplit hs{heads, lg};
    const dim3 cgrid = launch_grid(cv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        if (dm) {
            hipLaunchKernelGGL((gat_bf16::gat_bf16_columns_backward<W(), NS(), true>), cgrid, block, 0, s, cv, hs, G, P, DX, *dm, GEr, GV);
        } else {
            hipLaunchKernelGGL((gat_bf16::gat_bf16_columns_backward<W(), NS(), false>), cgrid, block, 0, s, cv, hs, G, P, DX, DropMask{}, GEr, GV);
        }
    });
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex
