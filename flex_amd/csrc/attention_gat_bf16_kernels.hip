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
// This file holds the three kernels (namespace flex::gat_bf16: 7 forms x 3 x DROP off / on = 42 instantiations), their launchers
// (internal.h, launch_gat_bf16_*: a NULL mask launches DROP off) and the four entry points: flex_gat_attention's and
// flex_gat_attention_backward's checks with pick_rows<flex_bf16> as the alignment rule and, in the dropout pair, the drop_p check
// beside the slope check.  They are here and not in attention_entry.h because the host simulator includes that header and has no
// stand-ins for these launchers.
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

// ---- the entry points: flex_gat_attention / flex_gat_attention_backward of attention_entry.h, refusal for refusal, with
// pick_rows<flex_bf16> over V, Out / g, gV as the alignment rule; `drop` adds the drop_p check beside the slope check.  drop_p == 0:
// once nothing is refused the undropped launch runs, which is all the undropped entry point does from there on, so the bits are its own.

// attention_entry.h's slope_ok: that header is for its one translation unit
static bool gat_bf16_slope_ok(float slope) { return std::isfinite(slope) && slope > 0.f && slope <= 1.f; }

static int gat_bf16_forward(bool drop, const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, float slope,
                            float drop_p, uint64_t seed, flex_bf16 *dOut, float *dP, flex_stream_t stream) {
    if (!p || !p->at_ok || heads < 1 || !gat_bf16_slope_ok(slope) || (drop && !drop_p_ok(drop_p))) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dEl || !dEr || !dV || !dOut) return FLEX_ERR_INVALID;
    const AttentionPick pick = pick_rows<flex_bf16>(p->k, p->ldb, p->ldc, {dV, dOut});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    const bool masked = drop && drop_p != 0.f;
    const DropMask dm = masked ? drop_mask(drop_p, seed) : DropMask{};
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    if (const int rc = launch_gat_bf16_rows(p, pick, heads, lg, dEl, dEr, dV, slope, masked ? &dm : nullptr, dOut, dP,
                                            reinterpret_cast<hipStream_t>(stream)))
        return rc;
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

static int gat_bf16_backward(bool drop, const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, const float *dP,
                             const flex_bf16 *dGradOut, float slope, float drop_p, uint64_t seed, float *dGradEl, float *dGradEr,
                             flex_bf16 *dGradV, float *dWork, flex_stream_t stream) {
    if (!p || !p->ab_ok || heads < 1 || !gat_bf16_slope_ok(slope) || (drop && !drop_p_ok(drop_p))) return FLEX_ERR_INVALID;
    int lg;
    if (const int rc = head_split_lg(p->k, heads, &lg)) return rc;
    if (p->at_entries == 0) return FLEX_OK;
    if (!dEl || !dEr || !dV || !dP || !dGradOut || !dWork || dWork == dP) return FLEX_ERR_INVALID;
    // the forward's rule over every row operand of the two launches (a NULL output is aligned)
    const AttentionPick pick = pick_rows<flex_bf16>(p->k, p->ldb, p->ldc, {dV, dGradOut, dGradV});
    if (!pick.vec4) return FLEX_ERR_UNSUPPORTED;
    if (!dGradEl && !dGradEr && !dGradV) return FLEX_OK;
    const bool masked = drop && drop_p != 0.f;
    const DropMask dm = masked ? drop_mask(drop_p, seed) : DropMask{};
    const DropMask *dmp = masked ? &dm : nullptr;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dGradEl || dGradEr) {
        if (const int rc = launch_gat_bf16_rows_backward(p, pick, heads, lg, dEl, dEr, dV, dP, dGradOut, slope, dmp, dGradEl, dWork, s)) return rc;
    }
    if (dGradEr || dGradV) {
        if (const int rc = launch_gat_bf16_columns_backward(p, pick, heads, lg, dGradOut, dP, dWork, dmp, dGradEr, dGradV, s)) return rc;
    }
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex

extern "C" {

int flex_gat_attention_bf16(const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, float slope, flex_bf16 *dOut,
                            float *dP, flex_stream_t stream) {
    return flex::attention::gat_bf16_forward(false, p, heads, dEl, dEr, dV, slope, 0.f, 0, dOut, dP, stream);
}

int flex_gat_attention_bf16_backward(const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, const float *dP,
                                     const flex_bf16 *dGradOut, float slope, float *dGradEl, float *dGradEr, flex_bf16 *dGradV, float *dWork,
                                     flex_stream_t stream) {
    return flex::attention::gat_bf16_backward(false, p, heads, dEl, dEr, dV, dP, dGradOut, slope, 0.f, 0, dGradEl, dGradEr, dGradV, dWork, stream);
}

int flex_gat_attention_bf16_dropout(const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, float slope, float drop_p,
                                    uint64_t seed, flex_bf16 *dOut, float *dP, flex_stream_t stream) {
    return flex::attention::gat_bf16_forward(true, p, heads, dEl, dEr, dV, slope, drop_p, seed, dOut, dP, stream);
}

int flex_gat_attention_bf16_dropout_backward(const flex_plan *p, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, const float *dP,
                                             const flex_bf16 *dGradOut, float slope, float drop_p, uint64_t seed, float *dGradEl, float *dGradEr,
                                             flex_bf16 *dGradV, float *dWork, flex_stream_t stream) {
    return flex::attention::gat_bf16_backward(true, p, heads, dEl, dEr, dV, dP, dGradOut, slope, drop_p, seed, dGradEl, dGradEr, dGradV, dWork,
                                              stream);
}

}  // extern "C"
