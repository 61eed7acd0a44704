// attention_heads_device.h -- the sweeps of the per-head dot-product attention, over the element type E of the row operands (Q, K, V,
// Out, g, gQ, gK, gV): float in attention_heads_kernels.hip (flex_attention_heads, flex_attention_heads_backward), flex_bf16 in
// attention_bf16_kernels.hip (flex_attention_bf16, flex_attention_bf16_backward), and both, with the row sweeps' compile-time BIAS
// switch on, in attention_bias_kernels.hip (flex_attention_bias, flex_attention_bf16_bias and their backward calls: a per-edge, per-head
// term in the score and its gradient; off, the sweeps are what they were).  E enters through load_cols, store_cols and write_row
// (attention_device.h) and nowhere else: a row is widened to fp32 as it is loaded and narrowed at its one store, so the two objects run
// the same walk and the same fp32 expressions.  The edge arrays (dP, dWork) and LDS are fp32 for every E.
//
// The walk is the single-head kernels' (attention_kernels.hip, attention_backward_kernels.hip; attention_device.h, which also holds the
// head split: HeadSplit, HeadLane, head_total, merge_slots_heads, HeadsShared; its rule is internal.h's head_split_lg): the same view, items,
// groups, slot / wave / block ownership, W = sddmm_lanes(k) lanes per slot, four entries per pass and four columns per lane and slab.
// d is a power of two in [4, 256], so a head is HW = d / 4 whole lanes of one slab: the lane that holds columns c .. c + 3 belongs to
// head c / d, and the lanes of a head are HW consecutive lanes that start at a multiple of HW.  HW is a launch argument (its log2),
// the same for every lane.  Where k / 4 < W (k = 48: 12 of 16 lanes) the lanes past k hold zeros, form groups of their own and neither
// read nor write an edge array.  What changes against one head:
//   forward        a score is reduced over the HW lanes of the lane's head, per slab (head_total), so every lane holds the four scores
//                  of ITS head; the running maximum, the running sum, the rescale, the mask and poison rules and every merge are kept
//                  per lane and slab, i.e. per head (State<1> per slab: all lanes of a head hold the same bits); a block row's waves
//                  meet in LDS with one (m, l) per group of four columns
//   row backward   da is reduced the same way, delta is per lane and slab, ds of the lane's own head enters gQ
//   column backward p and ds are read at the lane's head; nothing else (there was never a reduction across lanes)
// Edge arrays (dP, dWork) are entry-major: (entry e, head h) at e H + h.  Of the HW lanes of a head, lane r (r = lane % HW) writes
// entry u of a pass where u == r (HW >= 4) or u % HW == r (HW = 1, 2); the same lane reads its element back in the second sweep.
// Fixed order everywhere, no atomics.  Only the vector form is built: one 16-byte access of four floats, one 8-byte access of four
// flex_bf16 (the host refuses the rest).
//
// DROP (attention_dropout_kernels.hip: flex_attention_dropout and its backward, bf16 and bias forms included; off, the sweeps are what
// they were): the dropout of the probabilities after the softmax.  Element (e, h) is kept iff dropout_bits(seed, e H + h) < thr
// (internal.h: DropMask), which every lane recomputes from the index it already holds -- no mask array.  The score, the maximum, the sum
// and P are untouched; a kept entry enters Out, da and gV with the factor c, a dropped one is selected out (its V and g rows are not
// even gathered), so a non-finite V row behind a dropped entry reaches nothing.
#pragma once
#include <cmath>
#include <cstdint>

#include "attention_host.h"

namespace flex {
namespace attention {

// ---- forward

// attention_kernels.hip, sweep, with the state per slab.  BIAS (attention_bias_kernels.hip): the score of a valid entry becomes
// t = fma(scale, s, Bias[e H + head]) -- every lane of a head loads its head's element, one address for the HW lanes -- and `sm`, the
// scale of everything after the score, is 1
// the keep bit of element i = e H + head of the edge arrays: every lane of a head computes the same bit
__device__ __forceinline__ bool kept(const DropMask &dm, uint64_t i) { return dropout_bits(dm.seed_lo, dm.seed_hi, i) < dm.thr; }

template <int W, int NS, bool BIAS, bool DROP, class E>
__device__ __forceinline__ void sweep_heads(const View &v, const HeadSplit &hs, const HeadLane &hl, const float4 (&q)[NS], const E *__restrict__ K,
                                            const E *__restrict__ V, const float *__restrict__ Bias, float scale, float sm, const DropMask &dm,
                                            float *__restrict__ P, const Place &pl, uint32_t lane, uint32_t li, State<1> (&st)[NS]) {
    const int slot_lane0 = static_cast<int>(lane - li);
    // four slabs: the V rows of a slab are gathered when its scores are done, not with the K rows -- the per-slab state would otherwise
    // take the kernel past 256 registers, to one wave per SIMD
    constexpr bool kLateV = NS == 4;
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
        bool valid[U];
        float4 kv[U][NS], vv[U][NS];
        const E *vrow[U];
        bool keep[U][NS];  // DROP: whether (entry u, the head of slab s) is kept; a dropped entry's V row is not gathered and stays 0
        const uint64_t i0 = DROP ? (pl.first + j0) * static_cast<uint64_t>(hs.H) : 0;  // the pass's first element of the edge arrays
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const E *kr = K + static_cast<size_t>(col) * v.ldb, *vr = V + static_cast<size_t>(col) * v.ldb;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int c = 4 * static_cast<int>(li) + 4 * W * s;
                keep[u][s] = true;
                if constexpr (DROP) keep[u][s] = valid[u] && kept(dm, i0 + static_cast<uint32_t>(u * hs.H) + ((li + static_cast<uint32_t>(W * s)) >> hs.lg));
                kv[u][s] = valid[u] ? load_cols<true>(kr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (!kLateV) vv[u][s] = (valid[u] && keep[u][s]) ? load_cols<true>(vr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            vrow[u] = vr;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = 4 * static_cast<int>(li) + 4 * W * s;
            if constexpr (kLateV) {
#pragma unroll
                for (int u = 0; u < U; ++u) vv[u][s] = (valid[u] && keep[u][s]) ? load_cols<true>(vrow[u], c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            float sc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) sc[u] = head_total<W>(dot_cols<true>(0.f, q[s], kv[u][s], c, v.k), hl.hw);
            const uint32_t head = (li + static_cast<uint32_t>(W * s)) >> hs.lg;
            if constexpr (BIAS) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (valid[u] && c < v.k) sc[u] = __builtin_fmaf(scale, sc[u], Bias[(pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + head]);
                }
            }
            float pm = -INFINITY;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!valid[u]) sc[u] = -INFINITY;
                pm = fmaxf(pm, max_key(sc[u]));
            }
            if (P && c < v.k) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (valid[u] && hl.writes(u)) P[(pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + head] = sc[u];
                }
            }
            State<1> &x = st[s];
            if (pm > x.m) {
                const float f = carry(x.m, pm, sm);
                x.l *= f;
                x.acc[0] = scaled(x.acc[0], f);
                x.m = pm;
            }
            if (x.m != INFINITY) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (valid[u]) {
                        const float tm = term(sc[u], x.m, sm);
                        x.l += tm;
                        if constexpr (DROP) {  // a dropped entry: vv is the 0 it was set to, whatever V holds
                            axpy(x.acc[0], keep[u][s] ? tm * dm.c : 0.f, vv[u][s]);
                        } else {
                            axpy(x.acc[0], tm, vv[u][s]);
                        }
                    }
                }
            }
        }
    }
}

template <int W, int NS, bool BIAS, bool DROP, class E>
__device__ __forceinline__ void run_item_heads(const View &v, const HeadSplit &hs, const uint4 &it, int kind, const E *__restrict__ Q,
                                               const E *__restrict__ K, const E *__restrict__ V, const float *__restrict__ Bias, float scale,
                                               const DropMask &dm, E *__restrict__ Out, float *__restrict__ P, uint32_t lane, uint32_t w, HeadsShared<W, NS> &sh) {
    const float sm = BIAS ? 1.f : scale;  // the scale of the softmax: with a bias it is already in the stored score
    const uint32_t slot = lane / W, li = lane % W;
    const HeadLane hl(hs, li);
    const Place pl = place_of<W>(v.rowptr, it, kind, slot, w);
    float4 q[NS];
    State<1> st[NS];
    const E *qrow = Q + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        q[s] = pl.has_line ? load_cols<true>(qrow, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        st[s].m = -INFINITY;
        st[s].l = 0.f;
        st[s].acc[0] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    sweep_heads<W, NS, BIAS, DROP>(v, hs, hl, q, K, V, Bias, scale, sm, dm, P, pl, lane, li, st);
    if (kind != kSlotLine) merge_slots_heads<W, NS>(st, lane, sm);
    bool writer = kind == kSlotLine ? pl.has_line : slot == 0;
    if (kind == kBlockLine) {
        if (slot == 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                *reinterpret_cast<float4 *>(&sh.acc[w][4 * li + 4 * W * s]) = st[s].acc[0];
                sh.ml[w][li + W * s] = make_float2(st[s].m, st[s].l);
            }
        }
        __syncthreads();
        writer = w == 0 && slot == 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {  // the waves in wave order: every lane folds (m, l) of its head, the writing lanes their columns as well
            State<1> tot;
            tot.m = sh.ml[0][li + W * s].x;
            tot.l = sh.ml[0][li + W * s].y;
            tot.acc[0] = writer ? *reinterpret_cast<const float4 *>(&sh.acc[0][4 * li + 4 * W * s]) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int i = 1; i < kWavesPerBlock; ++i) {
                State<1> o;
                o.m = sh.ml[i][li + W * s].x;
                o.l = sh.ml[i][li + W * s].y;
                o.acc[0] = writer ? *reinterpret_cast<const float4 *>(&sh.acc[i][4 * li + 4 * W * s]) : make_float4(0.f, 0.f, 0.f, 0.f);
                merge(tot, o, sm);
            }
            st[s] = tot;
        }
    }
    if (writer) {
        E *orow = Out + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
        for (int s = 0; s < NS; ++s) write_row<1, true>(orow + 4 * W * s, st[s], li, W, v.k - 4 * W * s);
    }
    if (P) {  // the second sweep of dP: the lane that wrote a raw score overwrites it with the probability under its head's final (M, L)
        for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
            const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (4 * static_cast<int>(li) + 4 * W * s >= v.k) continue;
                const uint32_t head = (li + static_cast<uint32_t>(W * s)) >> hs.lg;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j0 + u < pl.len && hl.writes(u)) {
                        const uint64_t e = (pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + head;
                        P[e] = prob(P[e], st[s].m, st[s].l, sm);
                    }
                }
            }
        }
    }
}

// The body of the forward kernel of either element type, which declares `sh`.  Grid: as attention_rows.  BIAS: Bias is nnz x H floats
// in the layout of P (it is not read otherwise).  DROP: dm is the mask and the factor of the kept entries (it is not read otherwise).
template <int W, int NS, bool BIAS = false, bool DROP = false, class E>
__device__ __forceinline__ void walk_rows_heads(const View &v, const HeadSplit &hs, const E *__restrict__ Q, const E *__restrict__ K,
                                                const E *__restrict__ V, float scale, E *__restrict__ Out, float *__restrict__ P,
                                                HeadsShared<W, NS> &sh, const float *__restrict__ Bias = nullptr, const DropMask &dm = DropMask{}) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        run_item_heads<W, NS, BIAS, DROP>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Q, K, V, Bias, scale, dm, Out, P, lane, w, sh);
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
        run_item_heads<W, NS, BIAS, DROP>(v, hs, it, kind, Q, K, V, Bias, scale, dm, Out, P, lane, w, sh);
    }
}

// ---- row backward

template <int W, int NS>
struct HeadsRowShared {
    float delta[kWavesPerBlock][W * NS];
    alignas(16) float acc[kWavesPerBlock][4 * W * NS];
};

// attention_backward_kernels.hip, run_row, with da, delta and ds per slab.  BIAS (attention_bias_kernels.hip): sweep 2 also stores the
// gradient in the bias, p (da - delta), into GB where GB is not NULL.  DROP: da of a kept entry is c <g, V>, da of a dropped one +0; the
// rest follows from da
template <int W, int NS, bool BIAS, bool DROP, class E>
__device__ __forceinline__ void run_row_heads(const View &v, const HeadSplit &hs, const uint4 &it, int kind, const E *__restrict__ K,
                                              const E *__restrict__ V, const float *__restrict__ P, const E *__restrict__ G, float scale,
                                              const DropMask &dm, E *__restrict__ GQ, float *__restrict__ GB, float *__restrict__ Work, uint32_t lane, uint32_t w,
                                              HeadsRowShared<W, NS> &sh) {
    const uint32_t slot = lane / W, li = lane % W;
    const int slot_lane0 = static_cast<int>(lane - li);
    const HeadLane hl(hs, li);
    const Place pl = place_of<W>(v.rowptr, it, kind, slot, w);
    float4 g[NS];
    const E *grow = G + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
    for (int s = 0; s < NS; ++s) g[s] = pl.has_line ? load_cols<true>(grow, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
    // sweep 1: da into dWork, delta of the lane's heads
    float delta[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) delta[s] = 0.f;
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
        bool valid[U];
        float4 vv[U][NS];
        bool keep[U][NS];  // DROP: as in the forward
        const uint64_t i0 = DROP ? (pl.first + j0) * static_cast<uint64_t>(hs.H) : 0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const E *vr = V + static_cast<size_t>(col) * v.ldb;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                keep[u][s] = true;
                if constexpr (DROP) keep[u][s] = valid[u] && kept(dm, i0 + static_cast<uint32_t>(u * hs.H) + ((li + static_cast<uint32_t>(W * s)) >> hs.lg));
                vv[u][s] = (valid[u] && keep[u][s]) ? load_cols<true>(vr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = 4 * static_cast<int>(li) + 4 * W * s;
            const uint32_t head = (li + static_cast<uint32_t>(W * s)) >> hs.lg;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float da = head_total<W>(dot_cols<true>(0.f, g[s], vv[u][s], c, v.k), hl.hw);
                if constexpr (DROP) da = keep[u][s] ? dm.c * da : 0.f;
                if (valid[u] && c < v.k) {
                    const uint64_t e = (pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + head;
                    if (hl.writes(u)) Work[e] = da;
                    delta[s] = __builtin_fmaf(P[e], da, delta[s]);
                }
            }
        }
    }
    if (kind != kSlotLine) sum_slot_scalars<W, NS>(delta, lane);
    if (kind == kBlockLine) {
        if (slot == 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) sh.delta[w][li + W * s] = delta[s];
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            delta[s] = sh.delta[0][li + W * s];
#pragma unroll
            for (int i = 1; i < kWavesPerBlock; ++i) delta[s] += sh.delta[i][li + W * s];
        }
    }
    // sweep 2: ds over da in dWork, gQ
    float4 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int head_lane0 = static_cast<int>(lane - hl.r);
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        float dse[NS][U];  // on the lane that owns (entry u, the head of slab s); 0 elsewhere
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bool live = 4 * static_cast<int>(li) + 4 * W * s < v.k;
            const uint32_t head = (li + static_cast<uint32_t>(W * s)) >> hs.lg;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                dse[s][u] = 0.f;
                if (live && j0 + u < pl.len && hl.writes(u)) {
                    const uint64_t e = (pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + head;
                    const float d = Work[e] - delta[s];
                    dse[s][u] = (scale * P[e]) * d;
                    Work[e] = dse[s][u];
                    if constexpr (BIAS) {
                        if (GB) GB[e] = P[e] * d;
                    }
                }
            }
        }
        if (!GQ) continue;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
        bool valid[U];
        float4 kv[U][NS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const E *kr = K + static_cast<size_t>(col) * v.ldb;
#pragma unroll
            for (int s = 0; s < NS; ++s) kv[u][s] = valid[u] ? load_cols<true>(kr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int owner = head_lane0 + static_cast<int>(static_cast<uint32_t>(u) & hl.wm);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float d = __shfl(dse[s][u], owner);
                if (valid[u]) axpy(acc[s], d, kv[u][s]);
            }
        }
    }
    if (!GQ) return;
    if (kind != kSlotLine) sum_slots<W, NS>(acc, lane);
    bool writer = kind == kSlotLine ? pl.has_line : slot == 0;
    if (kind == kBlockLine) {
        if (slot == 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) *reinterpret_cast<float4 *>(&sh.acc[w][4 * li + 4 * W * s]) = acc[s];
        }
        __syncthreads();
        writer = w == 0 && slot == 0;
        if (writer) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float4 tot = *reinterpret_cast<const float4 *>(&sh.acc[0][4 * li + 4 * W * s]);
#pragma unroll
                for (int i = 1; i < kWavesPerBlock; ++i) tot = add4(tot, *reinterpret_cast<const float4 *>(&sh.acc[i][4 * li + 4 * W * s]));
                acc[s] = tot;
            }
        }
    }
    if (writer) {
        E *orow = GQ + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
        for (int s = 0; s < NS; ++s) store_cols<true>(orow, 4 * static_cast<int>(li) + 4 * W * s, v.k, acc[s]);
    }
}

// the body of the row backward kernel of either element type
template <int W, int NS, bool BIAS = false, bool DROP = false, class E>
__device__ __forceinline__ void walk_rows_heads_backward(const View &v, const HeadSplit &hs, const E *__restrict__ K, const E *__restrict__ V,
                                                         const float *__restrict__ P, const E *__restrict__ G, float scale, E *__restrict__ GQ,
                                                         float *__restrict__ Work, HeadsRowShared<W, NS> &sh, float *__restrict__ GB = nullptr,
                                                         const DropMask &dm = DropMask{}) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        run_row_heads<W, NS, BIAS, DROP>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, K, V, P, G, scale, dm, GQ, GB, Work, lane, w, sh);
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
        run_row_heads<W, NS, BIAS, DROP>(v, hs, it, kind, K, V, P, G, scale, dm, GQ, GB, Work, lane, w, sh);
    }
}

// ---- column backward

template <int W, int NS>
struct HeadsColumnShared {
    alignas(16) float acc[2][kWavesPerBlock][4 * W * NS];
};

// attention_backward_kernels.hip, run_column, with p and ds of the lane's head.  DROP: gV alone sees the mask (ds holds it already): a
// kept entry adds (p c) g; a dropped one adds 0 x 0, neither its p nor its g row being read for gV
template <int W, int NS, bool DROP, class E>
__device__ __forceinline__ void run_column_heads(const ColumnView &v, const HeadSplit &hs, const uint4 &it, int kind, const E *__restrict__ Q,
                                                 const E *__restrict__ G, const float *__restrict__ P, const float *__restrict__ DS,
                                                 const DropMask &dm, E *__restrict__ GK, E *__restrict__ GV, uint32_t lane, uint32_t w, HeadsColumnShared<W, NS> &sh) {
    const uint32_t slot = lane / W, li = lane % W;
    const int slot_lane0 = static_cast<int>(lane - li);
    const Place pl = place_of<W>(v.colptr, it, kind, slot, w);
    float4 ak[NS], av[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) ak[s] = av[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint2 re = mine ? v.ent[pl.first + j0 + li] : make_uint2(0u, 0u);
        bool valid[U];
        float pe[U][NS], de[U][NS];
        float4 gg[U][NS], qq[U][NS];
        bool keep[U][NS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t row = __shfl(re.x, slot_lane0 + u), e = __shfl(re.y, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const E *gr = G + static_cast<size_t>(row) * v.ldc, *qr = Q + static_cast<size_t>(row) * v.ldc;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int c = 4 * static_cast<int>(li) + 4 * W * s;
                const bool live = valid[u] && c < v.k;
                const uint64_t eh = static_cast<uint64_t>(e) * static_cast<uint64_t>(hs.H) + ((li + static_cast<uint32_t>(W * s)) >> hs.lg);
                keep[u][s] = true;
                if constexpr (DROP) keep[u][s] = GV && live && kept(dm, eh);
                pe[u][s] = (GV && live && keep[u][s]) ? P[eh] : 0.f;
                if constexpr (DROP) pe[u][s] *= dm.c;
                de[u][s] = (GK && live) ? DS[eh] : 0.f;
                gg[u][s] = (GV && valid[u] && keep[u][s]) ? load_cols<true>(gr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
                qq[u][s] = (GK && valid[u]) ? load_cols<true>(qr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (valid[u]) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    axpy(av[s], pe[u][s], gg[u][s]);  // DROP, a dropped entry: pe and gg are the 0 they were set to
                    axpy(ak[s], de[u][s], qq[u][s]);
                }
            }
        }
    }
    if (kind != kSlotLine) {
        sum_slots<W, NS>(ak, lane);
        sum_slots<W, NS>(av, lane);
    }
    bool writer = kind == kSlotLine ? pl.has_line : slot == 0;
    if (kind == kBlockLine) {
        if (slot == 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                *reinterpret_cast<float4 *>(&sh.acc[0][w][4 * li + 4 * W * s]) = ak[s];
                *reinterpret_cast<float4 *>(&sh.acc[1][w][4 * li + 4 * W * s]) = av[s];
            }
        }
        __syncthreads();
        writer = w == 0 && slot == 0;
        if (writer) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float4 tk = *reinterpret_cast<const float4 *>(&sh.acc[0][0][4 * li + 4 * W * s]);
                float4 tv = *reinterpret_cast<const float4 *>(&sh.acc[1][0][4 * li + 4 * W * s]);
#pragma unroll
                for (int i = 1; i < kWavesPerBlock; ++i) {
                    tk = add4(tk, *reinterpret_cast<const float4 *>(&sh.acc[0][i][4 * li + 4 * W * s]));
                    tv = add4(tv, *reinterpret_cast<const float4 *>(&sh.acc[1][i][4 * li + 4 * W * s]));
                }
                ak[s] = tk;
                av[s] = tv;
            }
        }
    }
    if (writer) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = 4 * static_cast<int>(li) + 4 * W * s;
            if (GK) store_cols<true>(GK + static_cast<size_t>(pl.line) * v.ldb, c, v.k, ak[s]);
            if (GV) store_cols<true>(GV + static_cast<size_t>(pl.line) * v.ldb, c, v.k, av[s]);
        }
    }
}

// the body of the column backward kernel of either element type
template <int W, int NS, bool DROP = false, class E>
__device__ __forceinline__ void walk_columns_heads_backward(const ColumnView &v, const HeadSplit &hs, const E *__restrict__ Q, const E *__restrict__ G,
                                                            const float *__restrict__ P, const float *__restrict__ DS, E *__restrict__ GK,
                                                            E *__restrict__ GV, HeadsColumnShared<W, NS> &sh, const DropMask &dm = DropMask{}) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_cols) {
        run_column_heads<W, NS, DROP>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Q, G, P, DS, dm, GK, GV, lane, w, sh);
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
        run_column_heads<W, NS, DROP>(v, hs, it, kind, Q, G, P, DS, dm, GK, GV, lane, w, sh);
    }
}

}  // namespace attention
}  // namespace flex
