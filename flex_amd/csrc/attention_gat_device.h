// attention_gat_device.h -- the sweeps of the fused GAT attention, shared by attention_gat_kernels.hip (flex_gat_attention,
// flex_gat_attention_backward: DROP off, the sweeps are what they were), attention_gat_dropout_kernels.hip
// (flex_gat_attention_dropout, flex_gat_attention_dropout_backward: DROP on) and attention_gat_bf16_kernels.hip (the four
// flex_gat_attention_bf16 calls: E = flex_bf16, DROP off and on).
//
// The walk is attention_heads_kernels.hip's (attention_device.h): the same view, items, groups, slot / wave / block ownership by
// place_of, W = sddmm_lanes(k) lanes per slot, four entries per pass, four columns per lane and slab, the XCD remap, State<1> per lane
// and slab, merge, write_row, the mask and poison logic, ColumnView for the second backward launch.  A head is HW = d / 4 whole lanes
// of one slab; HW is a launch argument (its log2), so there is one instantiation per (W, NS).  The head split (HeadSplit, HeadLane,
// LaneHeads, head_total, merge_slots_heads, HeadsShared, sum_slot_scalars) is attention_device.h's, its rule internal.h's head_split_lg;
// namespace gat holds what is GAT's alone.  What differs from the dot-product heads:
//   forward        no K gather and no reduction across lanes for a score: per row a lane loads el[r, head] once, per entry
//                  er[src, head] -- one float, the lanes of a head reading the same address, the H heads of an entry one contiguous run --
//                  together with the four V gathers of the pass; scale = 1
//   row backward   sweep 1 is the heads kernel's (da by head_total, delta by fma); sweep 2 gathers nothing: the owning lane recomputes
//                  x = el + er, writes dx = (x > 0 ? 1 : slope) p (da - delta) over da and adds it into a per-head scalar gEl
//   column backward one accumulator row (gV) and one scalar per head and lane (gEr: all lanes of a head hold the same bits)
// Edge arrays (dP, dWork) are entry-major, (entry e, head h) at e H + h, written and read back by the lane HeadLane::writes names.
// Fixed order everywhere, no atomics.  Only the 16-byte form is built (the host refuses the rest).
//
// DROP: the dropout of the probabilities after the softmax, as in attention_heads_device.h.  Element (e, h) is kept iff
// dropout_bits(seed, e H + h) < thr (internal.h: DropMask; `kept` is attention_heads_device.h's), which every lane recomputes from the
// index it already holds -- no mask array.  The score, the maximum, the sum and P are untouched; a kept entry enters Out, da and gV with
// the factor c, a dropped one is selected out: its V row (forward, row backward sweep 1) or g row (column backward) is not gathered, so
// a non-finite row behind a dropped entry reaches nothing.  The er, P and dx loads do not see the mask; dx holds it through da, so gEl
// and gEr need no second look at it, and the column launch uses the mask for gV alone.
//
// E: the element type of the row operands V, Out, G and GV, deduced from the pointers: float, or flex_bf16 in
// attention_gat_bf16_kernels.hip.  The sweeps reach a row through load_cols, store_cols and write_row alone (attention_device.h), which
// hand over and take fp32: with flex_bf16 a lane's four columns are one 8-byte access, widened exactly and rounded once at the store.
// El, Er, P, DX, GEl, GEr, Work and every sum stay float, so on the widened operands the edge arrays and gEl, gEr have the fp32 bits.
//
// EDGE (attention_gat_edge_kernels.hip turns it on; off, which is the default, the sweeps are what they were): a per-entry, per-head
// term inside the LeakyReLU, x = (el + er) + ee in fp32 and in this order.  Ee is an edge array as dP: (entry e, head h) at e H + h, e
// the whole matrix's entry index.  Forward: every live lane of a head loads its element with the pass's er loads and V gathers -- the
// lanes of a head share the address, the H heads of an entry are one contiguous run; with DROP a dropped entry's term is read all the
// same.  Row backward, sweep 2: the owning lane forms the same x.  d x / d ee = 1, so gEe is dx, which sweep 2 writes to Work already.
#pragma once
#include <cmath>
#include <cstdint>

#include "attention_heads_device.h"

namespace flex {
namespace attention {
namespace gat {

// torch.nn.functional.leaky_relu: 0 and NaN take the slope branch (the comparison is false)
__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.f ? x : slope * x; }

// ---- forward

template <int W, int NS, bool DROP, bool EDGE = false, class E>
__device__ __forceinline__ void run_item(const View &v, const HeadSplit &hs, const uint4 &it, int kind, const float *__restrict__ El,
                                         const float *__restrict__ Er, const E *__restrict__ V, float slope, const DropMask &dm,
                                         E *__restrict__ Out, float *__restrict__ P, uint32_t lane, uint32_t w, HeadsShared<W, NS> &sh,
                                         const float *__restrict__ Ee = nullptr) {
    const uint32_t slot = lane / W, li = lane % W;
    const int slot_lane0 = static_cast<int>(lane - li);
    const HeadLane hl(hs, li);
    const Place pl = place_of<W>(v.rowptr, it, kind, slot, w);
    const LaneHeads<W, NS> lh(hs, li, v.k);
    float elr[NS];
    State<1> st[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        elr[s] = (pl.has_line && lh.live[s]) ? El[static_cast<size_t>(pl.line) * static_cast<size_t>(hs.H) + lh.head[s]] : 0.f;
        st[s].m = -INFINITY;
        st[s].l = 0.f;
        st[s].acc[0] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
        bool valid[U];
        float er[U][NS];
        float ee[U][NS];  // EDGE: the entry's own term of the score, a dropped entry's as well (it stays in the softmax)
        float4 vv[U][NS];
        bool keep[U][NS];  // DROP: whether (entry u, the head of slab s) is kept; a dropped entry's V row is not gathered and stays 0
        const uint64_t i0 = (DROP || EDGE) ? (pl.first + j0) * static_cast<uint64_t>(hs.H) : 0;  // the pass's first element of the edge arrays
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const E *vr = V + static_cast<size_t>(col) * v.ldb;
            const float *ec = Er + static_cast<size_t>(col) * static_cast<size_t>(hs.H);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                keep[u][s] = true;
                if constexpr (DROP) keep[u][s] = valid[u] && kept(dm, i0 + static_cast<uint32_t>(u * hs.H) + lh.head[s]);
                er[u][s] = (valid[u] && lh.live[s]) ? ec[lh.head[s]] : 0.f;
                ee[u][s] = 0.f;
                if constexpr (EDGE) ee[u][s] = (valid[u] && lh.live[s]) ? Ee[i0 + static_cast<uint32_t>(u * hs.H) + lh.head[s]] : 0.f;
                vv[u][s] = (valid[u] && keep[u][s]) ? load_cols<true>(vr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float sc[U];
            float pm = -INFINITY;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if constexpr (EDGE) {
                    sc[u] = valid[u] ? leaky((elr[s] + er[u][s]) + ee[u][s], slope) : -INFINITY;
                } else {
                    sc[u] = valid[u] ? leaky(elr[s] + er[u][s], slope) : -INFINITY;
                }
                pm = fmaxf(pm, max_key(sc[u]));
            }
            if (P && lh.live[s]) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (valid[u] && hl.writes(u)) P[(pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + lh.head[s]] = sc[u];
                }
            }
            State<1> &x = st[s];
            if (pm > x.m) {
                const float f = carry(x.m, pm, 1.f);
                x.l *= f;
                x.acc[0] = scaled(x.acc[0], f);
                x.m = pm;
            }
            if (x.m != INFINITY) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (valid[u]) {
                        const float tm = term(sc[u], x.m, 1.f);
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
    if (kind != kSlotLine) merge_slots_heads<W, NS>(st, lane, 1.f);
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
                merge(tot, o, 1.f);
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
                if (!lh.live[s]) continue;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (j0 + u < pl.len && hl.writes(u)) {
                        const uint64_t e = (pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + lh.head[s];
                        P[e] = prob(P[e], st[s].m, st[s].l, 1.f);
                    }
                }
            }
        }
    }
}

// ---- row backward

template <int W, int NS>
struct RowShared {
    float delta[kWavesPerBlock][W * NS];
    float gel[kWavesPerBlock][W * NS];
};

// DROP: da of a kept entry is c <g, V>, da of a dropped one +0 and its V row is not gathered; delta, dz, dx and gEl follow from da
template <int W, int NS, bool DROP, bool EDGE = false, class E>
__device__ __forceinline__ void run_row(const View &v, const HeadSplit &hs, const uint4 &it, int kind, const float *__restrict__ El,
                                        const float *__restrict__ Er, const E *__restrict__ V, const float *__restrict__ P,
                                        const E *__restrict__ G, float slope, const DropMask &dm, float *__restrict__ GEl,
                                        float *__restrict__ Work, uint32_t lane, uint32_t w, RowShared<W, NS> &sh,
                                        const float *__restrict__ Ee = nullptr) {
    const uint32_t slot = lane / W, li = lane % W;
    const int slot_lane0 = static_cast<int>(lane - li);
    const HeadLane hl(hs, li);
    const Place pl = place_of<W>(v.rowptr, it, kind, slot, w);
    const LaneHeads<W, NS> lh(hs, li, v.k);
    float4 g[NS];
    float elr[NS], delta[NS];
    const E *grow = G + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        g[s] = pl.has_line ? load_cols<true>(grow, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        elr[s] = (pl.has_line && lh.live[s]) ? El[static_cast<size_t>(pl.line) * static_cast<size_t>(hs.H) + lh.head[s]] : 0.f;
        delta[s] = 0.f;
    }
    // sweep 1: da into dWork, delta of the lane's heads
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
                if constexpr (DROP) keep[u][s] = valid[u] && kept(dm, i0 + static_cast<uint32_t>(u * hs.H) + lh.head[s]);
                vv[u][s] = (valid[u] && keep[u][s]) ? load_cols<true>(vr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = 4 * static_cast<int>(li) + 4 * W * s;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float da = head_total<W>(dot_cols<true>(0.f, g[s], vv[u][s], c, v.k), hl.hw);
                if constexpr (DROP) da = keep[u][s] ? dm.c * da : 0.f;
                if (valid[u] && lh.live[s]) {
                    const uint64_t e = (pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + lh.head[s];
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
    // sweep 2: dx over da in dWork, gEl.  Nothing is gathered: the edge arrays, the entry's column and er[src, head].
    float gel[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) gel[s] = 0.f;
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            if (j0 + u < pl.len && hl.writes(u)) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    if (!lh.live[s]) continue;
                    const uint64_t e = (pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + lh.head[s];
                    const float dz = P[e] * (Work[e] - delta[s]);
                    float x = elr[s] + Er[static_cast<size_t>(col) * static_cast<size_t>(hs.H) + lh.head[s]];
                    if constexpr (EDGE) x = x + Ee[e];  // the forward's two additions in its order: the same bits
                    const float dx = x > 0.f ? dz : slope * dz;
                    Work[e] = dx;
                    gel[s] += dx;
                }
            }
        }
    }
    if (!GEl) return;
    // the head's owning lanes, then the slots, then the waves: plain sums in the fixed order
#pragma unroll
    for (int s = 0; s < NS; ++s) gel[s] = head_total<W>(gel[s], hl.hw);
    if (kind != kSlotLine) sum_slot_scalars<W, NS>(gel, lane);
    bool writer = kind == kSlotLine ? pl.has_line : slot == 0;
    if (kind == kBlockLine) {
        if (slot == 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) sh.gel[w][li + W * s] = gel[s];
        }
        __syncthreads();
        writer = w == 0 && slot == 0;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            gel[s] = sh.gel[0][li + W * s];
#pragma unroll
            for (int i = 1; i < kWavesPerBlock; ++i) gel[s] += sh.gel[i][li + W * s];
        }
    }
    if (writer && hl.r == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (lh.live[s]) GEl[static_cast<size_t>(pl.line) * static_cast<size_t>(hs.H) + lh.head[s]] = gel[s];
        }
    }
}

// ---- column backward

template <int W, int NS>
struct ColumnShared {
    alignas(16) float acc[kWavesPerBlock][4 * W * NS];
    float ger[kWavesPerBlock][W * NS];
};

// DROP: gV alone sees the mask (dx holds it already): a kept entry adds (p c) g; a dropped one adds 0 x 0, neither its p nor its g row
// being read for gV
template <int W, int NS, bool DROP, class E>
__device__ __forceinline__ void run_column(const ColumnView &v, const HeadSplit &hs, const uint4 &it, int kind, const E *__restrict__ G,
                                           const float *__restrict__ P, const float *__restrict__ DX, const DropMask &dm,
                                           float *__restrict__ GEr, E *__restrict__ GV, uint32_t lane, uint32_t w, ColumnShared<W, NS> &sh) {
    const uint32_t slot = lane / W, li = lane % W;
    const int slot_lane0 = static_cast<int>(lane - li);
    const HeadLane hl(hs, li);
    const Place pl = place_of<W>(v.colptr, it, kind, slot, w);
    const LaneHeads<W, NS> lh(hs, li, v.k);
    float4 av[NS];
    float ger[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        av[s] = make_float4(0.f, 0.f, 0.f, 0.f);
        ger[s] = 0.f;
    }
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint2 re = mine ? v.ent[pl.first + j0 + li] : make_uint2(0u, 0u);
        bool valid[U];
        float pe[U][NS], de[U][NS];
        float4 gg[U][NS];
        bool keep[U][NS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t row = __shfl(re.x, slot_lane0 + u), e = __shfl(re.y, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const E *gr = G + static_cast<size_t>(row) * v.ldc;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const bool live = valid[u] && lh.live[s];
                const uint64_t eh = static_cast<uint64_t>(e) * static_cast<uint64_t>(hs.H) + lh.head[s];
                keep[u][s] = true;
                if constexpr (DROP) keep[u][s] = GV && live && kept(dm, eh);
                pe[u][s] = (GV && live && keep[u][s]) ? P[eh] : 0.f;
                if constexpr (DROP) pe[u][s] *= dm.c;
                de[u][s] = (GEr && live) ? DX[eh] : 0.f;
                gg[u][s] = (GV && valid[u] && keep[u][s]) ? load_cols<true>(gr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (valid[u]) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    axpy(av[s], pe[u][s], gg[u][s]);  // DROP, a dropped entry: pe and gg are the 0 they were set to
                    ger[s] += de[u][s];
                }
            }
        }
    }
    if (kind != kSlotLine) {
        sum_slots<W, NS>(av, lane);
        sum_slot_scalars<W, NS>(ger, lane);
    }
    bool writer = kind == kSlotLine ? pl.has_line : slot == 0;
    if (kind == kBlockLine) {
        if (slot == 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                *reinterpret_cast<float4 *>(&sh.acc[w][4 * li + 4 * W * s]) = av[s];
                sh.ger[w][li + W * s] = ger[s];
            }
        }
        __syncthreads();
        writer = w == 0 && slot == 0;
        if (writer) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                float4 tv = *reinterpret_cast<const float4 *>(&sh.acc[0][4 * li + 4 * W * s]);
                float te = sh.ger[0][li + W * s];
#pragma unroll
                for (int i = 1; i < kWavesPerBlock; ++i) {
                    tv = add4(tv, *reinterpret_cast<const float4 *>(&sh.acc[i][4 * li + 4 * W * s]));
                    te += sh.ger[i][li + W * s];
                }
                av[s] = tv;
                ger[s] = te;
            }
        }
    }
    if (writer) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (GV) store_cols<true>(GV + static_cast<size_t>(pl.line) * v.ldb, 4 * static_cast<int>(li) + 4 * W * s, v.k, av[s]);
            if (GEr && hl.r == 0 && lh.live[s]) GEr[static_cast<size_t>(pl.line) * static_cast<size_t>(hs.H) + lh.head[s]] = ger[s];
        }
    }
}

}  // namespace gat
}  // namespace attention
}  // namespace flex
