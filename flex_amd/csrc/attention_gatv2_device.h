// attention_gatv2_device.h -- the sweeps of the fused GATv2 attention (include/flex_spmm.h: flex_gatv2_attention,
// flex_gatv2_attention_backward; the kernels are attention_gatv2_kernels.hip's).  The score of entry e of row r, source c, head h is
//     s = sum_j att[hd + j] leaky(Xt[r, hd + j] + Xs[c, hd + j])
// which needs the full rows: it is the dot-product heads' walk (attention_heads_device.h), with att leaky(xt + xs) in place of q k and
// the ONE gathered row Xs[c] as score operand and value.  Everything the walk is made of is attention_device.h's, used by qualified
// name: View, ColumnView, Place and place_of, HeadSplit, HeadLane, head_total, State<1> with merge, merge_slots_heads and write_row,
// load_cols / store_cols, sum_slots, sum_slot_scalars and the LDS layouts of attention_heads_device.h.  What is GATv2's alone:
//   forward        per row a lane holds its four columns per slab of Xt[r] and of att; per entry the lane's partial is a chain of four
//                  fmas over att leaky(xt + xs), the head's lanes meet in head_total
//   row backward   sweep 1 is the heads kernel's on Xs (da, delta); sweep 2 gathers Xs again: the owning lane writes dz = p (da - delta)
//                  over da, every lane of the head adds dz (att f) into its gXt columns and dz leaky(x) into its gAtt partial, which it
//                  keeps across all the rows of its workgroup
//   column backward a slot holds Xs[c] and att; per entry it reads p and dz and gathers g[row] and Xt[row]; both terms of gXs go into
//                  one accumulator row, the score term first
// DROP (attention_gatv2_dropout_kernels.hip turns it on; off, the sweeps are what they were): the dropout of the probabilities after
// the softmax, w = kept(dm, e H + h) ? dm.c : 0 (internal.h: DropMask; `kept` is attention_heads_device.h's).  A dropped entry is
// gathered all the same and stays in the softmax; it is selected out of the value term of Out, of da in sweep 1 of the row backward
// and of the p g term of gXs, and nowhere else: the score term of gXs, gXt and gAtt hold the mask through dz.
// att f is a select between att and fl(att slope), so a term costs one fma.  Edge arrays are entry-major, (entry e, head h) at e H + h.
// Lanes past k hold zeros and touch no edge array.  Fixed order everywhere, no atomics.  Only the 16-byte form is built.
#pragma once
#include <cmath>
#include <cstdint>

#include "attention_heads_device.h"

namespace flex {
namespace gatv2 {

constexpr int U = attention::U;

// torch's leaky_relu: 0 and NaN take the slope branch
__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.f ? x : slope * x; }
__device__ __forceinline__ float4 leaky4(const float4 &t, const float4 &s, float slope) {
    return make_float4(leaky(t.x + s.x, slope), leaky(t.y + s.y, slope), leaky(t.z + s.z, slope), leaky(t.w + s.w, slope));
}
// att f on the lane's four columns: att where x = xt + xs > 0, fl(att slope) elsewhere
__device__ __forceinline__ float4 att_f(const float4 &a, const float4 &t, const float4 &s, float slope) {
    return make_float4(t.x + s.x > 0.f ? a.x : a.x * slope, t.y + s.y > 0.f ? a.y : a.y * slope, t.z + s.z > 0.f ? a.z : a.z * slope,
                       t.w + s.w > 0.f ? a.w : a.w * slope);
}

// ---- forward

// attention_heads_device.h, sweep_heads, with the score of GATv2 and one gather per entry
template <int W, int NS, bool DROP = false>
__device__ __forceinline__ void sweep(const attention::View &v, const attention::HeadSplit &hs, const attention::HeadLane &hl, const float4 (&xt)[NS],
                                      const float4 (&att)[NS], const float *__restrict__ Xs, float slope, float *__restrict__ P,
                                      const attention::Place &pl, uint32_t lane, uint32_t li, attention::State<1> (&st)[NS],
                                      const DropMask &dm = DropMask{}) {
    using namespace attention;
    const int slot_lane0 = static_cast<int>(lane - li);
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
        const uint64_t i0 = DROP ? (pl.first + j0) * static_cast<uint64_t>(hs.H) : 0;  // the pass's first element of the edge arrays
        bool valid[U];
        float4 xs[U][NS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const float *xr = Xs + static_cast<size_t>(col) * v.ldb;
#pragma unroll
            for (int s = 0; s < NS; ++s)
                xs[u][s] = valid[u] ? load_cols<true>(xr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        // DROP: bit s U + u is the keep bit of (entry u, the head of slab s): one register for the pass.  The loop is kept rolled, after
        // the gathers are issued: unrolled, the scheduler interleaves the hashes with the scores and the kernel grows by 22 registers
        uint32_t keep = 0;
        if constexpr (DROP) {
#pragma nounroll
            for (int t = 0; t < NS * U; ++t) {
                const uint32_t head = (li + static_cast<uint32_t>(W * (t / U))) >> hs.lg;
                keep |= (kept(dm, i0 + static_cast<uint32_t>((t % U) * hs.H) + head) ? 1u : 0u) << t;
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = 4 * static_cast<int>(li) + 4 * W * s;
            float sc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) sc[u] = head_total<W>(dot_cols<true>(0.f, att[s], leaky4(xt[s], xs[u][s], slope), c, v.k), hl.hw);
            const uint32_t head = (li + static_cast<uint32_t>(W * s)) >> hs.lg;
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
                        if constexpr (DROP) {  // a dropped entry stays in the sum and leaves the value term: selected out, not 0 x xs
                            if ((keep >> (s * U + u)) & 1u) axpy(x.acc[0], tm * dm.c, xs[u][s]);
                        } else {
                            axpy(x.acc[0], tm, xs[u][s]);
                        }
                    }
                }
            }
        }
    }
}

// attention_heads_device.h, run_item_heads: the merges, the Out row and the second sweep of dP are the same code
template <int W, int NS, bool DROP = false>
__device__ __forceinline__ void run_item(const attention::View &v, const attention::HeadSplit &hs, const uint4 &it, int kind, const float *__restrict__ Xt,
                                         const float *__restrict__ Xs, const float *__restrict__ Att, float slope, float *__restrict__ Out,
                                         float *__restrict__ P, uint32_t lane, uint32_t w, attention::HeadsShared<W, NS> &sh,
                                         const DropMask &dm = DropMask{}) {
    using namespace attention;
    const uint32_t slot = lane / W, li = lane % W;
    const HeadLane hl(hs, li);
    const Place pl = place_of<W>(v.rowptr, it, kind, slot, w);
    float4 xt[NS], att[NS];
    State<1> st[NS];
    const float *trow = Xt + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = 4 * static_cast<int>(li) + 4 * W * s;
        xt[s] = pl.has_line ? load_cols<true>(trow, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        att[s] = load_cols<true>(Att, c, v.k);
        st[s].m = -INFINITY;
        st[s].l = 0.f;
        st[s].acc[0] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    sweep<W, NS, DROP>(v, hs, hl, xt, att, Xs, slope, P, pl, lane, li, st, dm);
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
        float *orow = Out + static_cast<size_t>(pl.line) * v.ldc;
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
                        P[e] = prob(P[e], st[s].m, st[s].l, 1.f);
                    }
                }
            }
        }
    }
}

// ---- row backward

// attention_heads_device.h, run_row_heads.  ga: the lane's gAtt partial, which outlives the row (it is not read where GAtt is false)
template <int W, int NS, bool DROP = false>
__device__ __forceinline__ void run_row(const attention::View &v, const attention::HeadSplit &hs, const uint4 &it, int kind, const float *__restrict__ Xt,
                                        const float *__restrict__ Xs, const float *__restrict__ Att, const float *__restrict__ P,
                                        const float *__restrict__ G, float slope, float *__restrict__ GXt, bool GAtt, float *__restrict__ Work,
                                        float4 (&ga)[NS], uint32_t lane, uint32_t w, attention::HeadsRowShared<W, NS> &sh,
                                        const DropMask &dm = DropMask{}) {
    using namespace attention;
    const uint32_t slot = lane / W, li = lane % W;
    const int slot_lane0 = static_cast<int>(lane - li);
    const HeadLane hl(hs, li);
    const Place pl = place_of<W>(v.rowptr, it, kind, slot, w);
    // sweep 1: da into dWork, delta of the lane's heads
    float delta[NS];
    {
        float4 g[NS];
        const float *grow = G + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            g[s] = pl.has_line ? load_cols<true>(grow, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            delta[s] = 0.f;
        }
        for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
            const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
            const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
            const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
            bool valid[U];
            float4 xs[U][NS];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t col = __shfl(idx, slot_lane0 + u);
                valid[u] = j0 + u < pl.len;
                const float *xr = Xs + static_cast<size_t>(col) * v.ldb;
#pragma unroll
                for (int s = 0; s < NS; ++s)
                    xs[u][s] = valid[u] ? load_cols<true>(xr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            uint32_t keep = 0;  // DROP: bit s U + u, in a rolled loop after the gathers are issued, as in the forward's sweep
            if constexpr (DROP) {
                const uint64_t i0 = (pl.first + j0) * static_cast<uint64_t>(hs.H);
#pragma nounroll
                for (int t = 0; t < NS * U; ++t) {
                    const uint32_t head = (li + static_cast<uint32_t>(W * (t / U))) >> hs.lg;
                    keep |= (kept(dm, i0 + static_cast<uint32_t>((t % U) * hs.H) + head) ? 1u : 0u) << t;
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int c = 4 * static_cast<int>(li) + 4 * W * s;
                const uint32_t head = (li + static_cast<uint32_t>(W * s)) >> hs.lg;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    float da = head_total<W>(dot_cols<true>(0.f, g[s], xs[u][s], c, v.k), hl.hw);
                    if (valid[u] && c < v.k) {
                        const uint64_t e = (pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + head;
                        if constexpr (DROP) da = ((keep >> (s * U + u)) & 1u) ? dm.c * da : 0.f;  // dropped: +0 whatever the dot product is
                        if (hl.writes(u)) Work[e] = da;
                        delta[s] = __builtin_fmaf(P[e], da, delta[s]);
                    }
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
    // sweep 2: dz over da in dWork; gXt and the gAtt partial from a second gather of Xs
    const bool gather = GXt || GAtt;
    float4 xt[NS], att[NS], acc[NS];
    const float *trow = Xt + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = 4 * static_cast<int>(li) + 4 * W * s;
        xt[s] = (gather && pl.has_line) ? load_cols<true>(trow, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        att[s] = gather ? load_cols<true>(Att, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int head_lane0 = static_cast<int>(lane - hl.r);
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        float dze[NS][U];  // on the lane that owns (entry u, the head of slab s); 0 elsewhere
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const bool live = 4 * static_cast<int>(li) + 4 * W * s < v.k;
            const uint32_t head = (li + static_cast<uint32_t>(W * s)) >> hs.lg;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                dze[s][u] = 0.f;
                if (live && j0 + u < pl.len && hl.writes(u)) {
                    const uint64_t e = (pl.first + j0 + u) * static_cast<uint64_t>(hs.H) + head;
                    dze[s][u] = P[e] * (Work[e] - delta[s]);
                    Work[e] = dze[s][u];
                }
            }
        }
        if (!gather) continue;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            const bool valid = j0 + u < pl.len;
            const float *xr = Xs + static_cast<size_t>(col) * v.ldb;
            const int owner = head_lane0 + static_cast<int>(static_cast<uint32_t>(u) & hl.wm);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const float4 xs = valid ? load_cols<true>(xr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
                const float d = __shfl(dze[s][u], owner);
                if (valid) {
                    if (GXt) axpy(acc[s], d, att_f(att[s], xt[s], xs, slope));
                    if (GAtt) axpy(ga[s], d, leaky4(xt[s], xs, slope));
                }
            }
        }
    }
    if (!GXt) return;
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
        float *orow = GXt + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
        for (int s = 0; s < NS; ++s) store_cols<true>(orow, 4 * static_cast<int>(li) + 4 * W * s, v.k, acc[s]);
    }
}

// The workgroup's k-wide gAtt partial, stored once: the slots of a wave meet in a butterfly (lower slot first), the waves in LDS in
// wave order, and wave 0 writes row blockIdx.x of AttWork.  Every thread of the workgroup comes here, a wave without a group with zeros.
template <int W, int NS>
__device__ __forceinline__ void store_att_partial(float4 (&ga)[NS], int k, float *__restrict__ AttWork, uint32_t lane, uint32_t w,
                                                  attention::HeadsRowShared<W, NS> &sh) {
    using namespace attention;
    const uint32_t slot = lane / W, li = lane % W;
    sum_slots<W, NS>(ga, lane);
    __syncthreads();  // a block row's last reads of sh.acc are done
    if (slot == 0) {
#pragma unroll
        for (int s = 0; s < NS; ++s) *reinterpret_cast<float4 *>(&sh.acc[w][4 * li + 4 * W * s]) = ga[s];
    }
    __syncthreads();
    if (w == 0 && slot == 0) {
        float *prow = AttWork + static_cast<size_t>(blockIdx.x) * static_cast<size_t>(k);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float4 tot = *reinterpret_cast<const float4 *>(&sh.acc[0][4 * li + 4 * W * s]);
#pragma unroll
            for (int i = 1; i < kWavesPerBlock; ++i) tot = add4(tot, *reinterpret_cast<const float4 *>(&sh.acc[i][4 * li + 4 * W * s]));
            store_cols<true>(prow, 4 * static_cast<int>(li) + 4 * W * s, k, tot);
        }
    }
}

// ---- column backward

template <int W, int NS>
struct ColumnShared {
    alignas(16) float acc[kWavesPerBlock][4 * W * NS];
};

// attention_heads_device.h, run_column_heads, with one accumulator row: gXs[c] = sum over the column's entries of dz (att f) + p g[row]
template <int W, int NS, bool DROP = false>
__device__ __forceinline__ void run_column(const attention::ColumnView &v, const attention::HeadSplit &hs, const uint4 &it, int kind,
                                           const float *__restrict__ Xt, const float *__restrict__ Xs, const float *__restrict__ Att,
                                           const float *__restrict__ G, const float *__restrict__ P, const float *__restrict__ DZ, float slope,
                                           float *__restrict__ GXs, uint32_t lane, uint32_t w, ColumnShared<W, NS> &sh,
                                           const DropMask &dm = DropMask{}) {
    using namespace attention;
    const uint32_t slot = lane / W, li = lane % W;
    const int slot_lane0 = static_cast<int>(lane - li);
    const Place pl = place_of<W>(v.colptr, it, kind, slot, w);
    // four slabs: the Xt rows of a slab are gathered when its turn comes, not with the g rows -- both streams of four entries and four
    // slabs at once took the kernel to 256 registers, one wave per SIMD
    constexpr bool kLateXt = NS == 4;
    float4 xs[NS], att[NS], acc[NS];
    const float *srow = Xs + static_cast<size_t>(pl.line) * v.ldb;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int c = 4 * static_cast<int>(li) + 4 * W * s;
        xs[s] = pl.has_line ? load_cols<true>(srow, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        att[s] = load_cols<true>(Att, c, v.k);
        acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint2 re = mine ? v.ent[pl.first + j0 + li] : make_uint2(0u, 0u);
        bool valid[U];
        float pe[U][NS], de[U][NS];
        float4 gg[U][NS], tt[U][NS];
        const float *trow[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t row = __shfl(re.x, slot_lane0 + u), e = __shfl(re.y, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const float *gr = G + static_cast<size_t>(row) * v.ldc, *tr = Xt + static_cast<size_t>(row) * v.ldc;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int c = 4 * static_cast<int>(li) + 4 * W * s;
                const bool live = valid[u] && c < v.k;
                const uint64_t eh = static_cast<uint64_t>(e) * static_cast<uint64_t>(hs.H) + ((li + static_cast<uint32_t>(W * s)) >> hs.lg);
                if constexpr (DROP) {  // the mask folds into p; a dropped entry's g row is not gathered and its p g term adds 0 x 0
                    const bool keep = live && kept(dm, eh);
                    pe[u][s] = keep ? P[eh] * dm.c : 0.f;
                    de[u][s] = live ? DZ[eh] : 0.f;
                    gg[u][s] = keep ? load_cols<true>(gr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
                } else {
                    pe[u][s] = live ? P[eh] : 0.f;
                    de[u][s] = live ? DZ[eh] : 0.f;
                    gg[u][s] = valid[u] ? load_cols<true>(gr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                if constexpr (!kLateXt) tt[u][s] = valid[u] ? load_cols<true>(tr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            trow[u] = tr;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {  // a column's terms meet in entry order whichever loop is the outer one
            if constexpr (kLateXt) {
#pragma unroll
                for (int u = 0; u < U; ++u)
                    tt[u][s] = valid[u] ? load_cols<true>(trow[u], 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (valid[u]) {
                    axpy(acc[s], de[u][s], att_f(att[s], tt[u][s], xs[s], slope));
                    axpy(acc[s], pe[u][s], gg[u][s]);
                }
            }
        }
    }
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
        float *orow = GXs + static_cast<size_t>(pl.line) * v.ldb;
#pragma unroll
        for (int s = 0; s < NS; ++s) store_cols<true>(orow, 4 * static_cast<int>(li) + 4 * W * s, v.k, acc[s]);
    }
}

}  // namespace gatv2
}  // namespace flex
