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
#include <cmath>
#include <cstdint>

#include "attention_host.h"

namespace flex {
namespace attention {
namespace gat {

// torch.nn.functional.leaky_relu: 0 and NaN take the slope branch (the comparison is false)
__device__ __forceinline__ float leaky(float x, float slope) { return x > 0.f ? x : slope * x; }

// ---- forward

template <int W, int NS>
__device__ __forceinline__ void run_item(const View &v, const HeadSplit &hs, const uint4 &it, int kind, const float *__restrict__ El,
                                         const float *__restrict__ Er, const float *__restrict__ V, float slope, float *__restrict__ Out,
                                         float *__restrict__ P, uint32_t lane, uint32_t w, HeadsShared<W, NS> &sh) {
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
        float4 vv[U][NS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const float *vr = V + static_cast<size_t>(col) * v.ldb, *ec = Er + static_cast<size_t>(col) * static_cast<size_t>(hs.H);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                er[u][s] = (valid[u] && lh.live[s]) ? ec[lh.head[s]] : 0.f;
                vv[u][s] = valid[u] ? load_cols<true>(vr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float sc[U];
            float pm = -INFINITY;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                sc[u] = valid[u] ? leaky(elr[s] + er[u][s], slope) : -INFINITY;
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
                        axpy(x.acc[0], tm, vv[u][s]);
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
        float *orow = Out + static_cast<size_t>(pl.line) * v.ldc;
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

// Grid: as attention_rows.
template <int W, int NS>
__global__ __launch_bounds__(256) void gat_rows(View v, HeadSplit hs, const float *__restrict__ El, const float *__restrict__ Er, const float *__restrict__ V,
                                                 float slope, float *__restrict__ Out, float *__restrict__ P) {
    __shared__ HeadsShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        run_item<W, NS>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, slope, Out, P, lane, w, sh);
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
        run_item<W, NS>(v, hs, it, kind, El, Er, V, slope, Out, P, lane, w, sh);
    }
}

// ---- row backward

template <int W, int NS>
struct RowShared {
    float delta[kWavesPerBlock][W * NS];
    float gel[kWavesPerBlock][W * NS];
};

template <int W, int NS>
__device__ __forceinline__ void run_row(const View &v, const HeadSplit &hs, const uint4 &it, int kind, const float *__restrict__ El,
                                        const float *__restrict__ Er, const float *__restrict__ V, const float *__restrict__ P,
                                        const float *__restrict__ G, float slope, float *__restrict__ GEl, float *__restrict__ Work, uint32_t lane,
                                        uint32_t w, RowShared<W, NS> &sh) {
    const uint32_t slot = lane / W, li = lane % W;
    const int slot_lane0 = static_cast<int>(lane - li);
    const HeadLane hl(hs, li);
    const Place pl = place_of<W>(v.rowptr, it, kind, slot, w);
    const LaneHeads<W, NS> lh(hs, li, v.k);
    float4 g[NS];
    float elr[NS], delta[NS];
    const float *grow = G + static_cast<size_t>(pl.line) * v.ldc;
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
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const float *vr = V + static_cast<size_t>(col) * v.ldb;
#pragma unroll
            for (int s = 0; s < NS; ++s) vv[u][s] = valid[u] ? load_cols<true>(vr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int c = 4 * static_cast<int>(li) + 4 * W * s;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float da = head_total<W>(dot_cols<true>(0.f, g[s], vv[u][s], c, v.k), hl.hw);
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
                    const float x = elr[s] + Er[static_cast<size_t>(col) * static_cast<size_t>(hs.H) + lh.head[s]];
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

template <int W, int NS>
__global__ __launch_bounds__(256) void gat_rows_backward(View v, HeadSplit hs, const float *__restrict__ El, const float *__restrict__ Er,
                                                          const float *__restrict__ V, const float *__restrict__ P, const float *__restrict__ G,
                                                          float slope, float *__restrict__ GEl, float *__restrict__ Work) {
    __shared__ RowShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        run_row<W, NS>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, El, Er, V, P, G, slope, GEl, Work, lane, w, sh);
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
        run_row<W, NS>(v, hs, it, kind, El, Er, V, P, G, slope, GEl, Work, lane, w, sh);
    }
}

// ---- column backward

template <int W, int NS>
struct ColumnShared {
    alignas(16) float acc[kWavesPerBlock][4 * W * NS];
    float ger[kWavesPerBlock][W * NS];
};

template <int W, int NS>
__device__ __forceinline__ void run_column(const ColumnView &v, const HeadSplit &hs, const uint4 &it, int kind, const float *__restrict__ G,
                                           const float *__restrict__ P, const float *__restrict__ DX, float *__restrict__ GEr,
                                           float *__restrict__ GV, uint32_t lane, uint32_t w, ColumnShared<W, NS> &sh) {
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
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t row = __shfl(re.x, slot_lane0 + u), e = __shfl(re.y, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const float *gr = G + static_cast<size_t>(row) * v.ldc;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const bool live = valid[u] && lh.live[s];
                const uint64_t eh = static_cast<uint64_t>(e) * static_cast<uint64_t>(hs.H) + lh.head[s];
                pe[u][s] = (GV && live) ? P[eh] : 0.f;
                de[u][s] = (GEr && live) ? DX[eh] : 0.f;
                gg[u][s] = (GV && valid[u]) ? load_cols<true>(gr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (valid[u]) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    axpy(av[s], pe[u][s], gg[u][s]);
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

template <int W, int NS>
__global__ __launch_bounds__(256) void gat_columns_backward(ColumnView v, HeadSplit hs, const float *__restrict__ G, const float *__restrict__ P,
                                                             const float *__restrict__ DX, float *__restrict__ GEr, float *__restrict__ GV) {
    __shared__ ColumnShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_cols) {
        run_column<W, NS>(v, hs, v.item[v.n_wave_items + blockIdx.x], kBlockLine, G, P, DX, GEr, GV, lane, w, sh);
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
        run_column<W, NS>(v, hs, it, kind, G, P, DX, GEr, GV, lane, w, sh);
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
