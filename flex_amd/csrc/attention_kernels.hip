// attention_kernels.hip -- the fused attention forward of FLEX_PLAN_ATTENTION plans (include/flex_spmm.h: flex_attention): scores,
// their softmax over each row of hostA and the SpMM with the result, in one launch and without an nnz-sized intermediate.  The walk
// is built by the planner from hostA's row pointer and columns (plan_build.cpp, upload_attention_image; the classes and constants:
// internal.h, kAtPass) and verified by flex_plan_self_check (plan_check.cpp).
//
// Not an SpMM kernel and not one of flex::values / flex::softmax: a namespace of its own; tests/test_gpu_fused_attention.py covers it,
// the 16-byte and the generic form of every (W, NS): the cases are tests/attention_forms.py's, and tests/test_attention_routes.py holds
// every instantiation of flex::attention to a case that launches it.
// The view of the walk, the slot placement (place_of) and the helpers it shares with the other attention kernels: attention_device.h;
// the view, the grid and the (W, NS) dispatch of the launcher: attention_host.h.  The entry points of all six attention files are host
// code of their own, attention_entry.h, which this file includes at its end: it is their one translation unit in the library.
//
// Row-owned.  A SLOT of W lanes holds its Q row and its Out row (4 columns per lane and slab) in registers, with the running maximum m
// and the running sum l of the row's terms exp(scale (s - m)).  Per pass the slot takes kAtPass = 4 consecutive entries: its first
// four lanes load their K / V row indices (one coalesced access) and broadcast them, the four K rows and the four V rows are gathered
// together, K is folded into four fma chains that are reduced across the slot so that every lane holds all four scores, the maximum is
// raised once (one expf rescales l and the Out row), and the four terms are added.  A masked entry (-inf) adds a term of exactly 0 --
// but still multiplies its V row, as the composition's p = +0 does -- and a NaN or +inf score turns the maximum into +inf, the mark
// of a poisoned row (softmax_kernels.hip, max_key); nothing depends on inf - inf.
//   slot item   up to 64 / W consecutive short rows, slot s on row s: no slot meets another
//   wave row    the 64 / W slots take passes s, s + 64 / W, ...; their states merge in a butterfly over the slots, lower slot first
//   block row   a workgroup: the 4 x 64 / W slots stride the row, every wave merges as above, the waves meet in LDS in wave order
// dP: the raw score is written in the sweep by lane u of the slot for entry u of the pass; once the row's (M, L) is final the same lane
// reads it back and overwrites it with the probability -- no second gather of K.  Fixed order everywhere, no atomics.
#include <cmath>
#include <cstdint>

#include "attention_host.h"

namespace flex {
namespace attention {

// The sweep of one slot over its share of a row: first, len, t, T and n_pass are the slot's Place (attention_device.h).
template <int W, int NS, bool VEC>
__device__ __forceinline__ void sweep(const View &v, const float4 (&q)[NS], const float *__restrict__ K, const float *__restrict__ V, float scale,
                                      float *__restrict__ P, uint64_t first, uint32_t len, uint32_t t, uint32_t T, uint32_t n_pass, uint32_t lane,
                                      uint32_t li, State<NS> &st) {
    const int slot_lane0 = static_cast<int>(lane - li);
    for (uint32_t pass = 0; pass < n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * T + t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < len;
        const uint32_t idx = mine ? v.src[first - v.e0 + j0 + li] : 0u;
        bool valid[U];
        float4 kv[U][NS], vv[U][NS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < len;
            const float *kr = K + static_cast<size_t>(col) * v.ldb, *vr = V + static_cast<size_t>(col) * v.ldb;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int c = 4 * static_cast<int>(li) + 4 * W * s;
                kv[u][s] = valid[u] ? load_cols<VEC>(kr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
                vv[u][s] = valid[u] ? load_cols<VEC>(vr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        float pr[U], sc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float a = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) a = dot_cols<VEC>(a, q[s], kv[u][s], 4 * static_cast<int>(li) + 4 * W * s, v.k);
            pr[u] = a;
        }
        slot_totals<W>(pr, li, sc);
        float pm = -INFINITY;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (!valid[u]) sc[u] = -INFINITY;
            pm = fmaxf(pm, max_key(sc[u]));
        }
        if (P && mine) P[first + j0 + li] = li == 0 ? sc[0] : li == 1 ? sc[1] : li == 2 ? sc[2] : sc[3];
        if (pm > st.m) {  // one rescale per pass of what the slot has summed under the old maximum
            const float f = carry(st.m, pm, scale);
            st.l *= f;
#pragma unroll
            for (int s = 0; s < NS; ++s) st.acc[s] = scaled(st.acc[s], f);
            st.m = pm;
        }
        if (st.m != INFINITY) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (valid[u]) {
                    const float tm = term(sc[u], st.m, scale);  // 0 for a masked entry, and for every entry while the maximum is -inf
                    st.l += tm;
#pragma unroll
                    for (int s = 0; s < NS; ++s) axpy(st.acc[s], tm, vv[u][s]);
                }
            }
        }
    }
}

// the states of the 64 / W slots of a wave, merged on every lane: a butterfly over the slots, the lower slot's state first
template <int W, int NS>
__device__ __forceinline__ void merge_slots(State<NS> &st, uint32_t lane, float scale) {
#pragma unroll
    for (int off = W; off < 64; off <<= 1) {
        State<NS> o;
        o.m = __shfl_xor(st.m, off);
        o.l = __shfl_xor(st.l, off);
#pragma unroll
        for (int s = 0; s < NS; ++s) o.acc[s] = shfl_xor4(st.acc[s], off);
        if (lane & static_cast<uint32_t>(off)) {
            merge(o, st, scale);
            st = o;
        } else {
            merge(st, o, scale);
        }
    }
}

// the second sweep of dP: the lane that wrote a raw score reads it back and writes the probability under the row's final (M, L)
__device__ __forceinline__ void write_probs(float *__restrict__ P, uint64_t first, uint32_t len, uint32_t t, uint32_t T, uint32_t n_pass, uint32_t li,
                                            float M, float L, float scale) {
    if (li >= static_cast<uint32_t>(U)) return;
    for (uint32_t pass = 0; pass < n_pass; ++pass) {
        const uint64_t j = (static_cast<uint64_t>(pass) * T + t) * U + li;
        if (j < len) P[first + j] = prob(P[first + j], M, L, scale);
    }
}

// where the waves of a block row meet: (m, l) and the Out row of every wave
template <int W, int NS>
struct Shared {
    float2 ml[kWavesPerBlock];
    alignas(16) float acc[kWavesPerBlock][4 * W * NS];
};

template <int W, int NS, bool VEC>
__device__ __forceinline__ void run_item(const View &v, const uint4 &it, int kind, const float *__restrict__ Q, const float *__restrict__ K,
                                         const float *__restrict__ V, float scale, float *__restrict__ Out, float *__restrict__ P, uint32_t lane, uint32_t w,
                                         Shared<W, NS> &sh) {
    const uint32_t slot = lane / W, li = lane % W;
    const Place pl = place_of<W>(v.rowptr, it, kind, slot, w);
    float4 q[NS];
    State<NS> st;
    st.m = -INFINITY;
    st.l = 0.f;
    const float *qrow = Q + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        q[s] = pl.has_line ? load_cols<VEC>(qrow, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        st.acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    sweep<W, NS, VEC>(v, q, K, V, scale, P, pl.first, pl.len, pl.t, pl.T, pl.n_pass, lane, li, st);
    if (kind != kSlotLine) merge_slots<W, NS>(st, lane, scale);
    bool writer = kind == kSlotLine ? pl.has_line : slot == 0;
    if (kind == kBlockLine) {
        if (slot == 0) {
#pragma unroll
            for (int s = 0; s < NS; ++s) *reinterpret_cast<float4 *>(&sh.acc[w][4 * li + 4 * W * s]) = st.acc[s];
        }
        if (lane == 0) sh.ml[w] = make_float2(st.m, st.l);
        __syncthreads();
        writer = w == 0 && slot == 0;
        State<NS> tot;  // the waves in wave order: every lane folds (m, l), the writing lanes their columns as well
        tot.m = sh.ml[0].x;
        tot.l = sh.ml[0].y;
#pragma unroll
        for (int s = 0; s < NS; ++s) tot.acc[s] = writer ? *reinterpret_cast<const float4 *>(&sh.acc[0][4 * li + 4 * W * s]) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int i = 1; i < kWavesPerBlock; ++i) {
            State<NS> o;
            o.m = sh.ml[i].x;
            o.l = sh.ml[i].y;
#pragma unroll
            for (int s = 0; s < NS; ++s) o.acc[s] = writer ? *reinterpret_cast<const float4 *>(&sh.acc[i][4 * li + 4 * W * s]) : make_float4(0.f, 0.f, 0.f, 0.f);
            merge(tot, o, scale);
        }
        st = tot;
    }
    if (writer) write_row<NS, VEC>(Out + static_cast<size_t>(pl.line) * v.ldc, st, li, W, v.k);
    if (P) write_probs(P, pl.first, pl.len, pl.t, pl.T, pl.n_pass, li, st.m, st.l, scale);
}

// Grid: the block rows first (the longest work starts first), then the workgroups of the wave groups.
template <int W, int NS, bool VEC>
__global__ __launch_bounds__(256) void attention_rows(View v, const float *__restrict__ Q, const float *__restrict__ K, const float *__restrict__ V,
                                                       float scale, float *__restrict__ Out, float *__restrict__ P) {
    __shared__ Shared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        run_item<W, NS, VEC>(v, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Q, K, V, scale, Out, P, lane, w, sh);
        return;
    }
    uint32_t wg = blockIdx.x - v.n_block_rows;
    if (v.xcd_remap) {  // give each XCD one contiguous slice of the groups (the hardware deals workgroups round-robin)
        const uint32_t per = (gridDim.x - v.n_block_rows) / kXcds;
        wg = (wg % kXcds) * per + wg / kXcds;
    }
    const uint32_t grp = wg * kWavesPerBlock + w;
    if (grp >= v.n_groups) return;
    const uint32_t i1 = v.grp[grp + 1];
    for (uint32_t i = v.grp[grp]; i < i1; ++i) {
        const uint4 it = v.item[i];  // {first entry, entries, first row, rows}: the same for every lane
        const int kind = (it.w > 1 || it.y <= kAtSlotRow) ? kSlotLine : kWaveLine;  // internal.h, attention_row_class
        run_item<W, NS, VEC>(v, it, kind, Q, K, V, scale, Out, P, lane, w, sh);
    }
}

int launch_rows(const flex_plan *p, const AttentionPick &pick, const float *Q, const float *K, const float *V, float scale, float *Out, float *P,
                hipStream_t s) {
    const View v = row_view(p);
    const dim3 grid = launch_grid(v), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        if (pick.vec4) hipLaunchKernelGGL((attention_rows<W(), NS(), true>), grid, block, 0, s, v, Q, K, V, scale, Out, P);
        else hipLaunchKernelGGL((attention_rows<W(), NS(), false>), grid, block, 0, s, v, Q, K, V, scale, Out, P);
    });
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex

#include "attention_entry.h"  // the entry points of every attention file: this is their one translation unit in the library
