// attention_device.h -- what the kernels of the fused attention share on the device: the views of the row walk and of the column walk,
// the column, dot, axpy and slot-reduction helpers, the forward's softmax state, the backward's plain sums, the one slot placement of all
// nine kernels (place_of) and the head split of the per-head kernels.  Used by attention_kernels.hip (flex_attention),
// attention_backward_kernels.hip (flex_attention_backward), attention_heads_kernels.hip and attention_bf16_kernels.hip (their multi-head
// forms in fp32 and in bf16, through attention_heads_device.h) and attention_gat_kernels.hip (the GAT forms); what their entry points
// share on the host is attention_host.h.
#pragma once
#include <cmath>
#include <cstdint>

#include "internal.h"

namespace flex {
namespace attention {

struct View {
    const uint32_t *rowptr;  // the plan's rows, entries as hostA numbers them
    const uint32_t *src;     // K / V row of entry e at src[e - e0]
    const uint4 *item;
    const uint32_t *grp;
    uint32_t e0;
    uint32_t n_groups, n_wave_items, n_block_rows;
    uint32_t xcd_remap;
    int32_t k, ldb, ldc;
};

constexpr int U = static_cast<int>(kAtPass);
static_assert(U == 4, "the slot reduction below hands four scores to every lane");

// columns c .. c + 3 of a row; a column at or past k is not read and reads as 0
template <bool VEC>
__device__ __forceinline__ float4 load_cols(const float *__restrict__ row, int c, int k) {
    if constexpr (VEC) {
        if (c < k) return *reinterpret_cast<const float4 *>(row + c);
        return make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < k) r.x = row[c];
        if (c + 1 < k) r.y = row[c + 1];
        if (c + 2 < k) r.z = row[c + 2];
        if (c + 3 < k) r.w = row[c + 3];
        return r;
    }
}

template <bool VEC>
__device__ __forceinline__ void store_cols(float *__restrict__ row, int c, int k, const float4 &x) {
    if constexpr (VEC) {
        if (c < k) *reinterpret_cast<float4 *>(row + c) = x;
    } else {
        if (c < k) row[c] = x.x;
        if (c + 1 < k) row[c + 1] = x.y;
        if (c + 2 < k) row[c + 2] = x.z;
        if (c + 3 < k) row[c + 3] = x.w;
    }
}

// The same four columns of a row of flex_bf16 (the upper 16 bits of a float each), as the fp32 numbers they are: one 8-byte load,
// widened by shifts.  Only the vector form is built: the row and c are multiples of four elements.
template <bool VEC>
__device__ __forceinline__ float4 load_cols(const flex_bf16 *__restrict__ row, int c, int k) {
    static_assert(VEC, "bf16 rows have the 8-byte form only");
    if (c >= k) return make_float4(0.f, 0.f, 0.f, 0.f);
    const uint2 r = *reinterpret_cast<const uint2 *>(row + c);
    return make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xFFFF0000u), __uint_as_float(r.y << 16), __uint_as_float(r.y & 0xFFFF0000u));
}

// fp32 to bf16, round to nearest even; +-inf stays, what rounds past the largest finite bf16 becomes +-inf, a NaN stays a (quiet) NaN
__device__ __forceinline__ uint32_t bf16_bits(float x) {
    const uint32_t u = __float_as_uint(x);
    return x != x ? (u >> 16) | 0x40u : (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// four fp32 narrowed to flex_bf16 and stored by one 8-byte store: the one rounding of an output element
template <bool VEC>
__device__ __forceinline__ void store_cols(flex_bf16 *__restrict__ row, int c, int k, const float4 &x) {
    static_assert(VEC, "bf16 rows have the 8-byte form only");
    if (c < k) *reinterpret_cast<uint2 *>(row + c) = make_uint2(bf16_bits(x.x) | (bf16_bits(x.y) << 16), bf16_bits(x.z) | (bf16_bits(x.w) << 16));
}

// sum over the lane's columns of q * b; columns at or past k add nothing (not even 0 x b)
template <bool VEC>
__device__ __forceinline__ float dot_cols(float acc, const float4 &q, const float4 &b, int c, int k) {
    if (c < k) acc = __builtin_fmaf(q.x, b.x, acc);
    if (VEC ? c < k : c + 1 < k) acc = __builtin_fmaf(q.y, b.y, acc);  // VEC: k % 4 == 0, the four columns stand or fall together
    if (VEC ? c < k : c + 2 < k) acc = __builtin_fmaf(q.z, b.z, acc);
    if (VEC ? c < k : c + 3 < k) acc = __builtin_fmaf(q.w, b.w, acc);
    return acc;
}

// acc += t * v on the lane's columns; columns at or past k hold v = 0 and stay 0
__device__ __forceinline__ void axpy(float4 &acc, float t, const float4 &v) {
    acc.x = __builtin_fmaf(t, v.x, acc.x);
    acc.y = __builtin_fmaf(t, v.y, acc.y);
    acc.z = __builtin_fmaf(t, v.z, acc.z);
    acc.w = __builtin_fmaf(t, v.w, acc.w);
}
__device__ __forceinline__ float4 scaled(const float4 &a, float f) { return make_float4(a.x * f, a.y * f, a.z * f, a.w * f); }
__device__ __forceinline__ float4 shfl_xor4(const float4 &a, int off) {
    return make_float4(__shfl_xor(a.x, off), __shfl_xor(a.y, off), __shfl_xor(a.z, off), __shfl_xor(a.w, off));
}

// The four totals of the four per-lane partial sums over the W lanes of a slot, on every lane: the SDDMM's transposed reduction (two
// exchange steps leave each lane one record), a butterfly over the rest, and two exchange steps back.  Every addition has the same two
// operands on both lanes of its pair, so all lanes of the slot hold the same bits.
template <int W>
__device__ __forceinline__ void slot_totals(const float (&pr)[U], uint32_t li, float (&s)[U]) {
    const bool hi2 = (li & (W / 2)) != 0, hi4 = (li & (W / 4)) != 0;
    const float a0 = (hi2 ? pr[2] : pr[0]) + __shfl_xor(hi2 ? pr[0] : pr[2], W / 2);
    const float a1 = (hi2 ? pr[3] : pr[1]) + __shfl_xor(hi2 ? pr[1] : pr[3], W / 2);
    float t = (hi4 ? a1 : a0) + __shfl_xor(hi4 ? a0 : a1, W / 4);  // record 2 hi2 + hi4
#pragma unroll
    for (int o = W / 8; o >= 1; o >>= 1) t += __shfl_xor(t, o);
    const float x = __shfl_xor(t, W / 4);  // record 2 hi2 + !hi4
    const float even = hi4 ? x : t, odd = hi4 ? t : x;
    const float oe = __shfl_xor(even, W / 2), oo = __shfl_xor(odd, W / 2);
    s[0] = hi2 ? oe : even;
    s[1] = hi2 ? oo : odd;
    s[2] = hi2 ? even : oe;
    s[3] = hi2 ? odd : oo;
}

// ---- the forward's softmax state (attention_kernels.hip, attention_heads_kernels.hip)

// as softmax_kernels.hip: the score as the row maximum sees it, a term of the row sum under the finite maximum m, the probability
__device__ __forceinline__ float max_key(float s) { return (s != s || s == INFINITY) ? INFINITY : s; }
__device__ __forceinline__ float term(float s, float m, float scale) { return s == -INFINITY ? 0.f : expf(scale * (s - m)); }
__device__ __forceinline__ float prob(float s, float m, float sum, float scale) {
    return m == INFINITY ? __builtin_nanf("") : m == -INFINITY ? 0.f : term(s, m, scale) / sum;
}
// the factor that carries a state from its maximum m to the maximum M >= m of a merge (M finite or -inf)
__device__ __forceinline__ float carry(float m, float M, float scale) { return m == -INFINITY ? 0.f : expf(scale * (m - M)); }

template <int NS>
struct State {
    float m, l;
    float4 acc[NS];
};

// a <- a merged with b, `a` being the state that comes first in the fixed order
template <int NS>
__device__ __forceinline__ void merge(State<NS> &a, const State<NS> &b, float scale) {
    const float M = fmaxf(a.m, b.m);
    if (M == INFINITY) {
        a.m = INFINITY;
        return;
    }
    const float fa = carry(a.m, M, scale), fb = carry(b.m, M, scale);
    a.m = M;
    a.l = __builtin_fmaf(b.l, fb, a.l * fa);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float4 x = scaled(a.acc[s], fa);
        axpy(x, fb, b.acc[s]);
        a.acc[s] = x;
    }
}

// the Out row of a final state: NaN on a poisoned row, the sums as they are where no entry is live
template <int NS, bool VEC, class E>
__device__ __forceinline__ void write_row(E *__restrict__ orow, const State<NS> &st, uint32_t li, int W, int k) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        float4 o;
        if (st.m == INFINITY) {
            const float nan = __builtin_nanf("");
            o = make_float4(nan, nan, nan, nan);
        } else if (st.m == -INFINITY) {
            o = st.acc[s];  // no live entry: +0, or what 0 x a non-finite V left
        } else {
            o = make_float4(st.acc[s].x / st.l, st.acc[s].y / st.l, st.acc[s].z / st.l, st.acc[s].w / st.l);
        }
        store_cols<VEC>(orow, 4 * static_cast<int>(li) + 4 * W * s, k, o);
    }
}

// ---- the backward's column view and plain sums, and the ownership of a line in every kernel

struct ColumnView {
    const uint32_t *colptr;  // first position of every column in ent
    const uint2 *ent;        // {row, entry index}, by column, CSR order within a column
    const uint4 *item;
    const uint32_t *grp;
    uint32_t n_groups, n_wave_items, n_block_cols;
    uint32_t xcd_remap;
    int32_t k, ldb, ldc;
};

// how a line (a row of View, a column of ColumnView) is owned: internal.h, attention_row_class
enum LineKind : int { kSlotLine = 0, kWaveLine = 1, kBlockLine = 2 };

__device__ __forceinline__ float4 add4(const float4 &a, const float4 &b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// a <- the sum of the rows `a` of the 64 / W slots of a wave, on every lane: a butterfly over the slots, the lower slot's row first
template <int W, int NS>
__device__ __forceinline__ void sum_slots(float4 (&a)[NS], uint32_t lane) {
#pragma unroll
    for (int off = W; off < 64; off <<= 1) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float4 o = shfl_xor4(a[s], off);
            a[s] = (lane & static_cast<uint32_t>(off)) ? add4(o, a[s]) : add4(a[s], o);
        }
    }
}

// a <- the sum of the scalars `a` of the 64 / W slots of a wave, on every lane: a butterfly over the slots, the lower slot's first
template <int W, int NS>
__device__ __forceinline__ void sum_slot_scalars(float (&a)[NS], uint32_t lane) {
#pragma unroll
    for (int off = W; off < 64; off <<= 1) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float o = __shfl_xor(a[s], off);
            a[s] = (lane & static_cast<uint32_t>(off)) ? o + a[s] : a[s] + o;
        }
    }
}

// The slot's line (a row of a row kernel, a column of a column kernel), its entries and its place in the team that shares the line: member
// t of a team of T slots takes the passes t, t + T, ... of kAtPass entries.  n_pass is the same for every lane of the wave (a slot past
// its line's end idles under a predicate), so every shuffle of a sweep is wave-wide.  ptr is the row pointer or the column pointer.
struct Place {
    uint32_t line, len, t, T, n_pass;
    uint64_t first;
    bool has_line;
};
template <int W>
__device__ __forceinline__ Place place_of(const uint32_t *__restrict__ ptr, const uint4 &it, int kind, uint32_t slot, uint32_t w) {
    constexpr uint32_t S = 64 / W;
    Place pl{it.z, it.y, slot, S, 0u, it.x, true};
    if (kind == kSlotLine) {
        pl.has_line = slot < it.w;
        pl.line = it.z + (pl.has_line ? slot : 0u);
        pl.first = ptr[pl.line];
        pl.len = pl.has_line ? ptr[pl.line + 1] - ptr[pl.line] : 0u;
        pl.t = 0;
        pl.T = 1;
        uint32_t mx = (pl.len + U - 1) / U;
#pragma unroll
        for (int o = 32; o >= W; o >>= 1) {
            const uint32_t other = static_cast<uint32_t>(__shfl_xor(static_cast<int>(mx), o));
            mx = other > mx ? other : mx;
        }
        pl.n_pass = mx;
    } else {
        if (kind == kBlockLine) {
            pl.t = w * S + slot;
            pl.T = kWavesPerBlock * S;
        }
        pl.n_pass = static_cast<uint32_t>((static_cast<uint64_t>(pl.len) + static_cast<uint64_t>(pl.T) * U - 1) / (static_cast<uint64_t>(pl.T) * U));
    }
    return pl;
}

// ---- the head split of the per-head kernels (attention_heads_kernels.hip, attention_gat_kernels.hip)

// how the lanes of a slot split into heads: lg = log2(HW); H floats per entry in the edge arrays (and per row in GAT's el / er)
struct HeadSplit {
    int32_t H, lg;
};

// what a lane knows about its place in its head: r = its index among the head's lanes, wm = the mask of the writer rule: of the HW lanes
// of a head, lane r writes entry u of a pass where u == r (HW >= 4) or u % HW == r (HW = 1, 2)
struct HeadLane {
    uint32_t hw, r, wm;
    __device__ __forceinline__ HeadLane(const HeadSplit &hs, uint32_t li) : hw(1u << hs.lg), r(li & (hw - 1u)), wm((hw < static_cast<uint32_t>(U) ? hw : static_cast<uint32_t>(U)) - 1u) {}
    __device__ __forceinline__ bool writes(int u) const { return (static_cast<uint32_t>(u) & wm) == r; }
};

// what a lane knows of its columns per slab: the head they belong to and whether they lie below k
template <int W, int NS>
struct LaneHeads {
    uint32_t head[NS];
    bool live[NS];
    __device__ __forceinline__ LaneHeads(const HeadSplit &hs, uint32_t li, int k) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            head[s] = (li + static_cast<uint32_t>(W * s)) >> hs.lg;
            live[s] = 4 * static_cast<int>(li) + 4 * W * s < k;
        }
    }
};

// The sum of x over the hw lanes of the lane's head, on every one of them: a butterfly from the widest step down -- the tree of
// slot_totals<hw>.  Both lanes of a pair add the same two operands, so all lanes of the head hold the same bits.  hw is the same for the
// whole wave: every shuffle is wave-wide.
template <int W>
__device__ __forceinline__ float head_total(float x, uint32_t hw) {
#pragma unroll
    for (int o = W / 2; o >= 1; o >>= 1) {
        if (static_cast<uint32_t>(o) < hw) x += __shfl_xor(x, o);
    }
    return x;
}

// the per-slab states of the 64 / W slots of a wave, merged on every lane: a butterfly over the slots, the lower slot's state first
template <int W, int NS>
__device__ __forceinline__ void merge_slots_heads(State<1> (&st)[NS], uint32_t lane, float scale) {
#pragma unroll
    for (int off = W; off < 64; off <<= 1) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            State<1> o;
            o.m = __shfl_xor(st[s].m, off);
            o.l = __shfl_xor(st[s].l, off);
            o.acc[0] = shfl_xor4(st[s].acc[0], off);
            if (lane & static_cast<uint32_t>(off)) {
                merge(o, st[s], scale);
                st[s] = o;
            } else {
                merge(st[s], o, scale);
            }
        }
    }
}

// where the waves of a block row meet: (m, l) of every group of four columns (the lanes of a head hold the same pair) and the Out rows
template <int W, int NS>
struct HeadsShared {
    float2 ml[kWavesPerBlock][W * NS];
    alignas(16) float acc[kWavesPerBlock][4 * W * NS];
};

}  // namespace attention
}  // namespace flex
