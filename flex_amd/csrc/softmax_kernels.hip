// softmax_kernels.hip -- the edge softmax of FLEX_PLAN_MUTABLE_VALUES plans (include/flex_spmm.h: flex_edge_softmax,
// flex_edge_softmax_backward): the softmax of one score per entry over each row of hostA, and its gradient.  The walk is built by the
// planner from hostA's row pointer (plan_build.cpp, upload_softmax_image; the classes and constants: internal.h, kSmWindow) and
// verified by flex_plan_self_check (plan_check.cpp).
//
// Not SpMM kernels: a namespace of their own, outside the route table of tests/f64ref.py; tests/test_gpu_attention.py covers them, and
// tests/test_gpu_values_address_limits.py declares a case for each of the four instantiations (softmax_vec, internal.h).
//
// Entry-parallel.  A lane owns 4 consecutive entries of a WINDOW of 256 that starts at a multiple of 4 entries, so where the arrays
// are 16-byte aligned every full quad is one 16-byte access; the quads at the two ends of an item (and every quad of unaligned arrays:
// same lanes, same order, same bits) use 4-byte accesses under a validity mask, so nothing outside the item's entries is read or written.
//   packed item  several short rows in one window.  The lanes that hold the item's rows mark each row's first entry in a byte map in
//                LDS (private to the wave; LDS operations of one wave complete in order), every lane reads the four flags of its
//                quad, and the row maximum and the row sum are SEGMENTED scans over the wave: forward inside the lane and across
//                lanes (6 shuffle steps under the flags), which leaves each row's total at its last entry, and a backward copy scan
//                that hands the total to every entry of the row.  Every entry of a row divides by the same sum.
//   wave row     one row, up to 4 windows, held in registers: one read, the reduction is a butterfly over the wave.
//   block row    one row, a workgroup: wave w takes the chunks (4 windows) w, w + 4, ...; running maximum and rescaled sum per lane,
//                butterfly per wave, the four waves meet in LDS and add their sums in wave order.  Up to 4 chunks stay in registers;
//                a longer row is read again for the write.
// Fixed order everywhere, no atomics: bit-identical run to run, and in place is safe because every entry is read and written by the
// same lane, all reads of a pass before its writes.
#include <cmath>
#include <cstdint>

#include "plan.h"

namespace flex {
namespace softmax {

struct View {
    const uint32_t *rowptr;
    const uint4 *item;
    const uint32_t *grp;
    uint32_t n_groups, n_wave_items, n_block_rows;
    uint32_t xcd_remap;  // the plan's choice: each XCD walks one contiguous slice of the groups (as its SpMM does)
};

struct Quad {
    float v[4];
};

// entries q .. q + 3 of a; an entry outside [first, end) is not read and reads as `fill`.  *mask: bit j = entry q + j is inside
template <bool VEC>
__device__ __forceinline__ Quad load_quad(const float *__restrict__ a, uint64_t q, uint64_t first, uint64_t end, float fill, uint32_t *mask) {
    Quad r{{fill, fill, fill, fill}};
    *mask = 0;
    if (q >= end || q + 4 <= first) return r;
    if (q >= first && end - q >= 4) {
        *mask = 15u;
        if constexpr (VEC) {
            const float4 t = *reinterpret_cast<const float4 *>(a + q);
            r = Quad{{t.x, t.y, t.z, t.w}};
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) r.v[j] = a[q + j];
        }
        return r;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (q + j >= first && q + j < end) {
            r.v[j] = a[q + j];
            *mask |= 1u << j;
        }
    return r;
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float *__restrict__ a, uint64_t q, uint32_t mask, const Quad &r) {
    if (mask == 15u) {
        if constexpr (VEC) {
            *reinterpret_cast<float4 *>(a + q) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[q + j] = r.v[j];
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (mask & (1u << j)) a[q + j] = r.v[j];
}

struct MaxOp {
    __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
};
struct SumOp {
    __device__ __forceinline__ float operator()(float a, float b) const { return a + b; }
};

// The total of its row at every one of the wave's 256 window entries.  head / tail: bit j = the lane's entry j is the first / last of
// its row (an entry outside the item is a row of its own).
template <class Op>
__device__ __forceinline__ void seg_total(Quad &x, uint32_t head, uint32_t tail, uint32_t lane, Op op) {
    // forward: inclusive inside the lane, Kogge-Stone across the lanes on (has a head, value since the last head)
#pragma unroll
    for (int j = 1; j < 4; ++j)
        if (!(head & (1u << j))) x.v[j] = op(x.v[j - 1], x.v[j]);
    {
        int f = head != 0;
        float v = x.v[3];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float vo = __shfl_up(v, d);
            const int fo = __shfl_up(f, d);
            if (lane >= static_cast<uint32_t>(d)) {
                if (!f) v = op(vo, v);
                f |= fo;
            }
        }
        const float carry = __shfl_up(v, 1);  // the row that reaches into this lane, up to the end of the lane before
        if (lane > 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!(head & ((2u << j) - 1u))) x.v[j] = op(carry, x.v[j]);
        }
    }
    // backward: every entry takes the value at the last entry of its row
#pragma unroll
    for (int j = 2; j >= 0; --j)
        if (!(tail & (1u << j))) x.v[j] = x.v[j + 1];
    {
        int t = tail != 0;
        float v = x.v[0];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float vo = __shfl_down(v, d);
            const int to = __shfl_down(t, d);
            if (lane + d < 64u) {
                if (!t) v = vo;
                t |= to;
            }
        }
        const float carry = __shfl_down(v, 1);
        if (lane < 63u) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!(tail >> j)) x.v[j] = carry;
        }
    }
}

// The row-boundary flags of a packed item's window: *head, *tail as seg_total takes them.  `map` is the wave's 256-byte map in LDS.
__device__ __forceinline__ void row_flags(const View &v, const uint4 &it, uint32_t wb, uint32_t mask, uint32_t lane, uint32_t *map,
                                          uint32_t *head, uint32_t *tail) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (!(mask & (1u << j))) w |= 1u << (8 * j);
    map[lane] = w;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned char *bytes = reinterpret_cast<unsigned char *>(map);
    for (uint32_t i = lane; i < it.w; i += 64u) {
        const uint32_t s = v.rowptr[it.z + i], t = v.rowptr[it.z + i + 1];
        if (t > s && s - wb < kSmWindow) bytes[s - wb] = 1;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    w = map[lane];
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint32_t h = (w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u);
    const uint32_t next = __shfl_down(h, 1);
    *head = h;
    *tail = (h >> 1) | (((lane == 63u ? 1u : next) & 1u) << 3);
}

// the score as the row maximum sees it: a NaN or a +inf poisons its row, which is then known by its maximum +inf
__device__ __forceinline__ float max_key(float s) { return (s != s || s == INFINITY) ? INFINITY : s; }
// one term of the row sum under the row maximum m (finite); a masked entry (-inf, also what entries outside the item read as) adds +0
__device__ __forceinline__ float term(float s, float m, float scale) { return s == -INFINITY ? 0.f : expf(scale * (s - m)); }
__device__ __forceinline__ float prob(float t, float m, float sum) { return m == INFINITY ? __builtin_nanf("") : m == -INFINITY ? 0.f : t / sum; }

template <class Op>
__device__ __forceinline__ float wave_all(float x, Op op) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = op(x, __shfl_xor(x, o));
    return x;
}

template <bool VEC>
__device__ __forceinline__ void packed_forward(const View &v, const uint4 &it, const float *__restrict__ s, float scale, float *__restrict__ out,
                                               uint32_t lane, uint32_t *map) {
    const uint32_t wb = it.x & ~3u;
    const uint64_t q = static_cast<uint64_t>(wb) + 4u * lane, end = static_cast<uint64_t>(it.x) + it.y;
    uint32_t mask, head, tail;
    const Quad x = load_quad<VEC>(s, q, it.x, end, -INFINITY, &mask);
    row_flags(v, it, wb, mask, lane, map, &head, &tail);
    Quad m;
#pragma unroll
    for (int j = 0; j < 4; ++j) m.v[j] = max_key(x.v[j]);
    seg_total(m, head, tail, lane, MaxOp());
    Quad t, sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) sum.v[j] = t.v[j] = fabsf(m.v[j]) == INFINITY ? 0.f : term(x.v[j], m.v[j], scale);
    seg_total(sum, head, tail, lane, SumOp());
    Quad p;
#pragma unroll
    for (int j = 0; j < 4; ++j) p.v[j] = prob(t.v[j], m.v[j], sum.v[j]);
    store_quad<VEC>(out, q, mask, p);
}

template <bool VEC>
__device__ __forceinline__ void packed_backward(const View &v, const uint4 &it, const float *__restrict__ p, const float *__restrict__ g, float scale,
                                                float *__restrict__ out, uint32_t lane, uint32_t *map) {
    const uint32_t wb = it.x & ~3u;
    const uint64_t q = static_cast<uint64_t>(wb) + 4u * lane, end = static_cast<uint64_t>(it.x) + it.y;
    uint32_t mask, head, tail;
    const Quad pv = load_quad<VEC>(p, q, it.x, end, 0.f, &mask);
    const Quad gv = load_quad<VEC>(g, q, it.x, end, 0.f, &mask);
    row_flags(v, it, wb, mask, lane, map, &head, &tail);
    Quad dot;
#pragma unroll
    for (int j = 0; j < 4; ++j) dot.v[j] = pv.v[j] * gv.v[j];
    seg_total(dot, head, tail, lane, SumOp());
    Quad r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r.v[j] = (scale * (gv.v[j] - dot.v[j])) * pv.v[j];
    store_quad<VEC>(out, q, mask, r);
}

// One row over `nw` waves (1: a wave row; kWavesPerBlock: a block row, all waves of the workgroup call this): wave `w` takes the chunks
// w, w + nw, ...  `comb`: kWavesPerBlock slots in LDS where the waves of a block row meet.
template <bool VEC>
__device__ __forceinline__ void row_forward(const uint4 &it, const float *__restrict__ s, float scale, float *__restrict__ out, uint32_t lane,
                                            uint32_t w, uint32_t nw, float2 *comb) {
    const uint64_t first = it.x, end = first + it.y, wb = first & ~3ull;
    const uint64_t n_chunks = (end - wb + kSmChunk - 1) / kSmChunk;
    float m = -INFINITY, l = 0.f;
    Quad x[4];
    uint32_t mask[4];
    for (uint64_t c = w; c < n_chunks; c += nw) {
        const uint64_t base = wb + c * kSmChunk + 4u * lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = load_quad<VEC>(s, base + i * kSmWindow, first, end, -INFINITY, &mask[i]);
        float cm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) cm = fmaxf(cm, max_key(x[i].v[j]));
        if (cm > m) {  // rescale what the lane has summed under the old maximum
            l = m == -INFINITY ? 0.f : l * expf(scale * (m - cm));
            m = cm;
        }
        if (fabsf(m) != INFINITY) {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) l += term(x[i].v[j], m, scale);
        }
    }
    float M = wave_all(m, MaxOp());
    float L = wave_all((fabsf(M) == INFINITY || m == -INFINITY) ? 0.f : l * expf(scale * (m - M)), SumOp());
    if (nw > 1) {
        if (lane == 0) comb[w] = make_float2(M, L);
        __syncthreads();
        float2 part[kWavesPerBlock];
        M = -INFINITY;
#pragma unroll
        for (int i = 0; i < kWavesPerBlock; ++i) {
            part[i] = comb[i];
            M = fmaxf(M, part[i].x);
        }
        L = 0.f;
#pragma unroll
        for (int i = 0; i < kWavesPerBlock; ++i)
            if (fabsf(M) != INFINITY && part[i].x != -INFINITY) L += part[i].y * expf(scale * (part[i].x - M));
    }
    const bool in_regs = n_chunks <= nw;  // the lane still holds its only chunk
    for (uint64_t c = w; c < n_chunks; c += nw) {
        const uint64_t base = wb + c * kSmChunk + 4u * lane;
        if (!in_regs) {
#pragma unroll
            for (int i = 0; i < 4; ++i) x[i] = load_quad<VEC>(s, base + i * kSmWindow, first, end, -INFINITY, &mask[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Quad p;
#pragma unroll
            for (int j = 0; j < 4; ++j) p.v[j] = prob(fabsf(M) == INFINITY ? 0.f : term(x[i].v[j], M, scale), M, L);
            store_quad<VEC>(out, base + i * kSmWindow, mask[i], p);
        }
    }
}

template <bool VEC>
__device__ __forceinline__ void row_backward(const uint4 &it, const float *__restrict__ p, const float *__restrict__ g, float scale,
                                             float *__restrict__ out, uint32_t lane, uint32_t w, uint32_t nw, float2 *comb) {
    const uint64_t first = it.x, end = first + it.y, wb = first & ~3ull;
    const uint64_t n_chunks = (end - wb + kSmChunk - 1) / kSmChunk;
    float acc = 0.f;
    Quad pv[4], gv[4];
    uint32_t mask[4];
    for (uint64_t c = w; c < n_chunks; c += nw) {
        const uint64_t base = wb + c * kSmChunk + 4u * lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            pv[i] = load_quad<VEC>(p, base + i * kSmWindow, first, end, 0.f, &mask[i]);
            gv[i] = load_quad<VEC>(g, base + i * kSmWindow, first, end, 0.f, &mask[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_fmaf(pv[i].v[j], gv[i].v[j], acc);
    }
    float dot = wave_all(acc, SumOp());
    if (nw > 1) {
        if (lane == 0) comb[w] = make_float2(dot, 0.f);
        __syncthreads();
        dot = 0.f;
#pragma unroll
        for (int i = 0; i < kWavesPerBlock; ++i) dot += comb[i].x;
    }
    const bool in_regs = n_chunks <= nw;
    for (uint64_t c = w; c < n_chunks; c += nw) {
        const uint64_t base = wb + c * kSmChunk + 4u * lane;
        if (!in_regs) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                pv[i] = load_quad<VEC>(p, base + i * kSmWindow, first, end, 0.f, &mask[i]);
                gv[i] = load_quad<VEC>(g, base + i * kSmWindow, first, end, 0.f, &mask[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            Quad r;
#pragma unroll
            for (int j = 0; j < 4; ++j) r.v[j] = (scale * (gv[i].v[j] - dot)) * pv[i].v[j];
            store_quad<VEC>(out, base + i * kSmWindow, mask[i], r);
        }
    }
}

// Grid: the block rows first (the longest work starts first), then the workgroups of the wave groups.  BWD: a = p, b = grad p.
template <bool VEC, bool BWD>
__global__ __launch_bounds__(256) void edge_softmax_rows(View v, const float *__restrict__ a, const float *__restrict__ b, float scale,
                                                          float *__restrict__ out) {
    __shared__ uint32_t map[kWavesPerBlock][64];
    __shared__ float2 comb[kWavesPerBlock];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        const uint4 it = v.item[v.n_wave_items + blockIdx.x];
        if constexpr (BWD) row_backward<VEC>(it, a, b, scale, out, lane, w, kWavesPerBlock, comb);
        else row_forward<VEC>(it, a, scale, out, lane, w, kWavesPerBlock, comb);
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
        const bool packed = it.x % 4u + static_cast<uint64_t>(it.y) <= kSmWindow;  // internal.h, softmax_row_class
        if constexpr (BWD) {
            if (packed) packed_backward<VEC>(v, it, a, b, scale, out, lane, map[w]);
            else row_backward<VEC>(it, a, b, scale, out, lane, 0u, 1u, comb);
        } else {
            if (packed) packed_forward<VEC>(v, it, a, scale, out, lane, map[w]);
            else row_forward<VEC>(it, a, scale, out, lane, 0u, 1u, comb);
        }
    }
}

static int launch(const flex_plan *p, bool bwd, const float *a, const float *b, float scale, float *out, flex_stream_t stream) {
    if (!p || !p->mutable_vals) return FLEX_ERR_INVALID;
    if (!p->sm_ok) return FLEX_ERR_UNSUPPORTED;
    if (!std::isfinite(scale) || !(scale > 0.f)) return FLEX_ERR_INVALID;
    if (p->sm_entries == 0) return FLEX_OK;
    if (!a || !out || (bwd && !b)) return FLEX_ERR_INVALID;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const View v{p->d_sm_rowptr.get(), p->d_sm_item.get(), p->d_sm_grp.get(), p->n_sm_groups, p->n_sm_wave_items, p->n_sm_block_rows, p->xcd_remap ? 1u : 0u};
    uint32_t wgs = (p->n_sm_groups + kWavesPerBlock - 1) / kWavesPerBlock;
    if (v.xcd_remap) wgs = (wgs + kXcds - 1) / kXcds * kXcds;
    const dim3 grid(p->n_sm_block_rows + wgs), block(64 * kWavesPerBlock);
    const bool vec = softmax_vec(a, b, out);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (bwd && vec) hipLaunchKernelGGL((edge_softmax_rows<true, true>), grid, block, 0, s, v, a, b, scale, out);
    else if (bwd) hipLaunchKernelGGL((edge_softmax_rows<false, true>), grid, block, 0, s, v, a, b, scale, out);
    else if (vec) hipLaunchKernelGGL((edge_softmax_rows<true, false>), grid, block, 0, s, v, a, b, scale, out);
    else hipLaunchKernelGGL((edge_softmax_rows<false, false>), grid, block, 0, s, v, a, b, scale, out);
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // namespace softmax
}  // namespace flex

extern "C" {

int flex_edge_softmax(const flex_plan *p, const float *dScores, float scale, float *dOut, flex_stream_t stream) {
    return flex::softmax::launch(p, false, dScores, nullptr, scale, dOut, stream);
}

int flex_edge_softmax_backward(const flex_plan *p, const float *dP, const float *dGradP, float scale, float *dGradS, flex_stream_t stream) {
    return flex::softmax::launch(p, true, dP, dGradP, scale, dGradS, stream);
}

}  // extern "C"
