// attention_backward_kernels.hip -- the fused attention backward of FLEX_PLAN_ATTENTION_BACKWARD plans (include/flex_spmm.h:
// flex_attention_backward): from the probabilities p that flex_attention kept and the gradient g in Out, the gradients in Q, K and V in
// two launches, without the value refresh, the two transposed SpMMs and two of the three nnz-sized vectors of the chain
// flex_plan_set_values / flex_spmm / flex_sddmm / flex_edge_softmax_backward.  tests/test_gpu_fused_attention_backward.py covers it, the
// 16-byte and the generic form of every (W, NS), each kernel alone as well: the cases are tests/attention_forms.py's, and
// tests/test_attention_routes.py holds every instantiation to a case that launches it.
//
// Row kernel (attention_rows_backward): the forward's walk, slots, waves and blocks (attention_device.h; internal.h, kAtPass).  A slot
// holds its g row in registers and sweeps its share of the row twice, so that every entry gathers its V row once and its K row once:
//   sweep 1   per pass the four V rows are gathered, da_e = <g[r], V[src(e)]> is reduced across the slot as the forward's scores are,
//             lane u of the slot writes da of entry u to dWork, and delta += p_e da_e by fma in entry order; delta is then summed over
//             the slots of the wave (a butterfly, lower slot first) and over the waves (LDS, wave order)
//   sweep 2   the lane that wrote da_e reads it back with p_e, forms ds_e = scale p_e (da_e - delta) and overwrites dWork with it; the
//             four K rows are gathered and gQ += ds_e K[src(e)] by fma; the partial gQ rows merge as delta did
// No expf, no running maximum, no rescale: the sums are plain.
// Column kernel (attention_columns_backward): the same classes, items and groups over the COLUMNS of hostA (the second part of the
// image: plan_build.cpp, upload_attention_image).  A slot owns column c and holds two accumulator rows, gK[c] and gV[c]; per pass its
// first four lanes load {row, entry} of four entries and broadcast them, p[e] and ds[e] are loaded per entry, the four g rows and the
// four Q rows are gathered together, and eight axpys follow.  No lane meets another inside a slot; the slots of a wave and the waves
// of a workgroup merge by plain sums, lower slot first, waves in wave order.  Within a column the entries are in hostA's CSR order.
// Fixed order everywhere, no atomics.
#include <cmath>
#include <cstdint>

#include "attention_host.h"

namespace flex {
namespace attention {

// ---- the row kernel

template <int W, int NS>
struct RowShared {
    float delta[kWavesPerBlock];
    alignas(16) float acc[kWavesPerBlock][4 * W * NS];
};

template <int W, int NS, bool VEC>
__device__ __forceinline__ void run_row(const View &v, const uint4 &it, int kind, const float *__restrict__ K, const float *__restrict__ V,
                                        const float *__restrict__ P, const float *__restrict__ G, float scale, float *__restrict__ GQ,
                                        float *__restrict__ Work, uint32_t lane, uint32_t w, RowShared<W, NS> &sh) {
    const uint32_t slot = lane / W, li = lane % W;
    const int slot_lane0 = static_cast<int>(lane - li);
    const Place pl = place_of<W>(v.rowptr, it, kind, slot, w);
    float4 g[NS];
    const float *grow = G + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
    for (int s = 0; s < NS; ++s) g[s] = pl.has_line ? load_cols<VEC>(grow, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
    // sweep 1: da into dWork, delta
    float delta = 0.f;
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
        const float pe = mine ? P[pl.first + j0 + li] : 0.f;
        bool valid[U];
        float4 vv[U][NS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const float *vr = V + static_cast<size_t>(col) * v.ldb;
#pragma unroll
            for (int s = 0; s < NS; ++s) vv[u][s] = valid[u] ? load_cols<VEC>(vr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float pr[U], da[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float a = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s) a = dot_cols<VEC>(a, g[s], vv[u][s], 4 * static_cast<int>(li) + 4 * W * s, v.k);
            pr[u] = a;
        }
        slot_totals<W>(pr, li, da);
        if (mine) Work[pl.first + j0 + li] = li == 0 ? da[0] : li == 1 ? da[1] : li == 2 ? da[2] : da[3];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float pu = __shfl(pe, slot_lane0 + u);
            if (valid[u]) delta = __builtin_fmaf(pu, da[u], delta);
        }
    }
    if (kind != kSlotLine) {
#pragma unroll
        for (int off = W; off < 64; off <<= 1) {
            const float o = __shfl_xor(delta, off);
            delta = (lane & static_cast<uint32_t>(off)) ? o + delta : delta + o;
        }
    }
    if (kind == kBlockLine) {
        if (lane == 0) sh.delta[w] = delta;
        __syncthreads();
        delta = sh.delta[0];
#pragma unroll
        for (int i = 1; i < kWavesPerBlock; ++i) delta += sh.delta[i];
    }
    // sweep 2: ds over da in dWork, gQ
    float4 acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (uint32_t pass = 0; pass < pl.n_pass; ++pass) {
        const uint64_t j0 = (static_cast<uint64_t>(pass) * pl.T + pl.t) * U;
        const bool mine = li < static_cast<uint32_t>(U) && j0 + li < pl.len;
        float dse = 0.f;
        if (mine) {
            const uint64_t e = pl.first + j0 + li;
            const float d = Work[e] - delta;
            dse = (scale * P[e]) * d;
            Work[e] = dse;
        }
        if (!GQ) continue;
        const uint32_t idx = mine ? v.src[pl.first - v.e0 + j0 + li] : 0u;
        bool valid[U];
        float4 kv[U][NS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t col = __shfl(idx, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            const float *kr = K + static_cast<size_t>(col) * v.ldb;
#pragma unroll
            for (int s = 0; s < NS; ++s) kv[u][s] = valid[u] ? load_cols<VEC>(kr, 4 * static_cast<int>(li) + 4 * W * s, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float d = __shfl(dse, slot_lane0 + u);
            if (valid[u]) {
#pragma unroll
                for (int s = 0; s < NS; ++s) axpy(acc[s], d, kv[u][s]);
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
        float *orow = GQ + static_cast<size_t>(pl.line) * v.ldc;
#pragma unroll
        for (int s = 0; s < NS; ++s) store_cols<VEC>(orow, 4 * static_cast<int>(li) + 4 * W * s, v.k, acc[s]);
    }
}

// Grid: as attention_rows -- the block rows first, then the workgroups of the wave groups.
template <int W, int NS, bool VEC>
__global__ __launch_bounds__(256) void attention_rows_backward(View v, const float *__restrict__ K, const float *__restrict__ V, const float *__restrict__ P,
                                                                const float *__restrict__ G, float scale, float *__restrict__ GQ, float *__restrict__ Work) {
    __shared__ RowShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_rows) {
        run_row<W, NS, VEC>(v, v.item[v.n_wave_items + blockIdx.x], kBlockLine, K, V, P, G, scale, GQ, Work, lane, w, sh);
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
        run_row<W, NS, VEC>(v, it, kind, K, V, P, G, scale, GQ, Work, lane, w, sh);
    }
}

// ---- the column kernel

template <int W, int NS>
struct ColumnShared {
    alignas(16) float acc[2][kWavesPerBlock][4 * W * NS];
};

template <int W, int NS, bool VEC>
__device__ __forceinline__ void run_column(const ColumnView &v, const uint4 &it, int kind, const float *__restrict__ Q, const float *__restrict__ G,
                                           const float *__restrict__ P, const float *__restrict__ DS, float *__restrict__ GK, float *__restrict__ GV,
                                           uint32_t lane, uint32_t w, ColumnShared<W, NS> &sh) {
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
        float pe[U], de[U];
        float4 gg[U][NS], qq[U][NS];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t row = __shfl(re.x, slot_lane0 + u), e = __shfl(re.y, slot_lane0 + u);
            valid[u] = j0 + u < pl.len;
            pe[u] = (GV && valid[u]) ? P[e] : 0.f;
            de[u] = (GK && valid[u]) ? DS[e] : 0.f;
            const float *gr = G + static_cast<size_t>(row) * v.ldc, *qr = Q + static_cast<size_t>(row) * v.ldc;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int c = 4 * static_cast<int>(li) + 4 * W * s;
                gg[u][s] = (GV && valid[u]) ? load_cols<VEC>(gr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
                qq[u][s] = (GK && valid[u]) ? load_cols<VEC>(qr, c, v.k) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (valid[u]) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    axpy(av[s], pe[u], gg[u][s]);
                    axpy(ak[s], de[u], qq[u][s]);
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
            if (GK) store_cols<VEC>(GK + static_cast<size_t>(pl.line) * v.ldb, c, v.k, ak[s]);
            if (GV) store_cols<VEC>(GV + static_cast<size_t>(pl.line) * v.ldb, c, v.k, av[s]);
        }
    }
}

template <int W, int NS, bool VEC>
__global__ __launch_bounds__(256) void attention_columns_backward(ColumnView v, const float *__restrict__ Q, const float *__restrict__ G,
                                                                   const float *__restrict__ P, const float *__restrict__ DS, float *__restrict__ GK,
                                                                   float *__restrict__ GV) {
    __shared__ ColumnShared<W, NS> sh;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (blockIdx.x < v.n_block_cols) {
        run_column<W, NS, VEC>(v, v.item[v.n_wave_items + blockIdx.x], kBlockLine, Q, G, P, DS, GK, GV, lane, w, sh);
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
        const uint4 it = v.item[i];  // {first position, entries, first column, columns}
        const int kind = (it.w > 1 || it.y <= kAtSlotRow) ? kSlotLine : kWaveLine;
        run_column<W, NS, VEC>(v, it, kind, Q, G, P, DS, GK, GV, lane, w, sh);
    }
}

int launch_rows_backward(const flex_plan *p, const AttentionPick &pick, const float *K, const float *V, const float *P, const float *G, float scale,
                         float *GQ, float *Work, hipStream_t s) {
    const View rv = row_view(p);
    const dim3 rgrid = launch_grid(rv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        if (pick.vec4) hipLaunchKernelGGL((attention_rows_backward<W(), NS(), true>), rgrid, block, 0, s, rv, K, V, P, G, scale, GQ, Work);
        else hipLaunchKernelGGL((attention_rows_backward<W(), NS(), false>), rgrid, block, 0, s, rv, K, V, P, G, scale, GQ, Work);
    });
    return FLEX_OK;
}

int launch_columns_backward(const flex_plan *p, const AttentionPick &pick, const float *Q, const float *G, const float *P, const float *DS, float *GK,
                            float *GV, hipStream_t s) {
    const ColumnView cv = column_view(p);
    const dim3 cgrid = launch_grid(cv), block(64 * kWavesPerBlock);
    dispatch(pick, [&](auto W, auto NS) {
        if (pick.vec4) hipLaunchKernelGGL((attention_columns_backward<W(), NS(), true>), cgrid, block, 0, s, cv, Q, G, P, DS, GK, GV);
        else hipLaunchKernelGGL((attention_columns_backward<W(), NS(), false>), cgrid, block, 0, s, cv, Q, G, P, DS, GK, GV);
    });
    return FLEX_OK;
}

}  // namespace attention
}  // namespace flex
