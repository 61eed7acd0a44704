// axw_bf16_fused_kernels.hip -- order FLEX_AXW_AX_W_FUSED of the bf16 layer (libflex_axw.so): the gather of A X and the MFMA
// product with W in ONE launch, T = rn_bf16(A X) living only in LDS:
//     Out = rn_bf16( rn_bf16(A X) W )                       kPlain
//     Out = rn_bf16( act( b + rn_bf16(A X) W + X R ) )      kRoot (act = identity), kRelu, kDrop (ReLU, then dropout)
// How the work is split:
//   * a panel is 32 rows of A (the MFMA's N), listed in panel_rows in the handle's row order; the last panel repeats a row id, so no load
//     or store carries a row guard (the repeated rows are computed and stored twice, with the same bits).
//   * one persistent workgroup of 8 waves a CU owns a contiguous range of panels.  The ranges are cut by cost (nonzeros plus a fixed term
//     a row, prefix-summed at create): workgroup b finds [cut(b), cut(b + 1)), cut(b) = the first panel whose prefix reaches
//     cost_total b / gridDim.x, by binary search in the kernel -- any grid size is valid, nothing is uploaded per call, no atomics.
//   * W (and R behind it, as k-steps dim / 16 .. 2 dim / 16 - 1) is staged once per workgroup into LDS as MFMA fragments in stage_w's
//     layout, read from the caller's unpadded [dim x c] array with the columns >= c staged as zero: no pad copy, no pack launch.
//   * gather: each wave takes 4 rows of the panel.  A row of X is read coalesced by dim / V lanes of V = 8 elements (16 bytes; V = 4 at
//     dim <= 64, so that 4 rows still fill a wave), 64-bit row offsets; the lane groups of a wave run different rows side by side and a
//     lane keeps 2 kFlight = 16 nonzeros in flight.  Every output element is ONE fmaf(val, x, acc) chain from +0 over the row's nonzeros in CSR
//     order, rounded once (bf16_bits) into the LDS tile [32][dim], rows 2 dim + 16 bytes apart: an odd number of 16-byte units, so the
//     MFMA phase's 16-byte reads -- lane (j, h) reads [row j][16 s + 8 h .. + 7] -- fall on distinct banks across 16 rows.
//   * a row with more than kLongRow = 512 nonzeros is gathered by the whole workgroup: wave w takes the w-th ascending eighth of the
//     row's nonzeros (one chain each, 8 bytes a lane), the 8 fp32 partial rows go through LDS and are added in wave order, then rounded.
//     A fixed order: two calls give the same bits.  512 keeps the rows a wave gathers alone at no more than 64 batches of loads, and
//     leaves rows of a few hundred entries (where 8 partial sums and two barriers cost more than they save) to one wave.
//   * MFMA: the NT = cp / 32 output tiles of the panel are dealt over the waves (NT <= 8: at most one each).  A wave reads the T
//     fragments from the tile and the W fragments from LDS; in the root forms the panel's own X rows come straight from global memory
//     into operand registers (8 k-steps ahead) against the R fragments.  The chain is fp32 from bias[col] (or +0), ascending k-steps of
//     16, all of T W before all of X R, then the activation of the kRootAct form (axw_bf16_device.h), one rounding, and
//     FLEX_AXW_BF16_STORE_PANEL, which masks the padding columns to +0 bits; each lane takes its own row pointer from panel_rows.
//   * two LDS tiles where they fit: panel p + 1 is gathered while panel p is multiplied, one barrier a panel (a long row adds two).
//     LDS = fragments (K cp 2 bytes, K = dim or 2 dim) + tiles x 32 (2 dim + 16) + 8 dim 4 (long-row partials) + cp 4 (bias, root forms);
//     the launcher takes two tiles if that is within 160 KiB, else one, else (root forms only) refuses the shape.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "axw_bf16_device.h"

namespace flex_axw_bf16 {

constexpr int kLongRow = 512;  // nonzeros above which the workgroup gathers a row together
constexpr int kFlight = 8;     // nonzeros of a batch of loads; a lane keeps two batches in flight
constexpr size_t kLdsMax = 160 * 1024;

enum class Fused { kPlain, kRoot, kRelu, kDrop };

struct FusedGraph {
    const uint32_t *rowPtr, *col;
    const float *vals;
    const int32_t *panel_rows;    // [n_panels][32]
    const uint64_t *cost_prefix;  // [n_panels + 1], strictly ascending from 0
    int n_panels;
};

__host__ __device__ constexpr int tile_stride(int dim) { return 2 * dim + 16; }  // bytes between the rows of a T tile
constexpr size_t fused_lds(int dim, int cp, bool root, int tiles) {
    return static_cast<size_t>(root ? 2 * dim : dim) * cp * 2 + static_cast<size_t>(tiles) * kRows * tile_stride(dim) +
           static_cast<size_t>(kWaves) * dim * sizeof(float) + (root ? cp * sizeof(float) : 0);
}

// stage_w (axw_bf16_device.h) on the caller's unpadded W [dim x c]: rows c elements apart, the columns c .. 32 NT - 1 staged as zero
template <int NT>
__device__ __forceinline__ void stage_w_cols(const flex_bf16 *__restrict__ W, u32x4 *sW, int dim, int c) {
    constexpr int cp = 32 * NT;
    constexpr int kBatch = 4;
    const int total = (dim >> 3) * cp;
    for (int f0 = threadIdx.x; f0 < total; f0 += kBatch * 64 * kWaves) {
        uint32_t v[kBatch][8];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int f = min(f0 + b * 64 * kWaves, total - 1);  // a slot past the end re-reads the last one and is not written
            const int col = f % cp;
            const flex_bf16 *src = W + static_cast<size_t>(f / cp) * 8 * c + min(col, c - 1);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[b][e] = col < c ? static_cast<uint32_t>(src[e * c]) : 0u;
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int f = f0 + b * 64 * kWaves;
            if (f < total) {
                const int kq = f / cp, col = f % cp;
                const u32x4 w = {v[b][0] | (v[b][1] << 16), v[b][2] | (v[b][3] << 16), v[b][4] | (v[b][5] << 16), v[b][6] | (v[b][7] << 16)};
                sW[((kq >> 1) * NT + (col >> 5)) * 64 + 32 * (kq & 1) + (col & 31)] = w;
            }
        }
    }
}

// acc[v] = fmaf(vals[e], X[col[e]][v], acc[v]) for e = e0 .. e1 - 1 in that order: V columns of one row, xl = X + this lane's first column.
// The chain is serial, the loads are not: two batches of kFlight nonzeros alternate, the next one requested before the current one is
// added, so 2 kFlight row reads a lane are in flight (a row is latency-bound otherwise: one round trip per batch).  A slot past e1
// re-reads the last nonzero and is not added (not even as 0 x inf).
template <int V>
__device__ __forceinline__ void gather_chain(float (&acc)[V], const uint32_t *__restrict__ col, const float *__restrict__ vals,
                                             const flex_bf16 *__restrict__ xl, int dim, size_t e0, size_t e1) {
    using Vec = std::conditional_t<V == 8, u32x4, u32x2>;
    struct Batch {
        float a[kFlight];
        Vec x[kFlight];
    };
    auto load = [&](Batch &b, size_t e) {
#pragma unroll
        for (int u = 0; u < kFlight; ++u) {
            const size_t i = min(e + u, e1 - 1);
            b.a[u] = vals[i];
            b.x[u] = *reinterpret_cast<const Vec *>(xl + static_cast<size_t>(col[i]) * dim);
        }
    };
    auto add = [&](const Batch &b, size_t e) {
#pragma unroll
        for (int u = 0; u < kFlight; ++u) {
            if (e + u < e1) {
#pragma unroll
                for (int w = 0; w < V / 2; ++w) {
                    acc[2 * w] = __builtin_fmaf(b.a[u], __uint_as_float(b.x[u][w] << 16), acc[2 * w]);
                    acc[2 * w + 1] = __builtin_fmaf(b.a[u], __uint_as_float(b.x[u][w] & 0xFFFF0000u), acc[2 * w + 1]);
                }
            }
        }
    };
    Batch even, odd;
    if (e0 < e1) load(even, e0);
    for (size_t e = e0; e < e1; e += 2 * kFlight) {
        if (e + kFlight < e1) load(odd, e + kFlight);
        add(even, e);
        if (e + 2 * kFlight < e1) load(even, e + 2 * kFlight);
        if (e + kFlight < e1) add(odd, e + kFlight);
    }
}

// T tile of one panel: tile[r][0 .. dim) = rn_bf16(sum over row panel_rows[r] of A) -- the wave rows, then the long rows together
template <int V>
__device__ __forceinline__ void gather_panel(const FusedGraph &g, const flex_bf16 *__restrict__ X, int dim, int panel, char *tile, float *part) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int stride = tile_stride(dim);
    const int lpr = dim / V, groups = 64 / lpr, grp = lane / lpr, sub = lane - grp * lpr;  // lanes a row, rows side by side
    const int32_t *rows = g.panel_rows + static_cast<size_t>(panel) * kRows;
    const int32_t jr = rows[lane & 31];
    // the panel's long rows, one bit a row; the same value in every wave
    uint32_t long_rows = static_cast<uint32_t>(__ballot(g.rowPtr[jr + 1] - g.rowPtr[jr] > static_cast<uint32_t>(kLongRow)));
    if (grp < groups) {
        for (int r = grp; r < 4; r += groups) {
            const int pr = 4 * wave + r;
            if ((long_rows >> pr) & 1u) continue;
            const int32_t row = rows[pr];
            float acc[V];
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] = 0.f;
            gather_chain<V>(acc, g.col, g.vals, X + V * sub, dim, g.rowPtr[row], g.rowPtr[row + 1]);
            uint32_t w[V / 2];
#pragma unroll
            for (int v = 0; v < V / 2; ++v) w[v] = bf16_bits(acc[2 * v]) | (bf16_bits(acc[2 * v + 1]) << 16);
            char *dst = tile + pr * stride + 2 * V * sub;
            if constexpr (V == 8) *reinterpret_cast<u32x4 *>(dst) = u32x4{w[0], w[1], w[2], w[3]};
            else *reinterpret_cast<u32x2 *>(dst) = u32x2{w[0], w[1]};
        }
    }
    while (long_rows) {  // workgroup-uniform
        const int pr = __builtin_ctz(long_rows);
        long_rows &= long_rows - 1;
        const int32_t row = rows[pr];
        const size_t e0 = g.rowPtr[row], e1 = g.rowPtr[row + 1], per = (e1 - e0 + kWaves - 1) / kWaves;
        const size_t b = min(e1, e0 + wave * per), e = min(e1, b + per);
        if (lane < (dim >> 2)) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            gather_chain<4>(acc, g.col, g.vals, X + 4 * lane, dim, b, e);
            *reinterpret_cast<f32x4 *>(part + wave * dim + 4 * lane) = f32x4{acc[0], acc[1], acc[2], acc[3]};
        }
        __syncthreads();
        if (tid < dim) {
            float s = part[tid];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) s += part[w * dim + tid];
            reinterpret_cast<uint16_t *>(tile + pr * stride)[tid] = static_cast<uint16_t>(bf16_bits(s));
        }
        __syncthreads();  // part is free again
    }
}

// Out rows of one panel, tile `wave` of its NT: the chain, the activation, the store
template <int NT, Fused kForm>
__device__ __forceinline__ void multiply_panel(const FusedGraph &g, const flex_bf16 *__restrict__ X, flex_bf16 *__restrict__ Out, const u32x4 *sW,
                                               const char *tile, const float *sBias, int dim, int c, int panel, const flex::DropMask &dm) {
    constexpr bool kInit = kForm != Fused::kPlain, kAct = kForm == Fused::kRelu || kForm == Fused::kDrop;
    constexpr int cp = 32 * NT;
    const int lane = threadIdx.x & 63, t = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (t >= NT) return;  // wave-uniform
    const int j = lane & 31, h = lane >> 5, steps = dim >> 4;
    const size_t row = static_cast<size_t>(g.panel_rows[static_cast<size_t>(panel) * kRows + j]);
    f32x16 acc[1];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 b = {0.f, 0.f, 0.f, 0.f};
        if constexpr (kInit) b = *reinterpret_cast<const f32x4 *>(sBias + 32 * t + 8 * q + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[0][4 * q + e] = b[e];
    }
    [[maybe_unused]] const char *xrow = reinterpret_cast<const char *>(X + row * dim + 8 * h);
    [[maybe_unused]] bf16x8 pre[kUnit] = {};
    if constexpr (kInit) {
#pragma unroll
        for (int q = 0; q < kUnit; ++q)
            if (q < steps) pre[q] = *reinterpret_cast<const bf16x8 *>(xrow + 32 * q);
    }
    const bf16x8 *wf = reinterpret_cast<const bf16x8 *>(sW) + t * 64 + lane;
    const char *trow = tile + j * tile_stride(dim) + 16 * h;
    for (int s = 0; s < steps; ++s)
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[s * (NT * 64)], *reinterpret_cast<const bf16x8 *>(trow + 32 * s), acc[0], 0, 0, 0);
    if constexpr (kInit) {
        const bf16x8 *rf = wf + steps * (NT * 64);
        for (int s0 = 0; s0 < steps; s0 += kUnit) {
#pragma unroll
            for (int q = 0; q < kUnit; ++q) {
                const bf16x8 b = pre[q];
                if (s0 + kUnit + q < steps) pre[q] = *reinterpret_cast<const bf16x8 *>(xrow + 32 * (s0 + kUnit + q));
                if (s0 + q < steps) acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(rf[(s0 + q) * (NT * 64)], b, acc[0], 0, 0, 0);
            }
        }
    }
    if constexpr (kAct) {  // the kRootAct form of axw_gemm_bf16_stream_kernel: same select, same hash, same 64-bit index
        [[maybe_unused]] const uint64_t idx = row * c + 32 * t + 4 * h;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const float z = acc[0][reg], a = z <= 0.f ? 0.f : z;
            if constexpr (kForm == Fused::kDrop) {
                const bool keep = flex::dropout_bits(dm.seed_lo, dm.seed_hi, idx + (8 * (reg >> 2) + (reg & 3))) < dm.thr;
                acc[0][reg] = keep ? a * dm.c : 0.f;
            } else {
                acc[0][reg] = a;
            }
        }
    }
    flex_bf16 *dst = Out + row * cp + 32 * t + 16 * h;
    const int tile_c = c - 32 * t;
    FLEX_AXW_BF16_STORE_PANEL(1, acc, dst, tile_c, h)
}

template <int NT, Fused kForm>
__global__ __launch_bounds__(64 * kWaves) void axw_fused_bf16_kernel(FusedGraph g, const flex_bf16 *__restrict__ X, const flex_bf16 *__restrict__ W,
                                                                     const flex_bf16 *__restrict__ R, const float *__restrict__ bias,
                                                                     flex_bf16 *__restrict__ Out, int dim, int c, int two, flex::DropMask dm) {
    extern __shared__ u32x4 sW[];  // [K / 16][NT][64] fragments, the T tiles, the long-row partials [8][dim], the bias [cp]
    constexpr bool kInit = kForm != Fused::kPlain;
    constexpr int cp = 32 * NT;
    // this workgroup's panels: [cut(b), cut(b + 1)), cut(b) = the first i with cost_prefix[i] >= total b / gridDim.x
    const uint64_t total = g.cost_prefix[g.n_panels];
    auto cut = [&](uint32_t b) {
        const uint64_t target = total * b / gridDim.x;
        int lo = 0, hi = g.n_panels;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (g.cost_prefix[mid] >= target) hi = mid;
            else lo = mid + 1;
        }
        return lo;
    };
    const int first = cut(blockIdx.x), last = cut(blockIdx.x + 1);
    if (first >= last) return;  // workgroup-uniform, before any barrier

    const int frags = ((kInit ? 2 * dim : dim) >> 4) * NT * 64, tile_bytes = kRows * tile_stride(dim);
    char *tiles = reinterpret_cast<char *>(sW + frags);
    float *part = reinterpret_cast<float *>(tiles + (two ? 2 : 1) * tile_bytes);
    [[maybe_unused]] float *sBias = part + kWaves * dim;
    stage_w_cols<NT>(W, sW, dim, c);
    if constexpr (kInit) {
        stage_w_cols<NT>(R, sW + (dim >> 4) * NT * 64, dim, c);
        if (threadIdx.x < cp) sBias[threadIdx.x] = bias && static_cast<int>(threadIdx.x) < c ? bias[threadIdx.x] : 0.f;
    }
    auto gather = [&](int panel, char *tile) {  // dim <= 64: 8 bytes a lane, so that 4 rows fill the wave
        if (dim <= 64) gather_panel<4>(g, X, dim, panel, tile, part);
        else gather_panel<8>(g, X, dim, panel, tile, part);
    };
    if (two) {
        gather(first, tiles);
        __syncthreads();  // the fragments, the bias and the first tile
        for (int p = first; p < last; ++p) {
            const int cur = (p - first) & 1;
            if (p + 1 < last) gather(p + 1, tiles + (cur ^ 1) * tile_bytes);
            multiply_panel<NT, kForm>(g, X, Out, sW, tiles + cur * tile_bytes, sBias, dim, c, p, dm);
            __syncthreads();  // tile cur ^ 1 is whole, tile cur was read
        }
    } else {
        for (int p = first; p < last; ++p) {
            gather(p, tiles);
            __syncthreads();
            multiply_panel<NT, kForm>(g, X, Out, sW, tiles, sBias, dim, c, p, dm);
            __syncthreads();
        }
    }
}

// T tiles of the launch: 2, 1, or 0 where [W; R] and one tile do not fit (root forms at dim = 256, c > 128)
int fused_tiles(int dim, int cp, bool root) { return fused_lds(dim, cp, root, 2) <= kLdsMax ? 2 : fused_lds(dim, cp, root, 1) <= kLdsMax ? 1 : 0; }

// The one launch of order FLEX_AXW_AX_W_FUSED (axw.cpp: flex_axw_fused_bf16_launch checks the operands against the handle).  R == NULL: the
// plain layer; else the root forms: relu, and with drop_p > 0 dropout.  hipErrorInvalidValue for a shape that does not fit.
hipError_t fused_launch(const uint32_t *rowPtr, const uint32_t *col, const float *vals, const int32_t *panel_rows, const uint64_t *cost_prefix,
                        int n_panels, const flex_bf16 *X, const flex_bf16 *W, const flex_bf16 *R, const float *bias, flex_bf16 *Out, int dim, int c,
                        int cp, int relu, float drop_p, uint64_t seed, int n_workgroups, hipStream_t s) {
    const bool root = R != nullptr;
    const int tiles = dim > 0 && dim <= 256 && dim % 16 == 0 && cp > 0 && cp <= 256 && cp % 64 == 0 ? fused_tiles(dim, cp, root) : 0;
    if (!rowPtr || !col || !vals || !panel_rows || !cost_prefix || n_panels <= 0 || !X || !W || !Out || c <= 0 || c > cp || tiles == 0 ||
        n_workgroups <= 0 || misaligned(X) || misaligned(Out) || (!root && (bias || relu)) || !flex::drop_p_ok(drop_p) || (drop_p > 0.f && !relu))
        return hipErrorInvalidValue;
    const FusedGraph g{rowPtr, col, vals, panel_rows, cost_prefix, n_panels};
    const flex::DropMask dm = flex::drop_mask(drop_p, seed);
    const dim3 grid(static_cast<unsigned>(n_workgroups));
    const size_t lds = fused_lds(dim, cp, root, tiles);
    return dispatch_tiles<2, 4, 6, 8>(cp / 32, [&](auto nt) {
        constexpr int NT = decltype(nt)::value;
        auto go = [&](auto kernel) { return launch(kernel, grid, 64 * kWaves, lds, s, g, X, W, R, bias, Out, dim, c, tiles == 2 ? 1 : 0, dm); };
        if (!root) return go(axw_fused_bf16_kernel<NT, Fused::kPlain>);
        if (!relu) return go(axw_fused_bf16_kernel<NT, Fused::kRoot>);
        if (drop_p == 0.f) return go(axw_fused_bf16_kernel<NT, Fused::kRelu>);
        return go(axw_fused_bf16_kernel<NT, Fused::kDrop>);
    });
}

}  // namespace flex_axw_bf16
