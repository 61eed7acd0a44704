// axw_bf16_device.h -- what the bf16 GEMM files of libflex_axw.so share (axw_bf16_kernels.hip, axw_bf16_wide_kernels.hip,
// axw_bf16_root_kernels.hip, axw_bf16_act_kernels.hip):
//   * stage_w, FLEX_AXW_BF16_STORE_PANEL and axw_gemm_bf16_kernel: the GEMM with the whole W resident in LDS (the narrow forward and dX,
//     the wide dX's windows).  Its data path is described at the top of axw_bf16_kernels.hip.
//   * axw_gemm_bf16_stream_kernel: the GEMM with W streamed through two LDS slab buffers -- ONE body for the wide forward, the root
//     forward, its ReLU-and-dropout form and the root dX's windows (Stream).  The pipeline is described at the top of axw_bf16_wide_kernels.hip, the two sources,
//     the addend and the bias at the top of axw_bf16_root_kernels.hip.
//   * the host side of every launcher: misaligned, the panel arithmetic, launch and dispatch_tiles.  axw_bf16_dw_device.h includes this
//     file for them.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "attention_device.h"  // flex_bf16, bf16_bits: the project's one fp32 -> bf16 rounding

namespace flex_axw_bf16 {

using flex::attention::bf16_bits;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kRows = 32;   // rows of a panel: the MFMA's N
constexpr int kWaves = 8;
constexpr int kUnit = 8;    // k-steps (of 16) whose L fragments a wave holds: 256 bytes of each row
constexpr int kSlab = kUnit;  // k-steps of a slab of streamed W

// Wp[dim x 32 NT], rows ldw elements apart -> LDS fragments, once per workgroup.  Fragment-lane f = (k-octet kq, column col) gathers
// Wp[8 kq .. 8 kq + 7][col] (eight 2-byte loads, a wave's 64 on 128 contiguous bytes) and writes them as ONE 16-byte LDS store to the slot
// of (s = kq >> 1, t = col >> 5, lane = 32 (kq & 1) + (col & 31)); 16 fragment-lanes in flight a thread.
template <int NT>
__device__ __forceinline__ void stage_w(const flex_bf16 *__restrict__ Wp, u32x4 *sW, int dim, int ldw) {
    constexpr int cp = 32 * NT;
    constexpr int kBatch = 4;
    const int total = (dim >> 3) * cp;
    for (int f0 = threadIdx.x; f0 < total; f0 += kBatch * 64 * kWaves) {
        uint32_t v[kBatch][8];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int f = min(f0 + b * 64 * kWaves, total - 1);  // a slot past the end re-reads the last one and is not written
            const flex_bf16 *src = Wp + static_cast<size_t>(f / cp) * 8 * ldw + f % cp;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[b][e] = src[e * ldw];
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

// A panel's accumulators acc[NT], rounded to bf16, to the 64 NT bytes at dst = &Out[row of this lane][16 h], h = lane >> 5:
// acc[t][reg] = Out[r0 + j][32 t + 8 (reg >> 2) + 4 h + (reg & 3)]
// A tile that holds padding (a wave-uniform test) masks the rounded bits of its columns >= c to +0: the mask is the sign of
// column - c, integer arithmetic on one register (a compare per element kept 2 SGPRs each alive across the panel loop:
// 192 spilled at NT = 8); the empty asm keeps the 16 masks from being hoisted out of the loop into registers of their own.
// The 8-byte chunks of a row's 64 bytes of a tile alternate between lanes j (h = 0: chunks 0 2 4 6) and j + 32 (1 3 5 7);
// v_permlane32_swap trades chunk 2g + 1 of the lower half for chunk 2g + 4 of the upper, so that h = 0 ends with chunks 0..3 and
// h = 1 with 4..7: 32 contiguous bytes a lane, two 16-byte stores.  Plain stores, not nontemporal ones: a line arrives in
// pieces, which the L2 has to merge before it writes the line back (measured with 8-byte nontemporal stores: the reddit
// shape's 60 MB of Out took 138 us, the time of a read-modify-write of every piece -- DESIGN.md 3.26).
// A macro, not a function: as a function taking acc by reference it changed the register allocation of axw_gemm_bf16_kernel's
// instantiations, whose code the wide kernels' arrival was to leave as it is.
#define FLEX_AXW_BF16_STORE_PANEL(NT, acc, dst, c, h)                                                                             \
    _Pragma("unroll") for (int t = 0; t < NT; ++t) {                                                                              \
        const bool pad = 32 * t + 32 > c;                                                                                         \
        int lim = 32 * t + 4 * h - c; /* column of reg 0, minus c */                                                              \
        asm volatile("" : "+v"(lim));                                                                                             \
        auto bits = [&](int reg) {                                                                                                \
            const uint32_t b = bf16_bits(acc[t][reg]);                                                                            \
            return pad ? b & static_cast<uint32_t>((lim + 8 * (reg >> 2) + (reg & 3)) >> 31) : b;                                 \
        };                                                                                                                        \
        uint32_t w[8]; /* w[2 g], w[2 g + 1]: the lane's chunk g */                                                               \
        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                                           \
            w[2 * g] = bits(4 * g) | (bits(4 * g + 1) << 16);                                                                     \
            w[2 * g + 1] = bits(4 * g + 2) | (bits(4 * g + 3) << 16);                                                             \
        }                                                                                                                         \
        _Pragma("unroll") for (int p = 0; p < 2; ++p) { /* chunk p against chunk p + 2 */                                         \
            const auto lo = __builtin_amdgcn_permlane32_swap(w[2 * p], w[2 * p + 4], false, false);                               \
            const auto hi = __builtin_amdgcn_permlane32_swap(w[2 * p + 1], w[2 * p + 5], false, false);                           \
            const u32x4 v = {lo[0], hi[0], lo[1], hi[1]};                                                                         \
            *reinterpret_cast<u32x4 *>(dst + 32 * t + 8 * p) = v;                                                                 \
        }                                                                                                                         \
    }

// Out[n x 32 NT] = L[n x dim] Wp[dim x 32 NT], the whole Wp in LDS for the life of the workgroup (axw_bf16_kernels.hip).  kWindow (the wide
// dX kernel): Wp and Out are the 32 NT columns from 256 blockIdx.y on of arrays whose rows are ld elements apart.
template <int NT, bool kWindow = false>  // 32-column tiles of Out: cp = 32 NT
__global__ __launch_bounds__(64 * kWaves) void axw_gemm_bf16_kernel(const flex_bf16 *__restrict__ L, const flex_bf16 *__restrict__ Wp,
                                                                    flex_bf16 *__restrict__ Out, int n, int dim, int c, int ld) {
    extern __shared__ u32x4 sW[];  // [dim / 16][NT][64] fragments of 8 bf16
    const int ldw = kWindow ? ld : 32 * NT, ldo = ldw;
    if constexpr (kWindow) {
        Wp += 256 * blockIdx.y;
        Out += 256 * blockIdx.y;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int steps = dim >> 4;
    const int n_panels = (n + kRows - 1) / kRows;
    auto panel_row = [&](int pnl) { return min(min(pnl, n_panels - 1) * kRows, n - kRows); };  // past the end: the last panel again
    const int first_panel = wave < 4 ? blockIdx.x * 4 + wave : gridDim.x * 4 + blockIdx.x * 4 + (wave - 4);
    const int panel_step = gridDim.x * kWaves;
    // this lane's 16 bytes of k-step s of a panel
    auto lfrag = [&](int pnl, int s) {
        return *reinterpret_cast<const bf16x8 *>(L + static_cast<size_t>(panel_row(pnl) + j) * dim + 16 * s + 8 * h);
    };

    bf16x8 pre[kUnit] = {};  // the L fragments of the unit about to be multiplied
#pragma unroll
    for (int q = 0; q < kUnit; ++q)
        if (q < steps) pre[q] = lfrag(first_panel, q);
    stage_w<NT>(Wp, sW, dim, ldw);
    __syncthreads();  // the only barrier

    const bf16x8 *wf = reinterpret_cast<const bf16x8 *>(sW) + lane;
    for (int panel = first_panel; panel < n_panels; panel += panel_step) {
        f32x16 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
        for (int s0 = 0; s0 < steps; s0 += kUnit) {
            const bool last = s0 + kUnit >= steps;  // wave-uniform, like everything that guards a load or an MFMA below
            const int np = last ? panel + panel_step : panel, ns0 = last ? 0 : s0 + kUnit;
            const int n_cur = min(kUnit, steps - s0), n_next = min(kUnit, steps - ns0);
#pragma unroll
            for (int q = 0; q < kUnit; ++q) {
                const bf16x8 b = pre[q];
                if (q < n_next) pre[q] = lfrag(np, ns0 + q);
                if (q < n_cur) {
                    const bf16x8 *w = wf + (s0 + q) * (NT * 64);
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(w[t * 64], b, acc[t], 0, 0, 0);
                }
            }
        }
        flex_bf16 *dst = Out + static_cast<size_t>(panel_row(panel) + j) * ldo + 16 * h;
        FLEX_AXW_BF16_STORE_PANEL(NT, acc, dst, c, h)
    }
}

// The four uses of the streamed GEMM below; everything that tells them apart is decided at compile time.
//   kWide    Out[n x cp] = L1[n x d1] Wf: one source, the chain from +0 (flex_axw_gemm_bf16_wide_launch; L2, d2, Cin and bias are not read)
//   kRoot    Out[n x cp] = L1 W1 + L2 W2 + Cin + bias: two sources, acc = fp32(Cin) + bias (flex_axw_gemm_bf16_root_launch)
//   kWindow  the dual-source dX of flex_axw_dx_bf16_root_launch: two sources, the chain from +0; Out is a window of 32 NT whole columns,
//            from 256 blockIdx.y on, of an array whose rows are `c` elements apart (the parameter carries the row stride: a window has
//            no padding to mask), and Wf holds one fragment stream of (d1 + d2) / 16 k-steps per 256-column pass
//   kRootAct kRoot with ReLU, and with a flex::DropMask as `drop` dropout too, on the accumulators between the chain and the store
//            (flex_axw_gemm_bf16_root_act_launch, axw_bf16_act_kernels.hip)
enum class Stream { kWide, kRoot, kWindow, kRootAct };

// Out = L1 Wf[0 .. d1) + L2 Wf[d1 .. d1 + d2): Wf in fragment order (axw_bf16_pack_kernel), streamed through two LDS buffers of kSlab k-steps.
// `drop` is a parameter pack so that the forms without dropout keep the kernel arguments, and with them the code, they had.
template <int NT, int P, Stream kForm, class... Drop>  // 32-column tiles of Out, panels a wave; kRootAct: no Drop or one flex::DropMask
__global__ __launch_bounds__(64 * kWaves) void axw_gemm_bf16_stream_kernel(const flex_bf16 *__restrict__ L1, int d1, const flex_bf16 *__restrict__ L2,
                                                                           int d2, const u32x4 *__restrict__ Wf, const flex_bf16 *__restrict__ Cin,
                                                                           const float *__restrict__ bias, flex_bf16 *__restrict__ Out, int n,
                                                                           int c, Drop... drop) {
    extern __shared__ u32x4 sW[];  // [2 buffers][kSlab][NT][64] fragments of 8 bf16, then (kRoot, kRootAct) cp floats of bias
    constexpr bool kOne = kForm == Stream::kWide, kWindow = kForm == Stream::kWindow, kAct = kForm == Stream::kRootAct;
    constexpr bool kInit = kForm == Stream::kRoot || kAct, kDrop = sizeof...(Drop) > 0;
    static_assert(kAct || !kDrop, "only kRootAct takes a mask");
    constexpr int cp = 32 * NT, kStepFrags = NT * 64, kSlabFrags = kSlab * kStepFrags;
    float *sBias = reinterpret_cast<float *>(sW + 2 * kSlabFrags);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = kOne ? tid >> 6 : __builtin_amdgcn_readfirstlane(tid >> 6);  // two sources: in an SGPR, and so is every panel's row
    const int j = lane & 31, h = lane >> 5;
    const int s1 = d1 >> 4, steps = kOne ? s1 : (d1 + d2) >> 4, slabs = (steps + kSlab - 1) / kSlab;
    if constexpr (kWindow) {
        Wf += static_cast<size_t>(blockIdx.y) * steps * (8 * 64);  // a full pass is 8 tiles wide
        Out += 256 * blockIdx.y;
    }
    const int n_panels = (n + kRows - 1) / kRows;
    const int n_rounds = (n_panels + kWaves * P - 1) / (kWaves * P);  // gridDim.x <= n_rounds: every workgroup has a round
    auto panel_of = [&](int round, int p) { return (round * P + p) * kWaves + wave; };
    auto panel_row = [&](int pnl) { return min(min(pnl, n_panels - 1) * kRows, n - kRows); };  // past the end: the last panel again
    // A fragment's address is a wave-uniform 64-bit base (the panel's first row in L1 or in L2, the latter set back by d1 / 16 k-steps, so
    // that k-step s of the WHOLE contraction is 32 s bytes on in either) plus this lane's 32-bit byte offset inside a panel (at most 32 rows
    // of 8 KiB), which no round changes: one register a source instead of a pointer a source and panel.  The root launcher passes
    // L2 = L1 when d2 = 0, and no k-step then selects it.  kWide, with one source, keeps the plain form it was measured with -- this
    // lane's own 64-bit row pointer a panel -- as a compile-time choice: on the two-source form its NT = 4 instantiation ran the reddit
    // shape (dim 608, c 128) 4.5 % slower.
    const uint32_t lane1 = (static_cast<uint32_t>(j) * d1 + 8 * h) * 2, lane2 = (static_cast<uint32_t>(j) * d2 + 8 * h) * 2;
    struct Rows {
        const char *a, *b;
    };
    auto rows_of = [&](int pnl) {
        const size_t r = static_cast<size_t>(panel_row(pnl));
        if constexpr (kOne) return Rows{reinterpret_cast<const char *>(L1 + (r + j) * d1 + 8 * h), nullptr};
        else return Rows{reinterpret_cast<const char *>(L1 + r * d1), reinterpret_cast<const char *>(L2 + r * d2) - 32 * static_cast<ptrdiff_t>(s1)};
    };
    auto lfrag = [&](const Rows &r, int s) {  // two sources: a wave-uniform choice of base and stride
        if constexpr (kOne) return *reinterpret_cast<const bf16x8 *>(r.a + 32 * s);
        else return *reinterpret_cast<const bf16x8 *>(s < s1 ? r.a + 32 * s + lane1 : r.b + 32 * s + lane2);
    };
    const bool stager = tid < kStepFrags;  // a k-step of W is NT KiB: one 16-byte fragment a thread of the first NT waves

    bf16x8 pre[P][kSlab] = {};  // the L fragments of the slab about to be multiplied
    {
        Rows r[P];
#pragma unroll
        for (int p = 0; p < P; ++p) r[p] = rows_of(panel_of(blockIdx.x, p));
#pragma unroll
        for (int q = 0; q < kSlab; ++q) {
            if (kOne || q < steps) {  // two sources: the first slab may be the only one, and a partial one; kWide: dim > 256, it is full
#pragma unroll
                for (int p = 0; p < P; ++p) pre[p][q] = lfrag(r[p], q);
                if (stager) sW[q * kStepFrags + tid] = Wf[q * kStepFrags + tid];
            }
        }
    }
    if constexpr (kInit)
        if (tid < cp) sBias[tid] = bias && tid < c ? bias[tid] : 0.f;
    if constexpr (!kOne) __syncthreads();  // sBias is read before a round's first slab barrier (kWindow keeps the barrier it was built with)

    int buf = 0;
    const bf16x8 *wf = reinterpret_cast<const bf16x8 *>(sW) + lane;
    for (int round = blockIdx.x; round < n_rounds; round += gridDim.x) {
        f32x16 acc[P][NT];
#pragma unroll
        for (int p = 0; p < P; ++p) {  // acc = Cin + bias, in the layout of the store: four columns from 32 t + 8 g + 4 h on
            auto init = [&](int t, int g, u32x2 v) {
                const f32x4 b = *reinterpret_cast<const f32x4 *>(sBias + 32 * t + 8 * g + 4 * h);
                acc[p][t][4 * g] = __uint_as_float(v[0] << 16) + b[0];
                acc[p][t][4 * g + 1] = __uint_as_float(v[0] & 0xFFFF0000u) + b[1];
                acc[p][t][4 * g + 2] = __uint_as_float(v[1] << 16) + b[2];
                acc[p][t][4 * g + 3] = __uint_as_float(v[1] & 0xFFFF0000u) + b[3];
            };
            if constexpr (!kInit) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int i = 0; i < 16; ++i) acc[p][t][i] = 0.f;
            } else if (Cin) {  // workgroup-uniform
                const flex_bf16 *crow = Cin + static_cast<size_t>(panel_row(panel_of(round, p))) * cp + (j * cp + 4 * h);
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) init(t, g, *reinterpret_cast<const u32x2 *>(crow + 32 * t + 8 * g));
            } else {
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int g = 0; g < 4; ++g) init(t, g, u32x2{0u, 0u});  // +0 without a Cin
            }
        }
        for (int sl = 0; sl < slabs; ++sl, buf ^= 1) {
            // slab sl is whole in buffer buf (every store into it came before this barrier), and buffer buf ^ 1 was last read before it
            __syncthreads();
            const bool last = sl + 1 == slabs;  // workgroup-uniform, like everything that guards a load, a store or an MFMA below
            const int nr = last ? round + gridDim.x : round, ns0 = last ? 0 : (sl + 1) * kSlab;
            const int n_cur = min(kSlab, steps - sl * kSlab), n_next = nr < n_rounds ? min(kSlab, steps - ns0) : 0;
            const u32x4 *src = Wf + static_cast<size_t>(ns0) * kStepFrags + tid;
            u32x4 *dst = sW + (buf ^ 1) * kSlabFrags + tid;
            const bf16x8 *w = wf + buf * kSlabFrags;
            Rows r[P];
#pragma unroll
            for (int p = 0; p < P; ++p) r[p] = rows_of(panel_of(nr, p));
            u32x4 stage[kSlab];
#pragma unroll
            for (int q = 0; q < kSlab; ++q) {
                if (q >= 2 && q - 2 < n_next && stager) dst[(q - 2) * kStepFrags] = stage[q - 2];
                bf16x8 b[P];
#pragma unroll
                for (int p = 0; p < P; ++p) b[p] = pre[p][q];
                if (q < n_next) {
#pragma unroll
                    for (int p = 0; p < P; ++p) pre[p][q] = lfrag(r[p], ns0 + q);
                    if (stager) stage[q] = src[q * kStepFrags];
                }
                if (q < n_cur) {
#pragma unroll
                    for (int t = 0; t < NT; ++t) {
                        const bf16x8 a = w[(q * NT + t) * 64];
#pragma unroll
                        for (int p = 0; p < P; ++p) acc[p][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b[p], acc[p][t], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int q = kSlab - 2; q < kSlab; ++q)
                if (q < n_next && stager) dst[q * kStepFrags] = stage[q];
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const int panel = panel_of(round, p);
            if (panel >= n_panels) continue;  // wave-uniform: the round's panels past the end were multiplied as copies of the last
            const f32x16(&panel_acc)[NT] = acc[p];  // the macro has a loop variable p of its own
            if constexpr (kAct) {
                // a = z > 0 ? z : (z is NaN ? z : +0), then keep(seed, row c + column) ? a cs : +0 -- a select, so a dropped inf or NaN is
                // +0 -- on one tile's 16 accumulators at a time, just before the store rounds them: the hash of a whole panel ahead of the
                // store would be 16 NT more live values.  The mask index is 64-bit: the row's, one value a lane, plus the element's
                // compile-time column offset.  The rows that an overlapping last panel stores twice get the same bits twice.
                const size_t row = static_cast<size_t>(panel_row(panel) + j);
                flex_bf16 *dst = Out + row * cp + 16 * h;
                [[maybe_unused]] const uint64_t idx = row * c + 4 * h;
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    f32x16 tile[1] = {acc[p][t]};
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const float z = tile[0][reg], a = z <= 0.f ? 0.f : z;
                        if constexpr (kDrop) {
                            const flex::DropMask dm = [](const flex::DropMask &m) { return m; }(drop...);
                            const bool keep = flex::dropout_bits(dm.seed_lo, dm.seed_hi, idx + (32 * t + 8 * (reg >> 2) + (reg & 3))) < dm.thr;
                            tile[0][reg] = keep ? a * dm.c : 0.f;
                        } else {
                            tile[0][reg] = a;
                        }
                    }
                    flex_bf16 *tile_dst = dst + 32 * t;  // the macro has a t of its own
                    const int tile_c = c - 32 * t;
                    FLEX_AXW_BF16_STORE_PANEL(1, tile, tile_dst, tile_c, h)
                }
            } else if constexpr (kWindow) {
                flex_bf16 *dst = Out + static_cast<size_t>(panel_row(panel) + j) * c + 16 * h;
                FLEX_AXW_BF16_STORE_PANEL(NT, panel_acc, dst, cp, h)
            } else {
                flex_bf16 *dst = Out + static_cast<size_t>(panel_row(panel) + j) * cp + 16 * h;
                FLEX_AXW_BF16_STORE_PANEL(NT, panel_acc, dst, c, h)
            }
        }
    }
}

// ---- the host side of the launchers ----

inline bool misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// workgroups of a persistent launch over the 32-row panels of n rows, `share` panels each before any gets a second helping: 4 for the
// resident kernel (a panel a SIMD), a round of 8 P for the streamed one; no workgroup without a panel, at most one a CU
inline unsigned panel_groups(int n, int share, int n_cus) {
    const int n_panels = (n + kRows - 1) / kRows;
    return static_cast<unsigned>(std::min(n_cus, (n_panels + share - 1) / share));
}
constexpr int stream_panels(int nt) { return nt <= 2 ? 2 : 1; }  // P: two panels a wave while the accumulators are 64 registers or fewer
constexpr size_t stream_lds(int nt) { return static_cast<size_t>(2) * kSlab * nt * 64 * sizeof(u32x4); }

// one launch: more than 64 KiB of dynamic LDS has to be asked for.  Returns the error of the attribute call or of the launch.
template <class... Params, class... Args>
hipError_t launch(void (*kernel)(Params...), dim3 grid, int threads, size_t lds, hipStream_t s, Args... args) {
    if (lds > 0) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds));
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, grid, dim3(static_cast<unsigned>(threads)), lds, s, static_cast<Params>(args)...);
    return hipGetLastError();
}

// f(std::integral_constant<int, NT>) for the NT of Tiles... that equals nt; the last of them serves every other nt, as a switch's default
template <int First, int... Rest, class F>
hipError_t dispatch_tiles(int nt, F f) {
    if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, First>());
    else return nt == First ? f(std::integral_constant<int, First>()) : dispatch_tiles<Rest...>(nt, f);
}

// [W1; W2] -> Wf in fragment order, zero from column c on (axw_bf16_root_kernels.hip: axw_bf16_pack_kernel); W2 may be NULL with d2 = 0
hipError_t pack_launch(const flex_bf16 *W1, const flex_bf16 *W2, u32x4 *wf, int d1, int d2, int c, int nt, hipStream_t s);

}  // namespace flex_axw_bf16
