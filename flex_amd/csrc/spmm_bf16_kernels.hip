// spmm_bf16_kernels.hip -- the SpMM on bf16 operands (include/flex_spmm.h: FLEX_PLAN_BF16, flex_spmm_bf16): B and C are flex_bf16, the
// sums are fp32.  DESIGN.md 3.16; tests/test_gpu_spmm_bf16.py covers it, both offset forms of every tile width; the cases are
// tests/spmm_bf16_ref.py's and tests/attention_forms.py's, and tests/test_attention_routes.py holds every instantiation to a case.
//
// A bf16 row of k elements is, byte for byte, an fp32 row of k / 2 words, and a FLEX_PLAN_BF16 plan is the fp32 plan of that word width
// (plan.cpp, create_common): PlanView's k, ldb and ldc are WORDS here, the records hold byte offsets of word rows, a lane owns 4 words
// of a row = 8 bf16 columns.  spmm_flat_bf16_kernel therefore runs spmm_flat_kernel's walk unchanged (spmm_device.h: the place of a wave
// in the chunk table, header -> descriptors and records -> gathers, the record windows and their staging, blocks of U gathers across
// row boundaries with one wave-uniform flush test per step, bundles by ds_bpermute, lanes past the row's end on the tile's first
// column) and differs in three places:
//   * a gathered word is two bf16: each is widened by a shift or a mask (exact) and multiplied into one of 8 fp32 accumulators with
//     fmaf, in the record order of the fp32 kernel;
//   * at a row's end the S = 64 / G slots are summed in fp32 by reduce_full<G> on both halves of the accumulator, the sum is rounded
//     ONCE to bf16 (attention_device.h, bf16_bits: to nearest even in integer arithmetic, NaN stays quiet NaN, +-inf stays) and the G
//     lanes of slot 0 write the tile's part of the row with one non-temporal 16-byte store each; a bundle's lanes narrow their own 8
//     sums and store 16 bytes each;
//   * a piece of a split row writes its 8 fp32 per lane to the piece's slot of 2 k floats (two plain 16-byte stores), and
//     spmm_fixup_bf16_kernel adds the pieces in piece order in fp32, rounds once and writes bf16.  There is no in-launch sum.
// Only this vector form exists: k, ldb and ldc are multiples of 8 elements and both operands 16-byte aligned, or the host refuses.
#include <cstdint>

#include "attention_device.h"
#include "plan.h"
#include "spmm_device.h"

namespace flex {
namespace spmm_bf16 {

using namespace spmm_dev;
using attention::bf16_bits;

// a lane's 8 sums: columns 0-3 and 4-7 of its 8
struct Acc8 {
    float4 lo, hi;
};

// acc += v x the 8 bf16 of the four gathered words (little endian: the low half of a word is the even column)
__device__ __forceinline__ void fma8(Acc8 &acc, float v, const float4 &w) {
    const uint32_t w0 = __float_as_uint(w.x), w1 = __float_as_uint(w.y), w2 = __float_as_uint(w.z), w3 = __float_as_uint(w.w);
    acc.lo.x = fmaf(v, as_f32(w0 << 16), acc.lo.x);
    acc.lo.y = fmaf(v, as_f32(w0 & 0xFFFF0000u), acc.lo.y);
    acc.lo.z = fmaf(v, as_f32(w1 << 16), acc.lo.z);
    acc.lo.w = fmaf(v, as_f32(w1 & 0xFFFF0000u), acc.lo.w);
    acc.hi.x = fmaf(v, as_f32(w2 << 16), acc.hi.x);
    acc.hi.y = fmaf(v, as_f32(w2 & 0xFFFF0000u), acc.hi.y);
    acc.hi.z = fmaf(v, as_f32(w3 << 16), acc.hi.z);
    acc.hi.w = fmaf(v, as_f32(w3 & 0xFFFF0000u), acc.hi.w);
}

// 8 fp32 sums narrowed to 8 bf16 = four words: the one rounding of an output element
__device__ __forceinline__ v4u narrow8(const float4 &lo, const float4 &hi) {
    const v4u r = {bf16_bits(lo.x) | (bf16_bits(lo.y) << 16), bf16_bits(lo.z) | (bf16_bits(lo.w) << 16),
                   bf16_bits(hi.x) | (bf16_bits(hi.y) << 16), bf16_bits(hi.z) | (bf16_bits(hi.w) << 16)};
    return r;
}

// compute_chunk of spmm_kernels.hip on bf16 rows.  Cw: C as words (two bf16 each); c0, p.k, p.ldb and p.ldc are in words.
template <int G, bool OFF32, int U>
__device__ __forceinline__ void compute_chunk_bf16(const PlanView &p, const ChunkRegs &d, uint2 *my_lds, const char *__restrict__ Bb,
                                                   uint32_t *__restrict__ Cw, int lane, int c0, bool col_ok, uint32_t tile) {
    constexpr int S = 64 / G;
    const int slot = lane / G;
    const uint64_t ldc = static_cast<uint64_t>(p.ldc);
    // lanes past the row's end gather the tile's FIRST column instead: a line this record's gather touches anyway
    const uint32_t lane_off = (col_ok ? c0 : c0 - (lane % G) * 4) * 4u;
    const uint64_t row_bytes = static_cast<uint64_t>(p.ldb) * 4u;
    const uint4 hdr = d.hdr;
    const uint2 cx = d.cx;
    const uint32_t my_beg = d.my_beg, my_dst = d.my_dst;

    const uint32_t nt = hdr.y, zb = hdr.z, ze = hdr.w;
    const bool packed_chunk = p.rec_packed != 0 && (cx.y & kChunkWide) == 0;
    const uint2 *__restrict__ rec = p.rec_packed != 0 ? p.rec + cx.x - zb : p.rec;
    uint32_t carry = 0;  // packed: the column the previous window ended on

    uint32_t ti = 0;                                          // current task
    uint32_t row_end = __builtin_amdgcn_readlane(my_beg, 1);  // where it ends in the record stream
    Acc8 acc = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const bool out_ok = col_ok && slot == 0;
    // Write out the task that ends at the current stream position (and any empty rows behind it), as the fp32 kernel's flush does.
    auto flush = [&](uint32_t pos) {
        do {
            const uint32_t dst = __builtin_amdgcn_readlane(my_dst, ti);
            if ((dst & (kPartialFlag | kBundleFlag)) == (kPartialFlag | kBundleFlag)) {  // wave-uniform
                // a BUNDLE: slot s held row s of it all along -- nothing to reduce; every lane narrows and stores the 8 columns it owns
                if constexpr (kTileHasBundles<G>) {
                    const uint32_t first = dst & (kBundleRowsPerChunk - 1u);
                    const uint32_t held = first < 64u ? d.my_bd0 : d.my_bd1;
                    const uint32_t row = static_cast<uint32_t>(
                        __builtin_amdgcn_ds_bpermute(static_cast<int>(((first & 63u) + slot) << 2), static_cast<int>(held)));
                    if (col_ok && row != kBundleNoRow) {
                        const bool none = (row & kBundleZero) != 0;  // a row without nonzeros: +0, whatever its slot summed
                        const v4u zero = {0u, 0u, 0u, 0u};
                        const v4u val = none ? zero : narrow8(acc.lo, acc.hi);
                        __builtin_nontemporal_store(val, reinterpret_cast<v4u *>(Cw + static_cast<uint64_t>(row & ~kBundleZero) * ldc + c0));
                    }
                }
            } else if (__builtin_expect((dst & kPartialFlag) != 0, 0)) {  // wave-uniform: a PIECE, summed by spmm_fixup_bf16_kernel
                const float4 lo = reduce_full<G>(acc.lo), hi = reduce_full<G>(acc.hi);
                if (out_ok) {
                    int l = lane;  // the lane's first column again, from the lane id: nothing of this rare path stays in registers
                    asm volatile("" : "+v"(l));
                    const int col = 2 * (static_cast<int>(tile) * (4 * G) + (l % G) * 4);  // in elements
                    float *prow = p.partial + static_cast<uint64_t>(dst & ~kPartialFlag) * (2u * static_cast<uint32_t>(p.k)) + col;
                    *reinterpret_cast<float4 *>(prow) = lo;
                    *reinterpret_cast<float4 *>(prow + 4) = hi;
                }
            } else {
                const float4 lo = reduce_full<G>(acc.lo), hi = reduce_full<G>(acc.hi);
                if (out_ok) __builtin_nontemporal_store(narrow8(lo, hi), reinterpret_cast<v4u *>(Cw + static_cast<uint64_t>(dst) * ldc + c0));
            }
            acc = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
            ++ti;
            row_end = ti < nt ? __builtin_amdgcn_readlane(my_beg, ti + 1) : 0xFFFFFFFFu;
        } while (row_end == pos);
    };
    if (nt == 0) row_end = 0xFFFFFFFFu;
    if (row_end == zb) flush(zb);  // leading empty rows

    uint32_t pos = zb;  // stream position after the steps consumed so far
    for (uint32_t wz = zb; wz < ze; wz += kWindowRecs<G>) {
        const uint32_t wn = min(static_cast<uint32_t>(kWindowRecs<G>), ze - wz);
        if (packed_chunk) carry = stage_window_packed<G, OFF32>(p, my_lds, zb, wz, wn, cx, hdr.x, nt, my_beg, carry, static_cast<uint32_t>(row_bytes), lane);
        else stage_window<G>(my_lds, rec, wz, wn, lane, p.rec_nt != 0);
        const uint32_t nsteps = wn / S;  // rows are padded to multiples of S
        const uint2 *lds_slot = my_lds + slot;
        uint32_t j = 0;
        // N steps from step j on: N LDS reads, N gathers back to back, then the sums in record order with the row-end test per step
        auto block = [&](auto n) {
            constexpr int N = decltype(n)::value;
            uint2 r[N];
            float4 b[N];
#pragma unroll
            for (int u = 0; u < N; ++u) r[u] = lds_slot[(j + u) * S];
#pragma unroll
            for (int u = 0; u < N; ++u) b[u] = gather4<OFF32>(Bb, r[u].x, lane_off, row_bytes);
#pragma unroll
            for (int u = 0; u < N; ++u) {
                fma8(acc, as_f32(r[u].y), b[u]);
                pos += S;
                if (pos == row_end) flush(pos);
            }
        };
        for (; j + U <= nsteps; j += U) block(std::integral_constant<int, U>{});  // full blocks: no bound checks in the instruction stream
        // the window's last, partial block: a wave-uniform case per number of steps left, so no gather fetches a line twice
        if (j < nsteps) tail_cases<1, U>(nsteps - j, block);
    }
}

// kWavesHint: what the allocator is told a wave is worth (amdgpu_waves_per_eu), chosen from the compile of THIS kernel (DESIGN.md
// 3.16, the register table), not from the fp32 table: the accumulator is 4 registers wider.
template <int G, bool OFF32>
constexpr int kWavesHint = G == 64 && OFF32 ? 6 : G >= 32 ? 5 : 7;

template <int G, bool OFF32, int U, int WPB>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(kWavesHint<G, OFF32>))) void spmm_flat_bf16_kernel(PlanView p, const flex_bf16 *__restrict__ B,
                                                                                                                  flex_bf16 *__restrict__ C) {
    __shared__ uint2 lds_rec[WPB][kWindowRecs<G>];
    const int lane = threadIdx.x & 63;
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint32_t tile, ktiles, chunk;
    if (!place_of_wave<G, WPB>(p, wib, tile, ktiles, chunk)) return;
    const int c0 = tile * (4 * G) + (lane % G) * 4;  // first of this lane's 4 words (8 columns)
    const bool col_ok = c0 < p.k;                    // k is a multiple of 4 words
    ChunkRegs d;
    if (!load_chunk<G>(p, chunk, lane, d)) return;
    compute_chunk_bf16<G, OFF32, U>(p, d, lds_rec[wib], reinterpret_cast<const char *>(B), reinterpret_cast<uint32_t *>(C), lane, c0, col_ok, tile);
}

// C[row, :] = rn_bf16(partial[first, :] + partial[first + 1, :] + ...) in that fixed order, in fp32: spmm_fixup_kernel with a lane on two
// adjacent columns (8-byte loads, one 4-byte store).  k: elements; ldcw: words between rows of C.
__global__ __launch_bounds__(256) void spmm_fixup_bf16_kernel(const float *__restrict__ partial, const SplitRow *__restrict__ rows, uint32_t n_rows,
                                                              int k, int ldcw, uint32_t *__restrict__ Cw) {
    const int lane = threadIdx.x & 63;
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x * kWavesPerBlock + wib;
    if (i >= n_rows) return;
    const SplitRow sr = rows[i];
    for (int c = lane; c < k / 2; c += 64) {
        const float *p = partial + static_cast<uint64_t>(sr.first) * k + 2 * c;
        float2 s = make_float2(0.f, 0.f);
        uint32_t j = 0;
        for (; j + 8 <= sr.count; j += 8) {
            float2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float2 *>(p + static_cast<uint64_t>(j + u) * k);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s.x += v[u].x;
                s.y += v[u].y;
            }
        }
        float2 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (j + u < sr.count) ? *reinterpret_cast<const float2 *>(p + static_cast<uint64_t>(j + u) * k) : make_float2(0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j + u < sr.count) {
                s.x += v[u].x;
                s.y += v[u].y;
            }
        Cw[static_cast<uint64_t>(sr.row) * ldcw + c] = bf16_bits(s.x) | (bf16_bits(s.y) << 16);
    }
}

template <int G, bool OFF32, int U>
int launch_flat(const PlanView &v, const flex_bf16 *dB, flex_bf16 *dC, hipStream_t s) {
    // the grid of launch_v4 (spmm_kernels.hip): one wave per chunk-table entry, a multiple of 8 workgroups, tiles of 4 G words
    uint32_t nblk = (v.n_chunks + kWavesPerBlock - 1) / kWavesPerBlock;
    nblk = (nblk + kXcds - 1) / kXcds * kXcds;
    const uint32_t ktiles = (v.k + 4 * G - 1) / (4 * G);
    const dim3 grid = v.tile_group ? dim3(nblk * ktiles, 1) : dim3(nblk, ktiles);
    hipLaunchKernelGGL((spmm_flat_bf16_kernel<G, OFF32, U, kWavesPerBlock>), grid, dim3(64 * kWavesPerBlock), v.lds_extra, s, v, dB, dC);
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

template <int G, int U>
int launch_flat_off(const PlanView &v, bool off32, const flex_bf16 *dB, flex_bf16 *dC, hipStream_t s) {
    return off32 ? launch_flat<G, true, U>(v, dB, dC, s) : launch_flat<G, false, U>(v, dB, dC, s);
}

// G x OFF32 x the U of launch_spmm's switch (no unroll = 8 experiment, no stamped twin)
int launch(const PlanView &v, int lanes_per_nz, bool off32, const flex_bf16 *dB, flex_bf16 *dC, hipStream_t s) {
    if (v.n_chunks == 0) return FLEX_OK;
    switch (lanes_per_nz) {
        case 4: return launch_flat_off<4, 4>(v, off32, dB, dC, s);
        case 8: return launch_flat_off<8, 4>(v, off32, dB, dC, s);
        case 16: return launch_flat_off<16, 4>(v, off32, dB, dC, s);
        case 32: return launch_flat_off<32, 8>(v, off32, dB, dC, s);
        case 64: return launch_flat_off<64, 8>(v, off32, dB, dC, s);
        default: return FLEX_ERR_UNSUPPORTED;
    }
}

int launch_fixup(const flex_plan *p, flex_bf16 *dC, hipStream_t s) {
    if (p->n_split == 0) return FLEX_OK;
    const uint32_t nblk = (p->n_split + kWavesPerBlock - 1) / kWavesPerBlock;
    hipLaunchKernelGGL(spmm_fixup_bf16_kernel, dim3(nblk), dim3(256), 0, s, p->d_partial.get(), p->d_split.get(), p->n_split, 2 * p->k, p->ldc,
                       reinterpret_cast<uint32_t *>(dC));
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // namespace spmm_bf16
}  // namespace flex

using namespace flex;

extern "C" int flex_spmm_bf16(flex_plan *p, const flex_bf16 *dB, flex_bf16 *dC, flex_stream_t stream) {
    if (!p || !p->bf16) return FLEX_ERR_INVALID;
    if (p->m == 0) return FLEX_OK;
    if (!dC || (!dB && p->nnz > 0)) return FLEX_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(dB) | reinterpret_cast<uintptr_t>(dC)) % 16 != 0) return FLEX_ERR_UNSUPPORTED;  // only the vector form is built
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const LaunchGuard guard(p, s);  // the split rows' workspace: one launch of a plan at a time, as flex_spmm (plan.h)
    if (guard.begin() != FLEX_OK) return FLEX_ERR_INVALID;
    int rc = spmm_bf16::launch(plan_view(p, false, nullptr), p->lanes_per_nz, p->off32, dB, dC, s);
    if (rc == FLEX_OK) rc = spmm_bf16::launch_fixup(p, dC, s);
    if (rc == FLEX_OK) guard.done();
    return rc;
}
