// spmm_kernels.hip -- gfx950 (CDNA4, wave64) SpMM kernels of libflex_spmm.so.
//
// Replaces the reference's kernel family flex.cu:80-4124 (selected kernel
// alpha_w_atomic_spmm_v36, flex.cu:4008-4124; closest in structure: spmm_test2,
// flex.cu:190-273).  None of that code is reused.  Design:
//
//  * A *task* is one C row (or one piece of a long row); a *chunk* is a short
//    contiguous run of tasks cut by the host planner so that every chunk holds
//    about the same number of (col,val) records.
//  * One wave per chunk; workgroup ids are remapped so that each XCD (private
//    4 MiB L2) walks its own contiguous eighth of the schedule with one cursor:
//    rows that are neighbours in the schedule share B rows through that L2, and
//    the hardware dispatcher (a new workgroup whenever one retires) does the
//    load balancing that the reference builds by hand with per-SM buckets plus
//    a balance bucket (flex.cu:2447-2518, 4008-4124).
//  * k/4 lanes (G) cooperate on one record, each lane owning 4 consecutive
//    columns of C, so one wave-instruction gathers 64/G different B rows with
//    16-byte loads (k=128: two 512-B rows = 1 KiB per global_load_dwordx4;
//    k=32: eight 128-B rows).  The S = 64/G slots of a wave walk the SAME row
//    and are combined by a log2(S)-step xor-shuffle at row end -- or, for SHORT rows on
//    the tiles of four or more slots, S DIFFERENT rows of one bundle (a task that holds
//    a row per slot): nothing to combine, one 16-byte store per lane at the bundle's end
//    (plan_build.cpp form_tasks; ≙ the reference's narrow kernel, flex.cu:81-118).
//  * Rows of GNN graphs are short (median degree < 10), so the wave treats ALL
//    records of a chunk as one stream of steps (S records per step; the planner
//    pads every row to a multiple of S with records that share its last value): the records are
//    fetched once, coalesced, into a wave-private LDS slice, then blocks of U
//    gathers are issued back to back regardless of row boundaries, and a
//    wave-uniform scalar check after each step flushes the accumulator when a row
//    ends.  No barriers: LDS slices are private to a wave.
//  * C is written once with non-temporal 16-byte stores; rows cut into several
//    pieces go to k-wide partial slots instead and are summed in piece order -- by
//    spmm_fixup_kernel after this launch (large launches: it needs nothing beyond
//    stream order) or by whichever piece finishes last inside the same launch (small
//    ones, where a second kernel boundary would show; flex_plan_tuning.split_rows forces).  Deterministic either way;
//    the reference uses atomicAdd for its split rows, mat.cu:816-824.
#include "spmm_device.h"

namespace flex {
namespace {

using namespace spmm_dev;  // gather4, the cross-slot sums, the record windows and their staging (shared with spmm_bf16_kernels.hip)

// What a lane holds of a finished row, and which column(s) of its tile.  Measured on MI355X (tools/ab.py):
// the scattered form saves ~30 VALU instructions per row at G=8, where short rows make the epilogue the
// largest VALU term (flickr k=32: 17.3 -> 14.8 us); at G=16/32 it only trades 16-byte stores from the 16/32
// lanes of one slot for 4/8-byte stores strided across the wave (flickr k=64 +3.5 %, k=128 +-0), so those
// widths keep the all-reduce and the contiguous float4 store:
//   G=64: 4 values at c0, every lane          (no reduction)
//   G=32: 4 values at c0, lanes of slot 0     (all-reduce over 2 slots)
//   G=16: 4 values at c0, lanes of slot 0     (all-reduce over 4 slots)
//   G=8 : 1 value  at c0 + 2*bit3 + bit4, lower wave half  (pair8 twice, pair16, then both halves summed)
//   G=4 : 1 value  at c0 + 2*bit2 + bit3, lanes 0-15       (pair4 twice, pair8, then the four 16-lane rows summed)   [k <= 16]
template <int G>
struct RowOut {
    static constexpr int kVals = G <= 8 ? 1 : 4;
    float v[kVals];
};

template <int G>
__device__ __forceinline__ int row_out_col(int lane, int c0) {
    if constexpr (G == 8) return c0 + 2 * ((lane >> 3) & 1) + ((lane >> 4) & 1);
    else if constexpr (G == 4) return c0 + 2 * ((lane >> 2) & 1) + ((lane >> 3) & 1);
    else return c0;
}

template <int G>
__device__ __forceinline__ bool row_out_lane(int lane) {  // does this lane store
    return G == 8 ? lane < 32 : G == 4 ? lane < 16 : lane < G;
}

template <int G>
__device__ __forceinline__ RowOut<G> reduce_row(const float4 &acc) {
    RowOut<G> o;
    if constexpr (G == 8) {
        const float t = pair16(pair8(acc.x, acc.z), pair8(acc.y, acc.w));
        o.v[0] = pair32(t, t);  // both halves hold the same columns: plain sum, the lower half stores
    } else if constexpr (G == 4) {
        const float t = pair8(pair4(acc.x, acc.z), pair4(acc.y, acc.w));
        const float h = pair16(t, t);  // the four 16-lane rows hold the same columns: plain sums, the first row stores
        o.v[0] = pair32(h, h);
    } else {
        float4 r = acc;
        if constexpr (G <= 16) {
            r.x = pair16(r.x, r.x);
            r.y = pair16(r.y, r.y);
            r.z = pair16(r.z, r.z);
            r.w = pair16(r.w, r.w);
        }
        if constexpr (G <= 32) {
            r.x = pair32(r.x, r.x);
            r.y = pair32(r.y, r.y);
            r.z = pair32(r.z, r.z);
            r.w = pair32(r.w, r.w);
        }
        o.v[0] = r.x; o.v[1] = r.y; o.v[2] = r.z; o.v[3] = r.w;
    }
    return o;
}

// non-temporal store of a lane's share of a C row (ptr already points at its first column)
template <int G>
__device__ __forceinline__ void store_row_out(float *ptr, const RowOut<G> &o) {
    if constexpr (RowOut<G>::kVals == 4) {
        const v4f val = {o.v[0], o.v[1], o.v[2], o.v[3]};
        __builtin_nontemporal_store(val, reinterpret_cast<v4f *>(ptr));
    } else {
        __builtin_nontemporal_store(o.v[0], ptr);
    }
}

// 16-byte agent-scope (sc1) load through a 64-bit address: served by the L2, never by this CU's L1.  The compiler does
// not count loads issued from inline asm, so the caller waits with wait_loads() before touching the values.
__device__ __forceinline__ v4f load_b128_sc1(const float *ptr) {
    v4f v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(v) : "v"(ptr) : "memory");
    return v;
}

template <int N>
__device__ __forceinline__ void wait_loads(v4f (&v)[N]) {
    static_assert(N == 8, "one batch of the piece sum");
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7])
                 :
                 : "memory");
}

[[maybe_unused]] __device__ __forceinline__ uint32_t xcc_id() {
    uint32_t x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    return x & (kXcds - 1);
}


// All the work of one chunk once its header {first task, #tasks, first record, end record} and its
// task descriptors (lane i: t_beg[t0+i], t_dst[t0+i]) are in registers.
template <int G, bool OFF32, int U>
__device__ __forceinline__ void compute_chunk(const PlanView &p, uint4 hdr, uint32_t my_beg, uint32_t my_dst,
                                              uint32_t my_bd0, uint32_t my_bd1, uint2 cx, uint2 *my_lds, const char *__restrict__ Bb,
                                              float *__restrict__ C, int lane, int c0, bool col_ok, uint32_t tile, uint32_t ktiles) {
    constexpr int S = 64 / G;
    const int slot = lane / G;
    const int k = p.k;
    const uint64_t ldc = static_cast<uint64_t>(p.ldc);
    // lanes past column k gather the tile's FIRST column instead: a line this record's gather touches anyway
    // (column 0 of the row would add a cache line per record to the last tile of a k that is not a multiple of 4G)
    const uint32_t lane_off = (col_ok ? c0 : c0 - (lane % G) * 4) * 4u;
    const uint64_t row_bytes = static_cast<uint64_t>(p.ldb) * 4u;

    const uint32_t nt = hdr.y, zb = hdr.z, ze = hdr.w;
    // A packed plan (wave-uniform): this chunk's records are values + 16-bit column differences, decoded by the staging step -- or, in a
    // wide chunk (one with a bundle), 8-byte records that start at cx.x of what `rec` holds instead of at zb.
    const bool packed_chunk = p.rec_packed != 0 && (cx.y & kChunkWide) == 0;
    const uint2 *__restrict__ rec = p.rec_packed != 0 ? p.rec + cx.x - zb : p.rec;
    uint32_t carry = 0;  // packed: the column the previous window ended on

    uint32_t ti = 0;                                          // current task
    uint32_t row_end = __builtin_amdgcn_readlane(my_beg, 1);  // where it ends in the record stream
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    const int out_col = row_out_col<G>(lane, c0);              // first column this lane stores of a finished row
    const bool out_ok = col_ok && row_out_lane<G>(lane);
    // Write out the task that ends at the current stream position (and any empty rows behind it).
    // row_end is kept at ~0 once the chunk's tasks are exhausted, so the per-step test in the hot
    // loop is ONE scalar compare.  A task whose destination carries kPartialFlag is a PIECE: one of several
    // partial sums of a C row (a row longer than one budget, or a row cut by column panel, plan_build.cpp); it goes to
    // its k-wide slot of `partial`, write-through when the pieces are combined inside this launch.
    auto flush = [&](uint32_t pos) {
        do {
            const uint32_t dst = __builtin_amdgcn_readlane(my_dst, ti);
            if ((dst & (kPartialFlag | kBundleFlag)) == (kPartialFlag | kBundleFlag)) {  // wave-uniform
                // a BUNDLE: slot s held row s of it all along -- nothing to reduce; every lane stores the 4 columns it owns of its
                // slot's row (G lanes x 16 bytes: the row's whole column tile).  The chunk's rows came in with the descriptors
                // (lane i: entries i and 64 + i of its part of bd_rows); the slot's lanes fetch theirs with one cross-lane read.
                if constexpr (kTileHasBundles<G>) {
                    const uint32_t first = dst & (kBundleRowsPerChunk - 1u);
                    const uint32_t held = first < 64u ? my_bd0 : my_bd1;
                    const uint32_t row = static_cast<uint32_t>(
                        __builtin_amdgcn_ds_bpermute(static_cast<int>(((first & 63u) + slot) << 2), static_cast<int>(held)));
                    if (col_ok && row != kBundleNoRow) {
                        const bool none = (row & kBundleZero) != 0;  // a row without nonzeros: zeros, whatever its slot summed
                        const v4f val = {none ? 0.f : acc.x, none ? 0.f : acc.y, none ? 0.f : acc.z, none ? 0.f : acc.w};
                        __builtin_nontemporal_store(val, reinterpret_cast<v4f *>(C + static_cast<uint64_t>(row & ~kBundleZero) * ldc + c0));
                    }
                }
            } else if (__builtin_expect((dst & kPartialFlag) != 0, 0)) {  // wave-uniform; the rare case on 1-D plans
                const float4 r = reduce_full<G>(acc);
                float *prow = p.partial + static_cast<uint64_t>(dst & ~kPartialFlag) * k;  // uniform
                if (slot == 0 && col_ok) {
                    // the lane's first column (c0) again, from the lane id: offsets and addresses of this rare path are formed here and not
                    // kept in registers across the gather loops
                    int l = lane;
                    asm volatile("" : "+v"(l));
                    const int col = static_cast<int>(tile) * (4 * G) + (l % G) * 4;
                    if (p.fused_fixup) {
                        const auto prsrc = __builtin_amdgcn_make_buffer_rsrc(prow, 0, k * 4, 0x00020000);
                        const v4u pv = {__float_as_uint(r.x), __float_as_uint(r.y), __float_as_uint(r.z), __float_as_uint(r.w)};
                        __builtin_amdgcn_raw_buffer_store_b128(pv, prsrc, col * 4, 0, 16 /* sc1 */);
                    } else {  // combined by spmm_fixup_kernel after this launch
                        *reinterpret_cast<float4 *>(prow + col) = r;
                    }
                }
            } else {
                const RowOut<G> o = reduce_row<G>(acc);
                if (out_ok) store_row_out<G>(C + static_cast<uint64_t>(dst) * ldc + out_col, o);
            }
            acc = {0.f, 0.f, 0.f, 0.f};
            ++ti;
            row_end = ti < nt ? __builtin_amdgcn_readlane(my_beg, ti + 1) : 0xFFFFFFFFu;
        } while (row_end == pos);
    };
    if (nt == 0) row_end = 0xFFFFFFFFu;
    if (row_end == zb) flush(zb);  // leading empty rows

    uint32_t pos = zb;  // stream position after the steps consumed so far
    for (uint32_t wz = zb; wz < ze; wz += kWindowRecs<G>) {
        const uint32_t wn = min(static_cast<uint32_t>(kWindowRecs<G>), ze - wz);
        // stage this window's records: coalesced loads of two records per lane (1 KiB per wave load, one ds_write_b128 each; the
        // one-slot tile and the packed stream: spmm_device.h)
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
                fma4(acc, as_f32(r[u].y), b[u]);
                pos += S;
                if (pos == row_end) flush(pos);
            }
        };
        for (; j + U <= nsteps; j += U) block(std::integral_constant<int, U>{});  // full blocks: no bound checks in the instruction stream
        // the window's last, partial block: a wave-uniform case per number of steps left, so no gather fetches a line twice
        if (j < nsteps) tail_cases<1, U>(nsteps - j, block);
    }
    // Pieces are combined INSIDE this launch by whichever piece arrives last (cdna guide G16, counter form with
    // write-through payload): (1) every partial sum of this chunk was stored write-through (sc1), so it is at
    // device scope once the store completes; (2) the wave drains its stores; (3) lane i bumps the arrival counter of
    // task i's row (agent-scope atomic; t_aux = {row's index in `split`, #pieces}); (4) a lane whose add returns
    // count-1 knows every piece of that row is visible: the wave reads them with sc1 loads (never through a CU's
    // L1) and adds them in PIECE order -- the sum is reproducible although the reducer is not -- S rows at a time,
    // one per slot, and re-arms the counters for the next launch.  OPT-IN since ABI 3 (p.fused_fixup): by default the
    // pieces are left to spmm_fixup_kernel, which measured faster on the large shapes and needs no such argument.
    // Why RELAXED + sc1 instead of an acq_rel atomic: a release at agent scope is `buffer_wbl2 sc1`, a
    // write-back of the whole XCD L2 (1.7-6.5 us, MI355X_MICROARCH.md "Workgroup dispatch ... visibility"),
    // paid by every chunk.  The form used here is that guide's hand-off "each storing wave for itself:
    // sc1 stores of whole 16-B granules -> the wave's own s_waitcnt vmcnt(0) -> agent-scope atomic add;
    // the wave whose add returned last reads every byte with ... sc1 loads" (its measured table of sc1
    // hand-offs on gfx950 / ROCm 7.2; measured, not an architectural guarantee, hence the 300-launch
    // test under uneven load, tests/test_gpu_spmm.py).  The workspace makes a plan non-reentrant: one
    // launch of a plan at a time (include/flex_spmm.h, flex_spmm).
    const bool mine_partial = static_cast<uint32_t>(lane) < nt && (my_dst & (kPartialFlag | kBundleFlag)) == kPartialFlag;
    if (p.fused_fixup && __builtin_amdgcn_ballot_w64(mine_partial) != 0) {  // wave-uniform
        // t_aux is read here and nowhere else: fetched now, under the drain of the stores, not with the chunk's other descriptors --
        // the two-launch form never loads it, and no register holds it across the gather loops
        const uint2 my_aux = mine_partial ? p.t_aux[hdr.x + lane] : make_uint2(0u, 0u);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint32_t arrived = 0;
        if (mine_partial)
            arrived = __hip_atomic_fetch_add(p.split_cnt + static_cast<uint64_t>(my_aux.x) * ktiles + tile, 1u,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint64_t done = __builtin_amdgcn_ballot_w64(mine_partial && arrived + 1 == my_aux.y);
        while (done != 0) {  // wave-uniform: up to S completed rows per round, slot s takes the s-th
            int take = -1;
#pragma unroll
            for (int s2 = 0; s2 < S; ++s2) {
                if (done != 0) {
                    const int i = __builtin_ctzll(done);
                    done &= done - 1;
                    if (slot == s2) take = i;
                }
            }
            const uint32_t sidx = __shfl(my_aux.x, take < 0 ? 0 : take);
            if (take >= 0) {
                const SplitRow sr = p.split[sidx];
                if (col_ok) {
                    int l = lane;  // c0 again, from the lane id (as in flush: nothing of this tail stays in registers across the gather loops)
                    asm volatile("" : "+v"(l));
                    const int c0 = static_cast<int>(tile) * (4 * G) + (l % G) * 4;
                    const float *base = p.partial + static_cast<uint64_t>(sr.first) * k + c0;
                    float4 s4 = {0.f, 0.f, 0.f, 0.f};
                    for (uint32_t j = 0; j < sr.count; j += 8) {
                        v4f v[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) v[u] = load_b128_sc1(base + static_cast<uint64_t>(min(j + u, sr.count - 1)) * k);
                        wait_loads(v);
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            if (j + u < sr.count) {
                                s4.x += v[u].x;
                                s4.y += v[u].y;
                                s4.z += v[u].z;
                                s4.w += v[u].w;
                            }
                        }
                    }
                    const v4f val = {s4.x, s4.y, s4.z, s4.w};
                    __builtin_nontemporal_store(val, reinterpret_cast<v4f *>(C + static_cast<uint64_t>(sr.row) * ldc + c0));
                }
                if (lane % G == 0)
                    __hip_atomic_store(p.split_cnt + static_cast<uint64_t>(sidx) * ktiles + tile, 0u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// G lanes per record, 4 columns per lane; covers k <= 4*G per blockIdx.y tile.
// One wave per chunk.  The hardware deals consecutive workgroup ids round-robin over the 8
// XCDs, so workgroup b is given chunk group (b % 8) * cpx + b / 8: XCD x walks the x-th
// contiguous eighth of the schedule with ONE cursor, and its resident waves form a sliding
// window over neighbouring rows whose shared B rows stay in that XCD's 4 MiB L2.  (A
// persistent variant with per-XCD ticket queues was measured and rejected: DESIGN.md 3.4.)
// STAMP = true is the measuring twin of the product kernel (flex_plan_measure_imbalance; ≙ the reference's per-warp
// %smid + clock() stamps, flex.cu:27-79): the same code plus, per wave, two reads of the 100 MHz constant clock and one
// 24-byte record {start, end, XCC id << 32 | HW_ID}.  The product launches (flex_spmm) never use it.
// amdgpu_waves_per_eu: the register count is decided in the gather loop (U float4 + U records + the chunk's descriptors); the hint tells
// the allocator what the next wave is worth, so that loop invariants of the staging step and of the rare flush paths are recomputed
// instead of kept.  G <= 8: 8 waves per SIMD (64 VGPRs); G = 16: 7 asked, 8 reached (56-58 VGPRs); wide tiles (U = 8): 7 with 32-bit
// offsets (72 VGPRs), 6 with 64-bit row addressing (76-78); all without scratch, checked with `make asm`.  The FLEX_U=8 experiment on the narrow tiles is left alone.
template <int G, bool OFF32, int U, int WPB, bool STAMP = false>
__global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(U == (G >= 32 ? 8 : 4) ? (G >= 32 ? (OFF32 ? 7 : 6) : G >= 16 ? 7 : 8) : 4))) void spmm_flat_kernel(PlanView p, const float *__restrict__ B,
                                                             float *__restrict__ C) {
    __shared__ uint2 lds_rec[WPB][kWindowRecs<G>];
    const int lane = threadIdx.x & 63;
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Which (workgroup of the chunk table, column tile) this workgroup is.  Classic: blockIdx.y = tile, one pass over the whole
    // table per tile.  Grouped (p.tile_group): a 1-D grid in which every XCD slice is walked group by group, the tiles of a group
    // back to back -- a group's records are then re-read from the Infinity Cache instead of HBM.
    uint32_t tile = blockIdx.y, ktiles = gridDim.y, bid;
    if (p.tile_group == 0) {
        const uint32_t cpx = gridDim.x / kXcds;  // gridDim.x % 8 == 0
        bid = p.xcd_remap ? (blockIdx.x % kXcds) * cpx + (blockIdx.x / kXcds) : blockIdx.x;
    } else {
        ktiles = (p.k + 4 * G - 1) / (4 * G);
        const uint32_t nwg = gridDim.x / ktiles;                        // workgroups of one pass (a multiple of 8)
        const uint32_t slice = p.xcd_remap ? nwg / kXcds : nwg;         // ... of one XCD's slice
        const uint32_t l = p.xcd_remap ? blockIdx.x / kXcds : blockIdx.x;  // position in this XCD's extended slice [0, slice * ktiles)
        const uint32_t g = l / (p.tile_group * ktiles), r = l % (p.tile_group * ktiles);
        const uint32_t g0 = g * p.tile_group, gs = min(p.tile_group, slice - g0);  // the last group of a slice may be short
        tile = r / gs;
        const uint32_t in_slice = g0 + r % gs;
        if (tile >= ktiles) return;  // only past the end of a short last group
        bid = p.xcd_remap ? (blockIdx.x % kXcds) * slice + in_slice : in_slice;
    }
    const uint32_t chunk = bid * WPB + wib;
    if (chunk >= p.n_chunks) return;
    const int c0 = tile * (4 * G) + (lane % G) * 4;  // first of this lane's 4 columns
    const bool col_ok = c0 < p.k;                            // k % 4 == 0 on this path
    // A chunk holds at most 63 tasks (planner invariant): all descriptors come with one coalesced
    // load per array and are handed out with v_readlane; the header carries the record range, so
    // the record fetch does not wait for them: header -> {descriptors, records} -> gathers.
    const uint4 hdr = p.chunk[chunk];
    // the chunk's part of the bundle rows: fetched beside the header, handed out at the end of each bundle (compute_chunk, flush)
    uint2 cb = make_uint2(0u, 0u);
    if constexpr (kTileHasBundles<G>)
        if (p.bd_rows != nullptr) cb = p.chunk_bd[chunk];  // uniform
    // packed plans: the chunk's exception table {first, entries}, or {first wide record, kChunkWide}
    uint2 cx = make_uint2(0u, 0u);
    if (p.rec_packed != 0) cx = p.chunk_exc[chunk];  // uniform
    if (hdr.y == 0) return;  // an empty entry that pads this XCD's slice of the table (plan_build.cpp, build_chunk_table)
    const uint32_t my_beg = (static_cast<uint32_t>(lane) <= hdr.y) ? p.t_beg[hdr.x + lane] : 0u;
    const uint32_t my_dst = (static_cast<uint32_t>(lane) < hdr.y) ? p.t_dst[hdr.x + lane] : 0u;
    uint32_t my_bd0 = kBundleNoRow, my_bd1 = kBundleNoRow;
    if (kTileHasBundles<G> && cb.y != 0) {  // uniform
        if (static_cast<uint32_t>(lane) < cb.y) my_bd0 = p.bd_rows[cb.x + lane];
        if (static_cast<uint32_t>(lane) + 64u < cb.y) my_bd1 = p.bd_rows[cb.x + 64u + lane];
    }
    uint64_t stamp_t0 = 0;
    if constexpr (STAMP) stamp_t0 = __builtin_amdgcn_s_memrealtime();
    compute_chunk<G, OFF32, U>(p, hdr, my_beg, my_dst, my_bd0, my_bd1, cx, lds_rec[wib], reinterpret_cast<const char *>(B), C, lane, c0, col_ok, tile, ktiles);
    if constexpr (STAMP) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // the wave's last stores have left
        const uint64_t stamp_t1 = __builtin_amdgcn_s_memrealtime();
        if (lane == 0 && p.trace != nullptr) {
            uint32_t hw_id;
            asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
            uint64_t *log = p.trace + (static_cast<uint64_t>(tile) * p.n_chunks + chunk) * 3;
            log[0] = stamp_t0;
            log[1] = stamp_t1;
            log[2] = (static_cast<uint64_t>(xcc_id()) << 32) | hw_id;
        }
    }
}

// Any k (k % 4 != 0 or unaligned B/C): one wave per task, lane owns columns
// lane, lane+64, lane+128, lane+192 of the blockIdx.y-th 256-column tile.
template <bool OFF32>
__global__ __launch_bounds__(256) void spmm_generic_kernel(PlanView p, const float *__restrict__ B,
                                                           float *__restrict__ C, uint32_t slots_per_step) {
    const int lane = threadIdx.x & 63;
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t cpx = gridDim.x / kXcds;
    const uint32_t bid = p.xcd_remap ? (blockIdx.x % kXcds) * cpx + (blockIdx.x / kXcds) : blockIdx.x;
    const uint32_t w = bid * kWavesPerBlock + wib;
    if (w >= p.n_chunks) return;
    const int k = p.k;
    const int cb = blockIdx.y * 256 + lane;
    const uint32_t t0 = p.chunk[w].x, t1 = t0 + p.chunk[w].y;
    // A packed plan launched with operands that are not 16-byte aligned: a wide chunk's records start at cx.x of what `rec` holds;
    // any other chunk is decoded record by record, every lane for itself (the exceptions are sorted by position, tasks run in order).
    uint2 cx = make_uint2(0u, 0u);
    if (p.rec_packed != 0 && t1 > t0) cx = p.chunk_exc[w];
    const bool packed_chunk = p.rec_packed != 0 && (cx.y & kChunkWide) == 0;
    const uint32_t cz = p.chunk[w].z;
    const uint2 *__restrict__ rec = p.rec_packed != 0 ? p.rec + cx.x - cz : p.rec;
    uint32_t ei = 0;  // packed: exceptions of the chunk consumed so far
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t zb = p.t_beg[t], ze = p.t_beg[t + 1];
        const uint32_t dst = p.t_dst[t];
        if ((dst & (kPartialFlag | kBundleFlag)) == (kPartialFlag | kBundleFlag)) {  // a bundle: its rows one after the other
            const uint2 a = p.t_aux[t];                                             // {first entry in bd_rows, steps}
            const uint32_t slots = slots_per_step;                                  // record j of row s at zb + j * slots + s
            for (uint32_t s = 0; s < slots; ++s) {
                const uint32_t row = p.bd_rows[a.x + s];
                if (row == kBundleNoRow) continue;
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
                if ((row & kBundleZero) == 0) {
                    for (uint32_t j = 0; j < a.y; ++j) {
                        const uint2 r = rec[zb + j * slots + s];
                        const float v = as_f32(r.y);
                        const float *brow = OFF32 ? reinterpret_cast<const float *>(reinterpret_cast<const char *>(B) + r.x)
                                                  : B + static_cast<uint64_t>(r.x) * p.ldb;
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int c = cb + 64 * i;
                            if (c < k) acc[i] = fmaf(v, brow[c], acc[i]);
                        }
                    }
                }
                float *orow = C + static_cast<uint64_t>(row & ~kBundleZero) * p.ldc;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = cb + 64 * i;
                    if (c < k) orow[c] = acc[i];
                }
            }
            continue;
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t col = packed_chunk ? p.t_col0[t] : 0u;
        for (uint32_t z = zb; z < ze; ++z) {
            uint2 r;
            if (packed_chunk) {
                uint32_t d = p.rec_dcol[z];  // 0 on the task's first record
                if (ei < cx.y && p.exc[cx.x + ei].x == z - cz) d += p.exc[cx.x + ei++].y;
                col += d;
                r = make_uint2(OFF32 ? col * (static_cast<uint32_t>(p.ldb) * 4u) : col, __float_as_uint(p.rec_val[z]));
            } else {
                r = rec[z];
            }
            const float v = as_f32(r.y);
            const float *brow = OFF32 ? reinterpret_cast<const float *>(reinterpret_cast<const char *>(B) + r.x)
                                      : B + static_cast<uint64_t>(r.x) * p.ldb;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = cb + 64 * i;
                if (c < k) acc[i] = fmaf(v, brow[c], acc[i]);
            }
        }
        float *orow = (dst & kPartialFlag) ? p.partial + static_cast<uint64_t>(dst & ~kPartialFlag) * k
                                           : C + static_cast<uint64_t>(dst) * p.ldc;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = cb + 64 * i;
            if (c < k) orow[c] = acc[i];
        }
    }
}

// C[row,:] = partial[first,:] + partial[first+1,:] + ... in that fixed order.  Eight pieces are
// loaded before the first add so the (tiny) kernel costs a couple of memory round trips, not
// one per piece; the adds stay strictly in piece order, so the result is reproducible.
__device__ __forceinline__ void fixup_scalar(const float *__restrict__ partial, const SplitRow *__restrict__ rows, uint32_t n_rows,
                                             int k, int ldc, float *__restrict__ C) {
    const int lane = threadIdx.x & 63;
    const uint32_t wib = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t i = blockIdx.x * kWavesPerBlock + wib;
    if (i >= n_rows) return;
    const SplitRow sr = rows[i];
    for (int c = lane; c < k; c += 64) {
        const float *p = partial + static_cast<uint64_t>(sr.first) * k + c;
        float s = 0.f;
        uint32_t j = 0;
        for (; j + 8 <= sr.count; j += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[static_cast<uint64_t>(j + u) * k];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = (j + u < sr.count) ? p[static_cast<uint64_t>(j + u) * k] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j + u < sr.count) s += v[u];
        C[static_cast<uint64_t>(sr.row) * ldc + c] = s;
    }
}

// The same sums with 16-byte loads and stores (k % 4 == 0, partial and the rows of C 16-byte aligned): a lane owns 4 adjacent columns,
// a row takes lanes_per_row = min(k / 4, 64) lanes, and rows_per_wave = 64 / lanes_per_row rows share a wave (k = 128: two, k = 32:
// eight), each with its own piece count -- the loops diverge between rows of a wave, not inside a row.  Eight pieces in flight before
// the first add; every column starts from 0.f and adds its pieces strictly in piece order, as the scalar form does: the same bits.
__device__ __forceinline__ void fixup_vec4(const float *__restrict__ partial, const SplitRow *__restrict__ rows, uint32_t n_rows, int k,
                                           int ldc, float *__restrict__ C, uint32_t lanes_per_row, uint32_t rows_per_wave) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const uint32_t sub = lane / lanes_per_row;
    const uint32_t i = wave * rows_per_wave + sub;
    if (sub >= rows_per_wave || i >= n_rows) return;
    const SplitRow sr = rows[i];
    for (uint32_t c = (lane - sub * lanes_per_row) * 4u; c < static_cast<uint32_t>(k); c += lanes_per_row * 4u) {
        const float *p = partial + static_cast<uint64_t>(sr.first) * k + c;
        float4 s = {0.f, 0.f, 0.f, 0.f};
        uint32_t j = 0;
        for (; j + 8 <= sr.count; j += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4 *>(p + static_cast<uint64_t>(j + u) * k);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s.x += v[u].x;
                s.y += v[u].y;
                s.z += v[u].z;
                s.w += v[u].w;
            }
        }
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u)
            v[u] = (j + u < sr.count) ? *reinterpret_cast<const float4 *>(p + static_cast<uint64_t>(j + u) * k) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (j + u < sr.count) {
                s.x += v[u].x;
                s.y += v[u].y;
                s.z += v[u].z;
                s.w += v[u].w;
            }
        *reinterpret_cast<float4 *>(C + static_cast<uint64_t>(sr.row) * ldc + c) = s;
    }
}

// lanes_per_row = 0: the scalar form (launch_fixup decides; uniform over the launch)
__global__ __launch_bounds__(256) void spmm_fixup_kernel(const float *__restrict__ partial, const SplitRow *__restrict__ rows, uint32_t n_rows,
                                                         int k, int ldc, float *__restrict__ C, uint32_t lanes_per_row,
                                                         uint32_t rows_per_wave) {
    if (lanes_per_row != 0) fixup_vec4(partial, rows, n_rows, k, ldc, C, lanes_per_row, rows_per_wave);
    else fixup_scalar(partial, rows, n_rows, k, ldc, C);
}

// dst[r,:] = src[idx[r],:]  (≙ flexspmm_v9_permuteX, flex.cu:276-289)
template <bool VEC4>
__global__ __launch_bounds__(256) void gather_rows_kernel(float *__restrict__ dst, const float *__restrict__ src,
                                                          const int32_t *__restrict__ idx, int64_t n, int k) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + (threadIdx.x >> 6); r < n; r += nwaves) {
        const int64_t s = idx[r];
        if constexpr (VEC4) {
            const float4 *sp = reinterpret_cast<const float4 *>(src + s * k);
            float4 *dp = reinterpret_cast<float4 *>(dst + r * k);
            for (int c = lane; c < k / 4; c += 64) dp[c] = sp[c];
        } else {
            for (int c = lane; c < k; c += 64) dst[r * k + c] = src[s * k + c];
        }
    }
}

template <int G, bool OFF32, int U>
int launch_v4(const PlanView &v, const float *dB, float *dC, hipStream_t s) {
    // one wave per chunk-table entry, kWavesPerBlock entries per workgroup, a multiple of 8 workgroups so
    // the XCD slices are equal (build_chunk_table pads them).  2 or 8 waves per workgroup measured the same as 4
    // (the launch is not dispatch-bound: an empty kernel over the same grid takes 3.4 us)
    uint32_t nblk = (v.n_chunks + kWavesPerBlock - 1) / kWavesPerBlock;
    nblk = (nblk + kXcds - 1) / kXcds * kXcds;
    const uint32_t ktiles = (v.k + 4 * G - 1) / (4 * G);
    const dim3 grid = v.tile_group ? dim3(nblk * ktiles, 1) : dim3(nblk, ktiles);
    hipLaunchKernelGGL((spmm_flat_kernel<G, OFF32, U, kWavesPerBlock>), grid, dim3(64 * kWavesPerBlock), v.lds_extra, s, v, dB, dC);
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

template <int G, int U>
int launch_stamped(const PlanView &v, bool off32, const float *dB, float *dC, hipStream_t s) {
    uint32_t nblk = (v.n_chunks + kWavesPerBlock - 1) / kWavesPerBlock;
    nblk = (nblk + kXcds - 1) / kXcds * kXcds;
    const uint32_t ktiles = (v.k + 4 * G - 1) / (4 * G);
    const dim3 grid = v.tile_group ? dim3(nblk * ktiles, 1) : dim3(nblk, ktiles);
    if (off32)
        hipLaunchKernelGGL((spmm_flat_kernel<G, true, U, kWavesPerBlock, true>), grid, dim3(64 * kWavesPerBlock), v.lds_extra, s, v, dB, dC);
    else
        hipLaunchKernelGGL((spmm_flat_kernel<G, false, U, kWavesPerBlock, true>), grid, dim3(64 * kWavesPerBlock), v.lds_extra, s, v, dB, dC);
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

template <int G, int U>
int launch_v4_off(const PlanView &v, bool off32, const float *dB, float *dC, hipStream_t s) {
    return off32 ? launch_v4<G, true, U>(v, dB, dC, s) : launch_v4<G, false, U>(v, dB, dC, s);
}

}  // namespace

int launch_spmm(const PlanView &v, int lanes_per_nz, bool off32, bool vec4, const float *dB, float *dC,
                hipStream_t s, int unroll) {
    if (v.n_chunks == 0) return FLEX_OK;
    if (!vec4) {
        uint32_t nblk = (v.n_chunks + kWavesPerBlock - 1) / kWavesPerBlock;
        nblk = (nblk + kXcds - 1) / kXcds * kXcds;
        const uint32_t ktiles = (v.k + 255) / 256;
        if (off32)
            hipLaunchKernelGGL((spmm_generic_kernel<true>), dim3(nblk, ktiles), dim3(256), 0, s, v, dB, dC, 64u / static_cast<uint32_t>(lanes_per_nz));
        else
            hipLaunchKernelGGL((spmm_generic_kernel<false>), dim3(nblk, ktiles), dim3(256), 0, s, v, dB, dC, 64u / static_cast<uint32_t>(lanes_per_nz));
        FLEX_HIP_TRY(hipGetLastError());
        return FLEX_OK;
    }
    if (unroll == 8) {  // tuning experiments (FLEX_U=8): twice the gathers in flight per wave on the narrow tiles
        switch (lanes_per_nz) {
            case 8: return launch_v4_off<8, 8>(v, off32, dB, dC, s);
            case 16: return launch_v4_off<16, 8>(v, off32, dB, dC, s);
            default: break;
        }
    }
    switch (lanes_per_nz) {  // U: 4 KiB in flight per wave on the narrow tiles, 8 KiB on the wide ones (U=8 on G<=16 measured the same)
        case 4: return launch_v4_off<4, 4>(v, off32, dB, dC, s);
        case 8: return launch_v4_off<8, 4>(v, off32, dB, dC, s);
        case 16: return launch_v4_off<16, 4>(v, off32, dB, dC, s);
        case 32: return launch_v4_off<32, 8>(v, off32, dB, dC, s);
        case 64: return launch_v4_off<64, 8>(v, off32, dB, dC, s);
        default: return FLEX_ERR_UNSUPPORTED;
    }
}

// the stamped twin of what launch_spmm launches for aligned operands (v.trace must hold 3 words per (k-tile, chunk-table entry))
int launch_spmm_stamped(const PlanView &v, int lanes_per_nz, bool off32, const float *dB, float *dC, hipStream_t s) {
    if (v.n_chunks == 0) return FLEX_OK;
    switch (lanes_per_nz) {
        case 4: return launch_stamped<4, 4>(v, off32, dB, dC, s);
        case 8: return launch_stamped<8, 4>(v, off32, dB, dC, s);
        case 16: return launch_stamped<16, 4>(v, off32, dB, dC, s);
        case 32: return launch_stamped<32, 8>(v, off32, dB, dC, s);
        case 64: return launch_stamped<64, 8>(v, off32, dB, dC, s);
        default: return FLEX_ERR_UNSUPPORTED;
    }
}

// Registers / LDS / occupancy of the kernel launch_spmm would pick (≙ Kernel_Info, flex.cu:4933-4941).
int kernel_attributes(int lanes_per_nz, bool off32, bool vec4, hipFuncAttributes *attr, int *waves_per_cu) {
    const void *fn = nullptr;
    if (!vec4) {
        fn = off32 ? reinterpret_cast<const void *>(spmm_generic_kernel<true>) : reinterpret_cast<const void *>(spmm_generic_kernel<false>);
    } else {
        switch (lanes_per_nz) {
            case 4: fn = off32 ? reinterpret_cast<const void *>(spmm_flat_kernel<4, true, 4, kWavesPerBlock>) : reinterpret_cast<const void *>(spmm_flat_kernel<4, false, 4, kWavesPerBlock>); break;
            case 8: fn = off32 ? reinterpret_cast<const void *>(spmm_flat_kernel<8, true, 4, kWavesPerBlock>) : reinterpret_cast<const void *>(spmm_flat_kernel<8, false, 4, kWavesPerBlock>); break;
            case 16: fn = off32 ? reinterpret_cast<const void *>(spmm_flat_kernel<16, true, 4, kWavesPerBlock>) : reinterpret_cast<const void *>(spmm_flat_kernel<16, false, 4, kWavesPerBlock>); break;
            case 32: fn = off32 ? reinterpret_cast<const void *>(spmm_flat_kernel<32, true, 8, kWavesPerBlock>) : reinterpret_cast<const void *>(spmm_flat_kernel<32, false, 8, kWavesPerBlock>); break;
            case 64: fn = off32 ? reinterpret_cast<const void *>(spmm_flat_kernel<64, true, 8, kWavesPerBlock>) : reinterpret_cast<const void *>(spmm_flat_kernel<64, false, 8, kWavesPerBlock>); break;
            default: return FLEX_ERR_UNSUPPORTED;
        }
    }
    FLEX_HIP_TRY(hipFuncGetAttributes(attr, fn));
    int blocks = 0;
    FLEX_HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, 64 * kWavesPerBlock, 0));
    *waves_per_cu = blocks * kWavesPerBlock;
    return FLEX_OK;
}

int launch_fixup(const float *partial, const SplitRow *rows, uint32_t n_rows, int k, int ldc, float *dC, hipStream_t s) {
    if (n_rows == 0) return FLEX_OK;
    const bool vec4 = k >= 4 && k % 4 == 0 && ldc % 4 == 0 && (reinterpret_cast<uintptr_t>(partial) | reinterpret_cast<uintptr_t>(dC)) % 16 == 0;
    // the float4 form: a row on min(k / 4, 64) lanes, the wave's other lanes on further rows
    const uint32_t lanes_per_row = !vec4 ? 0u : k / 4 < 64 ? static_cast<uint32_t>(k / 4) : 64u, rows_per_wave = vec4 ? 64u / lanes_per_row : 1u;
    const uint32_t nwaves = (n_rows + rows_per_wave - 1) / rows_per_wave;
    hipLaunchKernelGGL(spmm_fixup_kernel, dim3((nwaves + kWavesPerBlock - 1) / kWavesPerBlock), dim3(256), 0, s, partial, rows, n_rows, k, ldc,
                       dC, lanes_per_row, rows_per_wave);
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

int launch_gather_rows(float *dst, const float *src, const int32_t *idx, int64_t n, int k, hipStream_t s) {
    if (n <= 0) return FLEX_OK;
    const int64_t want = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    const uint32_t nblk = static_cast<uint32_t>(want < 2048 ? want : 2048);  // grid-stride beyond 8 blocks/CU
    const bool vec4 = (k % 4 == 0) && ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) % 16 == 0);
    if (vec4)
        hipLaunchKernelGGL((gather_rows_kernel<true>), dim3(nblk), dim3(256), 0, s, dst, src, idx, n, k);
    else
        hipLaunchKernelGGL((gather_rows_kernel<false>), dim3(nblk), dim3(256), 0, s, dst, src, idx, n, k);
    FLEX_HIP_TRY(hipGetLastError());
    return FLEX_OK;
}

}  // namespace flex
