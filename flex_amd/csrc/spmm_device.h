// spmm_device.h -- the device text the SpMM kernels share: the 16-byte B-row gather, the cross-slot sums of a row's end, the record
// windows of a wave's LDS slice and their staging from the 8-byte and the packed record stream, and a workgroup's place in the chunk
// table.  Used by spmm_kernels.hip (fp32: spmm_flat_kernel) and spmm_bf16_kernels.hip (bf16 B and C: spmm_flat_bf16_kernel), which
// walk a chunk in the same way and differ in what a gathered word holds and in how a finished row is stored.
#pragma once
#include <type_traits>

#include "internal.h"

namespace flex {
namespace spmm_dev {
__device__ __forceinline__ float as_f32(uint32_t u) { return __uint_as_float(u); }

template <bool OFF32>
__device__ __forceinline__ float4 gather4(const char *__restrict__ Bb, uint32_t recx, uint32_t lane_off,
                                          uint64_t row_bytes) {
    if constexpr (OFF32) {
        // base (SGPR pair) + 32-bit VGPR offset: global_load_dwordx4 v, v_off, s[base]
        return *reinterpret_cast<const float4 *>(Bb + static_cast<uint32_t>(recx + lane_off));
    } else {
        return *reinterpret_cast<const float4 *>(Bb + (static_cast<uint64_t>(recx) * row_bytes + lane_off));
    }
}

__device__ __forceinline__ void fma4(float4 &acc, float v, const float4 &b) {
    acc.x = fmaf(v, b.x, acc.x);
    acc.y = fmaf(v, b.y, acc.y);
    acc.z = fmaf(v, b.z, acc.z);
    acc.w = fmaf(v, b.w, acc.w);
}

typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));

// Row epilogue.  The S = 64/G slots of a wave each hold a partial float4 of the same C row.  They are
// combined by a reduce-SCATTER, not an all-reduce: at every level a lane adds its partner's half of the
// values and hands the other half over, so the value count halves with the lane distance and the row ends
// up spread over the lanes -- one cross-lane instruction and one add per PAIR of values, no copies:
//   pair8  (a,b): lanes with bit 3 clear get a[l]+a[l^8],  the others b[l]+b[l^8]   (two masked DPP adds)
//   pair16 (a,b): even 16-lane rows get a[l]+a[l^16], odd rows b[l]+b[l^16]         (v_permlane16_swap + add)
//   pair32 (a,b): the lower wave half gets a[l]+a[l^32], the upper half b[l]+b[l^32] (v_permlane32_swap + add)
__device__ __forceinline__ float pair8(float a, float b) {
    float r;
    // row_ror:8 = the lane 8 over in the same 16-lane row; bank_mask picks lanes 0-7 / 8-15 of every row.
    // s_nop: a DPP read needs two wait states after a VALU write of its source, and the compiler's hazard
    // recognizer does not look inside inline asm.
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %1, %1 row_ror:8 row_mask:0xf bank_mask:0x3\n\t"
        "v_add_f32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xc"
        : "=&v"(r)
        : "v"(a), "v"(b));
    return r;
}

// pair4 (a,b): lanes with bit 2 clear get a[l]+a[l^4], the others b[l]+b[l^4].  l^4 swaps quads 0<->1 and 2<->3 of a 16-lane row:
// quads 0 and 2 (bank_mask 0x5) take their partner from the quad ABOVE (row_ror:12 = rotate left by 4), quads 1 and 3
// (bank_mask 0xa) from the quad below (row_ror:4).
__device__ __forceinline__ float pair4(float a, float b) {
    float r;
    asm("s_nop 1\n\t"
        "v_add_f32_dpp %0, %1, %1 row_ror:12 row_mask:0xf bank_mask:0x5\n\t"
        "v_add_f32_dpp %0, %2, %2 row_ror:4 row_mask:0xf bank_mask:0xa"
        : "=&v"(r)
        : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ float pair16(float a, float b) {
    // v_permlane16_swap exchanges the odd rows of its first operand with the even rows of its second:
    // (a,b) -> {a0,b0,a2,b2}, {a1,b1,a3,b3}; their sum is a0+a1 on row 0, b0+b1 on row 1, ...
    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

__device__ __forceinline__ float pair32(float a, float b) {
    // v_permlane32_swap exchanges the upper half of its first operand with the lower half of its second:
    // (a,b) -> {a.lo,b.lo}, {a.hi,b.hi}; their sum is a.lo+a.hi on the lower half, b.lo+b.hi on the upper
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

// All-reduce form for every G: afterwards EVERY lane holds the sum over the S slots of its 4 columns, so the lanes of
// slot 0 can write the row as contiguous float4s.  Used for pieces (partial sums of rows that other chunks hold pieces
// of): their stores are write-through (sc1), and a 4-byte sc1 store costs ~6x a 16-byte one per byte
// (MI355X_MICROARCH.md, stores of each flavour), so the scattered G=8 form of RowOut is not used there.
template <int G>
__device__ __forceinline__ float4 reduce_full(const float4 &acc) {
    float4 r = acc;
    if constexpr (G <= 4) {  // lane ^ 4: quads 0 and 2 read the quad above (row_ror:12), quads 1 and 3 the quad below (row_ror:4)
        auto partner = [](float x) {
            const int lo = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x12C, 0xf, 0x5, false);
            return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(lo, __builtin_bit_cast(int, x), 0x124, 0xf, 0xa, false));
        };
        r.x += partner(r.x);
        r.y += partner(r.y);
        r.z += partner(r.z);
        r.w += partner(r.w);
    }
    if constexpr (G <= 8) {  // lane ^ 8 inside each 16-lane row: row_ror:8
        r.x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, r.x), 0x128, 0xf, 0xf, false));
        r.y += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, r.y), 0x128, 0xf, 0xf, false));
        r.z += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, r.z), 0x128, 0xf, 0xf, false));
        r.w += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, r.w), 0x128, 0xf, 0xf, false));
    }
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
    return r;
}

// records staged per wave and window: 256 (2 KiB of LDS) on the wide tiles, 512 on the G = 8 tile, whose chunk budget goes up to
// 512 records (plan_build.cpp, read_knobs) -- one window per chunk there; measured with the budget
template <int G>
constexpr int kWindowRecs = G <= 8 ? 512 : 256;
// Row bundles exist on the tiles with at least kBundleMinSlots slots per step (internal.h): the wide tiles have one or two slots --
// little to gain -- and no register to spare for a chunk's bundle rows (72 VGPRs for seven waves per SIMD, see spmm_flat_kernel).
template <int G>
constexpr bool kTileHasBundles = 64 / G >= static_cast<int>(kBundleMinSlots);

// One chunk = tasks [w_task[c], w_task[c+1]) = one contiguous run of the record stream.

// The last, partial block of a window's steps: f(integral_constant<N>) for N = left, 1 <= left < U.  `left` is wave-uniform, so this
// is a short chain of scalar compares in front of U - 1 straight-line bodies, each with exactly N LDS reads and N gathers.
template <int N, int U, class F>
__device__ __forceinline__ void tail_cases(uint32_t left, F &f) {
    if constexpr (N + 1 < U) {
        if (left == N) f(std::integral_constant<int, N>{});
        else tail_cases<N + 1, U>(left, f);
    } else {
        f(std::integral_constant<int, N>{});
    }
}

// Stage records [wz, wz+wn) of the stream into the wave's LDS slice: coalesced loads, lane l takes records
// 2 l and 2 l + 1 of every 128 (16 bytes; the one-slot tile: record l of every 64, 8 bytes).  Indices are
// clamped, not predicated (slots >= wn get a copy of the last load's worth and are never read), and the
// short-window case is a wave-uniform branch: every load is consumed
// inside its branch, so (a) a long window has all its loads (two or four) in flight together instead of
// one round trip each and (b) no pending load survives into the gather loop, where the compiler would otherwise put an
// s_waitcnt vmcnt(0) at the loop head.
typedef uint32_t v2u __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ uint2 load_rec(const uint2 *ptr) {
    if constexpr (NT) {  // records are read once per column tile: keep them out of the way of the B rows in L2 / Infinity Cache
        const v2u v = __builtin_nontemporal_load(reinterpret_cast<const v2u *>(ptr));
        return make_uint2(v.x, v.y);
    } else {
        return *ptr;
    }
}

// TWO (tiles of two or more slots per step: rows are padded to whole steps, so every window starts at an even record and holds an even
// number): a lane takes two consecutive records per load -- 16 bytes, one ds_write_b128 -- and a window costs half the loads; the LDS
// image is the same.  Non-temporal loads below 16 bytes run at 0.54-0.70x the 16-byte rate (MI355X_MICROARCH.md, visibility table).
template <bool NT>
__device__ __forceinline__ uint4 load_rec2(const uint4 *ptr) {
    if constexpr (NT) {
        const v4u v = __builtin_nontemporal_load(reinterpret_cast<const v4u *>(ptr));
        return make_uint4(v.x, v.y, v.z, v.w);
    } else {
        return *ptr;
    }
}

template <bool NT, bool TWO, int LOADS>
__device__ __forceinline__ void stage_n(uint2 *my_lds, const uint2 *__restrict__ rec, uint32_t wz, uint32_t wn, int lane) {
    if constexpr (TWO) {
        uint4 r[LOADS];
#pragma unroll
        for (int i = 0; i < LOADS; ++i) r[i] = load_rec2<NT>(reinterpret_cast<const uint4 *>(rec + wz) + min(static_cast<uint32_t>(i * 64 + lane), wn / 2 - 1));
#pragma unroll
        for (int i = 0; i < LOADS; ++i) *reinterpret_cast<uint4 *>(my_lds + 2 * (i * 64 + lane)) = r[i];
    } else {
        uint2 r[LOADS];
#pragma unroll
        for (int i = 0; i < LOADS; ++i) r[i] = load_rec<NT>(rec + wz + min(static_cast<uint32_t>(i * 64 + lane), wn - 1));
#pragma unroll
        for (int i = 0; i < LOADS; ++i) my_lds[i * 64 + lane] = r[i];
    }
}

template <bool NT, int G>
__device__ __forceinline__ void stage_window_t(uint2 *my_lds, const uint2 *__restrict__ rec, uint32_t wz, uint32_t wn, int lane) {
    if constexpr (64 / G >= 2) {  // 128 records per load of the wave
        constexpr int FULL = kWindowRecs<G> / 128;
        if (wn <= 128) stage_n<NT, true, 1>(my_lds, rec, wz, wn, lane);
        else if (FULL > 2 && wn <= 256) stage_n<NT, true, 2>(my_lds, rec, wz, wn, lane);
        else stage_n<NT, true, FULL>(my_lds, rec, wz, wn, lane);
    } else {  // the one-slot tile: a window may start at an odd record
        if (wn <= 64) stage_n<NT, false, 1>(my_lds, rec, wz, wn, lane);
        else stage_n<NT, false, kWindowRecs<G> / 64>(my_lds, rec, wz, wn, lane);
    }
}

template <int G>
__device__ __forceinline__ void stage_window(uint2 *my_lds, const uint2 *__restrict__ rec, uint32_t wz, uint32_t wn, int lane, bool nt) {
    if (nt) stage_window_t<true, G>(my_lds, rec, wz, wn, lane);  // wave-uniform
    else stage_window_t<false, G>(my_lds, rec, wz, wn, lane);
}

// ---- the packed stream (internal.h, PlanView::rec_packed): 6 bytes per record in global memory, and after this staging
// step exactly the window of 8-byte records {byte offset or column, value} the step loop reads above.
//   1. coalesced loads of the window's values and 16-bit differences, clamped and unpredicated as in stage_n, all issued before the
//      first is used; the differences go to the wave's LDS slice as {32-bit word, 0}, the values wait in registers: until the scan is
//      done the .y half of a record's slot is its segment flag, so the decode needs no LDS beyond the window itself;
//   2. the chunk's exceptions add their high halves (one lane each); lane 0 adds the column the previous window ended on to word 0 (a
//      window that starts inside a task); the lanes of the tasks that start in the window overwrite their first slot with
//      {t_col0, 1} -- now every word is a difference to its predecessor, or the flagged start of a segment;
//   3. a segmented inclusive scan: lane l takes the R = window / 64 consecutive words l R .. l R + R - 1 serially from 0 (x = where it
//      ends up: the sum of all of them, or of those from its last segment start on), one unsegmented wave scan gives E[l] = x[0] +
//      ... + x[l - 1], and what enters lane l from below is E[l] - E[q], q the highest lane below l that holds a segment start
//      (a ballot and a count of leading zeros), or E[l] when there is none;
//   4. the columns go back as byte offsets (OFF32) or as they are (the values took their .y halves once every lane had read its flags).
// Returns the column of the window's last slot: the next window's carry (read only when this window was full).
// LDS operations of one wave complete in order, and the record slice is private to the wave: no barrier, as above.
// PAIR (tiles of two or more slots per step: every task, hence every window, starts at an even record): a lane takes two
// consecutive records per load -- 8 bytes of values, 4 of differences, one 16-byte LDS write -- so a window costs as many loads as
// it did at 8 bytes per record.  The one-slot tile (G = 64) may start at an odd record and loads record by record.
// (Four values and four or eight differences per lane and load -- 16-byte loads, 3 per 512-record window instead of 8 -- measured
// SLOWER on the Amazon preset, 8.21 against 7.83 ms -- DESIGN.md 3.4 "what a window carries", profiles/record_staging_ab_series.json,
// `parts`: a lane that loads four or eight consecutive records writes them to LDS at a 32- or 64-byte lane stride.  The pair form
// stays on every tile.)
template <bool NT, class T>
__device__ __forceinline__ T load_stream(const T *ptr) {
    if constexpr (NT) return __builtin_nontemporal_load(ptr);
    else return *ptr;
}

// loads of LOADS <= FULL wave loads; vv: the values, in load order (PAIR: two per load); those of loads not made are 0
template <bool NT, bool PAIR, int LOADS, int R>
__device__ __forceinline__ void stage_packed_n(uint2 *my_lds, const float *__restrict__ val, const uint16_t *__restrict__ dcol, uint32_t wn, int lane,
                                               uint32_t (&vv)[R]) {
    // addresses as base (SGPR pair) + 32-bit byte offset in a VGPR, as gather4: a window is a few KiB, and one register per load
    // instead of an address pair keeps the staging step below the gather loop's register count
    const char *const vb = reinterpret_cast<const char *>(val), *const db = reinterpret_cast<const char *>(dcol);
#pragma unroll
    for (int i = 0; i < R; ++i) vv[i] = 0u;
    if constexpr (PAIR) {
        uint32_t d[LOADS];
#pragma unroll
        for (int i = 0; i < LOADS; ++i) {
            const uint32_t off = min(static_cast<uint32_t>(i * 64 + lane), wn / 2 - 1) * 4u;  // wn is even
            const v2u v = load_stream<NT>(reinterpret_cast<const v2u *>(vb + static_cast<uint32_t>(off * 2u)));
            vv[2 * i] = v.x;
            vv[2 * i + 1] = v.y;
            d[i] = load_stream<NT>(reinterpret_cast<const uint32_t *>(db + off));
        }
#pragma unroll
        for (int i = 0; i < LOADS; ++i) *reinterpret_cast<uint4 *>(my_lds + 2 * (i * 64 + lane)) = make_uint4(d[i] & 0xFFFFu, 0u, d[i] >> 16, 0u);
    } else {
        uint16_t d[LOADS];
#pragma unroll
        for (int i = 0; i < LOADS; ++i) {
            const uint32_t off = min(static_cast<uint32_t>(i * 64 + lane), wn - 1) * 2u;
            vv[i] = __float_as_uint(load_stream<NT>(reinterpret_cast<const float *>(vb + static_cast<uint32_t>(off * 2u))));
            d[i] = load_stream<NT>(reinterpret_cast<const uint16_t *>(db + off));
        }
#pragma unroll
        for (int i = 0; i < LOADS; ++i) my_lds[i * 64 + lane] = make_uint2(d[i], 0u);
    }
}

template <bool NT, int G, int R>
__device__ __forceinline__ void stage_packed_t(uint2 *my_lds, const float *__restrict__ val, const uint16_t *__restrict__ dcol, uint32_t wn, int lane,
                                               uint32_t (&vv)[R]) {
    constexpr bool PAIR = 64 / G >= 2;
    constexpr int PER = PAIR ? 128 : 64, FULL = kWindowRecs<G> / PER;  // records per load of the wave, loads of a full window
    if (wn <= PER) stage_packed_n<NT, PAIR, 1>(my_lds, val, dcol, wn, lane, vv);
    else if (FULL > 2 && wn <= 2 * PER) stage_packed_n<NT, PAIR, 2>(my_lds, val, dcol, wn, lane, vv);
    else stage_packed_n<NT, PAIR, FULL>(my_lds, val, dcol, wn, lane, vv);
}

// x of lane `from` (mod 64).  __shfl and its kin form their index from the hardware lane id, a loop invariant the compiler keeps in
// registers across the gather loop -- one per shuffle distance; this one takes the caller's `lane`, which stage_window_packed makes anew
// per window.  A register-allocation measure, checked against the compiler in use with `make asm` (the register
// table), like the empty asm statements around it: another compiler version may not need it, or may need more.
__device__ __forceinline__ uint32_t lane_read(uint32_t x, int from) {
    return static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute((from & 63) << 2, static_cast<int>(x)));
}

template <int G, bool OFF32>
__device__ __forceinline__ uint32_t stage_window_packed(const PlanView &p, uint2 *my_lds, uint32_t zb, uint32_t wz, uint32_t wn, uint2 cx,
                                                        uint32_t t0, uint32_t nt, uint32_t my_beg, uint32_t carry, uint32_t row_bytes32, int lane) {
    constexpr int W = kWindowRecs<G>, R = W / 64;
    constexpr bool PAIR = 64 / G >= 2;
    // everything below that depends on the lane alone (indices, LDS addresses, masks) is recomputed per window: hoisted out of the
    // window loop it would stay in registers across the gather loop, which is where the kernel's register count is decided
    asm volatile("" : "+v"(lane));
    uint32_t vv[R];
    if (p.rec_nt != 0) stage_packed_t<true, G>(my_lds, p.rec_val + wz, p.rec_dcol + wz, wn, lane, vv);  // wave-uniform
    else stage_packed_t<false, G>(my_lds, p.rec_val + wz, p.rec_dcol + wz, wn, lane, vv);
    // exceptions of the chunk that fall into this window (rare: the loop body runs for one chunk in a few)
    for (uint32_t j = lane; j < cx.y; j += 64) {
        const uint2 e = p.exc[cx.x + j];
        const uint32_t at = zb + e.x - wz;  // position in the window, if below wn
        if (at < wn) my_lds[at].x += e.y;
    }
    if (lane == 0) my_lds[0].x += carry;
    // task starts: lane i holds t_beg[t0 + i] (i <= nt); an empty task starts where its successor does and owns no record
    const uint32_t next_beg = lane_read(my_beg, lane == 63 ? lane : lane + 1);
    const uint32_t at = my_beg - wz;
    if (static_cast<uint32_t>(lane) < nt && next_beg != my_beg && at < wn) {
        uint32_t flag = 1u;  // made here: as a loop invariant the constant takes a register, or a scratch slot, across the gather loop
        asm volatile("" : "+v"(flag));
        my_lds[at] = make_uint2(p.t_col0[t0 + lane], flag);
    }
    __builtin_amdgcn_wave_barrier();
    // the lane's R words, serially from 0
    uint32_t w[R], fbits = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const uint2 s = my_lds[lane * R + i];
        w[i] = s.x;
        fbits |= s.y << i;  // 0 or 1; slots past what this window loaded hold old records: never read, whatever they scan to
    }
    fbits &= (1u << R) - 1u;
    // every lane has read its flags: the values take their .y halves now, where the loads' layout puts them, and leave their registers
    // to the scan.  The hardware completes a wave's LDS operations in order; the barrier keeps the compiler from moving a value write
    // (another lane's slot, a provably different address for this thread) above a flag read.
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < R; ++i) my_lds[PAIR ? 2 * ((i / 2) * 64 + lane) + (i & 1) : i * 64 + lane].y = vv[i];
    uint32_t run = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        run = ((fbits >> i) & 1u) ? w[i] : run + w[i];
        w[i] = run;
    }
    // unsegmented inclusive scan of the lanes' results, then the part that belongs to the lane's open segment
    uint32_t inc = run;
#pragma unroll
    for (int dlt = 1; dlt < 64; dlt <<= 1) {
        const uint32_t up = lane_read(inc, lane - dlt);  // lanes below dlt read a lane they do not use
        if (lane >= dlt) inc += up;
    }
    const uint32_t exc_sum = inc - run;  // E[lane]
    const uint64_t below = __builtin_amdgcn_ballot_w64(fbits != 0) & ((uint64_t(1) << lane) - 1u);
    const int q = below ? 63 - __builtin_clzll(below) : 0;
    const uint32_t e_q = lane_read(exc_sum, q);
    const uint32_t enter = below ? exc_sum - e_q : exc_sum;
    uint32_t last = 0;
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const bool open = (fbits & ((2u << i) - 1u)) == 0;  // no segment start at or before word i in this lane
        const uint32_t col = w[i] + (open ? enter : 0u);
        my_lds[lane * R + i].x = OFF32 ? col * row_bytes32 : col;
        last = col;
    }
    __builtin_amdgcn_wave_barrier();
    return __builtin_amdgcn_readlane(last, 63);
}

// Which (entry of the chunk table, column tile) the wave `wib` of this workgroup works on; false: none (past the table's end, or past
// the end of a short last group).  Classic: blockIdx.y = tile, one pass over the whole table per tile.  Grouped (p.tile_group): a 1-D
// grid in which every XCD slice is walked group by group, the tiles of a group back to back -- a group's records are then re-read from
// the Infinity Cache instead of HBM.  G: lanes per record, each owning 4 words of a B row (a tile is 4 G words wide; p.k is in words).
template <int G, int WPB>
__device__ __forceinline__ bool place_of_wave(const PlanView &p, uint32_t wib, uint32_t &tile, uint32_t &ktiles, uint32_t &chunk) {
    uint32_t bid;
    tile = blockIdx.y;
    ktiles = gridDim.y;
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
        if (tile >= ktiles) return false;  // only past the end of a short last group
        bid = p.xcd_remap ? (blockIdx.x % kXcds) * slice + in_slice : in_slice;
    }
    chunk = bid * WPB + wib;
    return chunk < p.n_chunks;
}

// What a wave holds of its chunk before the first record: the header {first task, #tasks, first record, end record}, the packed plan's
// exception table entry, and -- lane i -- the descriptors of task i (t_aux is not among them: only the fp32 kernel's in-launch piece
// sum reads it, and fetches it there).
struct ChunkRegs {
    uint4 hdr;
    uint2 cx;
    uint32_t my_beg, my_dst;
    uint32_t my_bd0, my_bd1;
};

// false: an empty entry that pads this XCD's slice of the table (plan_build.cpp, build_chunk_table)
template <int G>
__device__ __forceinline__ bool load_chunk(const PlanView &p, uint32_t chunk, int lane, ChunkRegs &d) {
    // A chunk holds at most 63 tasks (planner invariant): all descriptors come with one coalesced
    // load per array and are handed out with v_readlane; the header carries the record range, so
    // the record fetch does not wait for them: header -> {descriptors, records} -> gathers.
    const uint4 hdr = d.hdr = p.chunk[chunk];
    // the chunk's part of the bundle rows: fetched beside the header, handed out at the end of each bundle (compute_chunk, flush)
    uint2 cb = make_uint2(0u, 0u);
    if constexpr (kTileHasBundles<G>)
        if (p.bd_rows != nullptr) cb = p.chunk_bd[chunk];  // uniform
    // packed plans: the chunk's exception table {first, entries}, or {first wide record, kChunkWide}
    uint2 cx = make_uint2(0u, 0u);
    if (p.rec_packed != 0) cx = p.chunk_exc[chunk];  // uniform
    d.cx = cx;
    if (hdr.y == 0) return false;
    d.my_beg = (static_cast<uint32_t>(lane) <= hdr.y) ? p.t_beg[hdr.x + lane] : 0u;
    d.my_dst = (static_cast<uint32_t>(lane) < hdr.y) ? p.t_dst[hdr.x + lane] : 0u;
    d.my_bd0 = d.my_bd1 = kBundleNoRow;
    if (kTileHasBundles<G> && cb.y != 0) {  // uniform
        if (static_cast<uint32_t>(lane) < cb.y) d.my_bd0 = p.bd_rows[cb.x + lane];
        if (static_cast<uint32_t>(lane) + 64u < cb.y) d.my_bd1 = p.bd_rows[cb.x + 64u + lane];
    }
    return true;
}

}  // namespace spmm_dev
}  // namespace flex
