// internal.h -- shared between the host planner and the HIP kernels of libflex_spmm.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <vector>

#include "../../include/flex_spmm.h"

namespace flex {

// One split row: C[row,:] = sum of partial[first .. first+count) in that order.
struct SplitRow {
    uint32_t row, first, count;
};

// What the SpMM kernels read.  Passed by value as a kernel argument (the reference
// copies a ~270-byte Mat_POD into __constant__ memory instead: mat.cuh:18-65, mat.cu:32-41).
struct PlanView {
    const uint2 *rec;        // [nnz] {x = B-row byte offset (off32) or column id, y = value bits}, task order
    const uint32_t *t_beg;   // [n_tasks+1] first record of each task
    const uint32_t *t_dst;   // [n_tasks]   C row written by the task; MSB set -> partial slot id (the task is a PIECE), or, with
                             //             kBundleFlag as well, a BUNDLE: low bits = its first entry in the chunk's part of bd_rows
    const uint2 *t_aux;      // [n_tasks]   pieces: {index into `split` of the piece's row, #pieces of that row}; bundles: {first entry
                             //             in bd_rows, steps}; else {0,0}
    const uint4 *chunk;      // [n_chunks] {first task, #tasks (<= 63), first record, end record}; one wave per chunk
    float *partial;          // [n_partials][k] partial sums of split rows
    const SplitRow *split;   // [n_split] {C row, first partial, #pieces}
    uint32_t *split_cnt;     // [n_split][k-tiles] arrival counters, zero between launches
    uint32_t fused_fixup;    // 1: the last piece to finish sums the row inside the launch; 0: spmm_fixup_kernel does
    uint32_t n_chunks;
    int32_t k;
    int32_t ldb, ldc;        // floats between consecutive rows of B and of C (>= k; == k for dense operands)
    uint32_t xcd_remap;      // 1: remap workgroup ids so each XCD walks one contiguous slice of the schedule
    uint32_t lds_extra;      // bytes of unused dynamic LDS per workgroup (occupancy throttle, tuning only)
    uint32_t rec_nt;         // 1: the record stream is read with non-temporal loads
    uint32_t tile_group;     // 0: column tiles are the slow grid dimension (one pass over all chunks per tile).  Else: workgroups per group --
                             // every XCD slice of the chunk table is walked group by group, all column tiles of a group back to back, so that
                             // a group's records are re-read while they are still in the Infinity Cache (1-D grid of n_workgroups x tiles)
    uint64_t *trace;         // the stamped twin's log (flex_plan_measure_imbalance): 3 words per (k-tile, chunk-table entry); else nullptr
    // Row bundles (plan_build.cpp, form_tasks): a task that holds up to S = 64 / G SHORT rows side by side, slot s of every step working
    // on row s -- no cross-slot reduction, one 16-byte store per lane at the end.  nullptr when the plan has none.
    const uint32_t *bd_rows; // per bundle S entries: C row of slot s | kBundleZero (the row holds no nonzero: zeros are stored), or kBundleNoRow
    const uint2 *chunk_bd;   // [chunk-table entries] {first entry in bd_rows, entries (a multiple of S, <= kBundleRowsPerChunk)} of the chunk's bundles
    // The PACKED record stream (plan_build.cpp, pack_records): 6 bytes per record instead of 8.  rec_packed != 0: the
    // stream is rec_val / rec_dcol under the same record indices, and `rec` holds nothing but the records of the WIDE chunks (those with
    // a bundle task keep the 8-byte form), one chunk after the other; nullptr when the plan has none.
    uint32_t rec_packed;
    const float *rec_val;      // [records] the value of each record, after the padding rule
    const uint16_t *rec_dcol;  // [records] low 16 bits of (column - column of the record before it in the task) mod 2^32; 0 on a task's first record
    const uint32_t *t_col0;    // [n_tasks] column of the task's first record
    const uint2 *chunk_exc;    // [chunk-table entries] {first entry in `exc`, entries}; with kChunkWide in y: {first record of the chunk in `rec`, kChunkWide}
    const uint2 *exc;          // differences that do not fit 16 bits: {record's position in its chunk, the difference's high 16 bits << 16}, by position
};
constexpr uint32_t kChunkWide = 0x80000000u;  // in chunk_exc.y: the chunk keeps 8-byte records


// What the dense-tile kernel reads (tile_kernels.hip): 32x32 blocks of A that left the record stream.
struct TileView {
    const float *a;            // [n_tiles][4][64][4] tile values in MFMA A-operand order: (q,lane,e) = A[lane&31][2(4q+e) + (lane>>5)]
    const uint32_t *boff;      // [n_tiles][32] B row of each tile column: byte offset (off32) or row id
    const uint32_t *mask;      // [n_tiles][32] bit j of word i: the tile holds an entry at (row i, column j) -- an explicit zero counts, an absent one does not
    const uint32_t *rt_ptr;    // [n_row_tiles+1] tiles of each listed row tile, in column order
    const uint32_t *rt_rows;   // [n_row_tiles][32] C row of each row of the row tile, 0xFFFFFFFF = none
    uint32_t n_row_tiles;
};

// ---- the hot-block path (block_kernels.hip, block_plan.cpp): LDS-level reuse of B for the nonzeros that have it.
// Round 4 design.  The matrix is SPLIT: a nonzero whose column is used by at least `thr` nonzeros of its BLOCK (R = rounds x 60
// schedule-consecutive rows) is HOT and lives in the block image below; every other nonzero -- and every row too long for a
// slot -- stays in the flat plan, whose kernel is the one that moves L2 misses at the fabric's rate.  flex_spmm runs the flat
// kernel first (it writes every row of C), then spmm_hot_kernel ADDS the hot part: one workgroup of 16 waves per (block, 64-column
// tile): 15 CONSUMER waves of 4 slots x 16 lanes + 1 LOADER wave.  A slot holds ONE C row per round in registers (the lane owns 4
// of the tile's 64 columns); the hot B rows (256 bytes per row and tile) are staged panel by panel into LDS by the loader wave
// (LDS-DMA, double-buffered) and every use is a ds_read_b128 that is bank-conflict free by construction (a 16-lane slot reads one
// whole 256-byte row = all 64 banks).  Records never touch LDS: a RUN (the <= 16 steps of one (wave, panel, round)) is one coalesced
// 512-byte load into a register pair a whole panel ahead, and step j's record reaches the 16 lanes of its slot by a DPP row
// broadcast (row_newbcast:j) -- the LDS pipe carries nothing but B.
constexpr int kBkWaves = 15;                              // consumer waves per workgroup
constexpr int kBkSlots = 4;                               // slots per wave (16 lanes x float4 = one 64-column tile of one row)
constexpr int kBkTileCols = 64;                           // columns of C per pass
constexpr int kBkRowsPerRound = kBkWaves * kBkSlots;      // 60 row slots per round
constexpr int kBkMaxRounds = 8;
constexpr uint32_t kBkRunMax = 16;                        // steps of one run = lanes of a slot: what one DPP row holds
// Two panel buffers of 304 rows, the loader one panel ahead.  Measured (profiles/r04_hot_block_ring_probe.txt): three buffers of 200
// rows with the loader two panels ahead are SLOWER -- more panels mean more runs and barriers, and those, not staging latency, are
// what the kernel pays for.
constexpr uint32_t kBkNBuf = 2;                           // panel buffers
constexpr uint32_t kBkPanelMax = 304;                     // B rows per LDS panel
constexpr uint32_t kBkRowBytes = 256;                     // one B row of one column tile
constexpr uint32_t kBkZeroRow = kBkPanelMax * kBkRowBytes; // byte offset, inside a panel buffer, of a row of zeros (padding records point at it)
constexpr uint32_t kBkBufBytes = kBkZeroRow + kBkRowBytes;
constexpr uint32_t kBkLdsHcol = kBkNBuf * kBkBufBytes;    // two scratch slots for the byte offsets of the panels about to be staged
constexpr uint32_t kBkLdsBytes = kBkLdsHcol + 2 * kBkPanelMax * 4;  // 158 592 of the CU's 163 840 (two buffers of 304 rows)
static_assert(kBkLdsBytes <= 163840 && kBkPanelMax % 4 == 0 && kBkPanelMax <= 256 + 48 && kBkNBuf == 2, "the hot kernel's LDS image must fit one CU");
constexpr uint32_t kBkLdsNext = kBkMaxRounds * kBkRowsPerRound * kBkRowBytes;  // after the last panel: [slots] sums of later parts, then [slots] next part + 1
static_assert(kBkLdsNext + kBkMaxRounds * kBkRowsPerRound * 4 <= kBkLdsHcol, "the parts of long rows meet in the panel buffers");
constexpr uint32_t kBkEmptyRow = 0xFFFFFFFFu;             // brow entry of a slot that holds no row
constexpr uint32_t kBkMaxPanels = 63;                     // a wave holds its run counts one panel per lane (and looks one panel ahead)
// A long row holds several slots (its PARTS); they meet in LDS after the last panel.  link[slot]: bits 0-15 = 1 + the slot of the
// row's next part (0 = none), in the block's [round][wave][slot] numbering.
constexpr uint32_t kBkLinkOwner = 0x40000000u;            // this slot collects the chain that starts at its `next` and writes the row
constexpr uint32_t kBkLinkPart = 0x80000000u;             // this slot publishes its sum (and its `next`) for the owner

struct BlockView {
    const uint4 *hdr;        // [n_blocks] {panels | (some row has several parts) << 31, first entry in hcol, first word in cnt, words of cnt per wave (2 x panels)}
    const uint2 *wstart;     // [n_blocks][15] {first step of the wave's record stream, its steps}
    const uint32_t *cnt;     // per (block, wave, panel): a 64-bit word (two u32), byte r = the steps (<= 16) of the run (panel, round r)
    const uint32_t *hcol;    // per (block, panel): panel_rows byte offsets of the B rows staged (padded with a valid one)
    const uint32_t *brow;    // [n_blocks][rounds][15][4] C row the slot reads and writes (an owner); kBkEmptyRow = none (empty, or a later part of a row)
    const uint32_t *link;    // [n_blocks][rounds][15][4] kBkLinkOwner / kBkLinkPart | next part + 1; 0 for a row of one part
    const uint2 *rec;        // [steps][4] {byte offset inside the panel buffer, value bits}
    uint64_t n_rec;          // records in `rec` (loads past a wave's stream are clamped to the last one)
    uint32_t n_blocks, rounds, panel_rows;
    int32_t k, ldb, ldc;
    uint32_t xcd_remap;
};

constexpr uint32_t kPartialFlag = 0x80000000u;
constexpr uint32_t kBundleFlag = 0x40000000u;       // in t_dst, together with kPartialFlag: the task is a bundle of rows
constexpr uint32_t kBundleZero = 0x80000000u;       // in bd_rows: store zeros (a row without nonzeros)
constexpr uint32_t kBundleNoRow = 0xFFFFFFFFu;      // in bd_rows: the slot holds no row
constexpr uint32_t kBundleRowsPerChunk = 128;       // a wave keeps its chunk's bd_rows entries in two registers per lane
constexpr uint32_t kBundleMinSlots = 4;             // bundles only on tiles with at least this many record slots per step (G <= 16)
constexpr int kWavesPerBlock = 4;  // 256-thread workgroups
constexpr int kXcds = 8;           // MI355X: 8 XCDs, each with a private 4 MiB L2

// ---- the value rule of a task's padding, shared by the planner (plan_build.cpp, fill_records) and the value refresh on the GPU
// (values_kernels.hip, flex_plan_set_values), so that a refreshed plan is bit for bit the plan the planner would have built.
//
// Padding behind the `len` real records of a row (or piece, or bundle slot) at `first`, `stride` apart: n_pad more records.
// The padding never carries value 0 at a live B row where that could change the row's class -- 0 x inf would turn a row's
// +-inf into NaN (the oracle and the reference have no padding) -- but SHARES the value of one real record (c, v), so a
// non-finite B row contributes what v itself would and a finite one the same product up to the extra roundings:
//   * the last record, v normal and at least 2^(n_pad+1) above the subnormal range: v = v/2 + v/4 + ... + v/2^p + v/2^p, every
//     part exact (power-of-two scaling) -- the form of every plan of values of ordinary size;
//   * otherwise the last record that allows one of: v = +-inf / NaN / +-0: n_pad copies of (c, v) (the row holds v x B[c]
//     already, and adding it again keeps the class: inf + inf, NaN, +-0); v finite with an integer significand of at least
//     n_pad + 1 units (every normal value, a subnormal of at least n_pad + 1 units of 2^-149): n_pad + 1 same-sign parts of that
//     significand at v's scale, each exact, one of them replacing v;
//   * none does (every value a nonzero subnormal of at most n_pad units of 2^-149): (c_last, 0) -- the one residual,
//     include/flex_spmm.h.
// Integer arithmetic on the bits only: the result cannot depend on a floating-point mode of the host or of the device.
constexpr uint32_t kNoEntry = 0xFFFFFFFFu;  // FLEX_PLAN_MUTABLE_VALUES: the record -> entry map's mark of a padding record

// bits of the fp32 value u x 2^(e - 150), which the caller knows to be exact: 1 <= u < 2^24, 1 <= e <= 254
__host__ __device__ inline uint32_t units_at_scale(uint32_t u, uint32_t e) {
    const int lead = 31 - __builtin_clz(u);  // u in [2^lead, 2^(lead+1))
    const int biased = static_cast<int>(e) - 23 + lead;
    if (biased >= 1) return (static_cast<uint32_t>(biased - 1) << 23) + (u << (23 - lead));  // normal: the implicit bit lands on the exponent
    return u << (e - 1);  // subnormal: u x 2^(e-1) units of 2^-149 (< 2^23 because the value is exact and below 2^-126)
}

__host__ __device__ inline void pad_values(uint2 *first, uint32_t len, uint32_t n_pad, uint32_t stride) {
    if (n_pad == 0) return;
    uint2 *const last = first + static_cast<size_t>(len - 1) * stride;
    const uint32_t ex = (last->y >> 23) & 0xFFu;  // biased exponent of v
    if (ex > n_pad + 1 && ex < 0xFFu) {
        uint32_t bits = last->y;
        uint2 *q = last;  // the last real record takes v/2, the paddings v/4 ... v/2^p, v/2^p
        for (uint32_t i = 0; i < n_pad; ++i, q += stride) {
            bits -= 1u << 23;  // halving: the exponent stays >= 2, so it is exact
            q->y = bits;
            q[stride] = make_uint2(q->x, bits);
        }
        return;
    }
    uint2 *const pad = last + stride;
    for (uint32_t j = len; j-- > 0;) {
        uint2 *const d = first + static_cast<size_t>(j) * stride;
        const uint32_t dex = (d->y >> 23) & 0xFFu, man = d->y & 0x7FFFFFu;
        if (dex == 0xFFu || (dex == 0 && man == 0)) {  // +-inf, NaN, +-0: copies
            for (uint32_t i = 0; i < n_pad; ++i) pad[static_cast<size_t>(i) * stride] = *d;
            return;
        }
        const uint32_t sig = dex ? (man | 0x800000u) : man, parts = n_pad + 1;
        if (sig >= parts) {  // sig = parts * q + r: r parts of q + 1 units, the rest of q, all at v's scale (exact: < 2^24 units)
            const uint32_t q = sig / parts, r = sig % parts, sign = d->y & 0x80000000u, e = dex ? dex : 1u;
            d->y = units_at_scale(q + (0 < r ? 1u : 0u), e) | sign;
            for (uint32_t i = 0; i < n_pad; ++i)
                pad[static_cast<size_t>(i) * stride] = make_uint2(d->x, units_at_scale(q + (i + 1 < r ? 1u : 0u), e) | sign);
            return;
        }
    }
    for (uint32_t i = 0; i < n_pad; ++i) pad[static_cast<size_t>(i) * stride] = make_uint2(last->x, 0u);
}

// FLEX_PLAN_MUTABLE_VALUES: the work items of flex_sddmm -- runs of at most kSdItemRecords real records of one C row, {first record,
// records, stride between them (1, or S inside a bundle), C row} -- in task order, packed into one group per wave
constexpr uint32_t kSdItemRecords = 64;
constexpr uint32_t kSdGroupCost = 32;   // per wave: sum over its items of (passes of 4 records per slot + 1 for the G row)
constexpr uint32_t kSdGroupItems = 64;
// lanes of one SDDMM slot: a float4 of the G row each, the smallest power of two >= k / 4 in [4, 64]
inline int sddmm_lanes(int k) {
    int w = 4;
    while (4 * w < k && w < 64) w <<= 1;
    return w;
}

// The instantiation flex_sddmm launches, sddmm_slots<W, OFF32, VEC> (values_kernels.hip): W from k, OFF32 the plan's record format, VEC
// (16-byte loads of the G and B rows) where k, both leading dimensions and both operands allow it.  Host code, shared with the launch
// log of tests/hostsim/shim.cpp, so that the tests declare kernels by the library's own rule.
struct SddmmPick {
    int W;
    bool off32, vec4;
};
inline SddmmPick sddmm_pick(int k, int ldb, int ldc, bool off32, const void *dG, const void *dB) {
    const bool vec4 = k % 4 == 0 && ldb % 4 == 0 && ldc % 4 == 0 && ((reinterpret_cast<uintptr_t>(dG) | reinterpret_cast<uintptr_t>(dB)) % 16 == 0);
    return SddmmPick{sddmm_lanes(k), off32, vec4};
}
// The launches of flex_plan_set_values: refresh_records over every record, then refresh_padding where the plan has padded runs
inline int refresh_passes(uint64_t n_records, uint64_t n_segs) { return n_records == 0 ? 0 : n_segs == 0 ? 1 : 2; }

// FLEX_PLAN_MUTABLE_VALUES: the walk of flex_edge_softmax / flex_edge_softmax_backward (softmax_kernels.hip; plan_build.cpp,
// upload_softmax_image).  It is made from hostA's row pointer alone.  A wave looks at its entries through WINDOWS of kSmWindow
// consecutive entries that start at a multiple of 4 (a lane owns 4 consecutive entries: one 16-byte load where the arrays are aligned).
//   packed item   consecutive whole rows that fit ONE window together: (first entry % 4) + entries <= kSmWindow, at most kSmItemRows rows
//                 (empty ones count); the wave reduces them side by side under row-boundary flags
//   wave row      a row that does not fit a window but fits kSmChunk entries counted the same way: one wave, 4 windows held in registers
//   block row     a longer row: a workgroup of its own, wave w takes chunks w, w + 4, ...; up to 4 kSmChunk entries stay in registers,
//                 a longer row is read a second time for the write (from the L2 where it fits)
// Items are {first entry, entries, first row (index into the plan's row pointer), rows}.  Packed items and wave rows are packed, in row
// order, into one group per wave: a group of more than one item holds at most the plan's group budget of entries.
constexpr uint32_t kSmWindow = 256;
constexpr uint32_t kSmItemRows = 256;
constexpr uint32_t kSmChunk = 4 * kSmWindow;      // what a lane keeps in registers: 4 x 4 entries.  Also the block-row threshold
constexpr uint32_t kSmGroupMin = kSmWindow;       // group budget (entries): total / kSmTargetGroups rounded up to a window, within these
constexpr uint32_t kSmGroupMax = 8 * kSmWindow;
constexpr uint32_t kSmTargetGroups = 4096;        // 16 waves on each of the 256 CUs before a wave takes a second item
enum SmClass : int { kSmPacked = 0, kSmWaveRow = 1, kSmBlockRow = 2 };
// the class of a nonempty row of `len` entries whose first entry is `first`
inline int softmax_row_class(uint32_t first, uint32_t len) {
    const uint64_t span = static_cast<uint64_t>(first % 4u) + len;
    return span <= kSmWindow ? kSmPacked : span <= kSmChunk ? kSmWaveRow : kSmBlockRow;
}
inline uint32_t softmax_group_budget(uint64_t entries) {
    const uint64_t b = (entries / kSmTargetGroups + kSmWindow - 1) / kSmWindow * kSmWindow;
    return static_cast<uint32_t>(b < kSmGroupMin ? kSmGroupMin : b > kSmGroupMax ? kSmGroupMax : b);
}
// VEC of edge_softmax_rows<VEC, BWD> (softmax_kernels.hip): 16-byte accesses where every array of the call is 16-byte aligned
// (b: the backward's second input, NULL in the forward).  Shared with the launch log of tests/hostsim/shim.cpp, as sddmm_pick.
inline bool softmax_vec(const void *a, const void *b, const void *out) {
    return (reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
}
// a term of the order-free fingerprint of a row pointer slice (flex_plan_self_check)
inline uint64_t rowptr_fp(uint32_t local_row, uint32_t first_entry) {
    uint64_t z = ((static_cast<uint64_t>(local_row) << 32) | first_entry) + 0x9E3779B97F4A7C15ull;  // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// FLEX_PLAN_ATTENTION: the walk of flex_attention (attention_kernels.hip; plan_build.cpp, upload_attention_image).  It is made from
// hostA's row pointer and columns alone and walks hostA's rows in their order.  A SLOT is W = sddmm_lanes(k) lanes, each holding four
// columns per slab of its Q row and of its Out row in registers; a slot takes kAtPass entries per pass.  Rows are whole: by length a row is a
//   slot row    at most kAtSlotRow entries (an empty row too): one slot owns the row, the 64 / W slots of a wave work on 64 / W
//               consecutive rows side by side and never meet
//   wave row    at most kAtWaveRow entries: the slots of one wave stride the row pass by pass, their states (running maximum, sum, Out
//               row) are merged by shuffles, lower slot first
//   block row   longer: a workgroup of its own, its kWavesPerBlock x 64 / W slots stride the row, the waves meet in LDS in wave order
// kAtSlotRow: up to 8 passes of one slot; beyond that the log2(64 / W) merge steps of a wave row (two expf and a shuffle of the Out row
// each) cost less than the passes they save.  kAtWaveRow: 32 passes of the 4 slots of k = 64; a longer row takes the four waves.
// Items are {first entry, entries, first row (index into the plan's row pointer), rows}: a slot item holds up to 64 / W consecutive
// slot rows, a wave or block item its one row.  Slot items and wave rows are packed, in row order, into one group per wave: a group of
// more than one item costs at most the plan's group budget, an item costing its entries + its rows.
constexpr uint32_t kAtPass = 4;
constexpr uint32_t kAtSlotRow = 32;
constexpr uint32_t kAtWaveRow = 512;
constexpr uint32_t kAtGroupMin = 64;            // group budget: total cost / kAtTargetGroups rounded up to 64, within these
constexpr uint32_t kAtGroupMax = 2048;
constexpr uint32_t kAtTargetGroups = 4096;      // 16 waves on each of the 256 CUs before a wave takes a second item
constexpr int kAtMaxSlabs = 4;                  // k <= 4 x 64 lanes x 4 slabs
enum AtClass : int { kAtSlot = 0, kAtWave = 1, kAtBlock = 2 };
// the class of a nonempty row of `len` entries
inline int attention_row_class(uint32_t len) { return len <= kAtSlotRow ? kAtSlot : len <= kAtWaveRow ? kAtWave : kAtBlock; }
inline uint32_t attention_group_budget(uint64_t cost) {
    const uint64_t b = (cost / kAtTargetGroups + 63) / 64 * 64;
    return static_cast<uint32_t>(b < kAtGroupMin ? kAtGroupMin : b > kAtGroupMax ? kAtGroupMax : b);
}
// The instantiation flex_attention launches, attention_rows<W, NS, VEC> (attention_kernels.hip): W from k as the SDDMM, NS slabs of
// 4 W columns (1 below k = 257, then 2 or 4), VEC (16-byte loads and stores of the Q, K, V and Out rows) where k, both leading
// dimensions and all four operands allow it.  A host rule, as sddmm_pick.
struct AttentionPick {
    int W, NS;
    bool vec4;
};
inline AttentionPick attention_pick(int k, int ldb, int ldc, const void *dQ, const void *dK, const void *dV, const void *dOut) {
    const int W = sddmm_lanes(k), slabs = (k + 4 * W - 1) / (4 * W);
    const uintptr_t ptrs = reinterpret_cast<uintptr_t>(dQ) | reinterpret_cast<uintptr_t>(dK) | reinterpret_cast<uintptr_t>(dV) | reinterpret_cast<uintptr_t>(dOut);
    return AttentionPick{W, slabs <= 1 ? 1 : slabs == 2 ? 2 : 4, k % 4 == 0 && ldb % 4 == 0 && ldc % 4 == 0 && ptrs % 16 == 0};
}
// The one alignment rule of the per-head entry points, for either element type: W and NS of k, the vector form where k and both leading
// dimensions are multiples of four elements and every row operand is aligned to four elements (16 bytes of float, 8 of flex_bf16; a
// NULL output is aligned).  On float rows it is attention_pick over the same operands.
template <class E>
inline AttentionPick pick_rows(int k, int ldb, int ldc, std::initializer_list<const void *> rows) {
    AttentionPick pick = attention_pick(k, ldb, ldc, nullptr, nullptr, nullptr, nullptr);
    for (const void *r : rows) pick.vec4 = pick.vec4 && reinterpret_cast<uintptr_t>(r) % (4 * sizeof(E)) == 0;
    return pick;
}
// The head split of the per-head entry points (attention_entry.h): FLEX_OK and lg, with d = k / heads = 4 << lg, where heads
// (1 included) divides k into heads of d = 4 .. 256 columns, d a power of two.  A host rule, as attention_pick.
inline int head_split_lg(int k, int heads, int *lg_out) {
    if (k > 4 * 64 * kAtMaxSlabs || k % heads) return FLEX_ERR_UNSUPPORTED;
    const int d = k / heads;
    int lg = 0;
    while ((4 << lg) < d) ++lg;
    if (d < 4 || d > 256 || (4 << lg) != d) return FLEX_ERR_UNSUPPORTED;
    *lg_out = lg;
    return FLEX_OK;
}

// The mask of the attention dropout (include/flex_spmm.h, flex_attention_dropout; attention_dropout_kernels.hip), one definition for the
// kernels and for flex_dropout_mask (plan.cpp): element i = e H + h of the edge arrays is kept iff dropout_bits(seed, i) < thr.  The mixer
// is two rounds of a 32-bit multiply-xorshift on wrapping arithmetic; the high words of i and of the seed enter between the rounds.
struct DropMask {
    uint32_t seed_lo, seed_hi, thr;  // thr = min(floor((1 - (double)p) 2^32), 2^32 - 1)
    float c;                         // 1.0f / (1.0f - p), in fp32: what a kept probability is multiplied by
};
__host__ __device__ inline uint32_t dropout_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__host__ __device__ inline uint32_t dropout_bits(uint32_t seed_lo, uint32_t seed_hi, uint64_t i) {
    return dropout_mix(dropout_mix(static_cast<uint32_t>(i) + seed_lo + 0x9E3779B9u) ^ (static_cast<uint32_t>(i >> 32) + seed_hi));
}
inline bool drop_p_ok(float p) { return std::isfinite(p) && p >= 0.f && p < 1.f; }
inline DropMask drop_mask(float p, uint64_t seed) {
    const double t = std::floor((1.0 - static_cast<double>(p)) * 4294967296.0);
    return DropMask{static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), t >= 4294967295.0 ? 0xFFFFFFFFu : static_cast<uint32_t>(t),
                    1.0f / (1.0f - p)};
}

// per-thread record of the last HIP failure (flex_last_hip_error)
void note_hip_error(hipError_t e);

#define FLEX_HIP_TRY(expr)                          \
    do {                                            \
        hipError_t e_ = (expr);                     \
        if (e_ != hipSuccess) {                     \
            ::flex::note_hip_error(e_);             \
            return FLEX_ERR_HIP;                    \
        }                                           \
    } while (0)

// kernel launchers (spmm_kernels.hip)
int launch_spmm(const PlanView &v, int lanes_per_nz, bool off32, bool vec4, const float *dB, float *dC,
                hipStream_t s, int unroll = 0);
int launch_spmm_stamped(const PlanView &v, int lanes_per_nz, bool off32, const float *dB, float *dC, hipStream_t s);
int launch_fixup(const float *partial, const SplitRow *rows, uint32_t n_rows, int k, int ldc, float *dC,
                 hipStream_t s);
int kernel_attributes(int lanes_per_nz, bool off32, bool vec4, hipFuncAttributes *attr, int *waves_per_cu);
int launch_gather_rows(float *dst, const float *src, const int32_t *idx, int64_t n, int k, hipStream_t s);
int launch_tiles(const TileView &tv, bool off32, const float *dB, float *dC, int k, int ldb, int ldc, hipStream_t s);
int launch_blocks(const BlockView &bv, const float *dB, float *dC, hipStream_t s, bool vec4 = true);

// The launchers of the fused attention, one per kernel family and role (rows forward, rows backward, columns backward): what the entry
// points of attention_entry.h call, and all that the host simulator replaces.  The caller has checked the operands, decided that the
// launch is wanted and holds the plan's device; pick is the entry point's, (heads, lg) the head split of head_split_lg.
// FLEX_SIM_OPTIONAL: in a host simulator's build (-DFLEX_HOSTSIM) the launcher is a weak reference, so that a shim written before the
// launcher existed, which has no stand-in for it and calls none of its entry points, still links and loads against attention_entry.h.
// The library's build requires every launcher, and tests/test_attention_entry_host.py holds a built simulator to having them all.
#ifdef FLEX_HOSTSIM
#define FLEX_SIM_OPTIONAL __attribute__((weak))
#else
#define FLEX_SIM_OPTIONAL
#endif
namespace attention {
// single head (attention_kernels.hip, attention_backward_kernels.hip): the 16-byte or the generic form by pick.vec4
int launch_rows(const flex_plan *p, const AttentionPick &pick, const float *Q, const float *K, const float *V, float scale, float *Out, float *P,
                hipStream_t s);
int launch_rows_backward(const flex_plan *p, const AttentionPick &pick, const float *K, const float *V, const float *P, const float *G, float scale,
                         float *GQ, float *Work, hipStream_t s);
int launch_columns_backward(const flex_plan *p, const AttentionPick &pick, const float *Q, const float *G, const float *P, const float *DS, float *GK,
                            float *GV, hipStream_t s);
// per head, float rows (attention_heads_kernels.hip) and flex_bf16 rows (attention_bf16_kernels.hip)
int launch_heads_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Q, const float *K, const float *V, float scale,
                      float *Out, float *P, hipStream_t s);
int launch_heads_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const flex_bf16 *Q, const flex_bf16 *K, const flex_bf16 *V,
                      float scale, flex_bf16 *Out, float *P, hipStream_t s);
int launch_heads_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *K, const float *V, const float *P,
                               const float *G, float scale, float *GQ, float *Work, hipStream_t s);
int launch_heads_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const flex_bf16 *K, const flex_bf16 *V, const float *P,
                               const flex_bf16 *G, float scale, flex_bf16 *GQ, float *Work, hipStream_t s);
int launch_heads_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *Q, const float *G, const float *P,
                                  const float *DS, float *GK, float *GV, hipStream_t s);
int launch_heads_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const flex_bf16 *Q, const flex_bf16 *G,
                                  const float *P, const float *DS, flex_bf16 *GK, flex_bf16 *GV, hipStream_t s);
// per head with a bias, E = float or flex_bf16 (attention_bias_kernels.hip); the column launch is the unbiased one above
template <class E>
int launch_bias_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *Q, const E *K, const E *V, const float *Bias, float scale,
                     E *Out, float *P, hipStream_t s);
template <class E>
int launch_bias_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *K, const E *V, const float *P, const E *G,
                              float scale, E *GQ, float *GB, float *Work, hipStream_t s);
// per head with dropout after the softmax, E = float or flex_bf16, Bias / GB NULL without a bias (attention_dropout_kernels.hip)
template <class E>
FLEX_SIM_OPTIONAL
int launch_dropout_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *Q, const E *K, const E *V, const float *Bias,
                        float scale, const DropMask &dm, E *Out, float *P, hipStream_t s);
template <class E>
FLEX_SIM_OPTIONAL
int launch_dropout_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *K, const E *V, const float *P,
                                 const E *G, float scale, const DropMask &dm, E *GQ, float *GB, float *Work, hipStream_t s);
template <class E>
FLEX_SIM_OPTIONAL
int launch_dropout_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const E *Q, const E *G, const float *P,
                                    const float *DS, const DropMask &dm, E *GK, E *GV, hipStream_t s);
// GAT (attention_gat_kernels.hip)
int launch_gat_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *V, float slope,
                    float *Out, float *P, hipStream_t s);
int launch_gat_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *V,
                             const float *P, const float *G, float slope, float *GEl, float *Work, hipStream_t s);
int launch_gat_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *G, const float *P, const float *DX,
                                float *GEr, float *GV, hipStream_t s);
// GAT with dropout after the softmax (attention_gat_dropout_kernels.hip)
FLEX_SIM_OPTIONAL
int launch_gat_dropout_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const float *V,
                            float slope, const DropMask &dm, float *Out, float *P, hipStream_t s);
FLEX_SIM_OPTIONAL
int launch_gat_dropout_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er,
                                     const float *V, const float *P, const float *G, float slope, const DropMask &dm, float *GEl, float *Work,
                                     hipStream_t s);
FLEX_SIM_OPTIONAL
int launch_gat_dropout_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *G, const float *P,
                                        const float *DX, const DropMask &dm, float *GEr, float *GV, hipStream_t s);
// GAT on flex_bf16 V, Out, G and GV rows, dm NULL without dropout (attention_gat_bf16_kernels.hip)
FLEX_SIM_OPTIONAL
int launch_gat_bf16_rows(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er, const flex_bf16 *V,
                         float slope, const DropMask *dm, flex_bf16 *Out, float *P, hipStream_t s);
FLEX_SIM_OPTIONAL
int launch_gat_bf16_rows_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const float *El, const float *Er,
                                  const flex_bf16 *V, const float *P, const flex_bf16 *G, float slope, const DropMask *dm, float *GEl, float *Work,
                                  hipStream_t s);
FLEX_SIM_OPTIONAL
int launch_gat_bf16_columns_backward(const flex_plan *p, const AttentionPick &pick, int heads, int lg, const flex_bf16 *G, const float *P,
                                     const float *DX, const DropMask *dm, float *GEr, flex_bf16 *GV, hipStream_t s);
}  // namespace attention

// FLEX_PLAN_TIMING in the environment: phase times of the planner and the clustering on stderr.  The only environment
// variable the library reads; every tuning knob is a field of flex_plan_tuning (include/flex_spmm.h).
bool plan_timing_enabled();

// host-side helpers shared by the ABI files
int order_rcm_host(int64_t n, const uint32_t *rowPtr, const uint32_t *col, std::vector<uint32_t> &rank);
int order_cluster_host(int64_t n, const uint32_t *rowPtr, const uint32_t *col, std::vector<uint32_t> &rank,
                       const flex_cluster_tuning *tuning = nullptr);
int order_gorder_host(int64_t n, const uint32_t *rowPtr, const uint32_t *col, uint32_t window,
                      std::vector<uint32_t> &rank);
int validate_csr(const flex_csr *A);

}  // namespace flex
