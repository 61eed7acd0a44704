/*
 * flex_spmm.h -- C ABI of the MI355X-native SpMM engine (libflex_spmm.so).
 *
 * This is the drop-in boundary for the one hot path of guohaoqiang/Flex:
 *     C[m x k] = A[m x n, CSR, fp32] * B[n x k, row-major fp32]
 * The reference has no FFI layer; its seam is "host-side Mat/DataLoader objects
 * -> kernel launch" (flex.cu:4979-4988, 5057-5059, 5690-5693).  Each entry point
 * below names the reference code it replaces (paths relative to the reference
 * tree).  Plain pointers and sizes only; nothing here throws, every function
 * returns 0 (FLEX_OK) or a negative flex_status.  See INTEGRATION.md for the
 * reference-side binding.
 *
 * There is deliberately NO CPU SpMM in this library: a missing GPU or a missing
 * kernel is an error (FLEX_ERR_HIP / FLEX_ERR_UNSUPPORTED), never a fallback.
 * The reference's CPU loop (aspt/sspmm_128.cu:1415-1422) lives in oracle/ as
 * test infrastructure.
 */
#ifndef FLEX_SPMM_H
#define FLEX_SPMM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FLEX_ABI_VERSION 3 /* 3 also covers the purely additive FLEX_PLAN_MUTABLE_VALUES, flex_plan_set_values, flex_sddmm and the edge softmax (no struct grew),
                              the equally additive FLEX_PLAN_ATTENTION, flex_attention and flex_plan_attention_info (a new flag, two new calls, one new struct),
                              the equally additive FLEX_PLAN_ATTENTION_BACKWARD, flex_attention_backward and flex_plan_attention_backward_info (the same again),
                              the equally additive flex_attention_heads and flex_attention_heads_backward (two new calls, no flag, no struct),
                              the equally additive flex_gat_attention and flex_gat_attention_backward (the same again),
                              the equally additive flex_bf16, flex_attention_bf16 and flex_attention_bf16_backward (a typedef and two new calls, no flag, no struct),
                              the equally additive FLEX_PLAN_BF16, flex_spmm_bf16 and flex_plan_is_bf16 (a new flag and two new calls, no struct),
                              the equally additive flex_attention_bias, flex_attention_bf16_bias and their backward calls (four new calls, no flag, no struct),
                              the equally additive flex_attention_dropout, flex_attention_bf16_dropout, their backward calls and flex_dropout_mask (five new calls, no flag, no struct),
                              the equally additive flex_gat_attention_dropout and flex_gat_attention_dropout_backward (two new calls, no flag, no struct),
                              the equally additive flex_gat_attention_bf16, flex_gat_attention_bf16_dropout and their backward calls (four new calls, no flag, no struct),
                              the equally additive flex_gatv2_attention, flex_gatv2_attention_backward and flex_gatv2_attention_work_size (three new calls, no flag, no struct),
                              the equally additive flex_dropout_gatv2_attention and flex_dropout_gatv2_attention_backward (two new calls, no flag, no struct),
                              the equally additive flex_edge_gat_attention and flex_edge_gat_attention_backward (two new calls, no flag, no struct),
                              and the retired flex_plan_tuning.block_ablate, which keeps its place as block_ablate_retired and must be zero.
                              3: plan-time knobs leave the environment for the struct flex_plan_tuning, flex_plan_desc.tuning, flex_plan_get_tuning,
                              flex_order_cluster_ex, flex_set_host_threads; split rows are summed by a second launch by default.
                              2: flex_plan_info / flex_plan_stats grew; FLEX_PLAN_ROW_RANGE; flex_order_rabbit, flex_plan_measure_imbalance */

typedef enum flex_status {
    FLEX_OK = 0,
    FLEX_ERR_INVALID = -1,     /* bad argument (null, negative size, k<=0, unsorted rowPtr, col>=n) */
    FLEX_ERR_NOMEM = -2,       /* host allocation failed */
    FLEX_ERR_HIP = -3,         /* a HIP runtime call failed (≙ CUDA_CHECK, common.h:53-60); see flex_last_hip_error */
    FLEX_ERR_UNSUPPORTED = -4, /* shape outside what the kernels cover (nnz >= 2^32, m >= 2^31) */
    FLEX_ERR_IO = -5,          /* file could not be opened / read */
    FLEX_ERR_FORMAT = -6,      /* CSV does not parse (≙ stoi/stof throwing, assert(col.size()==vals.size()), DataLoader.cu:57) */
    FLEX_ERR_DUPLICATE = -7    /* duplicate (row,col) (≙ assert(e_inv[dst].count(r)==0), DataLoader.cu:97) */
} flex_status;

/* Host CSR view: the three vectors of DataLoader (DataLoader.cuh:32-34) + sizes (:70).
 * Indices are 32-bit unsigned exactly as in the reference. Not owned. */
typedef struct flex_csr {
    int32_t m, n;
    int64_t nnz;
    const uint32_t *rowPtr; /* m+1 */
    const uint32_t *col;    /* nnz, any order within a row, must be < n */
    const float *vals;      /* nnz */
} flex_csr;

/* HIP stream handle; identical to hipStream_t (pass torch's cuda_stream integer cast to a pointer). */
typedef struct ihipStream_t *flex_stream_t;

typedef struct flex_plan flex_plan;

/* flags for flex_plan_create: bits 0-3 = row schedule */
#define FLEX_ORDER_NATURAL 0u /* rows processed in the order given ("OVO") */
#define FLEX_ORDER_RCM 1u     /* rows scheduled in the reference's RCM order (order_rcm.cu:15-33);
                                 columns keep ORIGINAL ids, so B needs no permuteX pass and C
                                 comes out in original row order */
#define FLEX_ORDER_CLUSTER 2u /* rows scheduled community by community (agglomerative modularity
                                 clustering, ≙ DataLoaderRabbit, DataLoader.cu:453-655); same
                                 no-permutation contract as FLEX_ORDER_RCM */
#define FLEX_ORDER_GORDER 3u  /* rows scheduled in Gorder(window 3) order (≙ DataLoaderGorder, DataLoader.cu:789-857) */
#define FLEX_ORDER_MASK 0xFu
#define FLEX_PLAN_STATS 0x100u /* also collect flex_plan_stats while planning (one extra pass over the records) */
#define FLEX_PLAN_AUTOTUNE 0x200u /* measure instead of trusting the degree rule: plan the neighbouring column-tile
                                     widths too (same row schedule), time each on zero-filled operands of the real
                                     size, keep the fastest; likewise the other setting of tuning.bundle where the tile
                                     has row bundles and the caller left it to the rule.  Costs up to three extra plans
                                     and, for the duration of the call, device memory for one B and one C */
#define FLEX_PLAN_ROW_RANGE 0x1000u /* flex_plan_create_ex only: desc->row_begin/row_end name a row shard */
#define FLEX_PLAN_XCD_INTERLEAVE 0x2000u /* deal the chunks round-robin over the 8 XCDs instead of giving each XCD one
                                            contiguous eighth of the schedule.  For rows that arrive in a BFS-like order
                                            (a loader reordered by RCM / Gorder and planned as given): eighths of
                                            such an order run at different speeds.  FLEX_ORDER_RCM and FLEX_ORDER_GORDER
                                            imply it */
#define FLEX_PLAN_TRANSPOSE 0x8000u /* plan A^T instead of A: the plan is exactly the plan of the CSR of A^T passed as given (row c
                                       of A^T lists the rows of A that hold column c in ascending order, duplicates in CSR order),
                                       built on the host and freed before the call returns.  Every other argument refers to that
                                       CSR: k, ldb / ldc, the order bits, the shard rows of FLEX_PLAN_ROW_RANGE (columns of A),
                                       col_map, row_map, vo_mp (right as it is for a loader-permuted A' = P A P^T, whose transpose
                                       is P A^T P^T), tuning, autotune and stats.  flex_spmm then computes
                                       C[A.n x k] = A^T B[A.m x k] (the gradient of A B with respect to B), with the accuracy stated
                                       there for nnz(row) read as nnz(column of A); flex_plan_get_info reports m = A.n, n = A.m.
                                       A.n >= INT32_MAX: FLEX_ERR_UNSUPPORTED.  All five flex_plan_create* entry points take it */
#define FLEX_PLAN_MUTABLE_VALUES 0x10000u /* the plan's values may be replaced later (flex_plan_set_values) and the plan can run the SDDMM of
                                       its pattern (flex_sddmm).  Every nonzero stays on the flat record-stream route: the planner treats
                                       tuning.mfma and tuning.blocks as 2 ("never") and flex_plan_get_tuning reports 2 for both; an explicit
                                       mfma = 1 or blocks = 1 with this flag is FLEX_ERR_UNSUPPORTED (the dense-tile route picks its entries by
                                       their VALUES, and both routes store values in layouts of their own; neither is taken on any BASELINE
                                       graph).  Combines with every other flag and option of the five create entry points.  Extra device memory:
                                       8 bytes per record (the record -> entry map and the plan's copy of the values; records = nnz + padding,
                                       flex_plan_info.n_records), 16 bytes per padded run and per SDDMM work item (a run of at most 64 nonzeros
                                       of one row), 4 per group of items -- measured 8.6 bytes per nonzero on the reddit shape, 11-13 on graphs of short
                                       rows (more padding per nonzero), all counted in flex_plan_info.device_bytes; and the edge softmax's schedule
                                       (flex_softmax_info below): 4 bytes per row of hostA, 16 per work item, 4 per wave group.  Without the flag a plan is byte for byte what it was before the flag existed */

#define FLEX_PLAN_ATTENTION 0x40000u /* the plan can run the fused attention forward (flex_attention below).  Independent of
                                       FLEX_PLAN_MUTABLE_VALUES (an inference-only caller does not pay for the record -> entry map); the two
                                       combine.  Taken by flex_plan_create, _ld, _rows and _ex, in each case without a column or row map;
                                       FLEX_ERR_UNSUPPORTED together with FLEX_PLAN_TRANSPOSE or with a map (the softmax runs over hostA's rows:
                                       the transposed plan stays the gradient's tool).  Extra device memory, counted in
                                       flex_plan_info.device_bytes and reported by flex_plan_attention_info: 4 bytes per row and per entry of the
                                       plan's rows, 16 per work item, 4 per wave group.  Without the flag nothing is uploaded for it */

#define FLEX_PLAN_ATTENTION_BACKWARD 0x80000u /* (0x20000u is taken by flex_axw.h) the plan can also run the fused attention backward
                                       (flex_attention_backward below).  Requires FLEX_PLAN_ATTENTION (FLEX_ERR_INVALID without it) and is
                                       independent of FLEX_PLAN_MUTABLE_VALUES.  FLEX_ERR_UNSUPPORTED wherever FLEX_PLAN_ATTENTION is, and with
                                       FLEX_PLAN_ROW_RANGE or flex_plan_create_rows (a shard's gradients in K and V would be partial sums).
                                       Extra device memory, counted in flex_plan_info.device_bytes and reported by
                                       flex_plan_attention_backward_info: hostA's entries sorted by column -- 4 bytes per column, 8 per entry
                                       ({row, entry index}), 16 per work item, 4 per wave group.  Without the flag a plan uploads exactly what
                                       it uploads with FLEX_PLAN_ATTENTION alone */
#define FLEX_PLAN_BF16 0x100000u /* B and C are flex_bf16, the upper 16 bits of an IEEE float, and sums are fp32: the plan runs flex_spmm_bf16
                                       below and nothing else.  k, ldb and ldc stay in ELEMENTS and must be multiples of 8
                                       (FLEX_ERR_UNSUPPORTED otherwise): a bf16 row of k elements is, byte for byte, an fp32 row of k / 2 words,
                                       and the plan is the fp32 plan of that word width (lanes_per_nz, 32-bit offsets while n x ldb x 2 bytes
                                       <= 4 GiB, records, chunks, bundles, split rows; flex_plan_info keeps reporting k in elements).  Every
                                       nonzero stays on the flat record stream: tuning.mfma and tuning.blocks are forced to 2, split rows are
                                       summed by the second launch (tuning.split_rows = 2), and an explicit 1 in any of the three, or
                                       tuning.two_d = 1, is FLEX_ERR_UNSUPPORTED, as is the flag together with FLEX_PLAN_MUTABLE_VALUES,
                                       FLEX_PLAN_ATTENTION or FLEX_PLAN_AUTOTUNE.  Orders, row bundles, packed records, far_first, tile_group,
                                       FLEX_PLAN_TRANSPOSE, FLEX_PLAN_ROW_RANGE, maps, FLEX_PLAN_STATS and FLEX_PLAN_XCD_INTERLEAVE work as on
                                       the fp32 plan of the word width.  The partial sums of split rows are fp32: n_partials x k floats */

/* ≙ Mat::Mat + csr2_DiagTiling + alpha_transfer (mat.cu:7-31, 680-942, 268-293):
 * builds the row-panel plan for `hostA` and uploads it to `device`.  The reference's
 * pillar tiler is replaced by an nnz-balanced wave/row-panel planner. */
int flex_plan_create(flex_plan **out, const flex_csr *hostA, int k, int device, unsigned flags);

/* Same with strided dense operands: row r of B starts at dB + r*ldb, row r of C at dC + r*ldc (floats,
 * ldb >= k, ldc >= k); the ldc-k trailing floats of every C row are left untouched.  For callers whose
 * feature width is not a multiple of 32: a B row that is not a whole number of 128-byte cache lines costs
 * every gather an extra line (k=100 runs 50 % slower than k=128 on the reddit shape), so store k=100 with
 * ldb = ldc = 128.  No reference counterpart (the reference runs k = 32 and 128 only). */
int flex_plan_create_ld(flex_plan **out, const flex_csr *hostA, int k, int ldb, int ldc, int device, unsigned flags);

/* Same, for a CSR that a reordered loader already permuted (DataLoaderRcm &c.,
 * DataLoader.cu:723-857): row r' of hostA is original row vo_mp[r'] and column c' is
 * original column vo_mp[c'].  The plan folds both maps in at build time, so flex_spmm
 * still takes B and returns C in ORIGINAL order (the reference needs permuteX +
 * segVoMap for that: flex.cu:276-289, mat.cu:816-824). vo_mp==NULL means identity. */
int flex_plan_create_mapped(flex_plan **out, const flex_csr *hostA, const int32_t *vo_mp, int k,
                            int device, unsigned flags);

/* Plan for the row slice [row_begin,row_end) of hostA only (a shard of a row-sharded
 * multi-GPU run; the reference is single-GPU, flex.cu:4137).  flex_spmm then writes
 * (row_end-row_begin) x k into dC, slice row 0 first; dB is still the full B.
 * col_map (or NULL): column c of hostA reads B row col_map[c] -- pass the vo_mp of a
 * reordered CSR to keep using the un-permuted B.  Rows are scheduled in the order given
 * (flags must be FLEX_ORDER_NATURAL: reorder first, then shard). */
int flex_plan_create_rows(flex_plan **out, const flex_csr *hostA, int64_t row_begin, int64_t row_end,
                          const int32_t *col_map, int k, int device, unsigned flags);

/* Every option of the four entry points above in one call (they are thin wrappers over it), for the combinations
 * they do not name -- e.g. a row shard of a reordered matrix over padded storage.  Zero-initialise, set
 * struct_size = sizeof(flex_plan_desc), fill what is needed:
 *   row_begin/row_end  read only when flags has FLEX_PLAN_ROW_RANGE: the shard [row_begin,row_end), which may be
 *                      empty (the order bits must then be FLEX_ORDER_NATURAL); without the flag: all rows
 *   col_map            column c of A reads B row col_map[c] (NULL = c)
 *   row_map            row r of A writes C row row_map[r] (NULL = r - row_begin); all rows only, A square
 *   ldb/ldc            row strides of B and C in floats (0 = k) */
/* Plan-time tuning knobs (ABI 3; rounds 1-2 read them from the environment, which is process-global and racy).  Every
 * field: 0 = the planner's measured rule.  Nothing in the product sets them; they exist for the tests, the
 * soak and tools/.  flex_plan_get_tuning returns the values a plan was actually built with. */
typedef struct flex_cluster_tuning { /* flex_order_cluster_ex / FLEX_ORDER_CLUSTER plans */
    int32_t batch;     /* proposals per batch of the agglomeration (4096) */
    int32_t no_refine; /* 1: skip the second stage (vertex moves between stretches of the order) */
    int32_t stretch;   /* positions per stretch (1024), >= 16 */
    int32_t sweeps;    /* sweep limit (8) */
    int32_t stride;    /* largest sampling stride of a long row (4) */
} flex_cluster_tuning;
typedef struct flex_plan_tuning {
    int32_t lanes_per_nz;    /* G = 4 (k <= 16 only) / 8 / 16 / 32 / 64 lanes per record (column tile of 4G columns), capped by k */
    int32_t chunk_records;   /* chunk budget: records per wave */
    int32_t long_row;        /* rows longer than this are cut into pieces (chunk_records) */
    int32_t piece_records;   /* ... of about this many records (chunk_records) */
    int32_t row_cost;        /* records a row boundary counts for when chunks are cut (16) */
    int32_t xcd_slices;      /* 1: every XCD walks one contiguous slice of the schedule; 2: round-robin (rule: 1 except RCM / Gorder);
                                3: stretches of xcd_stretch workgroups dealt to the XCDs in turn (the eight XCDs walk ADJACENT stretches of the
                                schedule at any time, each still on its own stretch) */
    int32_t xcd_balance;     /* 2: slices cut by chunk count instead of by cost */
    int32_t chunk_cost, task_cost; /* cost model of the slice balancing (16, 2) */
    int32_t split_rows;      /* how the pieces of a split row are summed: 2 = by spmm_fixup_kernel after the launch (the default: it
                                needs nothing beyond stream order); 1 = inside the launch by the piece that arrives last (relaxed
                                agent atomics + sc1 stores and loads: measured on gfx950, not an architectural guarantee) */
    int32_t rec_nt;          /* record stream read with non-temporal loads: 1 on, 2 off */
    int32_t unroll;          /* 8: eight gathers in flight per wave on the narrow tiles too */
    int32_t two_d;           /* 1: rows are also cut by column panel (the 2-D schedule) */
    int32_t panel_kb;        /* ... panel = this many KiB of one column tile of B (2048) */
    int32_t seg_min;         /* ... runs shorter than this stay in the row's last piece (4) */
    int32_t mfma;            /* dense 32x32 tiles to the MFMA kernel: 1 always route, 2 never (rule: when a sample finds >= 10 % of nnz) */
    int32_t mfma_fill_pct;   /* ... tiles of at least this fill (60) */
    int32_t lds_extra;       /* bytes of idle LDS per workgroup (occupancy throttle; multiple of 16) */
    int32_t host_threads;    /* host threads of this call (rule: flex_set_host_threads, else the core count, at most 32) */
    flex_cluster_tuning cluster;
    /* the hot-block path (the matrix is SPLIT: nonzeros with reuse inside a block of rows are multiplied out of LDS-staged B panels by
       their own kernel after the flat kernel has done the rest) */
    int32_t blocks;           /* 1: split, 2: never (rule: k >= 64 and a very large input -- >= 983 040 rows of average degree >= 48 -- on which
                                 a sampled look finds >= 72 % of the nonzeros in columns that a block of 480 rows uses three times or more;
                                 operands that are not 16-byte aligned run through generic kernels, correct and slow, as for flat plans) */
    int32_t block_rounds;     /* rows per slot: 2, 4 or 8; a block is rounds x 60 rows (8; 4 / 2 while there are few blocks per CU) */
    int32_t block_panel_rows; /* B rows per LDS panel: a multiple of 4, at most 304 (304) */
    int32_t block_thr;        /* a column is hot (staged) when at least this many nonzeros of the block use it (3) */
    int32_t block_cap;        /* nonzeros per slot: a longer row is spread over ceil(len / cap) slots, summed through LDS (1.5 x the average degree) */
    int32_t block_ablate_retired; /* zero: once a timing-only knob, kept so that no later field moves */
    int32_t tile_group;       /* multi-tile launches: workgroups per group -- every XCD's slice of the schedule is walked group by group, all
                                 column tiles of a group back to back, so that a group's records are re-read from the Infinity Cache rather
                                 than from HBM (0 = rule; 1 = off: one pass over the whole schedule per tile) */
    int32_t xcd_stretch;     /* xcd_slices = 3: workgroups (4 chunks each) per stretch (256) */
    int32_t far_first;       /* > 0: inside every task the records whose column lies more than this many schedule positions from the row come
                                FIRST (a wave's gathers return in order: with the likely L2 misses issued together, only those groups of
                                gathers wait for the fabric) (rule: see plan_build.cpp, fill_records) */
    int32_t bundle;          /* row bundles: tasks that hold up to 64 / lanes_per_nz SHORT rows side by side, one per record slot -- no
                                cross-slot reduction and one store per lane at the end instead of a reduction and a store per row
                                (≙ the reference's narrow kernel giving every thread its own row, flex.cu:81-118): 1 on, 2 off
                                (rule: on when the plan holds a chunk for every wave slot of the card, or its average degree is below 16
                                -- and then on the tiles of 4 or more slots per step: wider k runs the 16-lane tile instead of the
                                32-lane one; plan_build.cpp, bundle_rule) */
    int32_t bundle_len;      /* ... rows of at most this many nonzeros are candidates (12 on the tiles of 8 or 16 slots per step, 16 on the 4-slot tile) */
    int32_t rec_pack;        /* the record stream at 6 bytes per record (value + 16-bit column difference) instead of 8: 1 on, 2 off
                                (rule: on for launches of two or more column tiles whose stream is at least 32 MB, holds less than 5 % of
                                its records in chunks with row bundles, which keep the 8-byte form, and needs fewer than one exception --
                                a column difference beyond 16 bits, 8 bytes each -- per 16 records).  Never on 2-D plans, on plans with
                                FLEX_PLAN_MUTABLE_VALUES or FLEX_PLAN_ATTENTION, or where k, ldb or ldc is no multiple of 4: flex_plan_get_tuning
                                then reports 2.  C is bit for bit the same either way */
    int32_t hub_row;         /* hub rows cut by schedule window (plan_build.cpp, cut_hub_rows): of a row of at least this many
                                nonzeros (1024), those whose columns' vertices sit in one window of the schedule become a piece that runs
                                among the rows of THAT window, beside the rows that read the same B rows.  > 1 also forces the cut on where
                                the kind of plan allows it: the whole square matrix on the 1-D record stream, contiguous XCD slices, no dense
                                tiles or hot blocks taken, rows and columns named alike -- no map, or ONE array passed as both col_map and row_map
                                (flex_plan_create_mapped); two separate arrays, even equal ones, leave the plan uncut; never with
                                FLEX_PLAN_MUTABLE_VALUES, FLEX_PLAN_ATTENTION, FLEX_PLAN_TRANSPOSE or a
                                row range.  1 in any of the three knobs forces it off, and is what flex_plan_get_tuning reports when it is
                                off.  C stays within rounding (a hub row's sum is taken in another order), reproducibly */
    int32_t hub_window;      /* ... schedule positions per window (8192) */
    int32_t hub_min_run;     /* ... a window's nonzeros move only if they are at least this many (32) */
    int32_t reserved[1];     /* zero */
} flex_plan_tuning;

typedef struct flex_plan_desc {
    size_t struct_size;
    const flex_csr *A;
    int k, ldb, ldc, device;
    unsigned flags;
    int64_t row_begin, row_end;
    const int32_t *col_map, *row_map;
    const flex_plan_tuning *tuning; /* ABI 3; NULL = rules.  A caller built against ABI 2 passes the shorter struct_size */
} flex_plan_desc;
int flex_plan_create_ex(flex_plan **out, const flex_plan_desc *desc);
int flex_plan_get_tuning(const flex_plan *plan, flex_plan_tuning *out);

/* Process-wide cap on the worker threads of the planner, the orderings and the generator (0 = the core count, at most
 * 32 either way); returns the previous value.  For N ranks on one host: host cores / N.  Thread-safe; results never
 * depend on the thread count (tests/test_planner_host.py). */
int flex_set_host_threads(int n);

/* ≙ launch_prep + cudaMemset(C) + kernel<<<>>> (mat.cu:32-41, flex.cu:5057-5059).
 * dB: n x k row-major device fp32; dC: m x k row-major device fp32, fully overwritten
 * (alpha=1, beta=0 as in cuSpmm, flex.cu:5728-5729).  Asynchronous on `stream`;
 * no allocation, no host sync (safe to capture in a hipGraph).  dB/dC must be
 * 16-byte aligned when k % 4 == 0.
 * NOT re-entrant per plan: a plan owns the partial-sum workspace and arrival counters of its split
 * rows, so at most ONE launch of a given plan may be in flight -- do not enqueue the same plan on two
 * streams, or replay two graphs holding it, concurrently (successive launches on one stream are fine;
 * different plans are independent).  Checked for eager launches: a launch on a DIFFERENT stream while the stream of the
 * plan's latest launch still has work pending returns FLEX_ERR_INVALID and enqueues nothing (a stream query when the
 * stream changes: no cost for a plan that stays on its stream; conservative -- unrelated work queued behind the plan's
 * launch on the old stream counts as pending too).  Launches captured into a graph are not checked (nor are replays):
 * ordering those is the caller's.  Plans without split rows (flex_plan_info.n_partials == 0) hold no workspace and may
 * overlap freely.
 * Accuracy (tests/f64ref.py): with C64 = the float64 product of the fp32 inputs, S = |A| |B|, u = 2^-24 and
 * n_r = nnz(row r) + 32, every entry whose C64 is finite is finite and within gamma(n_r) S + n_r 2^-149 of it (gamma(n) = n u / (1 - n u));
 * every entry whose C64 is not finite is NaN / +inf / -inf exactly as C64 is.  Both hold while no fp32 sum can overflow (S over the
 * finite terms < 2^120), with one residual: a row -- or a piece of a split row, or a row in a bundle -- whose stored values are ALL
 * nonzero subnormals of at most p units of 2^-149 each, p = the padding records its task needs (< 64 / lanes_per_nz, or < bundle_len
 * in a bundle), may give NaN where C64 is +-inf (its padding carries value 0).  Subnormal inputs and results are kept, not flushed. */
int flex_spmm(flex_plan *plan, const float *dB, float *dC, flex_stream_t stream);

typedef uint16_t flex_bf16; /* the upper 16 bits of an IEEE float */
/* flex_spmm on bf16 operands (FLEX_PLAN_BF16 plans only; FLEX_ERR_INVALID on any other plan, as flex_spmm, flex_plan_measure_imbalance
 * and the flex_axw calls are on a bf16 plan; nothing is enqueued).  dB: n x k row-major device flex_bf16, row stride ldb elements;
 * dC: m x k row-major device flex_bf16, row stride ldc elements, columns [0, k) of every row fully overwritten.  Both must be 16-byte aligned
 * (FLEX_ERR_UNSUPPORTED otherwise, C untouched): only the vector form is built.  Asynchronous, no allocation, no host sync, not
 * re-entrant per plan and guarded exactly as flex_spmm is.  Two launches: the row kernel, then the sum of the split rows' pieces.
 * Definition: read every element of B as the fp32 number it is; with x32 = what flex_spmm's contract allows for that fp32 input
 * (fp32 products and sums in the plan's order, pieces of a split row added in fp32), C = rn_bf16(x32): ONE rounding to bf16, to
 * nearest even, at the store; a NaN stays a quiet NaN, +-inf stays, what rounds past the largest finite bf16 becomes +-inf.  A row
 * without nonzeros is +0.  Accuracy (tests/spmm_bf16_ref.py): with C64 and bound32 = gamma(n_r) S + n_r 2^-149 as for flex_spmm on
 * the widened B, every entry whose C64 is finite satisfies |C - C64| <= bound32 + 2^-8 (|C64| + bound32) + 2^-134, and is finite
 * unless |C64| + bound32 reaches the largest finite bf16; every other entry has C64's class exactly, under flex_spmm's residual. */
int flex_spmm_bf16(flex_plan *plan, const flex_bf16 *dB, flex_bf16 *dC, flex_stream_t stream);
/* 1 for a FLEX_PLAN_BF16 plan, 0 for any other, FLEX_ERR_INVALID (negative) for NULL */
int flex_plan_is_bf16(const flex_plan *plan);

/* Learnable edge values (FLEX_PLAN_MUTABLE_VALUES plans only; FLEX_ERR_INVALID on any other plan).  No reference counterpart.
 *
 * Value refresh: dVals is a device array of hostA->nnz floats in the CSR order of the hostA passed to the create call -- for EVERY
 * kind of plan: a transposed plan takes the same vector as the plan of A, a shard plan reads its own rows' entries of the full
 * vector.  The value half of every record is rewritten on the GPU, padding included, so that afterwards the plan's device image is
 * bit for bit the image the create call would have built from the same CSR with these values (one padding rule for both:
 * flex_amd/csrc/internal.h, pad_values).  Asynchronous on `stream`; no allocation, no host synchronisation (safe to capture in a
 * hipGraph).  Ordering is the caller's, as for writing B: the call must be ordered after every launch of the plan that still reads
 * the old values, and the launches that should see the new values after it (one stream does both).  Moves 20 bytes per record
 * (map, value, the plan's copy, the record's value half) plus the padded runs again. */
int flex_plan_set_values(flex_plan *plan, const float *dVals, flex_stream_t stream);

/* SDDMM over the plan's pattern, defined as the adjoint of the plan's own SpMM with respect to its values: the plan computes
 * C[dst(e)] += v_e B[src(e)] over the entries e it holds, and this writes
 *     dOut[e] = sum_j G[dst(e), j] B[src(e), j]      (= d<G, C> / d v_e)
 * for every entry the plan holds, indexed like dVals above (hostA's CSR order); entries the plan does not hold (other shards) are
 * left untouched.  This one definition covers transposed, mapped and shard plans: for the plan of A it is the gradient of C = A(v) B
 * with respect to v (and the score kernel of graph attention, <G[row], B[col]>); for the plan of A^T, G is n x k and B is m x k.
 * G has C's shape and row stride (ldc), B has B's (ldb).  Operands that are not 16-byte aligned, or k % 4 != 0, run a generic
 * kernel: correct, slower.  k <= 1024 (wider: FLEX_ERR_UNSUPPORTED).  Asynchronous on `stream`, no allocation, no host
 * synchronisation; deterministic (bit-identical run to run: fixed reduction order, no atomics).  Reads no value of the plan, so it
 * needs no ordering against flex_plan_set_values.
 * Accuracy, against D64 = the float64 dot of the fp32 inputs, T = sum_j |G B| and u = 2^-24: where D64 is finite the result is finite
 * and within gamma(k) T + k 2^-149 of it (gamma(n) = n u / (1 - n u)); where D64 is not finite the result is NaN / +inf / -inf exactly
 * as D64, while no fp32 partial sum overflows (T over the finite terms < 2^120).  Columns past k (padding lanes, the ld - k tail of
 * a strided row) contribute nothing: they are never read, so no 0 x inf can turn an inf into NaN. */
int flex_sddmm(const flex_plan *plan, const float *dG, const float *dB, float *dOut, flex_stream_t stream);

/* Edge softmax: the softmax of a score per entry over each ROW of hostA, the step between the SDDMM's scores and the SpMM of graph
 * attention (Out = A(alpha) V, alpha = softmax over each row of scale x <Q[row], K[col]>).  FLEX_PLAN_MUTABLE_VALUES plans only
 * (FLEX_ERR_INVALID on any other plan).  No reference counterpart.
 *
 * All arrays are device arrays of hostA->nnz floats in the CSR order of the hostA passed to the create call, for every kind of plan, and
 * the rows are ALWAYS the rows of hostA: a transposed plan takes the same vectors as the plan of A and gives the same bits (the
 * schedule is made from hostA's row pointer alone).  A shard plan reads and writes the entries of its own rows only and leaves the rest
 * of the output untouched; a transposed plan with a row range holds pieces of hostA's rows: FLEX_ERR_UNSUPPORTED.
 *
 * Forward, row r with entries e:   dOut[e] = exp(scale (s_e - M_r)) / sum_j exp(scale (s_j - M_r)),   M_r = the row's largest score.
 * The difference is taken before the multiplication by scale.  scale must be finite and > 0 (else FLEX_ERR_INVALID).
 * Backward, p = dP (the forward's output), g = dGradP:   dGradS[e] = scale p_e (g_e - sum_j p_j g_j).
 * Special values of the forward:
 *   - a score of -inf is a masked edge: its p is exactly +0;
 *   - a row whose scores are ALL -inf gives +0 everywhere (a definition: the row attends to nothing and the SpMM writes a zero row);
 *   - a row that holds a +inf or a NaN gives NaN in every entry of that row (what exp(s - max) / sum gives in float64);
 *   - a row without entries: nothing is read, nothing written; nnz == 0: FLEX_OK, no launch.
 * The backward has no special cases: it is the formula in fp32, so a NaN row of p gives a NaN row, 0 x inf gives NaN.
 * In place is allowed (dOut == dScores, dGradS == dGradP); any other overlap is the caller's error.  Asynchronous on `stream`, one
 * launch, no allocation, no host synchronisation (safe to capture in a hipGraph), no atomics, fixed reduction order: bit-identical
 * run to run.  Arrays that are not 16-byte aligned run the same kernel with 4-byte accesses: same bits, slower.
 * A row is reduced by one wave (up to 1024 entries) or by one workgroup (longer): a row of millions of entries is correct and slow.
 *
 * Accuracy, against float64 on the fp32 inputs; u = 2^-24, gamma(n) = n u / (1 - n u), n_r = entries of the row, D_r = min(104, scale x
 * the spread of the row's finite scores), E = the error of the device's expf in ulp (measured: DESIGN.md 3.10):
 *   forward    |p - p64| <= gamma(n_r + 4 D_r + 2 E + 4) p64 + 2^-126
 *   backward   |gs - gs64| <= gamma(n_r + 4) scale p_e (|g_e| + sum_j |p_j g_j|) + max(1, scale) n_r 2^-149, float64 on the SAME fp32 p.
 * Forward, derivation.  The exponent a = fl(scale fl(s - M)) carries two roundings, |a - a64| <= 2 u |a64| (1 + u), and |a64| <= D_r for every
 * term that does not underflow (below -104 a term is < 2^-149 and contributes at most the absolute 2^-126 share), so the term
 * t = expf(a) has the relative error (1 + E u) exp(2 u D_r (1 + u)) - 1 <= gamma(2 D_r + E + 1).  The terms are positive: the sum L of the
 * computed terms, added in a tree of depth <= n_r, is within gamma(2 D_r + E + 1 + n_r) of the exact sum (>= 1: the largest term is
 * exactly 1).  p = fl(t / L) adds one rounding; numerator and denominator together: gamma(n_r + 4 D_r + 2 E + 3), stated with + 4.
 * Terms or quotients below 2^-126 may be flushed or rounded as subnormals: at most 2^-126 absolute.  Where a row is longer than one
 * wave's registers the partial sums of its parts are rescaled by exp(scale (m_part - M_r)) <= 1 before they are added, which costs each
 * part E + 3 more roundings: they are covered, because a tree over 64 lanes x parts has depth <= n_r / 64 + 8 where the bound grants n_r.
 * Backward: the products p_j g_j (one rounding each), their sum in a tree of depth <= n_r, one subtraction and two products. */
int flex_edge_softmax(const flex_plan *plan, const float *dScores, float scale, float *dOut, flex_stream_t stream);
int flex_edge_softmax_backward(const flex_plan *plan, const float *dP, const float *dGradP, float scale, float *dGradS, flex_stream_t stream);

/* The schedule of the two calls above (host side; what the plan uploaded for them is counted in flex_plan_info.device_bytes).
 * FLEX_ERR_INVALID on a plan without FLEX_PLAN_MUTABLE_VALUES, FLEX_ERR_UNSUPPORTED on a transposed plan with a row range. */
typedef struct flex_softmax_info {
    int64_t rows;          /* rows of hostA the plan computes the softmax of */
    int64_t entries;       /* their entries */
    int64_t items;         /* work items: packed runs of short rows + wave rows + block rows */
    int64_t groups;        /* wave groups: one wave each, four to a workgroup (block rows are workgroups of their own) */
    int64_t rows_empty;    /* rows without entries: in no item, or carried inside a packed item */
    int64_t rows_packed;   /* rows that share a window of 256 entries with their neighbours */
    int64_t rows_wave;     /* rows reduced by one wave of their own (up to 1024 entries) */
    int64_t rows_block;    /* rows reduced by a workgroup of their own */
    int64_t group_entries; /* the balance promised: a group of more than one item holds at most this many entries */
    int64_t device_bytes;  /* device memory of the schedule: 4 per row, 16 per item, 4 per group */
} flex_softmax_info;
int flex_plan_softmax_info(const flex_plan *plan, flex_softmax_info *out);

/* Fused attention forward (FLEX_PLAN_ATTENTION plans only; FLEX_ERR_INVALID on any other plan): scores, softmax and the SpMM with the
 * result in ONE launch, without the nnz-sized arrays of the composition flex_sddmm -> flex_edge_softmax -> flex_plan_set_values ->
 * flex_spmm.  No reference counterpart.  For every row r of the plan, with entries e in hostA's CSR order and src(e) = hostA->col[e]:
 *     s_e     = <Q[r], K[src(e)]>                                   (over the k columns)
 *     alpha_e = exp(scale (s_e - M_r)) / sum_j exp(scale (s_j - M_r)),   M_r = the row's largest score     (flex_edge_softmax's definition)
 *     Out[r]  = sum_e alpha_e V[src(e)]
 * Q and Out have C's shape, row stride (ldc) and row convention (flex_sddmm's G: a shard's row r0 + i is row i); K and V have B's, with
 * stride ldb.  Special values follow flex_edge_softmax: a score of -inf is a masked edge (alpha = +0); a row whose scores are all -inf,
 * and a row without entries, write a +0 row of Out; a row that holds a +inf or NaN score writes NaN in all k columns of Out and in all
 * its entries of dP.  Non-finite Q, K and V follow IEEE through the formulas: every entry of the row, masked or not, multiplies its V
 * row (+0 x inf = NaN), so a NaN or inf in a V row reaches exactly the Out rows that have an entry to it, as in the composition.
 * dP == NULL: nothing nnz-sized is written.  Otherwise dP (hostA->nnz floats, hostA's CSR order) receives alpha_e for the entries of the
 * plan's rows -- what flex_edge_softmax_backward and the existing backward chain start from -- and entries of other shards are untouched;
 * Out has the same bits either way.  scale must be finite and > 0 (else FLEX_ERR_INVALID); NULL Q, K, V or Out: FLEX_ERR_INVALID; a
 * plan without entries: FLEX_OK, no launch, nothing written.  k <= 1024 (wider: FLEX_ERR_UNSUPPORTED); no column at or past k is read.
 * Operands that are not 16-byte aligned, or k, ldb or ldc not a multiple of 4, run a generic instantiation: correct, slower.
 * One launch, asynchronous on `stream`, no allocation, no host synchronisation (safe to capture in a hipGraph), no atomics, fixed
 * reduction order: bit-identical run to run.  A row is owned by one slot of lanes, one wave or one workgroup (by its length, see
 * flex_attention_info); no row is split over workgroups: a row of millions of entries is correct and slow.
 *
 * Accuracy, against float64 on the fp32 inputs.  u = 2^-24, gamma(n) = n u / (1 - n u), n_r = entries of the row, E = the error of the
 * device's expf in ulp, D_r = min(104, scale x the spread of the row's finite scores) as for flex_edge_softmax, and R_r = the number of
 * times the state that reaches the result can be rescaled: R_r = ceil(n_r / 4) + 8 (the maximum is raised at most once per pass of
 * four entries, and no slot makes more passes than the row has; then at most 4 merges between the up to 16 slots of a wave and 3
 * between the waves of a workgroup, stated as 8).
 *   score   ds_e     = gamma(k) sum_j |Q K| + k 2^-149                     (flex_sddmm's bound: the reduction depth stays <= k)
 *   alpha   dalpha_e = alpha_e [gamma(n_r + 4 D_r + (E + 3) R_r + 2 E + 4) + expm1(2 scale max_row(ds + |s| u))] + 2^-126
 *   Out     |Out - Out64| <= sum_e (gamma(n_r + 3) alpha_e + dalpha_e) |V| + 2^-126
 * dP is held to dalpha on its own.  Derivation.  The scores are the SDDMM's: per lane a chain of fmas over its columns, then a tree over
 * the lanes of the slot, columns at or past k adding nothing, depth <= k.  Moving every score of a row by at most d = max_row(ds + |s| u)
 * (|s| u: the rounding of the float64 score to the fp32 one the softmax starts from) moves a softmax by at most the factor
 * exp(2 scale d): the expm1 term.  From the fp32 scores on it is flex_edge_softmax's derivation -- a term expf(fl(scale fl(s - m)))
 * carries gamma(2 D_r + E + 1), the positive terms are summed in a tree of depth <= n_r, one division -- with one addition: a term is
 * taken under the maximum m of the moment, and each later rise of the maximum (and each merge of two partial states) multiplies the
 * running sum and the running Out row by one more factor expf(fl(scale fl(m - m'))), E + 3 roundings each (two in the argument, whose
 * effect is bounded as for the terms inside the 4 D_r already granted once the chain's arguments add up to at most D_r, E for expf, one
 * for the product): (E + 3) R_r.  dP's numerator is taken directly under the final maximum and divided by the same sum.  The Out row adds
 * its terms alpha V by fma (one rounding per addition: n_r, inside a tree of the same shape as the sum's), is rescaled with the sum (the
 * roundings differ from the sum's by one product per rescale, already counted in R_r for both), and is divided once: c = 3 covers the
 * product-free fma, the division and the merge's final addition.  Results below 2^-126 may be flushed or rounded as subnormals: 2^-126. */
int flex_attention(const flex_plan *plan, const float *dQ, const float *dK, const float *dV, float scale, float *dOut, float *dP, flex_stream_t stream);

/* The schedule of flex_attention (host side).  FLEX_ERR_INVALID on a plan without FLEX_PLAN_ATTENTION. */
typedef struct flex_attention_info {
    int64_t rows;         /* rows of the plan: each writes one row of Out */
    int64_t entries;      /* their entries */
    int64_t items;        /* work items: runs of slot rows (one per slot of a wave) + wave rows + block rows */
    int64_t groups;       /* wave groups: one wave each, four to a workgroup (block rows are workgroups of their own) */
    int64_t rows_empty;   /* rows without entries: they ride in the slot items and write +0 */
    int64_t rows_slot;    /* rows of at most 32 entries: one slot of W lanes (W = 4 .. 64 by k, as the SDDMM) owns the row, 64 / W rows side by side */
    int64_t rows_wave;    /* rows of at most 512 entries: the slots of one wave stride the row and merge by shuffles */
    int64_t rows_block;   /* longer rows: the four waves of a workgroup share the row and merge through LDS */
    int64_t group_budget; /* the balance promised: a group of more than one item costs at most this much (an item costs its entries + its rows) */
    int64_t device_bytes; /* device memory of the image: 4 per row, 4 per entry, 16 per item, 4 per group */
} flex_attention_info;
int flex_plan_attention_info(const flex_plan *plan, flex_attention_info *out);

/* Fused attention backward (FLEX_PLAN_ATTENTION_BACKWARD plans only; FLEX_ERR_INVALID on any other plan): the gradients of flex_attention's
 * Out in Q, K and V from the probabilities it kept, in TWO launches, in place of the chain of three flex_plan_set_values, three flex_spmm
 * (two on a transposed plan), flex_sddmm and flex_edge_softmax_backward.  No reference counterpart.  Entries e of row r in hostA's CSR order,
 * src(e) = hostA->col[e], g = dGradOut (Out's shape and stride ldc), p = the dP that flex_attention wrote:
 *     da_e    = <g[r], V[src(e)]>                       (over the k columns)
 *     delta_r = sum_j p_j da_j                          (over the row's entries)
 *     ds_e    = scale p_e (da_e - delta_r)              (flex_edge_softmax_backward's formula)
 *     gQ[r]   = sum_{e in row r}      ds_e K[src(e)]
 *     gK[c]   = sum_{e: src(e) == c}  ds_e Q[row(e)]
 *     gV[c]   = sum_{e: src(e) == c}  p_e  g[row(e)]
 * No special cases, as in flex_edge_softmax_backward: the formulas in fp32 under IEEE.  A NaN row of p gives a NaN row of ds and of gQ and
 * NaN in the gK and gV rows of the columns it touches; a masked entry (p = +0) still multiplies (0 x inf = NaN).  No column at or past k
 * is read.  dWork: hostA->nnz floats in hostA's CSR order; on return it holds ds, the gradient in the scores, whenever dGradQ or dGradK
 * was asked for.  It must not alias dP (FLEX_ERR_INVALID where the two pointers are equal; any other overlap is the caller's error).
 * Each of dGradQ, dGradK, dGradV may be NULL: that output is not written, a launch whose outputs are all NULL is skipped, and an output
 * has the same bits whichever others are asked for.  gQ has Out's shape and stride (ldc), gK and gV have K's and V's (ldb).  Rows of gQ
 * without entries, and rows of gK / gV whose column has no entry, are written as +0.  The checks are flex_attention's: scale finite and
 * > 0 (else FLEX_ERR_INVALID); a plan without entries: FLEX_OK, no launch, nothing written; NULL Q, K, V, P, GradOut or Work:
 * FLEX_ERR_INVALID; k <= 1024 (wider: FLEX_ERR_UNSUPPORTED).  Operands that are not 16-byte aligned, or k, ldb or ldc not a multiple of
 * 4, run a generic instantiation: correct, slower.  Asynchronous on `stream`, no allocation, no host synchronisation (safe to capture in
 * a hipGraph), no atomics, fixed reduction order: bit-identical run to run.  The first launch walks the rows as flex_attention does
 * (every entry gathers its V row once and its K row once) and writes ds and gQ; the second walks hostA's columns (entries of a column in
 * CSR order) and writes gK and gV.  No row and no column is split over workgroups: one of millions of entries is correct and slow.
 *
 * Accuracy, against float64 on the SAME fp32 Q, K, V, p and g (as for flex_edge_softmax_backward).  u = 2^-24, gamma(n) = n u / (1 - n u),
 * n_r = entries of the row, n_c = entries of the column, a = 3, b = 0:
 *   dda_e    = gamma(k) sum_j |g V| + k 2^-149                                             (flex_sddmm's bound)
 *   dds_e    = gamma(n_r + a) scale p_e (|da_e| + sum_j |p_j da_j|) + scale p_e (dda_e + sum_j p_j dda_j) + max(1, scale) n_r 2^-149
 *   |gQ - gQ64| <= sum_{e in r} (gamma(n_r + b) |ds_e| + dds_e) |K[src]| + 2^-126
 *   |gK - gK64| <= sum_{e in c} (gamma(n_c + b) |ds_e| + dds_e) |Q[row]| + 2^-126
 *   |gV - gV64| <= sum_{e in c}  gamma(n_c + b) p_e |g[row]|            + 2^-126
 * Derivation.  da is the SDDMM's reduction (per lane a chain of fmas over its columns, a tree over the lanes of the slot, depth <= k).
 * delta: every slot adds its terms by delta = fma(p_j, da_j, delta) -- the product is not rounded, one rounding per addition -- and the
 * partial sums of the slots of a wave (at most 4 butterfly steps) and of the waves of a workgroup (3 additions) are added plainly: a tree
 * of depth <= n_r for every class of row (a slot row is a chain of exactly n_r; a wave row has n_r >= 33 and a slot of it at most
 * 4 ceil(n_r / (4 slots)) additions and 4 merges; a block row has n_r >= 513), so delta carries gamma(n_r) sum_j |p_j da_j| and the
 * da's own errors weighted by p.  ds = fl(fl(scale p_e) fl(da_e - delta)): one subtraction and two products, a = 3 -- one fewer than
 * flex_edge_softmax_backward, whose products p_j g_j are rounded.  Products below 2^-126 round as subnormals: the n_r 2^-149 term.
 * gQ, gK and gV add their terms by fma on each lane's own columns (no reduction across lanes) in a chain per slot, then the same
 * merges: depth <= n_r (n_c), the first fma into +0 being the rounding of the product, and no rounding besides: b = 0.  The ds that
 * enters gQ and gK is the computed fp32 one: dds.  gV takes p and g as given: a lone entry's term is rounded once, so err / bound can
 * come close to 1 there (|fl(x) - x| <= u |x| against gamma(1) |x|) -- tightness of the bound, not a fault.  First order, as the bounds above. */
int flex_attention_backward(const flex_plan *plan, const float *dQ, const float *dK, const float *dV, const float *dP,
                            const float *dGradOut, float scale, float *dGradQ, float *dGradK, float *dGradV, float *dWork,
                            flex_stream_t stream);

/* The schedule of flex_attention_backward's second launch (host side; its first launch walks flex_attention_info's items).
 * FLEX_ERR_INVALID on a plan without FLEX_PLAN_ATTENTION_BACKWARD. */
typedef struct flex_attention_backward_info {
    int64_t columns;       /* columns of hostA: each writes one row of gK and of gV */
    int64_t entries;       /* hostA's entries */
    int64_t items;         /* work items: runs of slot columns (one per slot of a wave) + wave columns + block columns */
    int64_t groups;        /* wave groups: one wave each, four to a workgroup (block columns are workgroups of their own) */
    int64_t columns_empty; /* columns without entries: they ride in the slot items and write +0 */
    int64_t columns_slot;  /* columns of at most 32 entries (flex_attention_info's classes, by the column's entry count) */
    int64_t columns_wave;  /* columns of at most 512 entries */
    int64_t columns_block; /* longer columns */
    int64_t group_budget;  /* a group of more than one item costs at most this much (an item costs its entries + its columns) */
    int64_t device_bytes;  /* device memory of the second part of the image: 4 per column, 8 per entry, 16 per item, 4 per group */
} flex_attention_backward_info;
int flex_plan_attention_backward_info(const flex_plan *plan, flex_attention_backward_info *out);

/* Multi-head fused attention: `heads` = H heads in the ONE forward launch and the TWO backward launches of flex_attention and
 * flex_attention_backward, on the same plans (FLEX_PLAN_ATTENTION; FLEX_PLAN_ATTENTION_BACKWARD for the second call; FLEX_ERR_INVALID on
 * any other plan).  No new plan flag and no new image: the schedule depends on k and the pattern only, so one plan serves every H.  No
 * reference counterpart.  k = H d.  Head h owns columns [h d, (h + 1) d) of Q, K, V, Out, g, gQ, gK and gV, and for every head on its
 * own everything is what flex_attention and flex_attention_backward define at width d on those columns, with the one `scale`: the
 * scores, the masked (-inf) and poisoned (+inf / NaN) rules, +0 rows, da, delta, ds, gQ, gK, gV, and "every entry multiplies its V
 * row".  Heads never mix: a poisoned row of head h writes NaN into head h's d columns of Out and head h's entries of dP, nowhere else.
 * dP and dWork hold hostA->nnz x H floats, entry-major: (entry e, head h) at e H + h, e in hostA's CSR order (a torch tensor [nnz, H]
 * is contiguous).  heads == 1, for any k: the call IS flex_attention / flex_attention_backward (forwarded before any other check of
 * this paragraph; bit-identical in every output, the generic instantiation included).  heads > 1: k % H == 0 and d in {4, 8, 16, 32,
 * 64, 128, 256} (a power of two: a head never straddles a slab of 256 columns; H itself need not be one, k = 48 = 3 x 16 is valid),
 * k <= 1024, and only the 16-byte form is built -- ldb % 4 == 0, ldc % 4 == 0 and every row operand 16-byte aligned; anything else
 * is FLEX_ERR_UNSUPPORTED.  heads < 1, a scale that is not finite and > 0, a NULL operand (Q, K, V, Out; in the backward Q, K, V, P,
 * GradOut, Work) and dWork == dP: FLEX_ERR_INVALID.  A plan without entries: FLEX_OK, no launch, nothing written.  Otherwise as the
 * single-head calls: dP may be NULL (Out has the same bits either way); the forward on a row-range shard writes the dP entries of its
 * rows and leaves the others untouched (the backward is not defined on shards); each of dGradQ, dGradK, dGradV may be NULL and an
 * output has the same bits whichever others are asked for; on return dWork holds ds whenever dGradQ or dGradK was asked for.
 * Asynchronous on `stream`, no allocation, no host synchronisation (safe to capture in a hipGraph), no atomics, fixed reduction
 * order: bit-identical run to run.  The walk is the single-head one; a score (and da) is reduced over the d / 4 lanes of its head, and
 * the running maximum and sum, delta and ds are kept per head.
 *
 * Accuracy: per head, flex_attention's and flex_attention_backward's bounds with k replaced by d -- the reduction of a score and of da
 * has depth <= d (a chain of four fmas per lane, then a tree over the d / 4 lanes of the head); the passes, rescales and merges
 * (R_r) and the depths of the sums of l, Out, delta, gQ, gK and gV are the single-head kernels', so c = 3, a = 3, b = 0 stand. */
int flex_attention_heads(const flex_plan *plan, int heads, const float *dQ, const float *dK, const float *dV, float scale, float *dOut,
                         float *dP, flex_stream_t stream);
int flex_attention_heads_backward(const flex_plan *plan, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                  const float *dGradOut, float scale, float *dGradQ, float *dGradK, float *dGradV, float *dWork,
                                  flex_stream_t stream);

/* Multi-head fused attention on bf16 row operands: flex_attention_heads and flex_attention_heads_backward with Q, K, V, Out, g, gQ, gK
 * and gV held as bf16 -- half the bytes of every gathered row -- in the same ONE forward launch and TWO backward launches, on the same
 * plans (FLEX_PLAN_ATTENTION; FLEX_PLAN_ATTENTION_BACKWARD for the second call; FLEX_ERR_INVALID on any other plan).  No new plan flag
 * and no new image.  No reference counterpart.  A flex_bf16 is the upper 16 bits of an IEEE float (torch.bfloat16).  Definition: read
 * every bf16 operand as the fp32 number it is (the conversion is exact); then everything is what flex_attention_heads and
 * flex_attention_heads_backward define, in fp32 -- the scores, the masked (-inf) and poisoned (+inf / NaN) rules per head, +0 rows,
 * "every entry multiplies its V row", da, delta, ds, gQ, gK, gV -- with accumulation and softmax in fp32, and at the single store of
 * each element of Out, gQ, gK and gV the fp32 value is rounded to bf16, round to nearest even: a NaN stays a NaN, +-inf stays +-inf, a
 * finite value beyond the largest finite bf16 becomes +-inf, and a poisoned head still writes NaN into its own d columns only.  dP and
 * dWork are fp32, hostA->nnz x H floats, entry-major, and are NOT rounded: they hold the values flex_attention_heads and
 * flex_attention_heads_backward write for the widened operands, bit for bit, and Out, gQ, gK and gV are the bf16 roundings of theirs.
 * The plan's ldb and ldc are element strides, as before (a row of K is ldb flex_bf16 after the one before it).
 * heads >= 1, and heads == 1 is served here directly: there is no forwarding to a generic form (as for flex_gat_attention), so for
 * every H, H = 1 included: k % H == 0, d = k / H in {4, 8, 16, 32, 64, 128, 256} (k = 48 with H = 1 and k = 300 are refused), k <= 1024,
 * and only the vector form is built -- ldb % 4 == 0, ldc % 4 == 0 and every row operand 8-byte aligned (one 8-byte access of four
 * elements per lane); anything else is FLEX_ERR_UNSUPPORTED.  A plan without the attention image (without the backward image, for the
 * second call), heads < 1, a scale that is not finite and > 0, a NULL operand (Q, K, V, Out; in the backward Q, K, V, P, GradOut, Work)
 * and dWork == dP: FLEX_ERR_INVALID.  A plan without entries: FLEX_OK, no launch, nothing written.  dP may be NULL (Out has the same
 * bits either way); the forward on a row-range shard writes the Out rows and the dP entries of its rows and leaves the others
 * untouched (the backward is not defined on shards: such a plan has no backward image); each of dGradQ, dGradK, dGradV may be NULL, an
 * output has the same bits whichever others are asked for, a launch without outputs is skipped and a call without outputs launches
 * nothing; on return dWork holds ds whenever dGradQ or dGradK was asked for.  Asynchronous on `stream`, no allocation, no host
 * synchronisation (safe to capture in a hipGraph), no atomics, fixed reduction order: bit-identical run to run.
 *
 * Accuracy, against float64 on the bf16 inputs (backward: on the same bf16 Q, K, V, g and fp32 p): dP and dWork carry the bounds of
 * flex_attention_heads and flex_attention_heads_backward unchanged.  An output element y = rn_bf16(x32), whose fp32 value x32 lies
 * within bound32 (the fp32 call's bound for that element) of the float64 value x64, satisfies
 *     |y - x64| <= bound32 + 2^-8 (|x64| + bound32) + 2^-134
 * 2^-8 being the unit roundoff of bf16 (8 significant bits) and 2^-134 half its smallest subnormal. */
int flex_attention_bf16(const flex_plan *plan, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, float scale,
                        flex_bf16 *dOut, float *dP, flex_stream_t stream);
int flex_attention_bf16_backward(const flex_plan *plan, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dP,
                                 const flex_bf16 *dGradOut, float scale, flex_bf16 *dGradQ, flex_bf16 *dGradK, flex_bf16 *dGradV, float *dWork,
                                 flex_stream_t stream);

/* Multi-head fused attention with a per-edge bias: flex_attention_heads / flex_attention_bf16 and their backward calls with one learned
 * term per entry and head added to the score before the softmax -- the edge term of the graph transformers (Graphormer, SAN, GraphGPS,
 * TransformerConv with edge features), which also mask edges per head with -inf -- in the same ONE forward launch and TWO backward
 * launches, on the same plans (FLEX_PLAN_ATTENTION; FLEX_PLAN_ATTENTION_BACKWARD for the backward calls; FLEX_ERR_INVALID on any other
 * plan).  No new plan flag and no new image.  No reference counterpart.  The plans, heads = H, d = k / H, head h on columns
 * [h d, (h + 1) d) and the layout of dP and dWork are those of flex_attention_heads.  dBias is hostA->nnz x H floats, entry-major, in
 * hostA's CSR order: (entry e, head h) at e H + h -- the layout of dP, so a contiguous torch tensor [nnz, H] fits; it is fp32 for both
 * element types and needs the alignment of a float only.  For row r, entry e, head h:
 *     s_eh     = <Q[r, head h], K[src(e), head h]>             (the reduction of flex_attention_heads: a chain of four fmas per lane,
 *                                                               a tree over the d / 4 lanes of the head)
 *     t_eh     = fma(scale, s_eh, bias[e, h])                  (ONE rounding)
 *     alpha_eh = flex_edge_softmax's softmax of t_.h over the row, scale 1     (flex_gat_attention's passes, rescales and merges)
 *     Out[r, head h] = sum_e alpha_eh V[src(e), head h]
 * Special values follow the existing rules through t, with no new rule: bias = -inf masks that entry for that head (its p is exactly
 * +0); a row whose t are all -inf, and a row without entries, write +0; a +inf or NaN t -- s = +inf against bias = -inf included --
 * poisons the row for that head only (NaN in that head's d columns of Out and that head's entries of dP); every entry, masked or not,
 * multiplies its V row.  On a row-range shard dBias is indexed by hostA's entry index, as dP is, and only the entries of the shard's
 * rows are read.  dP may be NULL (Out has the same bits either way).
 * Backward, with p = the dP the forward wrote and g = dGradOut.  It does not take the bias:
 *     da_eh, delta_rh                                          as flex_attention_heads_backward
 *     gBias[e, h] = fl(p_eh fl(da_eh - delta_rh))              new output: hostA->nnz x H floats, entry-major
 *     ds_eh       = fl(fl(scale p_eh) fl(da_eh - delta_rh))    -> dWork, the unchanged expression
 *     gQ, gK, gV                                               as flex_attention_heads_backward from ds and p
 * No special cases: the formulas in fp32 under IEEE.  Each of dGradQ, dGradK, dGradV and dGradBias may be NULL; an output has the same
 * bits whichever others are asked for, and a call without outputs launches nothing.  The rows' launch writes dWork, gQ and gBias and
 * runs when any of gQ, gK, gBias is asked for (dWork then holds ds); the columns' launch is flex_attention_heads_backward's (or
 * flex_attention_bf16_backward's) own kernel and runs when gK or gV is.  dGradBias must alias neither dP nor dWork (FLEX_ERR_INVALID
 * where equal; any other overlap is the caller's error).  The backward is not defined on shards.
 * flex_attention_bf16_bias / flex_attention_bf16_bias_backward: flex_attention_bf16's definition word for word.  Q, K, V, Out, g, gQ,
 * gK and gV are flex_bf16, read as the fp32 numbers they are, with one rounding to nearest even at the single store of each element
 * of Out, gQ, gK and gV; bias, gBias, dP and dWork are fp32, are not rounded, and equal the fp32 call's bits on the widened operands.
 * Checks, for both element types (those of flex_attention_bf16): heads == 1 is served directly -- there is no generic form to forward
 * to -- so for every H: k % H == 0, d in {4, 8, 16, 32, 64, 128, 256} (k = 48 with H = 1 and k = 300 are refused), k <= 1024, and only
 * the vector form is built -- ldb % 4 == 0, ldc % 4 == 0, fp32 rows 16-byte aligned, bf16 rows 8-byte aligned; anything else is
 * FLEX_ERR_UNSUPPORTED.  The wrong kind of plan, heads < 1, a scale that is not finite and > 0, a NULL operand (Q, K, V, Bias, Out; in
 * the backward Q, K, V, P, GradOut, Work), dWork == dP, dGradBias == dP and dGradBias == dWork: FLEX_ERR_INVALID.  A plan without
 * entries: FLEX_OK, no launch, nothing written.  Asynchronous on `stream`, no allocation, no host synchronisation (safe to capture in
 * a hipGraph), no atomics, fixed reduction order: bit-identical run to run.
 *
 * Accuracy, with the u, gamma, E, R_r and n_r of flex_attention; forward against float64 on the fp32 inputs (the fp32 value of scale,
 * the fp32 bias), backward against float64 on the SAME fp32 Q, K, V, p and g.
 *   score   dt_e     = scale (gamma(d) sum_j |Q K| + d 2^-149) + u |t_e| + 2^-149
 *   alpha   dalpha_e = alpha_e [gamma(n_r + 4 D_r + (E + 3) R_r + 2 E + 4) + expm1(2 max_row dt)] + 2^-126,
 *                      D_r = min(104, the spread of the row's finite t)
 *   Out     |Out - Out64| <= sum_e (gamma(n_r + 3) alpha_e + dalpha_e) |V| + 2^-126
 *   gBias   |gB - gB64| <= gamma(n_r + 3) p_e (|da_e| + sum_j |p_j da_j|) + p_e (dda_e + sum_j p_j dda_j) + n_r 2^-149
 *   dWork, gQ, gK, gV   flex_attention_heads_backward's bounds, unchanged (as there, for p that are zero or normal numbers: the
 *                       n_r 2^-149 they grant products below 2^-126 does not cover fl(scale p) of a SUBNORMAL p -- off by up to
 *                       2^-150 -- times a da - delta beyond n_r; a bias spread of more than about 87 - ln n_r produces such p)
 *   bf16 outputs        |y - x64| <= bound32 + 2^-8 (|x64| + bound32) + 2^-134                    (flex_attention_bf16's)
 * dP is held to dalpha on its own.  Derivation.  s is flex_attention_heads's reduction of depth <= d: |s - s64| <= gamma(d) sum |Q K| +
 * d 2^-149.  t = fl(scale s + bias) is one fma: the error of s enters multiplied by scale (the product is not rounded), the one rounding
 * of the sum is u |t|, or 2^-149 where t is subnormal.  From t on, alpha and Out are flex_attention's derivation with scale = 1, run by
 * the same code as flex_gat_attention runs it: moving every t of a row by at most max_row dt moves the softmax by the factor
 * exp(2 max_row dt); a term expf(fl(t - m)) carries gamma(2 D_r + E + 1) with D_r the spread of t itself (the product by scale = 1 is
 * exact); R_r, c = 3 and the depths of the sums are the same passes, rescales and merges.  The rounding of the float64 score to the fp32
 * one the softmax starts from, |s| u in flex_attention's line, is the u |t| already inside dt.  gBias = fl(p fl(da - delta)) is one
 * subtraction and one product on flex_attention_heads_backward's da and delta: flex_gat_attention's ddz, which is that call's dds with
 * scale = 1 (a = 3 covers a second product that is not made here).  ds, gQ, gK and gV are computed by the unchanged expressions from p
 * and g, which is all they see of the forward. */
int flex_attention_bias(const flex_plan *plan, int heads, const float *dQ, const float *dK, const float *dV, const float *dBias, float scale,
                        float *dOut, float *dP, flex_stream_t stream);
int flex_attention_bias_backward(const flex_plan *plan, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                 const float *dGradOut, float scale, float *dGradQ, float *dGradK, float *dGradV, float *dGradBias,
                                 float *dWork, flex_stream_t stream);
int flex_attention_bf16_bias(const flex_plan *plan, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV, const float *dBias,
                             float scale, flex_bf16 *dOut, float *dP, flex_stream_t stream);
int flex_attention_bf16_bias_backward(const flex_plan *plan, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV,
                                      const float *dP, const flex_bf16 *dGradOut, float scale, flex_bf16 *dGradQ, flex_bf16 *dGradK,
                                      flex_bf16 *dGradV, float *dGradBias, float *dWork, flex_stream_t stream);

/* Attention dropout in the multi-head fused attention: flex_attention_heads / flex_attention_bf16 / flex_attention_bias /
 * flex_attention_bf16_bias and their backward calls with the probabilities dropped after the softmax, as graph transformers and GAT
 * train (GAT's default p is 0.6), still in ONE forward launch and TWO backward launches on the same plans: the mask is a counter-based
 * hash of the entry's index, recomputed in all three launches -- no mask array, no extra pass, no new plan image.  No reference
 * counterpart.  dBias == NULL: no bias (flex_attention_heads's score); otherwise flex_attention_bias's.  Head h, its columns, scale and
 * the layout of dBias, dP, dGradBias and dWork are those calls'.  With c = 1.0f / (1.0f - drop_p), computed in fp32 on the host, the
 * factor of entry e and head h is
 *     w_eh = keep(seed, e H + h) ? c : 0
 * Forward.   Out[r, head h] = sum_e alpha_eh w_eh V[src(e), head h].  The score, the bias, the maximum, the sum l, the mask (-inf) and
 *   poison (+inf / NaN) rules and the dP written are those of the undropped call, bit for bit: dP holds the UNDROPPED alpha.  Dropout
 *   acts after the normalisation; it removes no entry from the softmax.
 * Dropped entries are SELECTED OUT, not multiplied by zero: a non-finite V row at a dropped entry does not reach Out; in the backward
 *   da of a dropped entry is exactly +0 and the entry adds nothing to gV.
 * Zero rows. A head of a row whose live entries are all dropped is +0 in every column of that head; a poisoned head stays NaN.
 * Backward, from the kept undropped p = dP:
 *     da_eh   = w_eh <g[r, head h], V[src(e), head h]>
 *     delta   = sum_e p da             ds = scale p (da - delta), written to dWork            gBias = p (da - delta)
 *     gQ[r]  += ds K[src(e)]           gK[src(e)] += ds Q[r]                                  gV[src(e)] += (p_eh w_eh) g[r]
 *   The columns' launch needs the mask for gV only.  dGradBias == NULL: no gradient in the bias (and the kernels without it).
 * The mask is part of the contract and is bit-defined.  On wrapping uint32 arithmetic
 *     mix(x):  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 * and with i = e H + h as uint64, e being the entry's index in the CSR the plan was made from (a row-range shard uses the same global
 * index, as the bias does),
 *     r = mix( mix(lo32(i) + lo32(seed) + 0x9E3779B9) ^ (hi32(i) + hi32(seed)) )
 * and the entry is kept iff r < thr, thr = min(floor((1 - (double)drop_p) 2^32), 2^32 - 1).  r(seed 0, i 0) = 0xae6f80f1; with seed
 * 0x0123456789abcdef: r(0) = 0x477cb3f3, r(1) = 0x7a8a410e, r(2^32 + 5) = 0xeb2c8d08, r(2^40 + 123) = 0x5cbb10ba.
 * flex_dropout_mask (host code, in every build): keep_host[j] = 1 if index first + j is kept, else 0, for j < count -- the mask's
 * reference for users and tests.
 * Checks: those of flex_attention_bf16 / flex_attention_bias and their backward calls, in their order, for both element types (heads
 * == 1 is served by the per-head kernels: k / heads a power of two in 4 .. 256 for every heads); drop_p must be finite with 0 <=
 * drop_p < 1, anything else is FLEX_ERR_INVALID, checked beside scale.  drop_p == 0: once nothing is refused the call launches what
 * the undropped entry point launches (flex_attention_heads, flex_attention_bf16 or the bias form), so every output has its bits.  Nothing is
 * enqueued by a refused call.  Safe to capture in a hipGraph, no atomics, fixed order: bit-identical run to run for one seed.
 * Accuracy: the undropped calls' bounds with every rounding count that now includes the product by c grown by one: Out gamma(n_r + 4) in
 * place of gamma(n_r + 3), on |V| of the kept entries times c; da gamma(d + 1); gV one more rounding per term; dP unchanged. */
int flex_attention_dropout(const flex_plan *plan, int heads, const float *dQ, const float *dK, const float *dV, const float *dBias /* NULL: no bias */,
                           float scale, float drop_p, uint64_t seed, float *dOut, float *dP, flex_stream_t stream);
int flex_attention_dropout_backward(const flex_plan *plan, int heads, const float *dQ, const float *dK, const float *dV, const float *dP,
                                    const float *dGradOut, float scale, float drop_p, uint64_t seed, float *dGradQ, float *dGradK, float *dGradV,
                                    float *dGradBias /* NULL */, float *dWork, flex_stream_t stream);
int flex_attention_bf16_dropout(const flex_plan *plan, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV,
                                const float *dBias /* NULL: no bias */, float scale, float drop_p, uint64_t seed, flex_bf16 *dOut, float *dP,
                                flex_stream_t stream);
int flex_attention_bf16_dropout_backward(const flex_plan *plan, int heads, const flex_bf16 *dQ, const flex_bf16 *dK, const flex_bf16 *dV,
                                         const float *dP, const flex_bf16 *dGradOut, float scale, float drop_p, uint64_t seed, flex_bf16 *dGradQ,
                                         flex_bf16 *dGradK, flex_bf16 *dGradV, float *dGradBias /* NULL */, float *dWork, flex_stream_t stream);
int flex_dropout_mask(uint64_t seed, float drop_p, uint64_t first, uint64_t count, uint8_t *keep_host);

/* Fused GAT attention: the additive score of graph attention networks in place of the dot product, H heads in the ONE forward launch and
 * the TWO backward launches of flex_attention_heads and flex_attention_heads_backward, on the same plans (FLEX_PLAN_ATTENTION;
 * FLEX_PLAN_ATTENTION_BACKWARD for the second call; FLEX_ERR_INVALID on any other plan).  No new plan flag and no new image: the
 * schedule depends on k and the pattern only, so one plan serves dot-product and GAT attention alike, for every H.  No reference
 * counterpart.  k = H d.  Head h owns columns [h d, (h + 1) d) of V, Out, g and gV.  dEl is [rows of the plan, H] floats, contiguous,
 * with Q's row convention (a shard's row r0 + i is row i); dEr is [hostA->n, H] floats, contiguous; both hold one scalar per node and
 * head (in a GAT layer el = <h_r W, a_l>, er = <h_c W, a_r>).  dP and dWork hold hostA->nnz x H floats, entry-major, exactly as for
 * flex_attention_heads.  For row r, entry e in hostA's CSR order, src(e) = hostA->col[e], head h:
 *     x_eh     = el[r, h] + er[src(e), h]
 *     s_eh     = x_eh > 0 ? x_eh : slope x_eh                   (torch.nn.functional.leaky_relu: 0 takes the slope branch)
 *     alpha_eh = flex_edge_softmax's softmax of s_.h over the row, scale 1
 *     Out[r, head h] = sum_e alpha_eh V[src(e), head h]
 * Backward, with p = the dP the forward wrote and g = dGradOut (Out's shape and stride ldc):
 *     da_eh    = <g[r, head h], V[src(e), head h]>              (over the head's d columns)
 *     delta_rh = sum_j p_jh da_jh                               (over the row's entries)
 *     dz_eh    = p_eh (da_eh - delta_rh)
 *     dx_eh    = x_eh > 0 ? dz_eh : slope dz_eh                 (x recomputed from el and er; nothing else is kept)
 *     gEl[r, h]      = sum_{e in row r}      dx_eh
 *     gEr[c, h]      = sum_{e: src(e) == c}  dx_eh
 *     gV[c, head h]  = sum_{e: src(e) == c}  p_eh g[row(e), head h]
 * gEl has dEl's shape, gEr has dEr's, gV has V's (stride ldb).  Special values follow the existing calls through the formulas, with no
 * new rule.  slope must be finite with 0 < slope <= 1 (else FLEX_ERR_INVALID); with slope > 0 a -inf sum stays -inf, so er[c, h] = -inf
 * masks source node c for head h and el[r, h] = -inf masks row r for head h: such entries have p exactly +0, and a fully masked row
 * and a row without entries write +0.  A NaN or +inf score (+inf + -inf included) poisons its row for that head only: NaN in that
 * head's d columns of Out and that head's entries of dP.  Every entry, masked or not, multiplies its V row.  The backward is the
 * formulas in fp32 under IEEE; a NaN x takes the slope branch, the comparison being false.  Rows of gEl without entries, and rows of
 * gEr / gV whose column has no entry, are written as +0.
 * Checks: heads < 1, a bad slope, a NULL operand (El, Er, V, Out; in the backward El, Er, V, P, GradOut, Work) and dWork == dP:
 * FLEX_ERR_INVALID.  k % heads != 0; d outside {4, 8, 16, 32, 64, 128, 256}, for every H, H = 1 included (there is no single-head
 * form to forward to: k = 300 is refused here); k > 1024; ldb % 4, ldc % 4 or a row operand (V, Out, g, gV) that is not 16-byte
 * aligned (only the 16-byte form is built, as for flex_attention_heads; el, er, gEl and gEr need the alignment of a float only):
 * FLEX_ERR_UNSUPPORTED.  A plan without entries: FLEX_OK, no launch, nothing written.  dP may be NULL (Out has the same bits either
 * way); the forward on a row-range shard writes the dP entries of its rows and leaves the others untouched (the backward is not
 * defined on shards, as for flex_attention_heads_backward); each of dGradEl, dGradEr, dGradV may be NULL, an output has the same bits
 * whichever others are asked for, and a launch without outputs is skipped (the rows' launch writes gEl, the columns' gEr and gV); on
 * return dWork holds dx whenever dGradEl or dGradEr was asked for.  Asynchronous on `stream`, no allocation, no host synchronisation
 * (safe to capture in a hipGraph), no atomics, fixed reduction order: bit-identical run to run.  The walk is flex_attention_heads's;
 * a score needs no K row and no reduction across lanes (per entry one V row and H floats of er are gathered), the second sweep of the
 * rows' backward launch gathers nothing, and the columns' launch gathers g alone.
 *
 * Accuracy, with the u, gamma, E, D_r and R_r of flex_attention; forward against float64 on the fp32 inputs, backward against float64 on
 * the SAME fp32 el, er, V, p and g.  The float64 reference takes the branch of the leaky ReLU from the sign of the fp32 sum
 * fl(el + er), which is what the kernel sees (the sum of two floats is zero only where it is exactly zero, so the signs agree wherever
 * the float64 sum is finite), and uses the fp32 value of slope.
 *   score   ds_e     = gamma(2) |s_e| + 2^-149                  (in place of gamma(k) sum |Q K| + k 2^-149)
 *   alpha   dalpha_e = alpha_e [gamma(n_r + 4 D_r + (E + 3) R_r + 2 E + 4) + expm1(2 max_row(ds + |s| u))] + 2^-126
 *   Out     |Out - Out64| <= sum_e (gamma(n_r + 3) alpha_e + dalpha_e) |V| + 2^-126
 *   dda_e    = gamma(d) sum_j |g V| + d 2^-149                  (over the head's d columns)
 *   ddz_e    = gamma(n_r + 3) p_e (|da_e| + sum_j |p_j da_j|) + p_e (dda_e + sum_j p_j dda_j) + n_r 2^-149
 *   ddx_e    = f_e ddz_e + u |dx_e| + 2^-149,   f_e = 1 where x_e > 0, else slope
 *   |gEl - gEl64| <= sum_{e in r} (gamma(n_r) |dx_e| + ddx_e) + 2^-126
 *   |gEr - gEr64| <= sum_{e in c} (gamma(n_c) |dx_e| + ddx_e) + 2^-126
 *   |gV  - gV64|  <= sum_{e in c}  gamma(n_c) p_e |g[row]|    + 2^-126
 * dP is held to dalpha and dWork to ddx on their own.  Derivation.  x = fl(el + er) is one rounded sum and s = fl(slope x) at most one
 * more product, which may round as a subnormal: gamma(2) |s| + 2^-149.  From the scores on, alpha and Out are flex_attention's derivation
 * with scale = 1: the passes, rescales and merges are the same code, so R_r and c = 3 stand.  da is flex_attention_heads_backward's
 * reduction over the d columns of the head (a chain of four fmas per lane, a tree over the d / 4 lanes).  delta is summed by fma in a tree
 * of depth <= n_r and dz = fl(p fl(da - delta)) is one subtraction and one product, inside flex_attention_backward's a = 3 (which counted a
 * second product, scale p): ddz is its dds with scale = 1.  dx = dz exactly or fl(slope dz), one rounding that may be subnormal: ddx.
 * gEl adds the computed dx plainly: a chain on each owning lane, a butterfly over the lanes of the head, then the merges over slots and
 * waves; additions of the zeros that the other lanes hold are exact, so the n_r terms meet in a tree of depth < n_r: gamma(n_r) |dx|.
 * gEr adds dx in a chain per slot and the same merges, depth <= n_c.  gV is flex_attention_backward's with b = 0, and its ratio comes
 * close to 1 on columns of one entry for the reason given there.  First order, as the bounds above. */
int flex_gat_attention(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const float *dV, float slope, float *dOut,
                       float *dP, flex_stream_t stream);
int flex_gat_attention_backward(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const float *dV, const float *dP,
                                const float *dGradOut, float slope, float *dGradEl, float *dGradEr, float *dGradV, float *dWork,
                                flex_stream_t stream);

/* Attention dropout in the fused GAT attention: flex_gat_attention and flex_gat_attention_backward with the probabilities dropped after
 * the softmax, as GAT trains (the paper's p is 0.6), still in ONE forward launch and TWO backward launches on the same plans.  The mask,
 * its threshold and its index are flex_attention_dropout's, bit for bit (flex_dropout_mask is its host reference): with
 * c = 1.0f / (1.0f - drop_p), computed in fp32 on the host, the factor of entry e and head h is
 *     w_eh = keep(seed, e H + h) ? c : 0
 * Entry index. e is the entry's index in the CSR the plan was made from; a row-range shard uses that global index.
 * Forward.   Out[r, head h] = sum_e alpha_eh w_eh V[src(e), head h].  The score x = el + er, the LeakyReLU, the maximum, the sum, the
 *   mask (-inf) and poison (+inf / NaN) rules and the dP written are flex_gat_attention's, bit for bit: dP holds the UNDROPPED alpha.
 * Dropped entries are SELECTED OUT, not multiplied by zero: the V row of a dropped entry is not gathered, so an inf or NaN V row behind
 *   a dropped entry reaches nothing.  A head of a row whose live entries are all dropped is +0 in every column of that head; a poisoned
 *   head stays NaN.
 * Backward, from the kept undropped p = dP:
 *     da_eh   = w_eh <g[r, head h], V[src(e), head h]>          (a dropped entry: exactly +0, its V row is not gathered)
 *     delta, dz = p (da - delta), dx by the sign of the recomputed x, gEl, gEr and dWork = dx exactly as in flex_gat_attention_backward
 *     gV[c, head h] += (p_eh w_eh) g[row(e), head h]            (a dropped entry: its g row is not gathered)
 *   dx holds the mask through da, so gEl and gEr do not see it a second time; the columns' launch needs the mask for gV only.
 * Checks: drop_p must be finite with 0 <= drop_p < 1, anything else is FLEX_ERR_INVALID, checked beside slope; every other refusal is
 * flex_gat_attention's and flex_gat_attention_backward's, code for code and in their order.  drop_p == 0: once nothing is refused the
 * call launches the undropped kernels, so every output has flex_gat_attention's bits.  The forward runs on row-range shards, the backward does
 * not.  Nothing is enqueued by a refused call.  Safe to capture in a hipGraph, no atomics, fixed order: bit-identical run to run for
 * one seed.
 * Accuracy: flex_gat_attention's bounds with every rounding count that now includes the product by c grown by one:
 *   Out     |Out - Out64| <= sum_{e kept} (gamma(n_r + 4) alpha_e + dalpha_e) c |V| + 2^-126
 *   dda_e    = c (gamma(d + 1) sum_j |g V| + d 2^-149) + 2^-149 on a kept entry, 0 on a dropped one
 *   ddz, ddx, gEl, gEr: flex_gat_attention_backward's lines on this da and dda
 *   |gV  - gV64|  <= sum_{e in c, kept} gamma(n_c + 1) p_e c |g[row]| + 2^-126 */
int flex_gat_attention_dropout(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const float *dV, float slope, float drop_p,
                               uint64_t seed, float *dOut, float *dP, flex_stream_t stream);
int flex_gat_attention_dropout_backward(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const float *dV, const float *dP,
                                        const float *dGradOut, float slope, float drop_p, uint64_t seed, float *dGradEl, float *dGradEr,
                                        float *dGradV, float *dWork, flex_stream_t stream);

/* A per-edge term in the score of the fused GAT attention (edge features): the score of the edge-feature GAT of the common libraries,
 * alpha = alpha_dst[i] + alpha_src[j] + alpha_edge[e] inside the LeakyReLU, with alpha_edge = <lin_edge(edge_attr), att_edge> computed
 * by the caller.  One pair of calls serves both modes: drop_p == 0 launches kernels without the mask, anything else the dropout of
 * flex_gat_attention_dropout.  Still ONE forward launch and TWO backward launches on the same plans; no plan flag, no new image.
 * Everything is flex_gat_attention's and flex_gat_attention_dropout's except one line:
 *     x_eh = fl(fl(el[r, h] + er[src(e), h]) + ee[e, h])      (fp32, in this order)
 * - ee is [nnz, H] fp32, entry-major, in the CSR order the plan was made from.
 * - s, alpha, Out, da, delta, dz, dx_eh = x_eh > 0 ? dz_eh : slope dz_eh, gEl, gEr, gV and the dropout mask of (seed, e H + h) are
 *   unchanged.
 * - gEe[e, h] = dx_eh.
 * - ee[e, h] = -inf masks that entry for that head: p is exactly +0, and the row is +0 if all its entries are masked.
 * - A NaN or +inf score poisons that head of that row only.  -inf + +inf counts as such a score.
 * - On a row-range shard ee is indexed by the whole matrix's entry index, as dBias and dP are.  Only the shard's entries are read.
 * - fp32 V only; d in {4, ..., 256}, a power of two, H = 1 included; k <= 1024; only the 16-byte form; 0 < slope <= 1.
 * Backward.  The work array is dGradEe when it is given, else dWork: exactly one is needed, and if both are given dGradEe is used and
 * dWork is untouched.  On return the work array holds dx: that IS gEe, not a copy of it (d x / d ee = 1 inside the pre-activation, so
 * the gradient needs no sum of its own).  The rows' launch runs iff dGradEl, dGradEr or dGradEe is given, the columns' launch iff
 * dGradEr or dGradV is given; the columns' launch is flex_gat_attention_backward's (flex_gat_attention_dropout_backward's with a mask),
 * which reads P, dx and g alone.  Every output has the same bits whichever others are asked for.  With ee = +0 everywhere and no
 * operand -0, every output has the bits of flex_gat_attention / flex_gat_attention_dropout and their backward calls.
 * Checks: the refusals of flex_gat_attention_dropout and flex_gat_attention_dropout_backward, code for code and in their order; dEe joins
 * the required operands (NULL: FLEX_ERR_INVALID); drop_p is checked beside the slope; both work pointers NULL, or the work array equal
 * to dP: FLEX_ERR_INVALID.  The forward runs on row-range shards, the backward returns FLEX_ERR_INVALID there.  Nothing is enqueued by
 * a refused call.  Safe to capture in a hipGraph, no atomics, fixed order: bit-identical run to run for one seed.
 * Accuracy: flex_gat_attention's lines (with dropout, flex_gat_attention_dropout's) on another ds; the float64 reference uses the exact
 * x = el + er + ee on the fp32 inputs and takes the LeakyReLU branch from the sign of the fp32 x formed in the order above.  Two rounded
 * additions, where the first sum may cancel against ee, give
 *     |x^ - x| <= u (1 + u) |el + er| + u |x|
 * so with f_e = 1 or slope:
 *     ds_e = gamma(2) f_e |el + er| + gamma(3) |s_e| + 2^-149
 * in place of gamma(2) |s_e| + 2^-149.  Derivation: a = fl(el + er) = (el + er)(1 + d1) and x^ = fl(a + ee) = (x + (el + er) d1)(1 + d2)
 * with |d1|, |d2| <= u, which is the first line; s^ = x^ or fl(slope x^), one more rounding that may be subnormal, so
 * |s^ - s| <= f u (1 + u)^2 |el + er| + (u (1 + u) + u) |s| + 2^-149, inside the second line.  Where x^ and x differ in sign, |x| is
 * below u (1 + u) |el + er| and either branch of the reference is within the same line.  alpha, Out, dda, ddz, ddx, gEl, gEr and gV
 * keep their formulas with this ds; gEe is held to ddx. */
int flex_edge_gat_attention(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const float *dEe, const float *dV, float slope,
                            float drop_p, uint64_t seed, float *dOut, float *dP /* optional */, flex_stream_t stream);
int flex_edge_gat_attention_backward(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const float *dEe, const float *dV,
                                     const float *dP, const float *dGradOut, float slope, float drop_p, uint64_t seed, float *dGradEl,
                                     float *dGradEr, float *dGradEe, float *dGradV, float *dWork, flex_stream_t stream);

/* The fused GAT attention on bf16 V rows, with and without dropout: flex_gat_attention, flex_gat_attention_backward,
 * flex_gat_attention_dropout and flex_gat_attention_dropout_backward, argument for argument, with V, Out, g and gV held as flex_bf16 --
 * half the bytes of the one row a nonzero gathers (the V row in the forward and in the rows' backward launch, the g row in the columns')
 * -- in the same ONE forward launch and TWO backward launches, on the same plans: no new plan flag and no new image.  No reference
 * counterpart.
 *   dV, dOut, dGradOut, dGradV          flex_bf16 rows (the upper 16 bits of an IEEE float, torch.bfloat16); ldb and ldc are element strides
 *   dEl, dEr, dGradEl, dGradEr          fp32 [rows, H] / [n, H] as before: one scalar per node and head has nothing to save, and a score
 *                                       rounded to 8 bits would not be GAT's softmax
 *   dP, dWork                           fp32 [nnz, H], entry-major, unrounded
 * Definition: read every bf16 operand as the fp32 number it is (the conversion is exact); then everything is what the four fp32 GAT
 * calls define -- x, the LeakyReLU, the mask (-inf) and poison (+inf / NaN) rules per head, +0 rows, "every entry (with dropout: every
 * kept entry) multiplies its V row", da, delta, dx, gEl, gEr, gV, the mask bit of (seed, e H + h), dP keeping the UNDROPPED alpha --
 * with every product and sum in fp32 in the fp32 kernels' order.  Only at the single store of each element of Out and gV the fp32 value
 * is rounded to bf16, to nearest even: a NaN stays a NaN, +-inf stays +-inf, a finite value beyond the largest finite bf16 becomes
 * +-inf, and a poisoned head still writes NaN into its own d columns only.  dP, dWork, gEl and gEr are what the fp32 calls write for
 * the widened operands, bit for bit, and Out and gV are the bf16 roundings of theirs.
 * Checks: the fp32 GAT calls' table, refusal for refusal and in the same order (heads < 1, a bad slope, in the dropout pair a drop_p
 * outside [0, 1), a NULL operand, dWork == dP: FLEX_ERR_INVALID; k % heads, d outside {4, ..., 256}, k > 1024: FLEX_ERR_UNSUPPORTED), with
 * one alignment rule over V, Out / g, gV: k % 4 == 0, ldb % 4 == 0, ldc % 4 == 0 in elements and every bf16 row operand 8-byte aligned
 * (a NULL output counts as aligned); anything else is FLEX_ERR_UNSUPPORTED.  drop_p == 0: once nothing is refused the call runs the
 * undropped bf16 launch, so every output has flex_gat_attention_bf16's bits.  A plan without entries: FLEX_OK, nothing written.  The
 * forward runs on row-range shards (the mask at the whole matrix's entry indices), the backward does not.  Nothing is enqueued by a
 * refused call.  Asynchronous on `stream`, no allocation, no host synchronisation (safe to capture in a hipGraph), no atomics, fixed
 * order: bit-identical run to run.
 * Accuracy, against float64 on the bf16 V and g (and the fp32 el, er and p): dP, dWork, gEl and gEr carry the bounds of the fp32 GAT
 * calls (with dropout: of flex_gat_attention_dropout) unchanged.  An element y = rn_bf16(x32) of Out or gV, whose fp32 value x32 lies
 * within those calls' bound32 of the float64 x64, satisfies
 *     |y - x64| <= bound32 + 2^-8 (|x64| + bound32) + 2^-134
 * 2^-8 being the unit roundoff of bf16 and 2^-134 half its smallest subnormal (flex_attention_bf16's bound). */
int flex_gat_attention_bf16(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, float slope,
                            flex_bf16 *dOut, float *dP, flex_stream_t stream);
int flex_gat_attention_bf16_backward(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV,
                                     const float *dP, const flex_bf16 *dGradOut, float slope, float *dGradEl, float *dGradEr,
                                     flex_bf16 *dGradV, float *dWork, flex_stream_t stream);
int flex_gat_attention_bf16_dropout(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV, float slope,
                                    float drop_p, uint64_t seed, flex_bf16 *dOut, float *dP, flex_stream_t stream);
int flex_gat_attention_bf16_dropout_backward(const flex_plan *plan, int heads, const float *dEl, const float *dEr, const flex_bf16 *dV,
                                             const float *dP, const flex_bf16 *dGradOut, float slope, float drop_p, uint64_t seed,
                                             float *dGradEl, float *dGradEr, flex_bf16 *dGradV, float *dWork, flex_stream_t stream);

/* The fused GATv2 attention (Brody, Alon, Yahav: "How attentive are graph attention networks?"; PyG's and DGL's GATv2Conv): the score
 * a_h . LeakyReLU(W_t h_r + W_s h_c) cannot be written as el[r] + er[c], so it is formed from the full rows, in one forward launch and
 * up to three backward launches on the plans of flex_attention_heads (FLEX_PLAN_ATTENTION, for the backward FLEX_PLAN_ATTENTION_BACKWARD
 * as well; no flag of its own).  dXt is [rows of the plan, k] with Q's row convention and stride ldc, dXs is [hostA->n, k] with stride
 * ldb.  Definition:
 * - k = H d.
 * - Head h owns columns [h d, (h + 1) d) of Xt, Xs, Out, g, gXt, gXs.
 * - att is [H, d], which is k floats.  The coefficient of column c is att[c].
 * - dP and dWork are [nnz, H], entry-major.
 * For entry e of row r with source c = src(e), head h, column j of the head:
 *     x_ej    = Xt[r, hd + j] + Xs[c, hd + j]
 *     s_eh    = sum_j att[hd + j] * (x_ej > 0 ? x_ej : slope * x_ej)        (0 and NaN take the slope branch, as torch's leaky_relu)
 *     alpha_.h = flex_edge_softmax's softmax over the row, scale 1
 *     Out[r, head h] = sum_e alpha_eh Xs[c, head h]                           (the source row is score operand AND value, as in the paper, PyG and DGL)
 *
 *     da_eh   = <g[r, head h], Xs[c, head h]>     delta_rh = sum_e p_eh da_eh     dz_eh = p_eh (da_eh - delta_rh)
 *     f_ej    = x_ej > 0 ? 1 : slope
 *     gXt[r, hd + j] = sum_{e in r}       dz_eh att[hd + j] f_ej
 *     gXs[c, hd + j] = sum_{src(e) = c}  (dz_eh att[hd + j] f_ej  +  p_eh g[row(e), hd + j])
 *     gAtt[hd + j]   = sum_{all e}        dz_eh leaky(x_ej)
 * Scope: fp32 only; d in {4, ..., 256}, a power of two, for every H, H = 1 included; k <= 1024; only the 16-byte form (k, ldb and ldc
 * multiples of 4, every row operand -- Xt, Xs, att, Out, g, gXt, gXs, dAttWork -- 16-byte aligned); 0 < slope <= 1 and finite.  dXt may
 * be the same buffer as dXs (share_weights; the plan is then square with ldb == ldc): every output has the bits of the call on two copies.
 * Non-finite values: the forward keeps the softmax rules (s = -inf gives p = +0; a NaN or +inf score poisons that head of that row
 * only: NaN in its d columns of Out and its entries of dP); there is no masking operand; the backward on non-finite operands is what
 * the formulas give under IEEE.  Rows of gXt without entries and rows of gXs whose column has no entry are written as +0.
 * Launches.  Forward: one.  Backward: the row launch runs whenever a gradient is wanted (each needs dz): it writes dz over da in
 * dWork, gXt where wanted and, where gAtt is wanted, one k-row of partial sums per workgroup into dAttWork; the column launch runs for
 * gXs alone; a small reduction launch, which sums the rows of dAttWork in an order that depends on the plan alone, runs for gAtt alone.
 * Each of dGradXt, dGradXs, dGradAtt may be NULL; with none wanted the call returns FLEX_OK and launches nothing; an output has the
 * same bits whichever others are asked for.  dAttWork must hold the floats that flex_gatv2_attention_work_size reports (k floats per
 * workgroup of the row launch: a figure of the plan's walk, not of nnz x k); it is required only where dGradAtt is wanted.
 * Checks, in this order: plan, flag, heads < 1, slope: FLEX_ERR_INVALID.  k % heads, d, k > 1024: FLEX_ERR_UNSUPPORTED.  A plan without
 * entries: FLEX_OK, nothing written.  A NULL operand (Xt, Xs, att, Out; in the backward Xt, Xs, att, P, GradOut, Work, and AttWork where
 * GradAtt is wanted) and dWork == dP: FLEX_ERR_INVALID.  Alignment: FLEX_ERR_UNSUPPORTED.  No output wanted: FLEX_OK.  The forward
 * runs on row-range shards and writes the dP entries of its rows only; the backward is FLEX_ERR_INVALID there.  Asynchronous on
 * `stream`, no allocation, no host synchronisation (safe to capture in a hipGraph), no atomics, fixed order: bit-identical run to run.
 *
 * Accuracy, with the u, gamma, E, D_r, R_r of flex_attention, n_r / n_c the entries of the row / column, L_ej = leaky(x_ej),
 * w_ej = att_j f_ej; forward against float64 on the fp32 inputs, backward against float64 on the SAME fp32 Xt, Xs, att, p and g.  The
 * float64 reference takes the branch of the leaky ReLU from the sign of the fp32 sum fl(Xt + Xs) and uses the fp32 value of slope.
 *   score   ds_e     = gamma(d + 2) sum_j |att_j| |L_ej| + (d + sum_j |att_j|) 2^-149
 *   alpha   dalpha_e = alpha_e [gamma(n_r + 4 D_r + (E + 3) R_r + 2 E + 4) + expm1(2 max_row(ds + |s| u))] + 2^-126
 *   Out     |Out - Out64| <= sum_e (gamma(n_r + 3) alpha_e + dalpha_e) |Xs| + 2^-126
 *   dda_e    = gamma(d) sum_j |g Xs| + d 2^-149
 *   ddz_e    = gamma(n_r + 3) p_e (|da_e| + sum_j |p_j da_j|) + p_e (dda_e + sum_j p_j dda_j) + n_r 2^-149        (dWork is held to it)
 *   |gXt - gXt64|   <= sum_{e in r} [(gamma(n_r + 1) |dz_e| + ddz_e) |w_ej| + |dz_e| 2^-149] + 2^-126
 *   |gXs - gXs64|   <= sum_{e in c} [(gamma(2 n_c + 1) |dz_e| + ddz_e) |w_ej| + gamma(2 n_c) p_e |g[row]| + |dz_e| 2^-149] + 2^-126
 *   |gAtt - gAtt64| <= sum_{all e}  [(gamma(T + 3) |dz_e| + ddz_e) |L_ej| + |dz_e| 2^-149] + 2^-126
 *   T = min(nnz, 2048 + ceil(max_r n_r / 4) + ceil(m / 4) + 24)
 * Derivation.  x = fl(xt + xs) is one rounding, L = x or fl(slope x) at most one more, which may be subnormal (2^-149, times |att_j|
 * in the score); the score is a chain of four fmas per lane and a tree over the d / 4 lanes of the head, d roundings at most, each
 * possibly subnormal: ds, which takes the place of flex_gat_attention's gamma(2) |s|.  From the scores on, alpha, Out, da, delta and dz are
 * flex_gat_attention's code and bounds.  w = att or fl(att slope): one rounding.  gXt adds dz w by one fma per entry and the merges of
 * the slots and waves, a tree of depth <= n_r; gXs adds two fmas per entry into one row, depth <= 2 n_c.  gAtt adds dz L by one fma per
 * entry on a lane across the rows of its wave's group (at most the group budget, 2048 entries, or a quarter of a block row), then the
 * slots (<= 4 steps), the waves (3), the chain of every fourth partial row (one row per workgroup, at most ceil(m / 4) + 2 of them to
 * a chain) and the four chains (3): T, and never more than nnz, additions of zeros being exact.  First order, as the bounds above. */
int flex_gatv2_attention(const flex_plan *plan, int heads, const float *dXt, const float *dXs, const float *dAtt, float slope, float *dOut,
                         float *dP /* optional */, flex_stream_t stream);
int flex_gatv2_attention_backward(const flex_plan *plan, int heads, const float *dXt, const float *dXs, const float *dAtt, const float *dP,
                                  const float *dGradOut, float slope, float *dGradXt, float *dGradXs, float *dGradAtt, float *dWork,
                                  float *dAttWork, flex_stream_t stream);
int flex_gatv2_attention_work_size(const flex_plan *plan, uint64_t *floats); /* the size of dAttWork */

/* The fused GATv2 attention with dropout of the probabilities after the softmax (the `dropout` of PyG's and DGL's GATv2Conv), in the
 * launches of flex_gatv2_attention and flex_gatv2_attention_backward, on the same plans, walk and grid.  The mask, its threshold and its
 * index are flex_attention_dropout's, bit for bit (flex_dropout_mask is its host reference): with c = 1.0f / (1.0f - drop_p) computed in
 * fp32 on the host, w_eh = keep(seed, e H + h) ? c : 0, where e is the entry's index in the CSR the plan was made from (a row-range
 * shard uses the global index).  x, s, alpha, f and L are flex_gatv2_attention's, unchanged:
 *     Out[r, head h] = sum_e alpha_eh w_eh Xs[c, head h]
 *     da_eh    = w_eh <g[r, head h], Xs[c, head h]>     delta_rh = sum_e p_eh da_eh     dz_eh = p_eh (da_eh - delta_rh)
 *     gXt[r, hd + j] = sum_{e in r}       dz_eh att[hd + j] f_ej
 *     gAtt[hd + j]   = sum_{all e}        dz_eh L_ej
 *     gXs[c, hd + j] = sum_{src(e) = c}  (dz_eh att[hd + j] f_ej  +  p_eh w_eh g[row(e), hd + j])
 * In GATv2 the gathered row Xs[c] is score operand and value, so a dropped entry is still gathered and still takes part in the softmax.
 * The mask enters in three places only: the value term of Out, da, and the p g term of gXs; not the score term of gXs, nor gXt, nor
 * gAtt, which carry it through dz.
 * - P.  The score, maximum, sum, poison rules and dP are flex_gatv2_attention's bit for bit: dP holds the UNDROPPED alpha.
 * - Selection.  A dropped entry is selected out, not multiplied by zero: its value term in Out, its da (exactly +0, the dot product is
 *   not used) and its p g term in gXs.  So a head of a row whose entries are all dropped is +0 bits in Out, and g[r, head h] of such a
 *   head reaches no output, inf and NaN included.  A dropped entry with s = -inf and a -inf in its Xs row adds nothing to Out; a kept
 *   one adds 0 x -inf = NaN, as the undropped call does.  A poisoned head stays NaN.  A head of a row of gXs without a kept entry is
 *   NOT +0: the score term remains (unlike flex_gat_attention_dropout's gV).
 * - drop_p must be finite and in [0, 1), else FLEX_ERR_INVALID, checked beside the slope.  drop_p == 0 launches the kernels of the
 *   undropped calls after the refusals: every output has their bits.
 * - Every other refusal, the operands, dWork, dAttWork (sized by flex_gatv2_attention_work_size), the launches per wanted gradient, the
 *   scope and the stream rules are flex_gatv2_attention's and flex_gatv2_attention_backward's.  The forward runs on row-range shards;
 *   the backward is FLEX_ERR_INVALID there.  The same (drop_p, seed) must be passed to the forward and to the backward.
 *
 * Accuracy, in the terms of flex_gatv2_attention, against float64 on the same fp32 operands under the same mask.  A kept probability is
 * multiplied by c before it enters a sum, one more rounding wherever that product stands:
 *   Out     |Out - Out64| <= sum_{kept e} (gamma(n_r + 4) alpha_e + dalpha_e) c |Xs| + 2^-126
 *   dda_e    = c (gamma(d + 1) sum_j |g Xs| + d 2^-149) + 2^-149 on a kept entry, 0 on a dropped one
 *   ddz, gXt, gAtt: flex_gatv2_attention's lines on this da and dda
 *   |gXs - gXs64|   <= sum_{e in c} [(gamma(2 n_c + 1) |dz_e| + ddz_e) |w_ej| + |dz_e| 2^-149]
 *                      + sum_{kept e in c} gamma(2 n_c + 1) p_e c |g[row]| + 2^-126 */
int flex_dropout_gatv2_attention(const flex_plan *plan, int heads, const float *dXt, const float *dXs, const float *dAtt, float slope,
                                 float drop_p, uint64_t seed, float *dOut, float *dP /* optional */, flex_stream_t stream);
int flex_dropout_gatv2_attention_backward(const flex_plan *plan, int heads, const float *dXt, const float *dXs, const float *dAtt,
                                          const float *dP, const float *dGradOut, float slope, float drop_p, uint64_t seed, float *dGradXt,
                                          float *dGradXs, float *dGradAtt, float *dWork, float *dAttWork, flex_stream_t stream);

/* ≙ alpha_freeMatGPU (mat.cuh:184-193). */
int flex_plan_destroy(flex_plan *plan);

typedef struct flex_plan_info {
    int32_t m, n, k, device;
    int64_t nnz;
    int64_t n_tasks;      /* tasks: rows + pieces of split rows + row bundles (the rows inside a bundle are not tasks of their own) */
    int64_t n_chunks;     /* schedule chunks (runs of tasks): one wave each, four to a workgroup */
    int64_t n_split_rows; /* rows long enough to be split over several waves */
    int64_t n_partials;   /* k-wide partial sums held in the workspace */
    int64_t device_bytes; /* HBM held by the plan */
    int32_t lanes_per_nz; /* G: lanes that cooperate on one nonzero (k/4 rounded up to a power of two) */
    int32_t order;        /* FLEX_ORDER_* actually applied */
    double plan_ms;       /* host time spent planning + uploading */
    int64_t n_slots;      /* chunk-table entries launched: n_chunks + the empty entries that pad the XCD slices */
    int32_t two_d;        /* 1: rows are cut by column panel as well (each XCD slice runs phase by phase), else 0 */
    int32_t panel_rows;   /* two_d: B rows per column panel (a power of two), else 0 */
    int64_t n_tiles;      /* dense 32x32 tiles of A routed to the MFMA kernel (0: the vector kernel does everything) */
    int64_t tile_nnz;     /* nonzeros held by those tiles */
    int64_t n_records;    /* (col,val) records the vector kernel streams per column tile: nnz - tile_nnz + padding */
    /* the hot-block path (0 everywhere when the plan has no blocks) */
    int64_t n_blocks;         /* blocks: one workgroup each (per 64-column tile) */
    int64_t block_rows;       /* rows that hold slots in a block (empty rows, and rows longer than a whole block of slots, hold none) */
    int64_t block_nnz;        /* nonzeros of those rows */
    int64_t block_hot_nnz;    /* nonzeros in the block image: they read their B row from an LDS panel and are NOT in the flat plan's records */
    int64_t block_hot_cols;   /* B rows staged, summed over blocks: block_hot_nnz / block_hot_cols = u, the reuse of a staged row */
    int64_t block_panels;     /* panels staged per column tile, summed over blocks */
    int64_t block_records;    /* records the hot kernel streams per 64-column tile: block_hot_nnz + padding */
    /* row bundles (0 when the plan has none) */
    int64_t n_bundles;        /* tasks that hold several short rows side by side */
    int64_t bundle_rows;      /* rows inside them */
    /* hub rows cut by schedule window (flex_plan_tuning.hub_row; 0 when the cut is off) */
    int64_t n_moved_pieces;   /* pieces of hub rows that run at their columns' place in the schedule instead of their row's */
    int64_t moved_records;    /* nonzeros they hold */
} flex_plan_info;
int flex_plan_get_info(const flex_plan *plan, flex_plan_info *out);

/* The record stream of a plan and how it is stored on the device (flex_plan_tuning.rec_pack). */
typedef struct flex_record_info {
    int32_t packed;        /* 1: 6 bytes per record (value + 16-bit column difference), 0: 8 bytes */
    int32_t reserved;      /* zero */
    int64_t records;       /* = flex_plan_info.n_records */
    int64_t wide_records;  /* packed: records of the chunks that keep the 8-byte form (those with a row bundle) */
    int64_t exceptions;    /* packed: column differences that do not fit 16 bits (8 bytes each, listed per chunk) */
    int64_t stream_bytes;  /* device bytes one column tile reads of the stream: values, differences, exceptions, wide records */
} flex_record_info;
int flex_plan_record_info(const flex_plan *plan, flex_record_info *out);
/* Debug / test aid, synchronous: the record stream read back from the device image -- decoded, where it is packed, by the decoder of
 * flex_plan_self_check -- as `records` pairs {B-row byte offset or column id, value bits} (2 x uint32 each) in stream order.
 * records must equal flex_plan_info.n_records (else FLEX_ERR_INVALID); FLEX_ERR_FORMAT if a packed image does not decode. */
int flex_plan_read_records(const flex_plan *plan, uint32_t *out, int64_t records);

/* ≙ Mat::alpha_stats_collect (mat.cu:944-1065) and the B-Re1 / B-Re2 columns of run()'s table
 * (flex.cu:5217-5223): how much B-row reuse the schedule exposes to each level of the machine,
 * and how evenly the work is cut.  "B rows" are distinct column ids; padding records excluded.
 * Needs FLEX_PLAN_STATS at plan creation, otherwise FLEX_ERR_UNSUPPORTED. */
typedef struct flex_plan_stats {
    int64_t records;       /* nnz + per-row padding to whole gather steps */
    int64_t cols_wave;     /* sum over chunks of distinct B rows  (≙ n_col_sum: reuse inside one unit of work) */
    int64_t cols_wg;       /* sum over workgroups (4 chunks, one CU's L1) */
    int64_t cols_xcd;      /* sum over the 8 XCD slices of the chunk table (≙ acc_col: reuse inside one L2) */
    double reuse_wave;     /* nnz / cols_wave  -- B-Re1: 1 = none, ideal = average degree */
    double reuse_wg;       /* nnz / cols_wg */
    double reuse_xcd;      /* nnz / cols_xcd   -- B-Re2 */
    double gather_bytes;   /* no-reuse gather model: 4(n+1) + 8 nnz + 4 nnz k + 4 n k   (u = 1) */
    double l2_bytes;       /* same with B rows fetched once per XCD: 4(n+1) + 8 records + 4 k cols_xcd + 4 m k */
    int64_t chunk_rec_max; /* largest chunk, records */
    double chunk_rec_mean;
    double chunk_imb_pct;  /* 100 max/mean - 100   (≙ "wp imb") */
    double xcd_imb_pct;    /* records per XCD slice, 100 max/mean - 100   (≙ "sm imb") */
    double split_nnz_pct;  /* share of nonzeros in rows cut into pieces (≙ share of work needing atomics) */
    double pad_pct;        /* 100 (records - nnz) / nnz */
    int64_t n_workgroups;
    /* block-density detector (32x32 tiles in schedule coordinates; ≙ tools/block_density.py of round 1, now in the planner) */
    double tile_nnz_pct_10; /* share of the nonzeros in tiles of fill >= 0.10 */
    double tile_nnz_pct_25; /* ... >= 0.25 */
    double tile_nnz_pct_50; /* ... >= 0.50 */
    double tile_mean_fill;  /* nnz / (1024 * non-empty tiles) */
    int64_t mfma_tiles;     /* tiles routed to the MFMA kernel */
    double mfma_nnz_pct;    /* share of the nonzeros they hold */
    /* reuse a workgroup could have ABOVE the L2 (ABI 3): a column is hot in a block of 480 schedule-consecutive rows when
       at least thr of the block's nonzeros use it -- those B rows could be staged in LDS once and used u times (≙ the `u` of the
       reference's cost model, flex.cu:5513-5528, at the scope of one CU).  Every 4th block is looked at. */
    double lds_hot_pct_2, lds_hot_pct_4; /* share of the nonzeros in hot columns, thr = 2 / 4 */
    double lds_u_2, lds_u_4;             /* hot nonzeros per staged B row */
} flex_plan_stats;
int flex_plan_get_stats(const flex_plan *plan, flex_plan_stats *out);

/* ≙ the per-SM imbalance column of run()'s table (flex.cu:27-79 stamps %smid + clock() per warp, flex.cu:5087-5126
 * turns them into "Imb"): ONE extra launch of the plan with the stamped twin of the SpMM kernel (every wave records the
 * 100 MHz constant clock at start and end and the CU it ran on: XCC id + HW_ID), reduced on the host.  dB / dC as for
 * flex_spmm (16-byte aligned, k % 4 == 0; dC receives the ordinary result); synchronises `stream`.  Not part of
 * flex_spmm: the product launch carries no stamps. */
typedef struct flex_imbalance {
    int64_t waves;            /* waves that ran (chunk-table entries x column tiles, minus padding entries) */
    int32_t cus_seen;         /* distinct CUs that ran at least one wave (256 on MI355X) */
    int32_t xcds_seen;
    double span_us;           /* first wave start -> last wave end */
    double cu_busy_imb_pct;   /* per CU: sum of its waves' lifetimes; 100 max/mean - 100   (≙ "Imb") */
    double cu_end_spread_pct; /* 100 (latest CU end - earliest CU end) / span: how long the first idle CU waits for the last */
    double xcd_busy_imb_pct;  /* the same sums per XCD */
    double xcd_end_spread_pct;
    double wave_us_mean, wave_us_max;
} flex_imbalance;
int flex_plan_measure_imbalance(flex_plan *plan, const float *dB, float *dC, flex_stream_t stream, flex_imbalance *out);

/* ≙ Kernel_Info / GPU_Info (flex.cu:4127-4142, 4933-4941: "Kernel %s: %d regs, %zd local, %zd B shared"): what
 * the kernel this plan launches (for 16-byte aligned dense operands) costs per wave and how many waves fit a CU. */
typedef struct flex_kernel_info {
    int32_t vgprs, sgprs;      /* per wave */
    int32_t lds_bytes;         /* static LDS per workgroup */
    int32_t scratch_bytes;     /* per lane */
    int32_t threads_per_block; /* 256: four independent waves */
    int32_t waves_per_cu;      /* resident waves the occupancy calculator allows */
} flex_kernel_info;
int flex_plan_kernel_info(const flex_plan *plan, flex_kernel_info *out);

/* ≙ the tiler round-trip self-check of csr2_DiagTiling (mat.cu:905-940): reads the plan's device image back
 * and verifies that it is a partition of the work -- chunks tile the tasks, tasks tile the records, every
 * record names a valid B row, every C row is written exactly once (directly or by one split row with
 * contiguous pieces), table padding is empty.  FLEX_ERR_FORMAT if any invariant fails.  Debug / test aid:
 * synchronous, O(plan size) host memory. */
int flex_plan_self_check(const flex_plan *plan);

/* What this box's HBM delivers, for the roofline's denominator (verify BW_peak with a
 * device-to-device copy and report both): GB/s of a read-only streaming pass and of a copy (bytes
 * read + bytes written) over `bytes`-sized buffers (use >= 1 GiB: the Infinity Cache is 256 MiB),
 * mean of `reps` launches each.  temporal = 0: non-temporal loads (HBM rate at any size beyond L2);
 * temporal = 1: ordinary loads, so buffers up to the Infinity Cache's size show ITS rate -- the roof
 * of gathers that miss L2 but whose B is cache-resident (reddit: B = 119 MB).  Allocates and frees
 * 2 x bytes on `device`; synchronises. */
int flex_hbm_probe(int device, int64_t bytes, int reps, int temporal, double *read_gbps, double *copy_gbps);

/* ≙ flexspmm_v9_permuteX (flex.cu:276-289): dst[r,:] = src[idx[r],:], n rows of k floats.
 * Not needed by flex_spmm (plans fold the permutation in); provided for callers that
 * keep the reference's B' ("shadow_b") layout. All pointers are device pointers. */
int flex_gather_rows(float *dst, const float *src, const int32_t *idx, int64_t n, int k,
                     flex_stream_t stream);

/* ---- host-side ingest / reordering (C++ in the reference: DataLoader.cu) ---- */

/* Owned host CSR + the statistics DataLoader computes (DataLoader.cu:26-29, 86-115). */
typedef struct flex_host_csr {
    int32_t m, n;
    int64_t nnz;
    uint32_t *rowPtr;
    uint32_t *col;
    float *vals;
    int64_t uni_nb;
    int64_t n_edges_one_way, n_edges_asymmetric;
    int32_t n_nodes_z_out, n_nodes_z_in, n_nodes_z_deg;
    int32_t is_directed;
    int32_t c;
} flex_host_csr;

/* ≙ DataLoader::DataLoader (DataLoader.cu:9-124): 3-line CSV -> CSR (+ amazon.csv rule:
 * no value line, vals = 2*rand()/RAND_MAX-1). */
int flex_csv_load(const char *path, flex_host_csr *out);
void flex_host_csr_free(flex_host_csr *a);

/* ≙ data/SuiteSparse/mtx2csr.cc:57-247 (mmio_allinone): MatrixMarket coordinate file -> CSR.
 * real / integer / pattern (value 1) / complex (real part); `symmetric` and `hermitian` files are
 * expanded to both triangles.  sort_columns = 0 keeps the reference's layout (entries of a row in
 * file order, which the reference's tilers mis-handle: mtx2csr.cc:171-195); 1 sorts each row by
 * column.  m != n is allowed; graph statistics are filled only for square matrices. */
int flex_mtx_load(const char *path, int sort_columns, flex_host_csr *out);

/* ≙ writeCSR2csv (mtx2csr.cc:249-268): the 3-line CSV that DataLoader reads.  Values are written
 * with 9 significant digits so that the file round-trips fp32 exactly (the reference's ofstream
 * default keeps 6). */
int flex_csv_save(const char *path, const flex_csr *A);

/* Binary CSR cache (new; avoids re-parsing GB-sized CSVs): little-endian
 * {magic "FLEXCSR1", int64 m, n, nnz} + rowPtr + col + vals. */
int flex_csr_save_bin(const char *path, const flex_csr *A);
int flex_csr_load_bin(const char *path, flex_host_csr *out);

/* Permutation cache (the reference recomputes every ordering on every run): `rank`
 * (rank[old] = new, n entries) as a small binary file keyed by a 64-bit fingerprint of the CSR
 * structure (flex_csr_fingerprint: n, nnz, rowPtr, col), so a stale file is refused, not applied.
 * flex_perm_load returns FLEX_ERR_IO if the file is absent, FLEX_ERR_FORMAT if it is not a
 * permutation of 0..n-1 or was written for another matrix. */
uint64_t flex_csr_fingerprint(const flex_csr *A);
int flex_perm_save(const char *path, const uint32_t *rank, int64_t n, uint64_t fingerprint);
int flex_perm_load(const char *path, uint32_t *rank, int64_t n, uint64_t fingerprint);

/* ≙ cpuX fill in DataLoader::cuda_alloc_cpy (DataLoader.cu:198-209), glibc rand() stream. */
int flex_fill_dense_rand(float *hostB, int64_t n, int k);

/* ≙ order_rcm(h) (order_rcm.cu:15-33): rank[old] = new. */
int flex_order_rcm(const flex_csr *A, uint32_t *rank);

/* ≙ complete_gorder(h, window) (order_gorder.cu:13-31; DataLoaderGorder uses window 3,
 * DataLoader.cu:808): RCM, then Gorder with the lazy unit heap.  FLEX_ERR_UNSUPPORTED for a graph
 * with an isolated vertex (the reference cannot order one either, unitheap.cu:35-38). */
int flex_order_gorder(const flex_csr *A, uint32_t window, uint32_t *rank);

/* ≙ the ordering of DataLoaderDFS (DataLoader.cu:324-395): depth-first pre-order from vertex 0. */
int flex_order_dfs(const flex_csr *A, uint32_t *rank);
/* ≙ DataLoaderRabbit (DataLoader.cu:455-655) as the reference compiles it (iterative rounds in degree order, no hub
 * grouping): modularity-driven agglomeration + left-to-right walk of the dendrograms.  is_directed = the loader's flag
 * (the clustering then runs on the undirected version).  rank[old] = new; identical to the oracle's restatement.
 * The engine's own community schedule is flex_order_cluster (parallel, built for 10^8 nonzeros). */
int flex_order_rabbit(const flex_csr *A, int is_directed, uint32_t *rank);

/* ≙ order_deg(h, desc) (order_deg.cu:19-45): rank by in+out degree, ties by vertex id. */
int flex_order_deg(const flex_csr *A, int descending, uint32_t *rank);

/* ≙ the clustering half of DataLoaderRabbit (DataLoader.cu:453-655): rank[old] = new such
 * that communities (and their sub-communities) are consecutive.  Two stages (cluster.cpp): modularity-driven agglomeration
 * + a walk of the merge forest, then a few sweeps of vertex moves between stretches of that order (kept only when they
 * put more edges within 2048 positions).  Deterministic: the same rank for any number of host threads. */
int flex_order_cluster(const flex_csr *A, uint32_t *rank);
int flex_order_cluster_ex(const flex_csr *A, const flex_cluster_tuning *tuning /* NULL = rules */, uint32_t *rank);

/* ≙ DataLoaderRcm body (DataLoader.cu:741-779): vo_mp[new]=old + permuted CSR, columns
 * ascending per row. Outputs caller-allocated with the sizes of A. */
int flex_perm_csr(const flex_csr *A, const uint32_t *rank, int32_t *vo_mp, uint32_t *rowPtr2,
                  uint32_t *col2, float *vals2);

/* ---- multi-GPU row sharding (new; the reference is single-GPU, flex.cu:4137) ---- */

/* Contiguous row ranges of about equal cost, cost(row) = nnz(row)*(4k+8) + 4k bytes
 * (gathered B bytes + records + the C row).  Writes nparts+1 row boundaries,
 * row_bounds[0]=0 .. row_bounds[nparts]=m.  Each rank then builds its own plan on
 * rows [row_bounds[r], row_bounds[r+1]) with flex_plan_create_rows. */
int flex_shard_rows(const flex_csr *A, int k, int nparts, int64_t *row_bounds);

/* ---- synthetic graphs with the README's shapes (README.md:13-20); data files are absent ---- */
typedef struct flex_synth_params {
    int64_t n;           /* vertices */
    int64_t nnz;         /* exact nnz incl. one self-loop per row; nnz-n must be even (symmetric) */
    double alpha;        /* power-law exponent of expected degrees (e.g. 2.1) */
    int64_t community;   /* mean planted-community size (0 = none) */
    double p_in;         /* fraction of edges kept inside a community */
    double p_near;       /* fraction of edges that go to one of the 2*near_window neighbouring communities */
    int32_t near_window; /* communities on either side counted as "near" */
    int32_t shuffle;     /* 1: random vertex relabel so the natural order is not banded */
    int32_t gcn_norm;    /* 1: vals = 1/sqrt(d_i d_j) (pubmed-like); 0: U(-1,1) */
    int32_t directed;    /* 1: every edge kept in ONE random direction, no self loops, so nnz = #edges and
                            rows may be empty (the SuiteSparse stand-ins); 0: symmetric + self loops */
    uint64_t seed;
} flex_synth_params;
int flex_synth_graph(const flex_synth_params *p, flex_host_csr *out);
/* Parameters of the stand-in for a named graph of the README / the SuiteSparse sweep
 * ("pubmed","flickr","reddit","ppi","yelp","amazon","wiki-vote","soc-sign-epinions"),
 * scaled to `scale` x vertices and nonzeros (weak-scaling runs). */
int flex_synth_preset(const char *name, int scale, flex_synth_params *out);

const char *flex_strerror(int status);
/* hipError_t of the last failed HIP call on this thread (0 if none) and its text. */
int flex_last_hip_error(void);
const char *flex_last_hip_error_string(void);
int flex_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* FLEX_SPMM_H */
