// plan.cpp -- life cycle and launch half of the C ABI (include/flex_spmm.h): plan creation entry points, the autotuner,
// flex_spmm, destroy and the info getters.  The planner proper is plan_build.cpp (see plan.h for the map).
//
// Replaces Mat::Mat / csr2_DiagTiling / alpha_transfer / launch_prep /
// alpha_freeMatGPU (mat.cu:7-41, 268-293, 680-942; mat.cuh:184-193).  The
// reference re-cuts A into diagonal "pillars" with per-SM queues and marks most
// rows for atomicAdd; here the plan is a *schedule*: rows (in the given, RCM,
// community or Gorder order) are packed into per-wave chunks of about equal cost,
// rows longer than one chunk budget are cut into pieces that write k-wide partial
// sums (combined in piece order inside the launch), the chunk table is cut into
// eight cost-balanced XCD slices, and column ids are pre-multiplied into B-row
// byte offsets.  Columns always refer to
// the ORIGINAL B, rows always write the ORIGINAL C row, so no permuteX pass and
// no shadow copy of B exist (flex.cu:276-289, mat.cu:287-290).
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <memory>
#include <new>
#include <vector>

#include "host_parallel.h"
#include "plan.h"

namespace flex {

static thread_local hipError_t g_last_hip = hipSuccess;
void note_hip_error(hipError_t e) { g_last_hip = e; }

int validate_csr(const flex_csr *A) {
    if (!A || A->m < 0 || A->n < 0 || A->nnz < 0) return FLEX_ERR_INVALID;
    if (!A->rowPtr) return FLEX_ERR_INVALID;
    if (A->nnz > 0 && (!A->col || !A->vals)) return FLEX_ERR_INVALID;
    if (A->nnz >= (int64_t(1) << 32)) return FLEX_ERR_UNSUPPORTED;
    if (A->rowPtr[0] != 0 || A->rowPtr[A->m] != static_cast<uint32_t>(A->nnz)) return FLEX_ERR_INVALID;
    for (int32_t r = 0; r < A->m; ++r)
        if (A->rowPtr[r] > A->rowPtr[r + 1]) return FLEX_ERR_INVALID;
    const uint32_t n = static_cast<uint32_t>(A->n);
    constexpr int64_t kBlk = 1 << 20;
    std::atomic<int> bad{0};
    parallel_chunks((A->nnz + kBlk - 1) / kBlk, [&](int64_t b) {
        uint32_t worst = 0;
        for (int64_t e = b * kBlk; e < std::min<int64_t>(A->nnz, (b + 1) * kBlk); ++e) worst = std::max(worst, A->col[e]);
        if (worst >= n) bad.store(1);
    });
    return bad.load() ? FLEX_ERR_INVALID : FLEX_OK;
}

bool plan_timing_enabled() {
    static const bool on = std::getenv("FLEX_PLAN_TIMING") != nullptr;
    return on;
}

}  // namespace flex

using namespace flex;

extern "C" int flex_spmm(flex_plan *p, const float *dB, float *dC, flex_stream_t stream);

namespace {

// FLEX_PLAN_AUTOTUNE: the degree rule picks the column-tile width G from two thresholds measured on a handful of
// shapes; this measures instead.  The neighbouring widths are planned too (same row schedule, computed once),
// each candidate is timed on zero-filled operands of the real size (what a gather costs depends on its address,
// not on the value), and the fastest plan is kept.  Costs up to three extra plans and 2 * 4*(n*ldb + m*ldc) bytes for
// the duration of the call.
int autotune(std::unique_ptr<flex_plan> &best, const flex_csr *A, int32_t r0, int32_t r1, const int32_t *col_map, const int32_t *dst_map,
             unsigned flags, const flex_plan_tuning &tuning, std::vector<uint32_t> &sched_cache, const uint32_t *entry_of) {
    if (best->m == 0 || best->k % 4 != 0 || best->ldb % 4 != 0 || best->ldc % 4 != 0) return FLEX_OK;
    int g_max = 8;
    while (4 * g_max < best->k && g_max < 32) g_max <<= 1;
    DeviceArray<float> dB, dC;
    if (dB.allocate(std::max<size_t>(static_cast<size_t>(best->n) * best->ldb, 4)) != hipSuccess ||
        dC.allocate(std::max<size_t>(static_cast<size_t>(best->c_rows) * best->ldc, 4)) != hipSuccess) {
        (void)hipGetLastError();
        return FLEX_OK;  // no room to measure: keep the rule's choice
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = FLEX_OK;
    auto time_plan = [&](flex_plan *q, double *us) {
        for (int i = 0; i < 2 && !rc; ++i) rc = flex_spmm(q, dB.get(), dC.get(), nullptr);
        if (!rc && hipEventRecord(e0, nullptr) != hipSuccess) rc = FLEX_ERR_HIP;
        for (int i = 0; i < 5 && !rc; ++i) rc = flex_spmm(q, dB.get(), dC.get(), nullptr);
        float ms = 0.f;
        if (!rc && (hipEventRecord(e1, nullptr) != hipSuccess || hipEventSynchronize(e1) != hipSuccess ||
                    hipEventElapsedTime(&ms, e0, e1) != hipSuccess))
            rc = FLEX_ERR_HIP;
        *us = ms * 1e3 / 5;
    };
    if (hipMemset(dB.get(), 0, dB.size() * sizeof(float)) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess)
        rc = FLEX_ERR_HIP;
    double best_us = 0.0;
    if (!rc) time_plan(best.get(), &best_us);
    // a candidate: a blank plan of best's shape, built with `t` at width force_G, kept if it is strictly faster.  toggles_bundles: it
    // is compared only if it has best's width and the other bundle setting (else there is nothing to compare, e.g. no row short enough)
    auto consider = [&](const flex_plan_tuning &t, int force_G, bool toggles_bundles) {
        std::unique_ptr<flex_plan> q(new (std::nothrow) flex_plan());
        if (!q) return;
        q->m = best->m; q->n = best->n; q->k = best->k; q->device = best->device;
        q->ldb = best->ldb; q->ldc = best->ldc; q->nnz = best->nnz;
        if (build_plan(q.get(), A, r0, r1, col_map, dst_map, flags, t, &sched_cache, force_G, entry_of) != FLEX_OK || hipDeviceSynchronize() != hipSuccess)
            return;
        if (toggles_bundles && (q->lanes_per_nz != best->lanes_per_nz || (q->n_bundles != 0) == (best->n_bundles != 0))) return;
        double us = 0.0;
        time_plan(q.get(), &us);
        if (!rc && us < best_us) {
            std::swap(best, q);
            best_us = us;
        }
    };
    const int g0 = best->lanes_per_nz;
    for (int g : {g0 / 2, g0 * 2})
        if (!rc && g >= 8 && g <= g_max) consider(tuning, g, false);
    // Row bundles the same way: their rule is one threshold (a chunk per wave slot of the card) between two measured regimes, so on
    // the tiles that have them the other setting is planned and timed too, at the width that won above -- unless the caller chose.
    if (!rc && tuning.bundle == 0 && 64 / best->lanes_per_nz >= static_cast<int>(kBundleMinSlots)) {
        flex_plan_tuning other = tuning;
        other.bundle = best->n_bundles ? 2 : 1;
        consider(other, best->lanes_per_nz, true);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

}  // namespace

extern "C" {

// ABI 3's layout: block_ablate_retired holds the place of a retired knob, so that no later field moves
static_assert(sizeof(flex_plan_tuning) == 160 && offsetof(flex_plan_tuning, block_ablate_retired) == 116 && sizeof(flex_plan_desc) == 80);

// every knob is "0 = rule" or a small positive number; anything negative or absurd is a caller bug, not a request
static bool tuning_ok(const flex_plan_tuning &t) {
    const int32_t *f = reinterpret_cast<const int32_t *>(&t);
    for (size_t i = 0; i < sizeof(t) / sizeof(int32_t); ++i)
        if (f[i] < 0 || f[i] > (1 << 28)) return false;
    for (int32_t r : t.reserved)
        if (r != 0) return false;
    return t.block_ablate_retired == 0;
}

// FLEX_PLAN_TRANSPOSE: the CSR of A^T, built by a stable counting sort -- row c of A^T lists the rows of A that hold column c in
// ascending order, a duplicate (r, c) pair keeping its CSR order -- so that the plan is exactly the plan of that CSR passed as given.
// One sequential pass: the result cannot depend on the host thread count.  Owned by the caller's create call and freed with it.
// want_entries (FLEX_PLAN_MUTABLE_VALUES): also entry[d] = the entry of A that became entry d of A^T -- the sort's permutation, so
// that the plan's record -> entry map refers to A's CSR order.
struct TransposedCsr {
    std::vector<uint32_t> rowPtr, col, entry;
    std::vector<float> vals;
    flex_csr csr{};
};

static int transpose_csr(const flex_csr *A, TransposedCsr *t, bool want_entries) {
    int rc = validate_csr(A);
    if (rc) return rc;
    if (A->n >= INT32_MAX) return FLEX_ERR_UNSUPPORTED;
    const size_t nnz = static_cast<size_t>(A->nnz);
    try {
        t->rowPtr.assign(static_cast<size_t>(A->n) + 1, 0u);
        t->col.resize(nnz);
        t->vals.resize(nnz);
        if (want_entries) t->entry.resize(nnz);
    } catch (const std::bad_alloc &) {
        return FLEX_ERR_NOMEM;
    }
    for (size_t e = 0; e < nnz; ++e) ++t->rowPtr[A->col[e] + 1];
    for (int32_t c = 0; c < A->n; ++c) t->rowPtr[c + 1] += t->rowPtr[c];
    std::vector<uint32_t> pos;  // next free slot of every row of A^T
    try {
        pos.assign(t->rowPtr.begin(), t->rowPtr.end() - 1);
    } catch (const std::bad_alloc &) {
        return FLEX_ERR_NOMEM;
    }
    for (int32_t r = 0; r < A->m; ++r)
        for (uint32_t e = A->rowPtr[r]; e < A->rowPtr[r + 1]; ++e) {
            const uint32_t d = pos[A->col[e]]++;
            t->col[d] = static_cast<uint32_t>(r);
            t->vals[d] = A->vals[e];
            if (want_entries) t->entry[d] = e;
        }
    t->csr = flex_csr{A->n, A->m, A->nnz, t->rowPtr.data(), nnz ? t->col.data() : nullptr, nnz ? t->vals.data() : nullptr};
    return FLEX_OK;
}

// FLEX_PLAN_MUTABLE_VALUES: the fingerprint (entry_fp) of the (entry, B row) pairs a plan of rows [r0, r1) holds, taken straight from
// the caller's CSR A -- for a transposed plan, the entries of A whose COLUMN lies in [r0, r1), each reading B row col_map(its row) --
// so that flex_plan_self_check compares the device image with the input and not with the planner's own arrays.
static uint64_t held_entries_fp(const flex_csr *A, bool transposed, int64_t r0, int64_t r1, const int32_t *col_map) {
    auto brow = [&](uint32_t c) { return col_map ? static_cast<uint32_t>(col_map[c]) : c; };
    uint64_t fp = 0;
    if (!transposed) {
        for (uint32_t e = A->rowPtr[r0]; e < A->rowPtr[r1]; ++e) fp += entry_fp(e, brow(A->col[e]));
        return fp;
    }
    for (int32_t r = 0; r < A->m; ++r)
        for (uint32_t e = A->rowPtr[r]; e < A->rowPtr[r + 1]; ++e)
            if (A->col[e] >= r0 && A->col[e] < r1) fp += entry_fp(e, brow(static_cast<uint32_t>(r)));
    return fp;
}

// all_rows: every row of the CSR that is planned (A's, or A^T's under FLEX_PLAN_TRANSPOSE; row_begin / row_end are not read),
// otherwise the caller's range [row_begin, row_end) of that CSR
static int create_common(flex_plan **out, const flex_csr *hostA, bool all_rows, int64_t row_begin, int64_t row_end,
                         const int32_t *col_map, const int32_t *dst_map, int k, int device, unsigned flags,
                         int ldb = 0, int ldc = 0, const flex_plan_tuning *tuning_in = nullptr) {
    if (!out) return FLEX_ERR_INVALID;
    *out = nullptr;
    flex_plan_tuning tuning = tuning_in ? *tuning_in : flex_plan_tuning{};
    if (!tuning_ok(tuning)) return FLEX_ERR_INVALID;
    const HostThreadsScope threads_for_this_call(tuning.host_threads);
    if (k <= 0 || device < 0) return FLEX_ERR_INVALID;
    if (ldb == 0) ldb = k;
    if (ldc == 0) ldc = k;
    if (ldb < k || ldc < k) return FLEX_ERR_INVALID;
    const unsigned order = flags & FLEX_ORDER_MASK;
    if (order > FLEX_ORDER_GORDER ||
        (flags & ~(FLEX_ORDER_MASK | FLEX_PLAN_STATS | FLEX_PLAN_AUTOTUNE | FLEX_PLAN_XCD_INTERLEAVE | FLEX_PLAN_TRANSPOSE | FLEX_PLAN_MUTABLE_VALUES | FLEX_PLAN_ATTENTION | FLEX_PLAN_ATTENTION_BACKWARD | FLEX_PLAN_BF16)))
        return FLEX_ERR_INVALID;
    // FLEX_PLAN_BF16: the fp32 plan of the row width in 4-byte words.  From here on k, ldb and ldc are words; the planner proper never
    // sees the flag, only flex_plan::bf16 where fp32 values are counted (plan.h).
    const bool bf16 = (flags & FLEX_PLAN_BF16) != 0;
    if (bf16) {
        if (flags & (FLEX_PLAN_MUTABLE_VALUES | FLEX_PLAN_ATTENTION | FLEX_PLAN_ATTENTION_BACKWARD | FLEX_PLAN_AUTOTUNE)) return FLEX_ERR_UNSUPPORTED;
        if (k % 8 != 0 || ldb % 8 != 0 || ldc % 8 != 0) return FLEX_ERR_UNSUPPORTED;  // 16-byte gathers and stores only
        // every nonzero on the flat record stream, split rows summed by the second launch: the dense-tile and hot-block kernels and the
        // in-launch sum's sc1 hand-off exist for fp32 rows only
        if (tuning.mfma == 1 || tuning.blocks == 1 || tuning.split_rows == 1 || tuning.two_d == 1) return FLEX_ERR_UNSUPPORTED;
        tuning.mfma = 2;
        tuning.blocks = 2;
        tuning.split_rows = 2;
        k /= 2;
        ldb /= 2;
        ldc /= 2;
        flags &= ~FLEX_PLAN_BF16;
    }
    const bool mut = (flags & FLEX_PLAN_MUTABLE_VALUES) != 0;
    if (mut) {  // every nonzero on the flat record stream: the dense-tile and hot-block routes keep values in layouts of their own
        if (tuning.mfma == 1 || tuning.blocks == 1 || tuning.rec_pack == 1) return FLEX_ERR_UNSUPPORTED;
        tuning.mfma = 2;
        tuning.blocks = 2;
        tuning.rec_pack = 2;  // the refresh, the SDDMM and the softmax read or write the 8-byte records
    }
    int rc = FLEX_OK;
    const flex_csr *const callerA = hostA;
    const bool transposed = (flags & FLEX_PLAN_TRANSPOSE) != 0;
    // the fused attention walks hostA's rows and reads K / V by hostA's columns: no transposed plan, no map
    const bool attn = (flags & FLEX_PLAN_ATTENTION) != 0;
    if (attn && (transposed || col_map || dst_map || tuning.rec_pack == 1)) return FLEX_ERR_UNSUPPORTED;
    if (attn) tuning.rec_pack = 2;
    // the fused backward's column walk is over every entry of hostA: with a row range gK / gV would be partial sums
    const bool attn_bwd = (flags & FLEX_PLAN_ATTENTION_BACKWARD) != 0;
    if (attn_bwd && !attn) return FLEX_ERR_INVALID;
    if (attn_bwd && !all_rows) return FLEX_ERR_UNSUPPORTED;
    // hub rows are cut by schedule window (plan_build.cpp, cut_hub_rows) on plans of the caller's own square matrix, all rows, only
    if (attn || transposed || !all_rows) tuning.hub_row = 1;
    flags &= ~(FLEX_PLAN_ATTENTION | FLEX_PLAN_ATTENTION_BACKWARD);  // the planner proper never sees them: the record stream is what it is without the flags
    TransposedCsr at;
    if (transposed) {
        rc = transpose_csr(hostA, &at, mut);
        if (rc) return rc;
        hostA = &at.csr;
        flags &= ~FLEX_PLAN_TRANSPOSE;
    }
    rc = validate_csr(hostA);
    if (rc) return rc;
    if (hostA->m >= INT32_MAX) return FLEX_ERR_UNSUPPORTED;
    if (all_rows) {
        row_begin = 0;
        row_end = hostA->m;
    }
    if (row_begin < 0 || row_end < row_begin || row_end > hostA->m) return FLEX_ERR_INVALID;
    if (col_map)
        for (int32_t c = 0; c < hostA->n; ++c)
            if (col_map[c] < 0 || col_map[c] >= hostA->n) return FLEX_ERR_INVALID;
    if (dst_map)
        for (int64_t r = row_begin; r < row_end; ++r)
            if (dst_map[r] < 0 || dst_map[r] >= hostA->m) return FLEX_ERR_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    const DeviceScope on(device);  // before the plans: they are freed while their device is current
    FLEX_HIP_TRY(on.error());
    std::unique_ptr<flex_plan> p(new (std::nothrow) flex_plan());
    if (!p) return FLEX_ERR_NOMEM;
    p->m = static_cast<int32_t>(row_end - row_begin);
    p->n = hostA->n;
    p->k = k;
    p->ldb = ldb;
    p->ldc = ldc;
    p->bf16 = bf16;
    p->nnz = static_cast<int64_t>(hostA->rowPtr[row_end]) - hostA->rowPtr[row_begin];
    p->device = device;
    std::vector<uint32_t> sched_cache;
    const bool tune = (flags & FLEX_PLAN_AUTOTUNE) != 0;
    const uint32_t *entry_of = transposed && mut && hostA->nnz > 0 ? at.entry.data() : nullptr;
    try {
        rc = build_plan(p.get(), hostA, static_cast<int32_t>(row_begin), static_cast<int32_t>(row_end), col_map, dst_map, flags, tuning,
                        tune ? &sched_cache : nullptr, 0, entry_of);
        if (rc == FLEX_OK && tune) rc = autotune(p, hostA, static_cast<int32_t>(row_begin), static_cast<int32_t>(row_end), col_map, dst_map, flags, tuning, sched_cache, entry_of);
        if (rc == FLEX_OK && mut) {
            p->src_nnz = callerA->nnz;
            p->ent_fp = held_entries_fp(callerA, transposed, row_begin, row_end, col_map);
            // the edge softmax runs over hostA's rows: all of them under a transposed plan of every row, none under a transposed shard
            // (it holds pieces of hostA's rows)
            if (!transposed) rc = upload_softmax_image(p.get(), callerA->rowPtr, row_begin, row_end);
            else if (all_rows) rc = upload_softmax_image(p.get(), callerA->rowPtr, 0, callerA->m);
        }
        if (rc == FLEX_OK && attn) {
            p->at_ent_fp = held_entries_fp(callerA, false, row_begin, row_end, nullptr);
            if (attn_bwd)
                for (int32_t r = 0; r < callerA->m; ++r)
                    for (uint32_t e = callerA->rowPtr[r]; e < callerA->rowPtr[r + 1]; ++e) p->ab_fp += rowptr_fp(static_cast<uint32_t>(r), e);
            rc = upload_attention_image(p.get(), callerA, row_begin, row_end, attn_bwd);
        }
    } catch (const std::bad_alloc &) {  // nothing crosses the C ABI as an exception
        rc = FLEX_ERR_NOMEM;
    } catch (...) {
        rc = FLEX_ERR_INVALID;
    }
    if (rc == FLEX_OK && hipDeviceSynchronize() != hipSuccess) rc = FLEX_ERR_HIP;
    if (rc) return rc;
    p->plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *out = p.release();
    return FLEX_OK;
}

int flex_plan_create(flex_plan **out, const flex_csr *hostA, int k, int device, unsigned flags) {
    if (!hostA) return FLEX_ERR_INVALID;
    // dst_map == NULL means slice-local rows, which for the full range is the identity
    return create_common(out, hostA, true, 0, 0, nullptr, nullptr, k, device, flags);
}

int flex_plan_create_ld(flex_plan **out, const flex_csr *hostA, int k, int ldb, int ldc, int device, unsigned flags) {
    if (!hostA || ldb < k || ldc < k) return FLEX_ERR_INVALID;
    return create_common(out, hostA, true, 0, 0, nullptr, nullptr, k, device, flags, ldb, ldc);
}

int flex_plan_create_mapped(flex_plan **out, const flex_csr *hostA, const int32_t *vo_mp, int k, int device,
                            unsigned flags) {
    if (!hostA) return FLEX_ERR_INVALID;
    if (vo_mp && hostA->m != hostA->n) return FLEX_ERR_INVALID;
    return create_common(out, hostA, true, 0, 0, vo_mp, vo_mp, k, device, flags);
}

int flex_plan_create_rows(flex_plan **out, const flex_csr *hostA, int64_t row_begin, int64_t row_end,
                          const int32_t *col_map, int k, int device, unsigned flags) {
    if ((flags & FLEX_ORDER_MASK) != FLEX_ORDER_NATURAL) return FLEX_ERR_INVALID;
    return create_common(out, hostA, false, row_begin, row_end, col_map, nullptr, k, device, flags);
}

int flex_plan_create_ex(flex_plan **out, const flex_plan_desc *d) {
    constexpr size_t kSizeAbi2 = offsetof(flex_plan_desc, tuning);  // a caller built against ABI 2: no tuning member
    if (!d || !d->A || (d->struct_size != sizeof(flex_plan_desc) && d->struct_size != kSizeAbi2)) return FLEX_ERR_INVALID;
    const flex_plan_tuning *tuning = d->struct_size == sizeof(flex_plan_desc) ? d->tuning : nullptr;
    const bool all_rows = (d->flags & FLEX_PLAN_ROW_RANGE) == 0;  // with the flag, (0,0) is an EMPTY shard, not "everything"
    // without the flag the range members must be zero: a shard range passed by a caller that forgot the flag (or was built before
    // the flag existed) would otherwise get a plan over ALL rows and flex_spmm would write past the shard's C buffer
    if (all_rows && (d->row_begin != 0 || d->row_end != 0)) return FLEX_ERR_INVALID;
    const int64_t r0 = d->row_begin, r1 = d->row_end;
    if (d->row_map && (!all_rows || d->A->m != d->A->n)) return FLEX_ERR_INVALID;  // a row map renames ALL rows of a graph
    if (!all_rows && (d->flags & FLEX_ORDER_MASK) != FLEX_ORDER_NATURAL) return FLEX_ERR_INVALID;  // reorder first, then shard
    return create_common(out, d->A, all_rows, r0, r1, d->col_map, d->row_map, d->k, d->device, d->flags & ~FLEX_PLAN_ROW_RANGE, d->ldb, d->ldc, tuning);
}

int flex_spmm(flex_plan *p, const float *dB, float *dC, flex_stream_t stream) {
    if (!p || p->bf16) return FLEX_ERR_INVALID;  // a bf16 plan runs flex_spmm_bf16 (spmm_bf16_kernels.hip) and nothing else
    if (p->m == 0) return FLEX_OK;
    if (!dC || (!dB && p->nnz > 0)) return FLEX_ERR_INVALID;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const bool vec4 = operands_vec4(p, dB, dC);
    const bool fused = vec4 && p->fused_fixup;  // the generic kernel always leaves the sum to spmm_fixup_kernel
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = FLEX_OK;
    // a plan with split rows owns their partial-sum workspace (and, in the in-launch form, their arrival counters): plan.h, LaunchGuard
    const LaunchGuard guard(p, s);
    if (guard.begin() != FLEX_OK) return FLEX_ERR_INVALID;
    rc = launch_spmm(plan_view(p, fused, nullptr), p->lanes_per_nz, p->off32, vec4, dB, dC, s, p->unroll);
    if (rc == FLEX_OK && !fused) rc = launch_fixup(p->d_partial.get(), p->d_split.get(), p->n_split, p->k, p->ldc, dC, s);
    // the dense tiles' share, added to the rows the kernels above have written
    if (rc == FLEX_OK && p->n_tiles) rc = launch_tiles(tile_view(p), p->off32, dB, dC, p->k, p->ldb, p->ldc, s);
    // the hot blocks' share (the nonzeros with reuse on chip: B rows staged in LDS), added to the rows the flat kernel has written
    if (rc == FLEX_OK && p->bk_blocks) rc = launch_blocks(block_view(p), dB, dC, s, vec4);  // unaligned operands: the generic hot kernel
    if (rc == FLEX_OK) guard.done();
    return rc;
}

int flex_plan_destroy(flex_plan *p) {
    if (!p) return FLEX_OK;
    const DeviceScope on(p->device);
    delete p;
    return FLEX_OK;
}

int flex_plan_get_info(const flex_plan *p, flex_plan_info *o) {
    if (!p || !o) return FLEX_ERR_INVALID;
    o->m = p->m;
    o->n = p->n;
    o->k = p->k * p->elems_per_word();  // elements, also on a bf16 plan
    o->device = p->device;
    o->nnz = p->nnz;
    o->n_tasks = p->n_tasks;
    o->n_chunks = p->n_chunks;
    o->n_split_rows = p->n_split;
    o->n_partials = p->n_partials;
    o->device_bytes = p->device_bytes;
    o->lanes_per_nz = p->lanes_per_nz;
    o->order = static_cast<int32_t>(p->order);
    o->plan_ms = p->plan_ms;
    o->n_slots = p->n_slots;
    o->two_d = p->two_d ? 1 : 0;
    o->n_tiles = p->n_tiles;
    o->tile_nnz = p->tile_nnz;
    o->n_records = p->n_records;
    o->panel_rows = p->two_d ? static_cast<int32_t>(p->panel_rows) : 0;
    o->n_blocks = p->bk_blocks;
    o->block_rows = p->bk_rows;
    o->block_nnz = p->bk_nnz;
    o->block_hot_nnz = p->bk_hot_nnz;
    o->block_hot_cols = p->bk_hot_cols;
    o->block_panels = p->bk_panels;
    o->block_records = static_cast<int64_t>(p->d_bk_rec.size());
    o->n_bundles = p->n_bundles;
    o->bundle_rows = p->bundle_rows;
    o->n_moved_pieces = p->n_moved_pieces;
    o->moved_records = p->moved_records;
    return FLEX_OK;
}

int flex_plan_record_info(const flex_plan *p, flex_record_info *o) {
    if (!p || !o) return FLEX_ERR_INVALID;
    const int64_t exceptions = static_cast<int64_t>(p->d_exc.size());
    const int64_t bytes = p->rec_packed ? 6 * (p->n_records - p->wide_records) + 8 * (p->wide_records + exceptions) : 8 * p->n_records;
    *o = flex_record_info{p->rec_packed ? 1 : 0, 0, p->n_records, p->wide_records, exceptions, bytes};
    return FLEX_OK;
}

int flex_plan_softmax_info(const flex_plan *p, flex_softmax_info *o) {
    if (!p || !o || !p->mutable_vals) return FLEX_ERR_INVALID;
    if (!p->sm_ok) return FLEX_ERR_UNSUPPORTED;
    *o = flex_softmax_info{p->sm_rows, p->sm_entries, static_cast<int64_t>(p->d_sm_item.size()), p->n_sm_groups, p->sm_class_rows[3],
                           p->sm_class_rows[kSmPacked], p->sm_class_rows[kSmWaveRow], p->sm_class_rows[kSmBlockRow], p->sm_group_budget, p->sm_bytes};
    return FLEX_OK;
}

int flex_plan_attention_backward_info(const flex_plan *p, flex_attention_backward_info *o) {
    if (!p || !o || !p->ab_ok) return FLEX_ERR_INVALID;
    *o = flex_attention_backward_info{p->ab_cols, p->at_entries, static_cast<int64_t>(p->d_ab_item.size()), p->n_ab_groups, p->ab_class_cols[3],
                                      p->ab_class_cols[kAtSlot], p->ab_class_cols[kAtWave], p->ab_class_cols[kAtBlock], p->ab_group_budget, p->ab_bytes};
    return FLEX_OK;
}

int flex_plan_attention_info(const flex_plan *p, flex_attention_info *o) {
    if (!p || !o || !p->at_ok) return FLEX_ERR_INVALID;
    *o = flex_attention_info{p->at_rows, p->at_entries, static_cast<int64_t>(p->d_at_item.size()), p->n_at_groups, p->at_class_rows[3],
                             p->at_class_rows[kAtSlot], p->at_class_rows[kAtWave], p->at_class_rows[kAtBlock], p->at_group_budget, p->at_bytes};
    return FLEX_OK;
}

int flex_plan_is_bf16(const flex_plan *p) { return !p ? FLEX_ERR_INVALID : p->bf16 ? 1 : 0; }

int flex_plan_get_tuning(const flex_plan *p, flex_plan_tuning *o) {
    if (!p || !o) return FLEX_ERR_INVALID;
    *o = p->tuning;
    return FLEX_OK;
}

int flex_set_host_threads(int n) {
    if (n < 0) n = 0;
    return host_threads_cap().exchange(n);
}

int flex_plan_get_stats(const flex_plan *p, flex_plan_stats *o) {
    if (!p || !o) return FLEX_ERR_INVALID;
    if (!p->has_stats) return FLEX_ERR_UNSUPPORTED;
    *o = p->stats;
    return FLEX_OK;
}

int flex_plan_kernel_info(const flex_plan *p, flex_kernel_info *o) {
    if (!p || !o) return FLEX_ERR_INVALID;
    if (p->bf16) return FLEX_ERR_UNSUPPORTED;  // the bf16 kernels' registers: DESIGN.md 3.16
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    hipFuncAttributes a{};
    int waves = 0;
    const bool vec4 = p->k % 4 == 0 && p->ldb % 4 == 0 && p->ldc % 4 == 0;
    const int rc = kernel_attributes(p->lanes_per_nz, p->off32, vec4, &a, &waves);
    if (rc) return rc;
    *o = flex_kernel_info{a.numRegs, 0, static_cast<int32_t>(a.sharedSizeBytes), static_cast<int32_t>(a.localSizeBytes), 64 * kWavesPerBlock, waves};
    return FLEX_OK;
}

int flex_gather_rows(float *dst, const float *src, const int32_t *idx, int64_t n, int k, flex_stream_t stream) {
    if (n < 0 || k <= 0) return FLEX_ERR_INVALID;
    if (n == 0) return FLEX_OK;
    if (!dst || !src || !idx) return FLEX_ERR_INVALID;
    return launch_gather_rows(dst, src, idx, n, k, reinterpret_cast<hipStream_t>(stream));
}

int flex_dropout_mask(uint64_t seed, float drop_p, uint64_t first, uint64_t count, uint8_t *keep_host) {
    if (!drop_p_ok(drop_p) || (count && !keep_host)) return FLEX_ERR_INVALID;
    const DropMask dm = drop_mask(drop_p, seed);
    for (uint64_t j = 0; j < count; ++j) keep_host[j] = dropout_bits(dm.seed_lo, dm.seed_hi, first + j) < dm.thr ? 1 : 0;
    return FLEX_OK;
}

const char *flex_strerror(int status) {
    switch (status) {
        case FLEX_OK: return "ok";
        case FLEX_ERR_INVALID: return "invalid argument";
        case FLEX_ERR_NOMEM: return "host allocation failed";
        case FLEX_ERR_HIP: return "HIP runtime call failed (see flex_last_hip_error_string)";
        case FLEX_ERR_UNSUPPORTED: return "shape not supported";
        case FLEX_ERR_IO: return "file could not be read";
        case FLEX_ERR_FORMAT: return "input does not parse as a 3-line CSR CSV";
        case FLEX_ERR_DUPLICATE: return "duplicate (row,col) entry";
        default: return "unknown flex status";
    }
}

int flex_last_hip_error(void) { return static_cast<int>(g_last_hip); }
const char *flex_last_hip_error_string(void) { return hipGetErrorString(g_last_hip); }
int flex_abi_version(void) { return FLEX_ABI_VERSION; }

}  // extern "C"
