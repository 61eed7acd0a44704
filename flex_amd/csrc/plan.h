// plan.h -- the plan object and what the planner's translation units share (host side only).
//
//   plan.cpp          life cycle and launch half of the C ABI (create*, flex_spmm, destroy, info), the autotuner
//   plan_build.cpp    PlanBuilder: CSR rows -> schedule -> pieces -> tasks / chunks / records -> device image
//   dense_tiles.cpp   the block-density detector and the dense-tile store of the MFMA route
//   plan_check.cpp    what is read back from a finished plan: self-check, statistics, measured imbalance
#pragma once
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#include "internal.h"

namespace flex {

// One array of a plan's device image (or a scratch buffer): owns its allocation and frees it when it goes.  size() is the length
// of the host vector it was uploaded from; the allocation holds at least one element, so an array that was uploaded is never null,
// and one that was not is empty with a null pointer.
template <class T>
class DeviceArray {
  public:
    DeviceArray() = default;
    DeviceArray(DeviceArray &&o) noexcept : ptr_(std::exchange(o.ptr_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    DeviceArray &operator=(DeviceArray o) noexcept {
        std::swap(ptr_, o.ptr_);
        std::swap(n_, o.n_);
        return *this;
    }
    ~DeviceArray() { if (ptr_) (void)hipFree(ptr_); }
    T *get() const { return ptr_; }
    size_t size() const { return n_; }
    // max(1, n) elements, not initialised (what was held before is freed)
    hipError_t allocate(size_t n) {
        *this = DeviceArray();
        const hipError_t e = hipMalloc(reinterpret_cast<void **>(&ptr_), std::max<size_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) ptr_ = nullptr;
        else n_ = n;
        return e;
    }
    // a copy of h; the bytes allocated are added to *device_bytes
    template <class A>
    int upload(const std::vector<T, A> &h, int64_t *device_bytes) {
        FLEX_HIP_TRY(allocate(h.size()));
        if (!h.empty()) FLEX_HIP_TRY(hipMemcpy(ptr_, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
        *device_bytes += static_cast<int64_t>(std::max<size_t>(h.size(), 1) * sizeof(T));
        return FLEX_OK;
    }

  private:
    T *ptr_ = nullptr;
    size_t n_ = 0;
};

// `dev` is the current device for the length of a scope: one hipGetDevice, a hipSetDevice only when the device differs, and the
// caller's device set back on exit only then.  error(): the get or set failed (the scope then changed nothing).
class DeviceScope {
  public:
    explicit DeviceScope(int dev) {
        err_ = hipGetDevice(&prev_);
        if (err_ == hipSuccess && prev_ != dev) {
            err_ = hipSetDevice(dev);
            switched_ = err_ == hipSuccess;
        }
    }
    ~DeviceScope() { if (switched_) (void)hipSetDevice(prev_); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
    hipError_t error() const { return err_; }

  private:
    int prev_ = -1;
    bool switched_ = false;
    hipError_t err_ = hipSuccess;
};

}  // namespace flex

struct flex_plan {
    int32_t m = 0, n = 0, k = 0, device = 0;
    int32_t ldb = 0, ldc = 0;  // row strides of B and C in floats (== k unless flex_plan_create_ld)
    // FLEX_PLAN_BF16: B and C are flex_bf16 and k, ldb and ldc above are in 4-byte WORDS (two elements each): the planner, the record
    // offsets, the chunk table and PlanView are those of the fp32 plan of that width.  What counts fp32 VALUES instead -- the partial-sum
    // workspace, the multiply-add estimate, what flex_plan_get_info reports -- multiplies by elems_per_word().
    bool bf16 = false;
    int elems_per_word() const { return bf16 ? 2 : 1; }
    int64_t nnz = 0;
    int lanes_per_nz = 0;
    bool off32 = false;
    bool xcd_remap = true;
    unsigned lds_extra = 0;
    bool rec_nt = false;
    uint32_t tile_group = 0;
    int unroll = 0;
    unsigned order = 0;
    // the device image (internal.h, PlanView): records (nnz + padding), tasks, the chunk table
    flex::DeviceArray<uint2> d_rec;
    flex::DeviceArray<uint32_t> d_t_beg, d_t_dst;
    flex::DeviceArray<uint2> d_t_aux;
    flex::DeviceArray<uint4> d_chunk;
    flex::DeviceArray<uint32_t> d_bd_rows;  // row bundles (internal.h, PlanView): S entries per bundle; empty when the plan has none
    flex::DeviceArray<uint2> d_chunk_bd;
    // the packed record stream (internal.h, PlanView::rec_packed): d_rec then holds the wide chunks' records only
    bool rec_packed = false;
    flex::DeviceArray<float> d_rec_val;
    flex::DeviceArray<uint16_t> d_rec_dcol;
    flex::DeviceArray<uint32_t> d_t_col0;
    flex::DeviceArray<uint2> d_chunk_exc, d_exc;
    int64_t n_records = 0;        // records of the stream (nnz - what left for tiles or blocks + padding), packed or not
    int64_t wide_records = 0;     // packed plans: records in chunks that keep the 8-byte form
    uint64_t rec_fp = 0;          // packed plans: fingerprint of the 8-byte stream the image encodes (self-check)
    uint32_t n_bundles = 0;
    int64_t bundle_rows = 0;                // rows that sit in bundles
    int64_t n_moved_pieces = 0, moved_records = 0;  // hub rows cut by schedule window (plan_build.cpp, cut_hub_rows)
    flex::DeviceArray<float> d_partial;
    flex::DeviceArray<flex::SplitRow> d_split;
    flex::DeviceArray<uint32_t> d_split_cnt;
    bool fused_fixup = false;
    bool two_d = false;  // rows cut by column panel (phases), not only by length
    // dense 32x32 tiles routed to the MFMA kernel (tile_kernels.hip)
    flex::DeviceArray<float> d_tile_a;
    flex::DeviceArray<uint32_t> d_tile_boff, d_tile_mask, d_rt_ptr, d_rt_rows;
    uint32_t n_tiles = 0, n_row_tiles = 0;
    int64_t tile_nnz = 0;
    int64_t tile_hist[3] = {0, 0, 0}, tile_cells = 0;  // detector report
    bool tile_hist_valid = false;
    uint32_t panel_rows = 0;
    // hot blocks (block_kernels.hip): the nonzeros they hold are not in the record stream above; their rows are (the flat kernel
    // writes every row, the hot kernel adds to the rows of its blocks)
    flex::DeviceArray<uint4> d_bk_hdr;
    flex::DeviceArray<uint2> d_bk_wstart, d_bk_rec;
    flex::DeviceArray<uint32_t> d_bk_cnt, d_bk_hcol, d_bk_brow, d_bk_link;
    uint32_t bk_blocks = 0, bk_rounds = 0, bk_panel_rows = 0;
    int64_t bk_rows = 0, bk_nnz = 0, bk_hot_nnz = 0, bk_hot_cols = 0, bk_panels = 0;
    uint32_t n_tasks = 0, n_chunks = 0, n_slots = 0, n_split = 0, n_partials = 0;  // n_slots: chunk table incl. padding
    int64_t c_rows = 0;       // rows of C the plan writes into (m, or hostA->m for a mapped plan)
    int64_t device_bytes = 0;
    double plan_ms = 0;
    double lds_hot[2] = {0, 0}, lds_u[2] = {0, 0};  // FLEX_PLAN_STATS: hot share and u of 480-row blocks at thr 2 / 4
    bool has_stats = false;
    flex_plan_stats stats{};
    flex_plan_tuning tuning{};  // the knobs this plan was built with, rules resolved (flex_plan_get_tuning)
    // in-flight guard of a plan that owns a split-row workspace (flex_spmm): the stream of its latest launch
    hipStream_t last_stream = nullptr;
    bool launched = false;
    // FLEX_PLAN_MUTABLE_VALUES (values_kernels.hip: flex_plan_set_values, flex_sddmm); empty / 0 on other plans
    bool mutable_vals = false;
    flex::DeviceArray<uint32_t> d_src;     // [records] entry of hostA (CSR order) each record holds; kNoEntry = padding
    flex::DeviceArray<float> d_vrec;       // [records] the current value of each real record (the plan's copy; 0 on padding)
    flex::DeviceArray<uint4> d_seg;        // padded runs {first record, real records, padding records, stride}: pad_values redoes them
    flex::DeviceArray<uint4> d_sd_item;    // SDDMM work items (internal.h, kSdItemRecords)
    flex::DeviceArray<uint32_t> d_sd_grp;  // [n_sd_groups + 1] first item of each wave's group
    uint32_t n_sd_groups = 0;
    int64_t src_nnz = 0;          // nnz of hostA: entry ids are below it
    uint64_t ent_fp = 0;          // order-free fingerprint of the (entry, B row) pairs the plan holds, taken from hostA (self-check)
    // the edge softmax's walk (internal.h, kSmWindow; softmax_kernels.hip).  Empty on a transposed plan with a row range (sm_ok false)
    bool sm_ok = false;
    flex::DeviceArray<uint32_t> d_sm_rowptr;  // [sm_rows + 1] hostA's row pointer for the rows whose softmax the plan computes
    flex::DeviceArray<uint4> d_sm_item;       // wave items (packed items and wave rows, grouped), then the block rows
    flex::DeviceArray<uint32_t> d_sm_grp;     // [n_sm_groups + 1] first item of each wave's group
    uint32_t n_sm_groups = 0, n_sm_wave_items = 0, n_sm_block_rows = 0, sm_group_budget = 0;
    int64_t sm_rows = 0, sm_entries = 0, sm_bytes = 0;
    int64_t sm_class_rows[4] = {0, 0, 0, 0};  // rows that are packed / wave rows / block rows / empty
    uint64_t sm_fp = 0;                       // fingerprint of the row pointer slice, taken from hostA (self-check)
    // FLEX_PLAN_ATTENTION: the walk of flex_attention (internal.h, kAtPass; attention_kernels.hip); empty / 0 on other plans
    bool at_ok = false;
    flex::DeviceArray<uint32_t> d_at_rowptr;  // [at_rows + 1] hostA's row pointer for the plan's rows
    flex::DeviceArray<uint32_t> d_at_src;     // [at_entries] K / V row of every entry of those rows, in hostA's CSR order (entry - the first one)
    flex::DeviceArray<uint4> d_at_item;       // wave items (slot items and wave rows, grouped), then the block rows
    flex::DeviceArray<uint32_t> d_at_grp;     // [n_at_groups + 1] first item of each wave's group
    uint32_t n_at_groups = 0, n_at_wave_items = 0, n_at_block_rows = 0, at_group_budget = 0, at_first_entry = 0;
    int64_t at_rows = 0, at_entries = 0, at_bytes = 0;
    int64_t at_class_rows[4] = {0, 0, 0, 0};  // slot rows / wave rows / block rows / empty rows
    uint64_t at_fp = 0, at_ent_fp = 0;        // fingerprints of the row pointer slice and of the (entry, K / V row) pairs, taken from hostA (self-check)
    // FLEX_PLAN_ATTENTION_BACKWARD: the column walk of flex_attention_backward (internal.h, kAtPass; attention_backward_kernels.hip),
    // the second part of the attention image; empty / 0 on other plans
    bool ab_ok = false;
    flex::DeviceArray<uint32_t> d_ab_colptr;  // [ab_cols + 1] first entry of every column of hostA in the (column, then CSR) order
    flex::DeviceArray<uint2> d_ab_ent;        // [at_entries] {row, entry index} of every entry, by column and within a column in CSR order
    flex::DeviceArray<uint4> d_ab_item;       // as d_at_item over whole columns: {first position, entries, first column, columns}
    flex::DeviceArray<uint32_t> d_ab_grp;     // [n_ab_groups + 1] first item of each wave's group
    uint32_t n_ab_groups = 0, n_ab_wave_items = 0, n_ab_block_cols = 0, ab_group_budget = 0;
    int64_t ab_cols = 0, ab_bytes = 0;
    int64_t ab_class_cols[4] = {0, 0, 0, 0};  // slot columns / wave columns / block columns / empty columns
    uint64_t ab_fp = 0;                       // fingerprint of the (row, entry) pairs, taken from hostA (self-check; the (entry, column) pairs: at_ent_fp)
};

namespace flex {


// std::vector<T>(n) zero-fills: for the record stream (8 B per nonzero) that is a single-threaded pass over gigabytes that
// the parallel fill overwrites straight away.  With this allocator resize() leaves trivial elements uninitialised, and the
// pages are first touched by the threads that fill them.
template <typename T>
struct default_init_allocator : std::allocator<T> {
    template <typename U>
    struct rebind {
        using other = default_init_allocator<U>;
    };
    template <typename U>
    void construct(U *ptr) noexcept(std::is_nothrow_default_constructible_v<U>) {
        ::new (static_cast<void *>(ptr)) U;
    }
    template <typename U, typename... Args>
    void construct(U *ptr, Args &&...args) {
        ::new (static_cast<void *>(ptr)) U(std::forward<Args>(args)...);
    }
};
using RecordVec = std::vector<uint2, default_init_allocator<uint2>>;

// The kernels' view of a finished plan.  `fused`: split rows are summed inside the launch.
inline PlanView plan_view(const flex_plan *p, bool fused, uint64_t *trace) {
    return PlanView{p->d_rec.get(), p->d_t_beg.get(), p->d_t_dst.get(), p->d_t_aux.get(), p->d_chunk.get(), p->d_partial.get(), p->d_split.get(),
                    p->d_split_cnt.get(), fused ? 1u : 0u, p->n_slots, p->k, p->ldb, p->ldc,
                    p->xcd_remap ? 1u : 0u, p->lds_extra, p->rec_nt ? 1u : 0u, p->tile_group, trace, p->d_bd_rows.get(), p->d_chunk_bd.get(),
                    p->rec_packed ? 1u : 0u, p->d_rec_val.get(), p->d_rec_dcol.get(), p->d_t_col0.get(), p->d_chunk_exc.get(), p->d_exc.get()};
}
inline BlockView block_view(const flex_plan *p) {
    return BlockView{p->d_bk_hdr.get(), p->d_bk_wstart.get(), p->d_bk_cnt.get(), p->d_bk_hcol.get(), p->d_bk_brow.get(), p->d_bk_link.get(), p->d_bk_rec.get(),
                     static_cast<uint64_t>(std::max<size_t>(p->d_bk_rec.size(), 1)),
                     p->bk_blocks, p->bk_rounds, p->bk_panel_rows, p->k, p->ldb, p->ldc, 1u};
}
inline TileView tile_view(const flex_plan *p) {
    return TileView{p->d_tile_a.get(), p->d_tile_boff.get(), p->d_tile_mask.get(), p->d_rt_ptr.get(), p->d_rt_rows.get(), p->n_row_tiles};
}
// The in-flight guard of a plan that owns a split-row workspace, shared by flex_spmm and flex_spmm_bf16.  Two launches of such a plan
// must not overlap.  Launches on ONE stream are ordered by the stream; a launch on ANOTHER stream while the stream of the latest one
// still has work pending is refused instead of silently corrupting those rows.  The check is a stream query at the moment the stream
// changes -- nothing is added to the launch path of a plan that stays on its stream (an event per launch cost the Flickr-size launches
// 2-4 us of device time each).  It is conservative: unrelated work queued behind the plan's launch on the old stream also counts as
// pending.  A launch being captured into a graph is neither checked nor remembered.
//   begin(): FLEX_ERR_INVALID = refuse, enqueue nothing;  done(): the launch went out, remember its stream.
class LaunchGuard {
  public:
    LaunchGuard(flex_plan *p, hipStream_t s) : p_(p), s_(s), on_(p->n_partials > 0) {
        if (!on_) return;
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();
        if (cap != hipStreamCaptureStatusNone) on_ = false;
    }
    int begin() const {
        if (on_ && p_->launched && s_ != p_->last_stream) {
            const hipError_t q = hipStreamQuery(p_->last_stream);
            if (q == hipErrorNotReady) return FLEX_ERR_INVALID;
            if (q != hipSuccess) (void)hipGetLastError();  // e.g. the old stream has been destroyed: nothing of ours can be pending on it
        }
        return FLEX_OK;
    }
    void done() const {
        if (!on_) return;
        p_->last_stream = s_;
        p_->launched = true;
    }

  private:
    flex_plan *p_;
    hipStream_t s_;
    bool on_;
};

// float4 path: k and both strides multiples of 4, both base addresses 16-byte aligned
inline bool operands_vec4(const flex_plan *p, const float *dB, const float *dC) {
    return (p->k % 4 == 0) && (p->ldb % 4 == 0) && (p->ldc % 4 == 0) &&
           ((reinterpret_cast<uintptr_t>(dB) | reinterpret_cast<uintptr_t>(dC)) % 16 == 0);
}

// Rows [r0,r1) of A.  col_map: B row read by column c (NULL = c).  dst_map: C row written by row r (NULL = r - r0,
// i.e. slice-local).  sched_cache (or NULL): holds the row schedule once it has been computed, so that several
// candidate plans of one matrix (autotune) order it only once.  force_G (or 0): lanes per record instead of the degree rule.
// entry_of (or NULL = identity): FLEX_PLAN_MUTABLE_VALUES, the index into the caller's CSR of entry e of A (a transposed plan's A
// is the caller's A^T, whose entries are a permutation of the caller's).
int build_plan(flex_plan *p, const flex_csr *A, int32_t r0, int32_t r1, const int32_t *col_map, const int32_t *dst_map,
               unsigned flags, const flex_plan_tuning &tuning, std::vector<uint32_t> *sched_cache = nullptr, int force_G = 0,
               const uint32_t *entry_of = nullptr);

// FLEX_PLAN_MUTABLE_VALUES: builds and uploads the edge softmax's walk over rows [r0, r1) of the row pointer `rowPtr` (hostA's)
int upload_softmax_image(flex_plan *p, const uint32_t *rowPtr, int64_t r0, int64_t r1);

// FLEX_PLAN_ATTENTION: builds and uploads the walk of flex_attention over rows [r0, r1) of A (hostA as the caller passed it);
// backward (FLEX_PLAN_ATTENTION_BACKWARD, every row of A only): the column walk of flex_attention_backward after it
int upload_attention_image(flex_plan *p, const flex_csr *A, int64_t r0, int64_t r1, bool backward = false);

// FLEX_PLAN_MUTABLE_VALUES: a term of the order-free fingerprint of the (entry, B row) pairs a plan holds (flex_plan_self_check)
inline uint64_t entry_fp(uint32_t entry, uint32_t brow) {
    uint64_t z = ((static_cast<uint64_t>(entry) << 32) | brow) + 0x9E3779B97F4A7C15ull;  // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- block-density detector (dense_tiles.cpp)
struct DenseTiles {
    std::vector<float> a;           // [T][4][64][4]
    std::vector<uint32_t> boff;     // [T][32]
    std::vector<uint32_t> mask;     // [T][32] which (row, column) cells of the tile hold an entry
    std::vector<uint32_t> rt_ptr;   // [R+1]
    std::vector<uint32_t> rt_rows;  // [R][32]
    int64_t nnz = 0;                // entries moved into tiles
    int64_t hist_nnz[3] = {0, 0, 0};
    int64_t n_cells = 0;            // (row tile, column tile) pairs with at least one entry
};
// stride > 1: look at every stride-th row tile only (thr must be 0)
int detect_dense_tiles(const flex_csr *A, int32_t r0, int32_t m, const std::vector<uint32_t> &sched, const std::vector<uint32_t> &colpos,
                       const int32_t *col_map, const int32_t *dst_map, bool off32, uint32_t row_bytes32, uint32_t thr, int64_t stride,
                       std::vector<uint8_t> &in_tile, DenseTiles &out);

// ---- hot blocks (block_plan.cpp)
struct BlockKnobs {
    uint32_t rounds = 8, panel_rows = kBkPanelMax, thr = 2, cap = 256, max_panels = 31, min_last_panel = 32, run_max = kBkRunMax;
};
struct BlockImage {  // host copy of what BlockView points at
    std::vector<uint4> hdr;
    std::vector<uint2> wstart;
    std::vector<uint32_t> cnt, hcol, brow, link;
    RecordVec rec;
    uint32_t n_blocks = 0, rounds = 0, panel_rows = 0;
    int64_t rows = 0, nnz = 0, hot_nnz = 0, hot_cols = 0, panels = 0;
    int64_t cand_nnz = 0, lost_panels = 0, lost_last = 0, lost_run = 0;  // candidates (column uses >= thr) and where some were left cold
};
// What share of the nonzeros of rows sched[...] would be HOT (their column used by >= thr nonzeros of the same block of `rows`
// schedule-consecutive rows), looked at in every `stride`-th block: the planner's cheap look before it commits to the block route.
double estimate_hot_share(const flex_csr *A, const std::vector<uint32_t> &sched, uint32_t rows, uint32_t thr, int64_t stride, double *u = nullptr);
// Rows sched[0..) of A (a row's C row: dst_map, or r - r0) into blocks.  hot_mask[e - rowPtr[r0]] = 1 for every nonzero that went
// into the block image; the caller plans the OTHER nonzeros with the flat planner.
int build_blocks(const flex_csr *A, const std::vector<uint32_t> &sched, const std::vector<uint32_t> &colpos, const int32_t *col_map,
                 const int32_t *dst_map, int32_t r0, uint32_t row_bytes32, const BlockKnobs &kn, BlockImage &img, std::vector<uint8_t> &hot_mask);

// a term of the order-free fingerprint of a record stream (packed plans: taken from the planner's 8-byte records, compared with what
// flex_plan_self_check decodes from the device image)
inline uint64_t record_fp(uint64_t index, uint2 r) {
    uint64_t z = index * 0xD6E8FEB86659FD93ull + ((static_cast<uint64_t>(r.x) << 32) | r.y) + 0x9E3779B97F4A7C15ull;  // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// ---- plan_check.cpp
void collect_stats(flex_plan *p, const RecordVec &rec, const std::vector<uint4> &chunk, int64_t split_nnz);

}  // namespace flex
