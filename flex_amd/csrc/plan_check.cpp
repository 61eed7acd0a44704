// plan_check.cpp -- what is read back from a finished plan: the B-reuse / imbalance statistics of the planner's
// arrays, the self-check of the DEVICE image, and the measured per-CU imbalance (stamped twin of the kernel).
#include <algorithm>
#include <new>

#include "plan.h"

using namespace flex;

namespace flex {

// ≙ alpha_stats_collect (mat.cu:944-1065): distinct B rows per chunk / workgroup / XCD slice by
// stamping, and how evenly records are cut.  Padding records repeat the row's last column, so they
// change no distinct count.
void collect_stats(flex_plan *p, const RecordVec &rec, const std::vector<uint4> &chunk, int64_t split_nnz) {
    flex_plan_stats &st = p->stats;
    st = flex_plan_stats{};
    const uint32_t n_chunks = static_cast<uint32_t>(chunk.size());
    uint32_t nblk = (n_chunks + kWavesPerBlock - 1) / kWavesPerBlock;
    nblk = (nblk + kXcds - 1) / kXcds * kXcds;  // as launch_spmm cuts the grid
    const uint32_t cpx = std::max(1u, nblk / kXcds);
    const uint32_t row_bytes32 = static_cast<uint32_t>(p->ldb) * 4u;
    std::vector<uint32_t> seen_wave(p->n, 0u), seen_wg(p->n, 0u), seen_xcd(p->n, 0u);
    int64_t xcd_rec[kXcds] = {0};
    for (uint32_t c = 0; c < n_chunks; ++c) {
        const uint32_t wg = c / kWavesPerBlock;
        const uint32_t xcd = p->xcd_remap ? std::min<uint32_t>(wg / cpx, kXcds - 1) : wg % kXcds;
        const uint32_t n_rec = chunk[c].w - chunk[c].z;
        if (chunk[c].y == 0) continue;  // padding slot
        for (uint32_t z = chunk[c].z; z < chunk[c].w; ++z) {
            const uint32_t col = p->off32 ? rec[z].x / row_bytes32 : rec[z].x;
            if (seen_wave[col] != c + 1) seen_wave[col] = c + 1, st.cols_wave++;
            if (seen_wg[col] != wg + 1) seen_wg[col] = wg + 1, st.cols_wg++;
            if (seen_xcd[col] != xcd + 1) seen_xcd[col] = xcd + 1, st.cols_xcd++;
        }
        xcd_rec[xcd] += n_rec;
        st.chunk_rec_max = std::max<int64_t>(st.chunk_rec_max, n_rec);
    }
    st.records = static_cast<int64_t>(rec.size());
    st.n_workgroups = nblk;
    const double nnz = static_cast<double>(p->nnz - p->tile_nnz);  // what the vector kernel processes
    st.reuse_wave = st.cols_wave ? nnz / st.cols_wave : 0.0;
    st.reuse_wg = st.cols_wg ? nnz / st.cols_wg : 0.0;
    st.reuse_xcd = st.cols_xcd ? nnz / st.cols_xcd : 0.0;
    st.gather_bytes = 4.0 * (p->m + 1) + 8.0 * nnz + 4.0 * nnz * p->k + 4.0 * p->m * p->k;
    st.l2_bytes = 4.0 * (p->m + 1) + 8.0 * st.records + 4.0 * p->k * st.cols_xcd + 4.0 * p->m * p->k;
    st.chunk_rec_mean = p->n_chunks ? static_cast<double>(st.records) / p->n_chunks : 0.0;
    st.chunk_imb_pct = st.chunk_rec_mean > 0 ? 100.0 * st.chunk_rec_max / st.chunk_rec_mean - 100.0 : 0.0;
    const int64_t xmax = *std::max_element(xcd_rec, xcd_rec + kXcds);
    st.xcd_imb_pct = st.records ? 100.0 * xmax * kXcds / st.records - 100.0 : 0.0;
    st.split_nnz_pct = nnz > 0 ? 100.0 * split_nnz / nnz : 0.0;
    st.pad_pct = nnz > 0 ? 100.0 * (st.records - nnz) / nnz : 0.0;
    // detector report + what was routed to the MFMA kernel
    const double all = static_cast<double>(p->nnz);
    st.tile_nnz_pct_10 = all > 0 ? 100.0 * p->tile_hist[0] / all : 0.0;
    st.tile_nnz_pct_25 = all > 0 ? 100.0 * p->tile_hist[1] / all : 0.0;
    st.tile_nnz_pct_50 = all > 0 ? 100.0 * p->tile_hist[2] / all : 0.0;
    st.tile_mean_fill = p->tile_cells > 0 ? all / (1024.0 * p->tile_cells) : 0.0;
    st.mfma_tiles = p->n_tiles;
    st.mfma_nnz_pct = all > 0 ? 100.0 * p->tile_nnz / all : 0.0;
    st.lds_hot_pct_2 = p->lds_hot[0];
    st.lds_hot_pct_4 = p->lds_hot[1];
    st.lds_u_2 = p->lds_u[0];
    st.lds_u_4 = p->lds_u[1];
    p->has_stats = true;
}

// The whole of one uploaded array, read back into h.
template <class T>
static bool read_back(const DeviceArray<T> &d, std::vector<T> &h) {
    h.resize(d.size());
    return h.empty() || hipMemcpy(h.data(), d.get(), h.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess;
}

// The record stream of the DEVICE image as 8-byte records {B-row byte offset or column id, value bits}: read back as it is, or, for a
// packed plan (internal.h, PlanView::rec_packed), decoded -- the host twin of the kernels' staging step.  t_beg and chunk are the
// plan's, read back by the caller with their lengths checked; nothing else of the image is trusted: every index is bounded before it
// is used, the exception lists must be sorted by position, name no task's first record and carry a high half only, a wide chunk's
// records must lie inside `rec`, the lists and the wide records must be used up exactly, every column must be a row of B, and the
// decoded stream must have the fingerprint the planner took from its own 8-byte records.
static int load_records(const flex_plan *p, const std::vector<uint32_t> &t_beg, const std::vector<uint4> &chunk, std::vector<uint2> &rec) {
    const size_t n_rec = static_cast<size_t>(p->n_records);
    if (!p->rec_packed) {
        if (p->d_rec.size() != n_rec) return FLEX_ERR_FORMAT;
        return read_back(p->d_rec, rec) ? FLEX_OK : FLEX_ERR_HIP;
    }
    if (p->d_rec_val.size() != n_rec || p->d_rec_dcol.size() != n_rec || p->d_t_col0.size() != p->n_tasks || p->d_chunk_exc.size() != chunk.size() ||
        p->d_rec.size() != static_cast<size_t>(p->wide_records) || (p->wide_records == 0) != (p->d_rec.get() == nullptr))
        return FLEX_ERR_FORMAT;
    std::vector<float> val;
    std::vector<uint16_t> dcol;
    std::vector<uint32_t> col0;
    std::vector<uint2> cex, exc, wide;
    if (!read_back(p->d_rec_val, val) || !read_back(p->d_rec_dcol, dcol) || !read_back(p->d_t_col0, col0) || !read_back(p->d_chunk_exc, cex) ||
        !read_back(p->d_exc, exc) || !read_back(p->d_rec, wide))
        return FLEX_ERR_HIP;
    const uint32_t row_bytes32 = static_cast<uint32_t>(p->ldb) * 4u;
    rec.assign(n_rec, make_uint2(0u, 0u));
    uint64_t exc_used = 0, wide_used = 0;
    for (size_t ci = 0; ci < chunk.size(); ++ci) {
        const uint4 &c = chunk[ci];
        const uint2 ce = cex[ci];
        if (c.y == 0) {
            if (ce.x | ce.y) return FLEX_ERR_FORMAT;
            continue;
        }
        if (static_cast<uint64_t>(c.x) + c.y > p->n_tasks || c.z != t_beg[c.x] || c.w != t_beg[c.x + c.y] || c.z > c.w || c.w > n_rec) return FLEX_ERR_FORMAT;
        if (ce.y & kChunkWide) {
            if (ce.y != kChunkWide || ce.x != wide_used || wide_used + (c.w - c.z) > wide.size()) return FLEX_ERR_FORMAT;
            // a wide chunk's records start at a whole step of `rec` as well: the kernels stage them with 16-byte loads (stage_n)
            if (ce.x % (64u / static_cast<uint32_t>(p->lanes_per_nz)) != 0) return FLEX_ERR_FORMAT;
            std::copy(wide.begin() + static_cast<ptrdiff_t>(wide_used), wide.begin() + static_cast<ptrdiff_t>(wide_used + (c.w - c.z)), rec.begin() + c.z);
            wide_used += c.w - c.z;
            continue;
        }
        if (ce.x != exc_used || exc_used + ce.y > exc.size()) return FLEX_ERR_FORMAT;
        const uint2 *e = exc.data() + exc_used, *const e_end = e + ce.y;
        for (uint32_t t = c.x; t < c.x + c.y; ++t) {
            if (t_beg[t] > t_beg[t + 1] || t_beg[t + 1] > c.w) return FLEX_ERR_FORMAT;
            uint32_t col = col0[t];
            for (uint32_t i = t_beg[t]; i < t_beg[t + 1]; ++i) {
                uint32_t d = dcol[i];
                if (e < e_end && e->x == i - c.z) {
                    if (i == t_beg[t] || (e->y & 0xFFFFu) != 0 || e->y == 0) return FLEX_ERR_FORMAT;
                    d |= e->y;
                    ++e;
                }
                if (i == t_beg[t] && d != 0) return FLEX_ERR_FORMAT;
                col += d;
                if (col >= static_cast<uint64_t>(p->n)) return FLEX_ERR_FORMAT;
                rec[i] = make_uint2(p->off32 ? col * row_bytes32 : col, __builtin_bit_cast(uint32_t, val[i]));
            }
        }
        if (e != e_end) return FLEX_ERR_FORMAT;  // an entry out of order, or one that names no record of the chunk
        exc_used += ce.y;
    }
    if (exc_used != exc.size() || wide_used != wide.size()) return FLEX_ERR_FORMAT;
    uint64_t fp = 0;
    for (size_t i = 0; i < n_rec; ++i) fp += record_fp(i, rec[i]);
    return fp == p->rec_fp ? FLEX_OK : FLEX_ERR_FORMAT;
}

}  // namespace flex

extern "C" {

int flex_plan_read_records(const flex_plan *p, uint32_t *out, int64_t records) try {
    if (!p || records != p->n_records || (!out && records > 0)) return FLEX_ERR_INVALID;
    if (records == 0) return FLEX_OK;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    if (p->d_t_beg.size() != p->n_tasks + size_t(1) || p->d_chunk.size() != p->n_slots) return FLEX_ERR_FORMAT;
    std::vector<uint32_t> t_beg;
    std::vector<uint4> chunk;
    std::vector<uint2> rec;
    if (!read_back(p->d_t_beg, t_beg) || !read_back(p->d_chunk, chunk)) return FLEX_ERR_HIP;
    const int rc = load_records(p, t_beg, chunk, rec);
    if (rc) return rc;
    for (size_t i = 0; i < rec.size(); ++i) {
        out[2 * i] = rec[i].x;
        out[2 * i + 1] = rec[i].y;
    }
    return FLEX_OK;
} catch (const std::bad_alloc &) {
    return FLEX_ERR_NOMEM;
}

int flex_plan_measure_imbalance(flex_plan *p, const float *dB, float *dC, flex_stream_t stream, flex_imbalance *out) try {
    if (!p || p->bf16 || !out || !dC || (!dB && p->nnz > 0)) return FLEX_ERR_INVALID;  // no stamped twin of the bf16 kernel
    *out = flex_imbalance{};
    if (p->m == 0 || p->n_slots == 0) return FLEX_OK;
    if (!operands_vec4(p, dB, dC) || p->bk_blocks) return FLEX_ERR_UNSUPPORTED;  // the stamped twin exists for the vector kernel only (not for row blocks)
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    const size_t ktiles = (static_cast<size_t>(p->k) + 4 * p->lanes_per_nz - 1) / (4 * p->lanes_per_nz);
    const size_t words = static_cast<size_t>(p->n_slots) * ktiles * 3;
    DeviceArray<uint64_t> d_log;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc = FLEX_OK;
    std::vector<uint64_t> log(words);
    if (d_log.allocate(words) != hipSuccess) rc = FLEX_ERR_HIP;
    if (!rc && hipMemsetAsync(d_log.get(), 0, words * 8, s) != hipSuccess) rc = FLEX_ERR_HIP;
    if (!rc) {
        rc = launch_spmm_stamped(plan_view(p, p->fused_fixup, d_log.get()), p->lanes_per_nz, p->off32, dB, dC, s);
        if (rc == FLEX_OK && !p->fused_fixup) rc = launch_fixup(p->d_partial.get(), p->d_split.get(), p->n_split, p->k, p->ldc, dC, s);
        if (rc == FLEX_OK && p->n_tiles) {
            rc = launch_tiles(tile_view(p), p->off32, dB, dC, p->k, p->ldb, p->ldc, s);
        }
    }
    if (!rc && (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(log.data(), d_log.get(), words * 8, hipMemcpyDeviceToHost) != hipSuccess)) rc = FLEX_ERR_HIP;
    if (rc) return rc;
    // reduce: CU = (XCC id, SE/SH/CU bits of HW_ID [15:8]); clock = 100 MHz
    struct Acc {
        uint64_t busy = 0, first = ~0ull, last = 0;
    };
    std::vector<Acc> cu(16 * 256), xcd(16);
    uint64_t t_min = ~0ull, t_max = 0, busy_all = 0, w_max = 0;
    int64_t waves = 0;
    for (size_t i = 0; i < words; i += 3) {
        const uint64_t t0 = log[i], t1 = log[i + 1], id = log[i + 2];
        if (t1 == 0 || t1 < t0) continue;  // a padding entry of the chunk table: the wave left before the stamps
        const uint32_t x = static_cast<uint32_t>(id >> 32) & 15u, c = (static_cast<uint32_t>(id) >> 8) & 255u;
        for (Acc *a : {&cu[x * 256 + c], &xcd[x]}) {
            a->busy += t1 - t0;
            a->first = std::min(a->first, t0);
            a->last = std::max(a->last, t1);
        }
        t_min = std::min(t_min, t0);
        t_max = std::max(t_max, t1);
        busy_all += t1 - t0;
        w_max = std::max(w_max, t1 - t0);
        ++waves;
    }
    if (waves == 0) return FLEX_OK;
    auto summarise = [&](const std::vector<Acc> &v, int32_t *seen, double *busy_imb, double *end_spread) {
        uint64_t bmax = 0, bsum = 0, emin = ~0ull, emax = 0;
        int cnt = 0;
        for (const Acc &a : v) {
            if (a.last == 0) continue;
            ++cnt;
            bmax = std::max(bmax, a.busy);
            bsum += a.busy;
            emin = std::min(emin, a.last);
            emax = std::max(emax, a.last);
        }
        *seen = cnt;
        *busy_imb = bsum ? 100.0 * bmax * cnt / bsum - 100.0 : 0.0;
        *end_spread = t_max > t_min ? 100.0 * (emax - emin) / (t_max - t_min) : 0.0;
    };
    out->waves = waves;
    out->span_us = (t_max - t_min) * 0.01;
    summarise(cu, &out->cus_seen, &out->cu_busy_imb_pct, &out->cu_end_spread_pct);
    summarise(xcd, &out->xcds_seen, &out->xcd_busy_imb_pct, &out->xcd_end_spread_pct);
    out->wave_us_mean = busy_all * 0.01 / waves;
    out->wave_us_max = w_max * 0.01;
    return FLEX_OK;
} catch (const std::bad_alloc &) {
    return FLEX_ERR_NOMEM;
}

// FLEX_PLAN_MUTABLE_VALUES: the value image read back.  Every entry the plan holds sits in exactly one real record, and the multiset of
// (entry, B row) pairs the records name has the fingerprint create_common took from the caller's CSR (so each record reads its entry's
// column, after col_map); the padded runs lie inside the stream, real records first and padding after; every record's bits are what
// pad_values -- the rule the planner and the refresh share -- derives from the plan's kept values, and padding outside every run
// carries value 0 (the empty slots of a bundle); the SDDMM's items cover every real record exactly once, in groups that tile them.
// Called by flex_plan_self_check, on the plan's device, once the lengths of these arrays have been checked.
static int check_value_image(const flex_plan *p, const std::vector<uint2> &rec, uint64_t row_bytes) {
    const size_t nr = rec.size();
    std::vector<uint32_t> src, grp;
    std::vector<float> vrec;
    std::vector<uint4> seg, item;
    if (!read_back(p->d_src, src) || !read_back(p->d_vrec, vrec) || !read_back(p->d_seg, seg) || !read_back(p->d_sd_item, item) ||
        !read_back(p->d_sd_grp, grp))
        return FLEX_ERR_HIP;
    // entries: each once, the pairs' fingerprint
    std::vector<uint8_t> seen(static_cast<size_t>(p->src_nnz), 0);
    int64_t real = 0;
    uint64_t fp = 0;
    for (size_t i = 0; i < nr; ++i) {
        if (src[i] == kNoEntry) continue;
        if (src[i] >= static_cast<uint64_t>(p->src_nnz) || seen[src[i]]++) return FLEX_ERR_FORMAT;
        ++real;
        fp += entry_fp(src[i], static_cast<uint32_t>(p->off32 ? rec[i].x / row_bytes : rec[i].x));
    }
    if (real != p->nnz || fp != p->ent_fp) return FLEX_ERR_FORMAT;
    // the records' bits, derived again from the kept values by the shared rule
    std::vector<uint2> want(rec);
    for (size_t i = 0; i < nr; ++i)
        if (src[i] != kNoEntry) want[i].y = __builtin_bit_cast(uint32_t, vrec[i]);
    std::vector<uint8_t> in_run(nr, 0);
    for (const uint4 &s : seg) {
        if (s.y == 0 || s.z == 0 || s.w == 0 || s.x + (static_cast<uint64_t>(s.y) + s.z - 1) * s.w >= nr) return FLEX_ERR_FORMAT;
        for (uint64_t j = 0; j < static_cast<uint64_t>(s.y) + s.z; ++j) {
            const size_t i = s.x + j * s.w;
            if (in_run[i]++ || (src[i] == kNoEntry) != (j >= s.y)) return FLEX_ERR_FORMAT;
        }
        pad_values(want.data() + s.x, s.y, s.z, s.w);
    }
    for (size_t i = 0; i < nr; ++i) {
        if (want[i].x != rec[i].x || want[i].y != rec[i].y) return FLEX_ERR_FORMAT;
        if (src[i] == kNoEntry && !in_run[i] && rec[i].y != 0) return FLEX_ERR_FORMAT;
    }
    // the SDDMM's walk
    if (grp.front() != 0 || grp.back() != item.size()) return FLEX_ERR_FORMAT;
    for (uint32_t g = 0; g < p->n_sd_groups; ++g)
        if (grp[g] >= grp[g + 1] || grp[g + 1] - grp[g] > kSdGroupItems) return FLEX_ERR_FORMAT;
    std::vector<uint8_t> walked(nr, 0);
    for (const uint4 &it : item) {
        if (it.y == 0 || it.y > kSdItemRecords || it.z == 0 || it.w >= p->c_rows || it.x + static_cast<uint64_t>(it.y - 1) * it.z >= nr) return FLEX_ERR_FORMAT;
        for (uint32_t j = 0; j < it.y; ++j) {
            const size_t i = it.x + static_cast<size_t>(j) * it.z;
            if (src[i] == kNoEntry || walked[i]++) return FLEX_ERR_FORMAT;
        }
    }
    for (size_t i = 0; i < nr; ++i)
        if ((src[i] != kNoEntry) != (walked[i] == 1)) return FLEX_ERR_FORMAT;
    return FLEX_OK;
}

// FLEX_PLAN_MUTABLE_VALUES: the edge softmax's walk read back (internal.h, kSmWindow).  The row pointer slice is monotone, spans the
// plan's entries and has the fingerprint create_common's builder took from hostA; every entry of the plan's rows lies in exactly one
// item; an item holds whole consecutive rows -- a packed item rows that fit one window together, a wave row or a block row exactly its
// one row, which it tiles from its first entry to its last -- and every row is of the class its item treats it as; every nonempty row
// lies in exactly one item; the groups tile the wave items in order, and a group of more than one item stays within the budget.
static int check_softmax_image(const flex_plan *p) {
    std::vector<uint32_t> rp, grp;
    std::vector<uint4> item;
    if (!read_back(p->d_sm_rowptr, rp) || !read_back(p->d_sm_item, item) || !read_back(p->d_sm_grp, grp)) return FLEX_ERR_HIP;
    const size_t rows = static_cast<size_t>(p->sm_rows);
    if (rp.size() != rows + 1 || grp.size() != p->n_sm_groups + size_t(1) || item.size() != size_t(p->n_sm_wave_items) + p->n_sm_block_rows) return FLEX_ERR_FORMAT;
    uint64_t fp = 0;
    for (size_t r = 0; r <= rows; ++r) {
        if (r < rows && rp[r] > rp[r + 1]) return FLEX_ERR_FORMAT;
        fp += rowptr_fp(static_cast<uint32_t>(r), rp[r]);
    }
    if (fp != p->sm_fp || static_cast<int64_t>(rp.back() - rp.front()) != p->sm_entries || p->sm_entries != p->nnz || rp.back() > static_cast<uint64_t>(p->src_nnz)) return FLEX_ERR_FORMAT;
    if (p->sm_group_budget != softmax_group_budget(static_cast<uint64_t>(p->sm_entries))) return FLEX_ERR_FORMAT;
    std::vector<uint8_t> row_seen(rows, 0);
    int64_t covered = 0, by_class[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < item.size(); ++i) {
        const uint4 &it = item[i];
        const bool is_block = i >= p->n_sm_wave_items;
        if (it.y == 0 || it.w == 0 || static_cast<uint64_t>(it.z) + it.w > rows) return FLEX_ERR_FORMAT;
        if (rp[it.z] != it.x || static_cast<uint64_t>(it.x) + it.y != rp[it.z + it.w]) return FLEX_ERR_FORMAT;  // whole consecutive rows, first to last entry
        const bool packed = !is_block && static_cast<uint64_t>(it.x % 4u) + it.y <= kSmWindow;
        if (packed ? it.w > kSmItemRows : it.w != 1) return FLEX_ERR_FORMAT;
        for (uint32_t r = it.z; r < it.z + it.w; ++r) {
            if (row_seen[r]++) return FLEX_ERR_FORMAT;
            const uint32_t len = rp[r + 1] - rp[r];
            if (len == 0) continue;
            const int cls = softmax_row_class(rp[r], len);
            if (cls != (packed ? kSmPacked : is_block ? kSmBlockRow : kSmWaveRow)) return FLEX_ERR_FORMAT;
            ++by_class[cls];
        }
        covered += it.y;
    }
    if (covered != p->sm_entries) return FLEX_ERR_FORMAT;
    for (size_t r = 0; r < rows; ++r) {
        if (rp[r + 1] == rp[r]) ++by_class[3];
        else if (row_seen[r] != 1) return FLEX_ERR_FORMAT;
    }
    for (int c = 0; c < 4; ++c)
        if (by_class[c] != p->sm_class_rows[c]) return FLEX_ERR_FORMAT;
    // items in row order, so that the groups are runs of rows
    for (size_t i = 1; i < item.size(); ++i)
        if (i != p->n_sm_wave_items && item[i].z < item[i - 1].z + item[i - 1].w) return FLEX_ERR_FORMAT;
    if (grp.front() != 0 || grp.back() != p->n_sm_wave_items) return FLEX_ERR_FORMAT;
    for (uint32_t g = 0; g < p->n_sm_groups; ++g) {
        if (grp[g] >= grp[g + 1]) return FLEX_ERR_FORMAT;
        uint64_t e = 0;
        for (uint32_t i = grp[g]; i < grp[g + 1]; ++i) e += item[i].y;
        if (grp[g + 1] - grp[g] > 1 && e > p->sm_group_budget) return FLEX_ERR_FORMAT;
    }
    return FLEX_OK;
}

// FLEX_PLAN_ATTENTION: the walk of flex_attention read back (internal.h, kAtPass).  The row pointer slice is monotone and has the
// fingerprint the builder took from hostA; the (entry, K / V row) pairs have the fingerprint create_common took from hostA's columns;
// every row of the plan, empty ones included, lies in exactly one item (each writes its row of Out) and so does every entry; an item
// holds whole consecutive rows -- a slot item at most 64 / W rows that are all slot rows or empty, a wave or block item exactly its one
// row -- and every row is of the class its item treats it as; the groups tile the wave items in order within the budget.
static int check_attention_image(const flex_plan *p) {
    std::vector<uint32_t> rp, src, grp;
    std::vector<uint4> item;
    if (!read_back(p->d_at_rowptr, rp) || !read_back(p->d_at_src, src) || !read_back(p->d_at_item, item) || !read_back(p->d_at_grp, grp)) return FLEX_ERR_HIP;
    const size_t rows = static_cast<size_t>(p->at_rows);
    if (p->at_rows != p->m || rp.size() != rows + 1 || grp.size() != p->n_at_groups + size_t(1) || item.size() != size_t(p->n_at_wave_items) + p->n_at_block_rows) return FLEX_ERR_FORMAT;
    uint64_t fp = 0;
    for (size_t r = 0; r <= rows; ++r) {
        if (r < rows && rp[r] > rp[r + 1]) return FLEX_ERR_FORMAT;
        fp += rowptr_fp(static_cast<uint32_t>(r), rp[r]);
    }
    if (fp != p->at_fp || static_cast<int64_t>(rp.back() - rp.front()) != p->at_entries || p->at_entries != p->nnz || src.size() != static_cast<size_t>(p->at_entries)) return FLEX_ERR_FORMAT;
    uint64_t efp = 0;
    for (size_t i = 0; i < src.size(); ++i) {
        if (src[i] >= static_cast<uint64_t>(p->n)) return FLEX_ERR_FORMAT;
        efp += entry_fp(static_cast<uint32_t>(rp.front() + i), src[i]);
    }
    if (efp != p->at_ent_fp) return FLEX_ERR_FORMAT;
    if (p->at_group_budget != attention_group_budget(static_cast<uint64_t>(p->at_entries) + rows)) return FLEX_ERR_FORMAT;
    const uint32_t slots = 64u / static_cast<uint32_t>(sddmm_lanes(p->k));
    std::vector<uint8_t> row_seen(rows, 0);
    int64_t covered = 0, by_class[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < item.size(); ++i) {
        const uint4 &it = item[i];
        const bool is_block = i >= p->n_at_wave_items;
        if (it.w == 0 || static_cast<uint64_t>(it.z) + it.w > rows) return FLEX_ERR_FORMAT;
        if (rp[it.z] != it.x || static_cast<uint64_t>(it.x) + it.y != rp[it.z + it.w]) return FLEX_ERR_FORMAT;  // whole consecutive rows, first to last entry
        const bool slot_item = !is_block && (it.w > 1 || it.y <= kAtSlotRow);  // the kernel's own test
        if (slot_item ? it.w > slots : it.w != 1) return FLEX_ERR_FORMAT;
        for (uint32_t r = it.z; r < it.z + it.w; ++r) {
            if (row_seen[r]++) return FLEX_ERR_FORMAT;
            const uint32_t len = rp[r + 1] - rp[r];
            if (len == 0) {
                if (!slot_item) return FLEX_ERR_FORMAT;
                ++by_class[3];
                continue;
            }
            const int cls = attention_row_class(len);
            if (cls != (slot_item ? kAtSlot : is_block ? kAtBlock : kAtWave)) return FLEX_ERR_FORMAT;
            ++by_class[cls];
        }
        covered += it.y;
    }
    if (covered != p->at_entries) return FLEX_ERR_FORMAT;
    for (size_t r = 0; r < rows; ++r)
        if (row_seen[r] != 1) return FLEX_ERR_FORMAT;
    for (int c = 0; c < 4; ++c)
        if (by_class[c] != p->at_class_rows[c]) return FLEX_ERR_FORMAT;
    for (size_t i = 1; i < item.size(); ++i)
        if (i != p->n_at_wave_items && item[i].z < item[i - 1].z + item[i - 1].w) return FLEX_ERR_FORMAT;
    if (grp.front() != 0 || grp.back() != p->n_at_wave_items) return FLEX_ERR_FORMAT;
    for (uint32_t g = 0; g < p->n_at_groups; ++g) {
        if (grp[g] >= grp[g + 1]) return FLEX_ERR_FORMAT;
        uint64_t cost = 0;
        for (uint32_t i = grp[g]; i < grp[g + 1]; ++i) cost += static_cast<uint64_t>(item[i].y) + item[i].w;
        if (grp[g + 1] - grp[g] > 1 && cost > p->at_group_budget) return FLEX_ERR_FORMAT;
    }
    return FLEX_OK;
}

// FLEX_PLAN_ATTENTION_BACKWARD: the column walk of flex_attention_backward read back, against the first part's read-back columns (which
// check_attention_image has compared with hostA).  The column pointer is monotone and ends at the entry count; every entry index occurs
// once, under the column the first part holds for it and with a row whose range of the row pointer contains it -- and the (row, entry)
// pairs have the fingerprint create_common took from hostA, the (entry, column) pairs the first part's; within a column the entries
// ascend (the kernel's order of summation is hostA's); every column, empty ones included, lies in exactly one item of the class its
// length dictates, and the groups tile the wave items in order within the budget -- as for the rows.
static int check_attention_backward_image(const flex_plan *p) {
    std::vector<uint32_t> rp, src, cp, grp;
    std::vector<uint2> ent;
    std::vector<uint4> item;
    if (!read_back(p->d_at_rowptr, rp) || !read_back(p->d_at_src, src) || !read_back(p->d_ab_colptr, cp) || !read_back(p->d_ab_ent, ent) ||
        !read_back(p->d_ab_item, item) || !read_back(p->d_ab_grp, grp))
        return FLEX_ERR_HIP;
    const size_t cols = static_cast<size_t>(p->ab_cols), rows = static_cast<size_t>(p->at_rows);
    if (p->ab_cols != p->n || p->at_first_entry != 0 || cp.size() != cols + 1 || ent.size() != src.size() || rp.size() != rows + 1 ||
        grp.size() != p->n_ab_groups + size_t(1) || item.size() != size_t(p->n_ab_wave_items) + p->n_ab_block_cols)
        return FLEX_ERR_FORMAT;
    if (cp.front() != 0 || cp.back() != ent.size()) return FLEX_ERR_FORMAT;
    for (size_t c = 0; c < cols; ++c)
        if (cp[c] > cp[c + 1]) return FLEX_ERR_FORMAT;
    std::vector<uint8_t> seen(ent.size(), 0);
    uint64_t fp = 0, efp = 0;
    for (size_t c = 0; c < cols; ++c) {
        for (uint32_t i = cp[c]; i < cp[c + 1]; ++i) {
            const uint2 re = ent[i];
            if (re.y >= ent.size() || re.x >= rows || seen[re.y]++) return FLEX_ERR_FORMAT;
            if (src[re.y] != c || re.y < rp[re.x] || re.y >= rp[re.x + 1]) return FLEX_ERR_FORMAT;
            if (i > cp[c] && ent[i - 1].y >= re.y) return FLEX_ERR_FORMAT;
            fp += rowptr_fp(re.x, re.y);
            efp += entry_fp(re.y, static_cast<uint32_t>(c));
        }
    }
    if (fp != p->ab_fp || efp != p->at_ent_fp) return FLEX_ERR_FORMAT;
    if (p->ab_group_budget != attention_group_budget(static_cast<uint64_t>(p->at_entries) + cols)) return FLEX_ERR_FORMAT;
    const uint32_t slots = 64u / static_cast<uint32_t>(sddmm_lanes(p->k));
    std::vector<uint8_t> col_seen(cols, 0);
    int64_t covered = 0, by_class[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < item.size(); ++i) {
        const uint4 &it = item[i];
        const bool is_block = i >= p->n_ab_wave_items;
        if (it.w == 0 || static_cast<uint64_t>(it.z) + it.w > cols) return FLEX_ERR_FORMAT;
        if (cp[it.z] != it.x || static_cast<uint64_t>(it.x) + it.y != cp[it.z + it.w]) return FLEX_ERR_FORMAT;  // whole consecutive columns
        const bool slot_item = !is_block && (it.w > 1 || it.y <= kAtSlotRow);  // the kernel's own test
        if (slot_item ? it.w > slots : it.w != 1) return FLEX_ERR_FORMAT;
        for (uint32_t c = it.z; c < it.z + it.w; ++c) {
            if (col_seen[c]++) return FLEX_ERR_FORMAT;
            const uint32_t len = cp[c + 1] - cp[c];
            if (len == 0) {
                if (!slot_item) return FLEX_ERR_FORMAT;
                ++by_class[3];
                continue;
            }
            const int cls = attention_row_class(len);
            if (cls != (slot_item ? kAtSlot : is_block ? kAtBlock : kAtWave)) return FLEX_ERR_FORMAT;
            ++by_class[cls];
        }
        covered += it.y;
    }
    if (covered != p->at_entries) return FLEX_ERR_FORMAT;
    for (size_t c = 0; c < cols; ++c)
        if (col_seen[c] != 1) return FLEX_ERR_FORMAT;
    for (int c = 0; c < 4; ++c)
        if (by_class[c] != p->ab_class_cols[c]) return FLEX_ERR_FORMAT;
    for (size_t i = 1; i < item.size(); ++i)
        if (i != p->n_ab_wave_items && item[i].z < item[i - 1].z + item[i - 1].w) return FLEX_ERR_FORMAT;
    if (grp.front() != 0 || grp.back() != p->n_ab_wave_items) return FLEX_ERR_FORMAT;
    for (uint32_t g = 0; g < p->n_ab_groups; ++g) {
        if (grp[g] >= grp[g + 1]) return FLEX_ERR_FORMAT;
        uint64_t cost = 0;
        for (uint32_t i = grp[g]; i < grp[g + 1]; ++i) cost += static_cast<uint64_t>(item[i].y) + item[i].w;
        if (grp[g + 1] - grp[g] > 1 && cost > p->ab_group_budget) return FLEX_ERR_FORMAT;
    }
    return FLEX_OK;
}

// ≙ the reference's tiler round-trip (mat.cu:905-940: every entry of the pillar format exists exactly once,
// the queues are contiguous): read the plan's DEVICE image back and check that it is a partition --
// chunks tile the tasks, tasks tile the records, every record names a valid B row, every C row is written by
// exactly one task or by exactly one split row whose pieces are contiguous partial slots, padding entries of
// the chunk table are empty.  Independent of the planner's host arrays: it validates what the kernels read.
int flex_plan_self_check(const flex_plan *p) try {
    if (!p) return FLEX_ERR_INVALID;
    if (p->m == 0) return FLEX_OK;
    const DeviceScope on(p->device);
    FLEX_HIP_TRY(on.error());
    // every array is as long as the plan's counts say, before any of them is read
    const size_t n_rec = static_cast<size_t>(p->n_records), n_tasks = p->n_tasks, n_slots = p->n_slots, n_blocks = p->bk_blocks;
    if (p->d_t_beg.size() != n_tasks + 1 || p->d_t_dst.size() != n_tasks || p->d_t_aux.size() != n_tasks || p->d_chunk.size() != n_slots ||
        p->d_chunk_bd.size() != (p->n_bundles ? n_slots : 0) || p->d_split.size() != p->n_split)
        return FLEX_ERR_FORMAT;
    if (p->mutable_vals && (p->d_src.size() != n_rec || p->d_vrec.size() != n_rec || p->d_sd_grp.size() != p->n_sd_groups + size_t(1))) return FLEX_ERR_FORMAT;
    if (p->n_tiles && (p->d_rt_ptr.size() != p->n_row_tiles + size_t(1) || p->d_rt_rows.size() != 32 * size_t(p->n_row_tiles) ||
                       p->d_tile_boff.size() != 32 * size_t(p->n_tiles)))
        return FLEX_ERR_FORMAT;
    if (n_blocks && (p->d_bk_hdr.size() != n_blocks || p->d_bk_wstart.size() != n_blocks * kBkWaves ||
                     p->d_bk_brow.size() != n_blocks * p->bk_rounds * kBkRowsPerRound || p->d_bk_link.size() != p->d_bk_brow.size()))
        return FLEX_ERR_FORMAT;
    if ((p->n_bundles != 0) != (p->d_bd_rows.get() != nullptr) || (p->n_bundles != 0) != (p->d_chunk_bd.get() != nullptr)) return FLEX_ERR_FORMAT;
    std::vector<uint2> rec, t_aux, chunk_bd;
    std::vector<uint32_t> t_beg, t_dst, bd_rows;
    std::vector<uint4> chunk;
    std::vector<SplitRow> split;
    if (!read_back(p->d_t_beg, t_beg) || !read_back(p->d_t_dst, t_dst) || !read_back(p->d_chunk, chunk) ||
        !read_back(p->d_split, split) || !read_back(p->d_t_aux, t_aux) || !read_back(p->d_chunk_bd, chunk_bd) || !read_back(p->d_bd_rows, bd_rows))
        return FLEX_ERR_HIP;
    // the record stream, decoded where it is packed: everything below checks the records the kernels will see
    if (const int rc = load_records(p, t_beg, chunk, rec)) return rc;

    // tasks tile the record stream
    if (t_beg[0] != 0 || t_beg[p->n_tasks] != n_rec) return FLEX_ERR_FORMAT;
    for (uint32_t t = 0; t < p->n_tasks; ++t)
        if (t_beg[t] > t_beg[t + 1]) return FLEX_ERR_FORMAT;
    // ... in whole steps: every task, hence every chunk and every record window, starts at a multiple of S = 64 / G records.  The
    // staging step relies on it (spmm_device.h): its 16-byte loads of two 8-byte records, and the pair loads of the packed stream,
    // are aligned because a window starts at an even record on every tile of two or more slots.
    for (uint32_t t = 0; t <= p->n_tasks; ++t)
        if (t_beg[t] % (64u / static_cast<uint32_t>(p->lanes_per_nz)) != 0) return FLEX_ERR_FORMAT;
    // chunks tile the tasks (in table order, skipping the empty padding entries), each within the kernel's limits
    // ... and a chunk's bundles name consecutive groups of S entries of ITS part of bd_rows (what the wave holds in two registers per
    // lane), each bundle's records are its steps x S, and the parts of the chunks tile bd_rows
    const uint32_t S = 64u / static_cast<uint32_t>(p->lanes_per_nz);
    uint32_t next_task = 0, real = 0, bundles = 0;
    uint64_t bd_total = 0;
    std::vector<std::pair<uint32_t, uint32_t>> seen;  // real chunks as (first task, #tasks)
    std::vector<std::pair<uint32_t, uint32_t>> bd_parts;
    for (size_t ci = 0; ci < chunk.size(); ++ci) {
        const uint4 &c = chunk[ci];
        const uint2 cb = chunk_bd.empty() ? make_uint2(0u, 0u) : chunk_bd[ci];
        if (c.y == 0) {
            if (c.x | c.z | c.w | cb.x | cb.y) return FLEX_ERR_FORMAT;
            continue;
        }
        if (c.y > 63 || c.x + c.y > p->n_tasks || c.z != t_beg[c.x] || c.w != t_beg[c.x + c.y]) return FLEX_ERR_FORMAT;
        if (cb.y > kBundleRowsPerChunk || cb.y % S != 0 || static_cast<uint64_t>(cb.x) + cb.y > bd_rows.size()) return FLEX_ERR_FORMAT;
        uint32_t at = 0;
        for (uint32_t t = c.x; t < c.x + c.y; ++t) {
            if ((t_dst[t] & (kPartialFlag | kBundleFlag)) != (kPartialFlag | kBundleFlag)) continue;
            if ((t_dst[t] & ~(kPartialFlag | kBundleFlag)) != at || t_aux[t].x != cb.x + at) return FLEX_ERR_FORMAT;
            if (static_cast<uint64_t>(t_aux[t].y) * S != t_beg[t + 1] - t_beg[t]) return FLEX_ERR_FORMAT;
            at += S;
            ++bundles;
        }
        if (at != cb.y) return FLEX_ERR_FORMAT;
        if (cb.y) bd_parts.emplace_back(cb.x, cb.y);
        bd_total += cb.y;
        seen.emplace_back(c.x, c.y);
        ++real;
    }
    if (bundles != p->n_bundles || bd_total != bd_rows.size() || (S < kBundleMinSlots && bundles)) return FLEX_ERR_FORMAT;
    std::sort(bd_parts.begin(), bd_parts.end());
    uint32_t bd_next = 0;
    for (const auto &part : bd_parts) {
        if (part.first != bd_next) return FLEX_ERR_FORMAT;
        bd_next += part.second;
    }
    if (real != p->n_chunks) return FLEX_ERR_FORMAT;
    std::sort(seen.begin(), seen.end());
    for (const auto &c : seen) {
        if (c.first != next_task) return FLEX_ERR_FORMAT;
        next_task += c.second;
    }
    if (next_task != p->n_tasks) return FLEX_ERR_FORMAT;
    // records name valid B rows
    const uint64_t row_bytes = static_cast<uint64_t>(p->ldb) * 4u;
    for (const uint2 &r : rec) {
        const uint64_t col = p->off32 ? r.x / row_bytes : r.x;
        if (col >= static_cast<uint64_t>(p->n) || (p->off32 && r.x % row_bytes != 0)) return FLEX_ERR_FORMAT;
    }
    // every C row exactly once: by one task, or by one split row whose pieces own consecutive partial slots; every
    // partial slot is written by exactly one task, and that task names its row and the row's piece count (t_aux:
    // what the arrival counter is compared with).  Pieces of a row need NOT be consecutive tasks (2-D schedules).
    std::vector<uint8_t> written(static_cast<size_t>(p->c_rows), 0), slot_taken(p->n_partials, 0);
    int64_t in_bundles = 0;
    for (uint32_t t = 0; t < p->n_tasks; ++t) {
        const uint32_t d = t_dst[t];
        if ((d & (kPartialFlag | kBundleFlag)) == (kPartialFlag | kBundleFlag)) {  // a bundle: every slot a row of its own, or none
            int64_t rows_here = 0;
            for (uint32_t s2 = 0; s2 < S; ++s2) {
                const uint32_t row = bd_rows[t_aux[t].x + s2];
                if (row == kBundleNoRow || (row & kBundleZero)) {  // nothing of what this slot sums is stored: it must sum zeros
                    for (uint32_t j = 0; j < t_aux[t].y; ++j)
                        if (rec[t_beg[t] + static_cast<size_t>(j) * S + s2].y != 0) return FLEX_ERR_FORMAT;
                }
                if (row == kBundleNoRow) continue;
                const uint32_t dr = row & ~kBundleZero;
                if (dr >= p->c_rows || written[dr]++) return FLEX_ERR_FORMAT;
                ++rows_here;
            }
            if (rows_here == 0) return FLEX_ERR_FORMAT;
            in_bundles += rows_here;
        } else if (d & kPartialFlag) {
            const uint32_t ps = d & ~kPartialFlag;
            if (ps >= p->n_partials || slot_taken[ps]++) return FLEX_ERR_FORMAT;
            const uint2 a = t_aux[t];
            if (a.x >= p->n_split || a.y != split[a.x].count || ps < split[a.x].first || ps >= split[a.x].first + split[a.x].count) return FLEX_ERR_FORMAT;
        } else {
            if (d >= p->c_rows || written[d]++) return FLEX_ERR_FORMAT;
        }
    }
    for (uint8_t w : slot_taken)
        if (w != 1) return FLEX_ERR_FORMAT;
    if (in_bundles != p->bundle_rows) return FLEX_ERR_FORMAT;
    uint32_t first = 0;
    for (uint32_t i = 0; i < p->n_split; ++i) {
        const SplitRow &sr = split[i];
        if (sr.first != first || sr.count < 2 || sr.row >= p->c_rows || written[sr.row]++) return FLEX_ERR_FORMAT;
        first += sr.count;
    }
    if (first != p->n_partials) return FLEX_ERR_FORMAT;
    // dense tiles: the row-tile directory tiles the tile list, every listed C row is valid and named by one row tile only,
    // every tile column names a valid B row
    if (p->n_tiles) {
        std::vector<uint32_t> rt_ptr, rt_rows, boff;
        if (!read_back(p->d_rt_ptr, rt_ptr) || !read_back(p->d_rt_rows, rt_rows) || !read_back(p->d_tile_boff, boff)) return FLEX_ERR_HIP;
        if (rt_ptr[0] != 0 || rt_ptr[p->n_row_tiles] != p->n_tiles) return FLEX_ERR_FORMAT;
        for (uint32_t i = 0; i < p->n_row_tiles; ++i)
            if (rt_ptr[i] >= rt_ptr[i + 1]) return FLEX_ERR_FORMAT;
        std::vector<uint8_t> in_rt(static_cast<size_t>(p->c_rows), 0);
        for (uint32_t d : rt_rows) {
            if (d == 0xFFFFFFFFu) continue;
            if (d >= p->c_rows || in_rt[d]++) return FLEX_ERR_FORMAT;
        }
        for (uint32_t o : boff) {
            const uint64_t col = p->off32 ? o / row_bytes : o;
            if (col >= static_cast<uint64_t>(p->n) || (p->off32 && o % row_bytes != 0)) return FLEX_ERR_FORMAT;
        }
    }
    // hot blocks: the block table tiles hcol / cnt / the record streams, every wave's run counts add up to its stream and no run is
    // longer than one DPP row, every record names a row of its panel buffer (padding = the row of zeros with value 0), every staged
    // B row is valid, and every C row that a block adds to is a row the flat plan writes and is named by one slot only
    if (p->bk_blocks) {
        const uint32_t nb = p->bk_blocks, rounds = p->bk_rounds, P = p->bk_panel_rows, RB = rounds * kBkRowsPerRound;
        if ((rounds != 2 && rounds != 4 && rounds != 8) || P == 0 || P % 4 != 0 || P > kBkPanelMax || !p->off32) return FLEX_ERR_FORMAT;
        std::vector<uint4> hdr;
        std::vector<uint2> wstart, brec;
        std::vector<uint32_t> brow, link, cnt, hcol;
        if (!read_back(p->d_bk_hdr, hdr) || !read_back(p->d_bk_wstart, wstart) || !read_back(p->d_bk_rec, brec) || !read_back(p->d_bk_brow, brow) ||
            !read_back(p->d_bk_link, link))
            return FLEX_ERR_HIP;
        // hcol and cnt: as long as the headers just read say
        uint64_t n_cnt = 0, n_hcol = 0;
        for (const uint4 &h : hdr) n_cnt += static_cast<uint64_t>(h.w) * kBkWaves, n_hcol += static_cast<uint64_t>(h.x & 0x7FFFFFFFu) * P;
        if (n_cnt != p->d_bk_cnt.size() || n_hcol != p->d_bk_hcol.size()) return FLEX_ERR_FORMAT;
        if (!read_back(p->d_bk_cnt, cnt) || !read_back(p->d_bk_hcol, hcol)) return FLEX_ERR_HIP;
        for (uint32_t o : hcol)
            if (o % row_bytes != 0 || o / row_bytes >= static_cast<uint64_t>(p->n)) return FLEX_ERR_FORMAT;
        uint64_t at_hcol = 0, at_cnt = 0, at_step = 0;
        int64_t panels = 0, real = 0;
        std::vector<uint8_t> added(static_cast<size_t>(p->c_rows), 0);
        for (uint32_t b = 0; b < nb; ++b) {
            uint4 h = hdr[b];
            const bool chains = (h.x >> 31) != 0;
            h.x &= 0x7FFFFFFFu;
            if (h.x == 0) {
                if (h.w != 0 || chains) return FLEX_ERR_FORMAT;
            } else if (h.y != at_hcol || h.z != at_cnt || h.w != 2 * h.x || h.x > kBkMaxPanels || h.y % 4 != 0) {
                return FLEX_ERR_FORMAT;
            }
            at_hcol += static_cast<uint64_t>(h.x) * P;
            at_cnt += static_cast<uint64_t>(h.w) * kBkWaves;
            panels += h.x;
            for (uint32_t w = 0; w < kBkWaves; ++w) {
                const uint2 ws = wstart[static_cast<size_t>(b) * kBkWaves + w];
                if (ws.x != at_step) return FLEX_ERR_FORMAT;
                uint64_t pos = static_cast<uint64_t>(ws.x) * kBkSlots, steps = 0;
                for (uint32_t idx = 0; idx < h.x * kBkMaxRounds; ++idx) {  // panel-major, eight byte counts per panel (rounds beyond the block's: 0)
                    const uint32_t ph = idx / kBkMaxRounds, rd = idx % kBkMaxRounds;
                    const uint32_t n = (cnt[h.z + static_cast<size_t>(w) * h.w + 2 * ph + rd / 4] >> (8 * (rd & 3))) & 0xFFu;
                    if (rd >= rounds && n != 0) return FLEX_ERR_FORMAT;
                    if (n > kBkRunMax || pos + static_cast<uint64_t>(n) * kBkSlots > brec.size()) return FLEX_ERR_FORMAT;
                    for (uint64_t q = 0; q < static_cast<uint64_t>(n) * kBkSlots; ++q) {
                        const uint2 r = brec[pos + q];
                        if (r.x == kBkZeroRow) {
                            if (r.y != 0) return FLEX_ERR_FORMAT;
                        } else if (r.x % kBkRowBytes != 0 || r.x / kBkRowBytes >= P) {
                            return FLEX_ERR_FORMAT;
                        } else {
                            ++real;
                        }
                    }
                    pos += static_cast<uint64_t>(n) * kBkSlots;
                    steps += n;
                }
                if (steps != ws.y) return FLEX_ERR_FORMAT;
                at_step += steps;
            }
            // slots: an owner names a C row the flat plan writes, once over all blocks; the chain of a multi-part row starts at its
            // owner, runs through slots that are marked as parts and hold no row, and every such part is on exactly one chain
            std::vector<uint8_t> on_chain(RB, 0);
            bool any_link = false;
            for (uint32_t s = 0; s < RB; ++s) {
                const uint32_t row = brow[static_cast<size_t>(b) * RB + s], l = link[static_cast<size_t>(b) * RB + s];
                any_link = any_link || l != 0;
                if (l & ~(kBkLinkOwner | kBkLinkPart | 0xFFFFu)) return FLEX_ERR_FORMAT;
                if ((l & kBkLinkOwner) && ((l & kBkLinkPart) || (l & 0xFFFFu) == 0 || row == kBkEmptyRow)) return FLEX_ERR_FORMAT;
                if ((l & kBkLinkPart) && row != kBkEmptyRow) return FLEX_ERR_FORMAT;
                if (!(l & (kBkLinkOwner | kBkLinkPart)) && l != 0) return FLEX_ERR_FORMAT;
                if (row == kBkEmptyRow) continue;
                if (row >= p->c_rows || !written[row] || added[row]++) return FLEX_ERR_FORMAT;
                if (l & kBkLinkOwner) {
                    uint32_t hops = 0;
                    for (uint32_t n = l & 0xFFFFu; n != 0; n = link[static_cast<size_t>(b) * RB + n - 1] & 0xFFFFu) {
                        if (n > RB || ++hops > RB || !(link[static_cast<size_t>(b) * RB + n - 1] & kBkLinkPart) || on_chain[n - 1]++) return FLEX_ERR_FORMAT;
                    }
                }
            }
            for (uint32_t s = 0; s < RB; ++s)
                if (((link[static_cast<size_t>(b) * RB + s] & kBkLinkPart) != 0) != (on_chain[s] == 1)) return FLEX_ERR_FORMAT;
            if (any_link != chains) return FLEX_ERR_FORMAT;
        }
        if (at_step * kBkSlots != brec.size() || at_hcol != hcol.size() || at_cnt != cnt.size() || panels != p->bk_panels || real != p->bk_hot_nnz) return FLEX_ERR_FORMAT;
    }
    // a full plan (not a row shard of a mapped matrix) writes every row of C
    if (p->c_rows == p->m)
        for (uint8_t w : written)
            if (w != 1) return FLEX_ERR_FORMAT;
    if (p->mutable_vals) {
        int rc = check_value_image(p, rec, row_bytes);
        if (rc == FLEX_OK && p->sm_ok) rc = check_softmax_image(p);
        if (rc) return rc;
    }
    if (p->at_ok) {
        int rc = check_attention_image(p);
        if (rc == FLEX_OK && p->ab_ok) rc = check_attention_backward_image(p);
        if (rc) return rc;
    }
    return FLEX_OK;
} catch (const std::bad_alloc &) {
    return FLEX_ERR_NOMEM;
} catch (...) {
    return FLEX_ERR_INVALID;
}

}  // extern "C"
