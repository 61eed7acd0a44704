// tests/hostsim/shim.cpp -- TEST INFRASTRUCTURE: lets the planner's HOST code run without a GPU.
// The planner (flex_amd/csrc/plan_build.cpp) ends by uploading its arrays with hipMalloc/hipMemcpy, and flex_plan_self_check
// reads that image back; linked against this file instead of the kernels, "device memory" is malloc'ed host memory, so the
// CPU suite (and the ASan/UBSan build of tools/asan_host.sh) can create every kind of plan and verify the image the kernels
// would read.  There is no compute here: every launcher reports FLEX_ERR_UNSUPPORTED, flex_spmm cannot produce a result.
// The one exception is the opt-in launch log (hostsim_launch_log(1)): while it is on, each launcher appends the name of the kernel
// instantiation the real launcher would launch -- as `nm -C` prints it, e.g. "spmm_flat_kernel<8, false, 4, 4, false>" -- and
// reports FLEX_OK, still computing nothing.  The selection below MIRRORS the rules of launch_spmm / launch_spmm_stamped / launch_fixup
// (spmm_kernels.hip), launch_tiles (tile_kernels.hip) and launch_blocks (block_kernels.hip): a change there must be made here too.
// flex_plan_set_values, flex_sddmm and flex_edge_softmax / _backward (values_kernels.hip, softmax_kernels.hip) are logged by the rules
// the real ones use -- refresh_passes, sddmm_pick and softmax_vec of internal.h -- so nothing is mirrored for them but their refusals.
// flex_spmm_bf16 is logged the same way.  The fused attention is logged the way the SpMM is: its 22 entry points are the library's own
// (attention_entry.h, included at the end of this file), and nothing of it is mirrored here but the names of the kernels its launchers launch.
// The "device memory" is counted (hostsim_live_allocations) and an allocation can be made to fail (hostsim_fail_malloc_at), so that
// a test can check that a plan gives back everything it allocated, also when its creation fails half way.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>

#include "internal.h"
#include "plan.h"

namespace {
bool g_log_on = false;
std::string g_log;  // one instantiation per line, in launch order

int logged(const char *name) {
    g_log += name;
    g_log += '\n';
    return FLEX_OK;
}

// U of launch_spmm's switch: 4 KiB in flight per wave on the narrow tiles, 8 KiB on the wide ones; 0 = no such tile
int unroll_of(int lanes_per_nz) { return lanes_per_nz == 4 || lanes_per_nz == 8 || lanes_per_nz == 16 ? 4 : lanes_per_nz == 32 || lanes_per_nz == 64 ? 8 : 0; }

int log_flat(int G, bool off32, int U, bool stamp) {
    if (U == 0) return FLEX_ERR_UNSUPPORTED;
    char name[96];
    std::snprintf(name, sizeof name, "spmm_flat_kernel<%d, %s, %d, %d, %s>", G, off32 ? "true" : "false", U, flex::kWavesPerBlock, stamp ? "true" : "false");
    return logged(name);
}
}  // namespace

namespace flex {
int launch_spmm(const PlanView &v, int lanes_per_nz, bool off32, bool vec4, const float *, float *, hipStream_t, int unroll) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    if (v.n_chunks == 0) return FLEX_OK;
    if (!vec4) return logged(off32 ? "spmm_generic_kernel<true>" : "spmm_generic_kernel<false>");
    if (unroll == 8 && (lanes_per_nz == 8 || lanes_per_nz == 16)) return log_flat(lanes_per_nz, off32, 8, false);
    return log_flat(lanes_per_nz, off32, unroll_of(lanes_per_nz), false);
}
int launch_spmm_stamped(const PlanView &v, int lanes_per_nz, bool off32, const float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    if (v.n_chunks == 0) return FLEX_OK;
    return log_flat(lanes_per_nz, off32, unroll_of(lanes_per_nz), true);
}
int launch_tiles(const TileView &tv, bool off32, const float *, float *, int, int, int, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    if (tv.n_row_tiles == 0) return FLEX_OK;
    return logged(off32 ? "spmm_tile_kernel<true>" : "spmm_tile_kernel<false>");
}
int launch_blocks(const BlockView &bv, const float *, float *, hipStream_t, bool vec4) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    if (bv.n_blocks == 0) return FLEX_OK;
    if (bv.rounds != 2 && bv.rounds != 4 && bv.rounds != 8) return FLEX_ERR_UNSUPPORTED;
    char name[64];
    std::snprintf(name, sizeof name, "%s<%u>", vec4 ? "spmm_hot_kernel" : "spmm_hot_generic_kernel", bv.rounds);
    return logged(name);
}
int launch_fixup(const float *, const SplitRow *, uint32_t n_rows, int, int, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return n_rows == 0 ? FLEX_OK : logged("spmm_fixup_kernel");
}
int launch_gather_rows(float *, const float *, const int32_t *, int64_t, int, hipStream_t) { return FLEX_ERR_UNSUPPORTED; }
int kernel_attributes(int, bool, bool, hipFuncAttributes *, int *) { return FLEX_ERR_UNSUPPORTED; }
}  // namespace flex

namespace {
int log_softmax(const flex_plan *p, bool bwd, const float *a, const float *b, float scale, float *out) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    if (!p || !p->mutable_vals) return FLEX_ERR_INVALID;
    if (!p->sm_ok) return FLEX_ERR_UNSUPPORTED;
    if (!std::isfinite(scale) || !(scale > 0.f)) return FLEX_ERR_INVALID;
    if (p->sm_entries == 0) return FLEX_OK;
    if (!a || !out || (bwd && !b)) return FLEX_ERR_INVALID;
    char name[64];
    std::snprintf(name, sizeof name, "edge_softmax_rows<%s, %s>", flex::softmax_vec(a, b, out) ? "true" : "false", bwd ? "true" : "false");
    return logged(name);
}

const char *vec_tail(const flex::AttentionPick &pick) { return pick.vec4 ? ", true" : ", false"; }
// "kernel<W, NS tail>": the (W, NS) form of attention_host.h's dispatch for the pick an entry point made
int log_form(const char *kernel, const flex::AttentionPick &pick, const char *tail) {
    char name[96];
    std::snprintf(name, sizeof name, "%s<%d, %d%s>", kernel, pick.W, pick.NS, tail);
    return logged(name);
}
template <class E>
constexpr const char *kElemTail = std::is_same_v<E, float> ? ", float" : ", unsigned short";
}  // namespace

// ---- the launchers of the fused attention (internal.h): the kernel each one's body launches in attention_*_kernels.hip, in the form of the pick
namespace flex::attention {
using Plan = const flex_plan *;  // short names for the unnamed parameters below
using Pick = const AttentionPick &;
using F = const float *;
using B = const flex_bf16 *;
int launch_rows(Plan, Pick pick, F, F, F, float, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_rows", pick, vec_tail(pick));
}
int launch_rows_backward(Plan, Pick pick, F, F, F, F, float, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_rows_backward", pick, vec_tail(pick));
}
int launch_columns_backward(Plan, Pick pick, F, F, F, F, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_columns_backward", pick, vec_tail(pick));
}
int launch_heads_rows(Plan, Pick pick, int, int, F, F, F, float, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_heads_rows", pick, "");
}
int launch_heads_rows(Plan, Pick pick, int, int, B, B, B, float, flex_bf16 *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_bf16_rows", pick, "");
}
int launch_heads_rows_backward(Plan, Pick pick, int, int, F, F, F, F, float, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_heads_rows_backward", pick, "");
}
int launch_heads_rows_backward(Plan, Pick pick, int, int, B, B, F, B, float, flex_bf16 *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_bf16_rows_backward", pick, "");
}
int launch_heads_columns_backward(Plan, Pick pick, int, int, F, F, F, F, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_heads_columns_backward", pick, "");
}
int launch_heads_columns_backward(Plan, Pick pick, int, int, B, B, F, F, flex_bf16 *, flex_bf16 *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_bf16_columns_backward", pick, "");
}
template <class E>
int launch_bias_rows(Plan, Pick pick, int, int, const E *, const E *, const E *, F, float, E *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_bias_rows", pick, kElemTail<E>);
}
template <class E>
int launch_bias_rows_backward(Plan, Pick pick, int, int, const E *, const E *, F, const E *, float, E *, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("attention_bias_rows_backward", pick, kElemTail<E>);
}
int launch_gat_rows(Plan, Pick pick, int, int, F, F, F, float, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("gat::gat_rows", pick, "");
}
int launch_gat_rows_backward(Plan, Pick pick, int, int, F, F, F, F, F, float, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("gat::gat_rows_backward", pick, "");
}
int launch_gat_columns_backward(Plan, Pick pick, int, int, F, F, F, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("gat::gat_columns_backward", pick, "");
}
// with dropout: Bias / GB NULL launches the kernels without the bias, as the real launchers decide it
template <class E>
int launch_dropout_rows(Plan, Pick pick, int, int, const E *, const E *, const E *, F Bias, float, const DropMask &, E *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("dropout::attention_dropout_rows", pick, (std::string(Bias ? ", true" : ", false") + kElemTail<E>).c_str());
}
template <class E>
int launch_dropout_rows_backward(Plan, Pick pick, int, int, const E *, const E *, F, const E *, float, const DropMask &, E *, float *GB, float *,
                                 hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("dropout::attention_dropout_rows_backward", pick, (std::string(GB ? ", true" : ", false") + kElemTail<E>).c_str());
}
template <class E>
int launch_dropout_columns_backward(Plan, Pick pick, int, int, const E *, const E *, F, F, const DropMask &, E *, E *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("dropout::attention_dropout_columns_backward", pick, kElemTail<E>);
}
int launch_gat_dropout_rows(Plan, Pick pick, int, int, F, F, F, float, const DropMask &, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("gat_dropout::gat_dropout_rows", pick, "");
}
int launch_gat_dropout_rows_backward(Plan, Pick pick, int, int, F, F, F, F, F, float, const DropMask &, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("gat_dropout::gat_dropout_rows_backward", pick, "");
}
int launch_gat_dropout_columns_backward(Plan, Pick pick, int, int, F, F, F, const DropMask &, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("gat_dropout::gat_dropout_columns_backward", pick, "");
}
// bf16 V rows: a NULL mask launches DROP off
int launch_gat_bf16_rows(Plan, Pick pick, int, int, F, F, B, float, const DropMask *dm, flex_bf16 *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("gat_bf16::gat_bf16_rows", pick, dm ? ", true" : ", false");
}
int launch_gat_bf16_rows_backward(Plan, Pick pick, int, int, F, F, B, F, B, float, const DropMask *dm, float *, float *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("gat_bf16::gat_bf16_rows_backward", pick, dm ? ", true" : ", false");
}
int launch_gat_bf16_columns_backward(Plan, Pick pick, int, int, B, F, F, const DropMask *dm, float *, flex_bf16 *, hipStream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    return log_form("gat_bf16::gat_bf16_columns_backward", pick, dm ? ", true" : ", false");
}
}  // namespace flex::attention

extern "C" {
int flex_plan_set_values(flex_plan *p, const float *dVals, flex_stream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    if (!p || !p->mutable_vals) return FLEX_ERR_INVALID;
    const int passes = flex::refresh_passes(p->d_rec.size(), p->d_seg.size());
    if (passes == 0) return FLEX_OK;
    if (!dVals && p->nnz > 0) return FLEX_ERR_INVALID;
    logged("refresh_records");
    return passes == 2 ? logged("refresh_padding") : FLEX_OK;
}
int flex_sddmm(const flex_plan *p, const float *dG, const float *dB, float *dOut, flex_stream_t) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    if (!p || !p->mutable_vals) return FLEX_ERR_INVALID;
    if (p->n_sd_groups == 0) return FLEX_OK;
    if (!dG || !dB || !dOut) return FLEX_ERR_INVALID;
    const flex::SddmmPick pick = flex::sddmm_pick(p->k, p->ldb, p->ldc, p->off32, dG, dB);
    char name[64];
    std::snprintf(name, sizeof name, "sddmm_slots<%d, %s, %s>", pick.W, pick.off32 ? "true" : "false", pick.vec4 ? "true" : "false");
    return logged(name);
}
int flex_edge_softmax(const flex_plan *p, const float *dScores, float scale, float *dOut, flex_stream_t) {
    return log_softmax(p, false, dScores, nullptr, scale, dOut);
}
int flex_edge_softmax_backward(const flex_plan *p, const float *dP, const float *dGradP, float scale, float *dGradS, flex_stream_t) {
    return log_softmax(p, true, dP, dGradP, scale, dGradS);
}
// the bf16 SpMM (spmm_bf16_kernels.hip): U is unroll_of's above, as spmm_bf16::launch has it; the refusals follow the entry point line by line
int flex_spmm_bf16(flex_plan *p, const flex_bf16 *dB, flex_bf16 *dC, flex_stream_t stream) {
    if (!g_log_on) return FLEX_ERR_UNSUPPORTED;
    if (!p || !p->bf16) return FLEX_ERR_INVALID;
    if (p->m == 0) return FLEX_OK;
    if (!dC || (!dB && p->nnz > 0)) return FLEX_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(dB) | reinterpret_cast<uintptr_t>(dC)) % 16 != 0) return FLEX_ERR_UNSUPPORTED;
    const flex::LaunchGuard guard(p, reinterpret_cast<hipStream_t>(stream));
    if (guard.begin() != FLEX_OK) return FLEX_ERR_INVALID;
    if (p->n_slots > 0) {  // spmm_bf16::launch: one wave per chunk-table entry
        const int U = unroll_of(p->lanes_per_nz);
        if (U == 0) return FLEX_ERR_UNSUPPORTED;
        char name[96];
        std::snprintf(name, sizeof name, "spmm_flat_bf16_kernel<%d, %s, %d, %d>", p->lanes_per_nz, p->off32 ? "true" : "false", U, flex::kWavesPerBlock);
        logged(name);
    }
    if (p->n_split > 0) logged("spmm_fixup_bf16_kernel");
    guard.done();
    return FLEX_OK;
}
int flex_hbm_probe(int, int64_t, int, int, double *, double *) { return FLEX_ERR_UNSUPPORTED; }
// the launch log: on != 0 turns it on, 0 off; either way it is emptied
void hostsim_launch_log(int on) {
    g_log_on = on != 0;
    g_log.clear();
}
// what was launched since the log was last emptied, one instantiation per line (valid until the next launch or hostsim_launch_log)
const char *hostsim_launch_log_read(void) { return g_log.c_str(); }
#ifdef FLEX_HOSTSIM  // malloc-backed stand-ins for the few HIP runtime calls the planner makes (bound locally: -Bsymbolic-functions)
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
static int64_t g_live = 0;      // hipMalloc successes minus hipFree calls on non-null pointers
static int64_t g_fail_at = -1;  // the g_fail_at-th hipMalloc from now reports hipErrorOutOfMemory (1 = the next one); -1 = none
hipError_t hipMalloc(void **p, size_t n) {
    *p = nullptr;
    if (g_fail_at > 0 && --g_fail_at == 0) {
        g_fail_at = -1;
        return hipErrorOutOfMemory;
    }
    *p = std::malloc(n ? n : 1);
    if (!*p) return hipErrorOutOfMemory;
    ++g_live;
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    if (p) --g_live;
    std::free(p);
    return hipSuccess;
}
// device allocations alive now (a plan that leaks one, or frees one twice, moves the count)
int64_t hostsim_live_allocations(void) { return g_live; }
// make the n-th hipMalloc from now (n >= 1) fail once with hipErrorOutOfMemory; -1 (or anything below 1) turns this off
void hostsim_fail_malloc_at(int64_t n) { g_fail_at = n > 0 ? n : -1; }
static uint64_t g_upload_hash = 1469598103934665603ull;  // FNV-1a over every byte "uploaded" since the last reset: a fingerprint of the plan image
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) {
    if (n) std::memcpy(d, s, n);
    const unsigned char *b = static_cast<const unsigned char *>(s);
    uint64_t h = g_upload_hash ^ n;
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    g_upload_hash = h;
    return hipSuccess;
}
uint64_t hostsim_upload_hash(int reset) {
    const uint64_t h = g_upload_hash;
    if (reset) g_upload_hash = 1469598103934665603ull;
    return h;
}
hipError_t hipMemset(void *d, int v, size_t n) { if (n) std::memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { if (n) std::memset(d, v, n); return hipSuccess; }  // measure_imbalance's log
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "hostsim"; }
// the in-flight guard of flex_spmm: nothing is ever in flight here
hipError_t hipStreamIsCapturing(hipStream_t, hipStreamCaptureStatus *st) { *st = hipStreamCaptureStatusNone; return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
#endif
}

#include "attention_entry.h"  // the fused attention's entry points themselves, on the launchers above
