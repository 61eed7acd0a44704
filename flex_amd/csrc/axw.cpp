// axw.cpp -- libflex_axw.so: Out = A * X * W around the engine's SpMM (include/flex_axw.h).
// ≙ run1 / run2 (cusp.cu:3-104, 106-208) with cusparseSpMM replaced by flex_spmm, cuBLAS by rocBLAS
// and row-major dense operands throughout.
#include <hip/hip_runtime.h>
#include <rocblas/rocblas.h>

#include <cmath>
#include <algorithm>
#include <cstdint>
#include <initializer_list>
#include <new>
#include <vector>

#include "../../include/flex_axw.h"
#include "device_scope.h"

extern "C" hipError_t flex_axw_gemm_launch(const float *L, const float *Wp, float *Out, int n, int dim, int c, int cp, int n_cus,
                                           hipStream_t s);  // axw_kernels.hip
extern "C" hipError_t flex_axw_dw_launch(const float *X, const float *G, float *dW, float *part, int n, int dim, int c, int cp, int n_cus,
                                         hipStream_t s);
extern "C" hipError_t flex_axw_transpose_launch(const float *W, float *Wt, int dim, int c, int ld, hipStream_t s);
extern "C" int flex_axw_dw_slices(int n, int n_cus);
extern "C" hipError_t flex_axw_gemm_bf16_launch(const flex_bf16 *L, const flex_bf16 *Wp, flex_bf16 *Out, int n, int dim, int c, int cp,
                                                int n_cus, hipStream_t s);  // axw_bf16_kernels.hip
extern "C" hipError_t flex_axw_bf16_clear_padding_launch(flex_bf16 *Out, int n, int c, int cp, hipStream_t s);
extern "C" hipError_t flex_axw_dx_bf16_launch(const flex_bf16 *G, const flex_bf16 *Wt, flex_bf16 *dX, int n, int cp, int dim, int n_cus,
                                              hipStream_t s);
extern "C" hipError_t flex_axw_bf16_transpose_launch(const flex_bf16 *W, flex_bf16 *Wt, int dim, int c, hipStream_t s);
extern "C" hipError_t flex_axw_dw_bf16_launch(const flex_bf16 *X, const flex_bf16 *G, flex_bf16 *dW, float *part, int n, int dim, int c, int cp,
                                              int n_cus, hipStream_t s);  // axw_bf16_backward_kernels.hip
extern "C" int flex_axw_dw_bf16_slices(int n, int n_cus);
extern "C" hipError_t flex_axw_gemm_bf16_wide_launch(const flex_bf16 *L, const flex_bf16 *W, flex_bf16 *Wf, flex_bf16 *Out, int n, int dim, int c,
                                                     int cp, int n_cus, hipStream_t s);  // axw_bf16_wide_kernels.hip: 256 < dim <= 4096
extern "C" hipError_t flex_axw_dx_bf16_wide_launch(const flex_bf16 *G, const flex_bf16 *Wt, flex_bf16 *dX, int n, int cp, int dim, int n_cus,
                                                   hipStream_t s);
extern "C" hipError_t flex_axw_dw_bf16_wide_launch(const flex_bf16 *X, const flex_bf16 *G, flex_bf16 *dW, float *part, int n, int dim, int c,
                                                   int cp, int n_cus, hipStream_t s);
extern "C" int flex_axw_dw_bf16_wide_slices(int n, int dim, int c, int n_cus);
extern "C" hipError_t flex_axw_gemm_bf16_root_launch(const flex_bf16 *L1, const flex_bf16 *W1, int d1, const flex_bf16 *L2, const flex_bf16 *W2,
                                                     int d2, const flex_bf16 *Cin, const float *bias, flex_bf16 *Wf, flex_bf16 *Out, int n, int c,
                                                     int cp, int n_cus, hipStream_t s);  // axw_bf16_root_kernels.hip
extern "C" hipError_t flex_axw_dx_bf16_root_launch(const flex_bf16 *G, const flex_bf16 *W, const flex_bf16 *dOut, const flex_bf16 *R,
                                                   flex_bf16 *Wf, flex_bf16 *dX, int n, int c, int cp, int dim, int n_cus, hipStream_t s);
extern "C" hipError_t flex_axw_dw_bf16_root_launch(const flex_bf16 *X, const flex_bf16 *G, const flex_bf16 *dOut, flex_bf16 *dW, flex_bf16 *dR,
                                                   float *db, float *part, int n, int dim, int c, int cp, int n_cus,
                                                   hipStream_t s);  // axw_bf16_root_backward_kernels.hip
extern "C" int flex_axw_dw_bf16_root_slices(int n, int dim, int c, int n_cus);
extern "C" hipError_t flex_axw_gemm_bf16_root_act_launch(const flex_bf16 *L1, const flex_bf16 *W1, int d1, const flex_bf16 *L2, const flex_bf16 *W2,
                                                         int d2, const flex_bf16 *Cin, const float *bias, flex_bf16 *Wf, flex_bf16 *Out, int n, int c,
                                                         int cp, int n_cus, float drop_p, uint64_t seed, hipStream_t s);  // axw_bf16_act_kernels.hip
extern "C" hipError_t flex_axw_act_grad_bf16_launch(const flex_bf16 *Out, const flex_bf16 *dOut, flex_bf16 *dZ, int n, int c, int cp, float cs,
                                                    hipStream_t s);
namespace flex_axw_bf16 {  // axw_bf16_fused_kernels.hip: order FLEX_AXW_AX_W_FUSED
int fused_tiles(int dim, int cp, bool root);
hipError_t fused_launch(const uint32_t *rowPtr, const uint32_t *col, const float *vals, const int32_t *panel_rows, const uint64_t *cost_prefix,
                        int n_panels, const flex_bf16 *X, const flex_bf16 *W, const flex_bf16 *R, const float *bias, flex_bf16 *Out, int dim, int c,
                        int cp, int relu, float drop_p, uint64_t seed, int n_workgroups, hipStream_t s);
}  // namespace flex_axw_bf16

struct flex_axw {
    int32_t n = 0;
    int n_cus = 0;
    bool use_blas = false;  // FLEX_AXW_USE_BLAS in `flags`, or a shape the MFMA kernel does not take (dim % 4 != 0, dim > 256, n < 32)
    bool a_nonfinite = false;  // A holds an inf or NaN: in order A_XW its SpMM turns the zero padding of X*W into NaN
    bool bf16 = false;  // FLEX_AXW_BF16: FLEX_PLAN_BF16 plans, the arrays below but d_part hold flex_bf16, the handle runs the _bf16 calls
    bool wide = false;  // bf16 && dim > 256: the dense half is axw_bf16_wide_kernels.hip, d_wp holds W in fragment order
    int dim = 0, c = 0, cp = 0, device = 0;
    flex_plan *plan_c = nullptr, *plan_dim = nullptr;
    float *d_xw = nullptr;  // n x cp
    float *d_ax = nullptr;  // n x dim
    float *d_wp = nullptr;  // dim x cp (W with zero columns appended; wide: the same elements as MFMA fragments)
    rocblas_handle blas = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // the fourth: FLEX_AXW_ROOT only
    // FLEX_AXW_BACKWARD only
    flex_plan *plan_t = nullptr;  // A^T at k = c (bf16: c rounded up to 8), ldb = ldc = cp
    float *d_g = nullptr;         // G = A^T dOut, n x cp; its padding columns are +0 for good (bf16: those from c rounded up to 8)
    float *d_wt = nullptr;        // W^T, cp x ld(dim), rows c .. cp-1 and columns dim .. zero (bf16: cp x dim)
    // FLEX_AXW_ROOT only (flex_bf16)
    float *d_s = nullptr;   // n x cp: A (X W) in order A_XW, the addend of the root kernel
    float *d_wf = nullptr;  // 2 dim x cp: [W; R] as MFMA fragments (axw_bf16_root_kernels.hip)
    // FLEX_AXW_FUSED only: A's CSR on the device and the panels of order FLEX_AXW_AX_W_FUSED (axw_bf16_fused_kernels.hip)
    uint32_t *d_row_ptr = nullptr, *d_col = nullptr;
    float *d_vals = nullptr;
    int32_t *d_panel_rows = nullptr;    // [n_panels][32] row ids in the handle's row order, the last panel filled with its last row
    uint64_t *d_cost_prefix = nullptr;  // [n_panels + 1]: nonzeros + kFusedRowCost a row, summed over the panels before
    int n_panels = 0;
    float *d_part = nullptr;      // dW partial sums: flex_axw_dw_slices(n, n_cus) x dim x c floats (bf16: flex_axw_dw_bf16_slices, wide: flex_axw_dw_bf16_wide_slices)
};

static thread_local int g_blas_status = 0;

namespace {

int hip_fail(hipError_t e) { return e == hipSuccess ? FLEX_OK : (e == hipErrorOutOfMemory ? FLEX_ERR_NOMEM : FLEX_ERR_HIP); }

// Columns c .. cp-1 of an n x cp row-major array := +0.0f
int zero_padding(flex_axw *h, float *Cout, hipStream_t s) {
    if (h->c == h->cp) return FLEX_OK;
    return hip_fail(hipMemset2DAsync(Cout + h->c, static_cast<size_t>(h->cp) * sizeof(float), 0, static_cast<size_t>(h->cp - h->c) * sizeof(float),
                                     static_cast<size_t>(h->n), s));
}

// C_rm[n x cp] = L_rm[n x dim] * Wp_rm[dim x cp], columns >= c of C_rm +0.0f   <=>   column-major  C^T = Wp^T * L^T.
// The MFMA kernel reads L with 16-byte loads: an L that is not 16-byte aligned goes to rocBLAS.  rocBLAS multiplies the c real
// columns only (0 x inf in Wp's zero columns would be NaN); the padding of the internal X*W was zeroed at create and is never written.
int gemm_rm(flex_axw *h, const float *L, float *Cout, hipStream_t s) {
    if (!h->use_blas && (reinterpret_cast<uintptr_t>(L) & 15) == 0)
        return hip_fail(flex_axw_gemm_launch(L, h->d_wp, Cout, h->n, h->dim, h->c, h->cp, h->n_cus, s));
    const float one = 1.0f, zero = 0.0f;
    const rocblas_status st = rocblas_sgemm(h->blas, rocblas_operation_none, rocblas_operation_none, h->c, h->n, h->dim, &one,
                                            h->d_wp, h->cp, L, h->dim, &zero, Cout, h->cp);
    if (st != rocblas_status_success) {
        g_blas_status = static_cast<int>(st);
        return FLEX_ERR_UNSUPPORTED;
    }
    return Cout == h->d_xw ? FLEX_OK : zero_padding(h, Cout, s);
}

// W -> Wp: dim rows of c elements of `es` bytes into rows of cp elements (the zero padding was written once at create)
int pad_w(flex_axw *h, const void *W, size_t es, hipStream_t s) {
    return hip_fail(hipMemcpy2DAsync(h->d_wp, h->cp * es, W, h->c * es, h->c * es, static_cast<size_t>(h->dim), hipMemcpyDeviceToDevice, s));
}

// The stage marks of a call that may be timed: mark(i) records event i, read(last, ms) waits for event `last` and sets ms[i] to the time
// from event i to event i + 1.  Neither does anything when the call is not timed.
struct Marks {
    flex_axw *h;
    hipStream_t s;
    bool timed;
    int operator()(int i) const { return timed ? hip_fail(hipEventRecord(h->ev[i], s)) : FLEX_OK; }
    int read(int last, float *ms) const {
        int rc = timed ? hip_fail(hipEventSynchronize(h->ev[last])) : FLEX_OK;
        for (int i = 0; timed && i < last && !rc; ++i) rc = hip_fail(hipEventElapsedTime(&ms[i], h->ev[i], h->ev[i + 1]));
        return rc;
    }
};

bool misaligned16(std::initializer_list<const void *> ptrs) {
    for (const void *p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & 15) return true;
    return false;
}

// the dense stage of the bf16 layer, Out = L W: the resident-W kernel on Wp (pad_w comes first) or, wide, the streamed one, which packs W
// into d_wp itself
int dense_bf16(flex_axw *h, const flex_bf16 *L, const flex_bf16 *W, flex_bf16 *Out, hipStream_t s) {
    flex_bf16 *wp = reinterpret_cast<flex_bf16 *>(h->d_wp);
    return hip_fail(h->wide ? flex_axw_gemm_bf16_wide_launch(L, W, wp, Out, h->n, h->dim, h->c, h->cp, h->n_cus, s)
                            : flex_axw_gemm_bf16_launch(L, wp, Out, h->n, h->dim, h->c, h->cp, h->n_cus, s));
}

// G = A^T dOut rounded once to bf16 (the transposed plan), for both bf16 backwards.  A non-finite A: inf x 0 = NaN in G's padding
// columns would meet the zero rows of W^T -- a NaN row of dGradX where the reference has inf -- so they are cleared
int grad_aggregate_bf16(flex_axw *h, const flex_bf16 *dOut, flex_stream_t stream) {
    flex_bf16 *g = reinterpret_cast<flex_bf16 *>(h->d_g);
    int rc = flex_spmm_bf16(h->plan_t, dOut, g, stream);
    if (!rc && h->a_nonfinite) rc = hip_fail(flex_axw_bf16_clear_padding_launch(g, h->n, h->c, h->cp, reinterpret_cast<hipStream_t>(stream)));
    return rc;
}

// the activation of flex_axw_run_root_act_bf16; drop_p_ok is the rule of the attention dropout (0 <= drop_p < 1, finite)
struct RootAct {
    float drop_p;
    uint64_t seed;
};
bool drop_p_ok(float p) { return std::isfinite(p) && p >= 0.f && p < 1.f; }

// What a row costs the fused kernel beside its nonzeros, in nonzeros: its share of the panel's MFMA chain and store, and the X row of the
// root forms.  It also makes the prefix strictly ascending, so that the kernel's cuts tile the panel list.
constexpr uint64_t kFusedRowCost = 8;

// FLEX_AXW_FUSED: A's CSR, panel_rows and panel_cost_prefix on the device.  The panels take the rows in the rank of the handle's row order.
int build_fused(flex_axw *h, const flex_csr *A, unsigned order) {
    const int64_t n = A->n;
    for (int64_t e = 0; e < A->nnz; ++e)
        if (A->col[e] >= static_cast<uint32_t>(n)) return FLEX_ERR_INVALID;
    std::vector<uint32_t> rank(static_cast<size_t>(n));
    int rc = FLEX_OK;
    if (order == FLEX_ORDER_RCM) rc = flex_order_rcm(A, rank.data());
    else if (order == FLEX_ORDER_CLUSTER) rc = flex_order_cluster(A, rank.data());
    else if (order == FLEX_ORDER_GORDER) rc = flex_order_gorder(A, 3, rank.data());
    else
        for (int64_t i = 0; i < n; ++i) rank[i] = static_cast<uint32_t>(i);
    if (rc) return rc;
    h->n_panels = static_cast<int>((n + 31) / 32);
    std::vector<int32_t> rows(static_cast<size_t>(h->n_panels) * 32, -1);
    for (int64_t i = 0; i < n; ++i) {
        if (rank[i] >= static_cast<uint32_t>(n) || rows[rank[i]] >= 0) return FLEX_ERR_INVALID;  // not a permutation
        rows[rank[i]] = static_cast<int32_t>(i);
    }
    for (size_t i = static_cast<size_t>(n); i < rows.size(); ++i) rows[i] = rows[n - 1];
    std::vector<uint64_t> prefix(static_cast<size_t>(h->n_panels) + 1, 0);
    for (int p = 0; p < h->n_panels; ++p) {
        uint64_t cost = 0;
        for (int j = 0; j < 32; ++j) cost += A->rowPtr[rows[32 * p + j] + 1] - A->rowPtr[rows[32 * p + j]] + kFusedRowCost;
        prefix[p + 1] = prefix[p] + cost;
    }
    auto upload = [&](auto **dst, const auto *src, size_t count) {
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(*src);
        int e = hip_fail(hipMalloc(reinterpret_cast<void **>(dst), bytes));
        if (!e && count) e = hip_fail(hipMemcpy(*dst, src, count * sizeof(*src), hipMemcpyHostToDevice));
        return e;
    };
    rc = upload(&h->d_row_ptr, A->rowPtr, static_cast<size_t>(n) + 1);
    if (!rc) rc = upload(&h->d_col, A->col, static_cast<size_t>(A->nnz));
    if (!rc) rc = upload(&h->d_vals, A->vals, static_cast<size_t>(A->nnz));
    if (!rc) rc = upload(&h->d_panel_rows, rows.data(), rows.size());
    if (!rc) rc = upload(&h->d_cost_prefix, prefix.data(), prefix.size());
    return rc;
}

// The launch of order FLEX_AXW_AX_W_FUSED, timed as one SpMM stage: the three run calls' whole body in that order
int run_fused(flex_axw *h, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const float *dBias, flex_bf16 *dOut, const RootAct *act,
              flex_stream_t stream, float *gemm_ms, float *spmm_ms) {
    if (!flex_axw_bf16::fused_tiles(h->dim, h->cp, dR != nullptr)) return FLEX_ERR_UNSUPPORTED;  // [W; R] and one tile do not fit in LDS
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const flex::DeviceScope on(h->device);
    int rc = hip_fail(on.error());
    const Marks mark{h, s, gemm_ms || spmm_ms};
    if (!rc) rc = mark(0);
    if (!rc)
        rc = hip_fail(flex_axw_bf16::fused_launch(h->d_row_ptr, h->d_col, h->d_vals, h->d_panel_rows, h->d_cost_prefix, h->n_panels, dX, dW, dR, dBias,
                                                  dOut, h->dim, h->c, h->cp, act != nullptr, act ? act->drop_p : 0.f, act ? act->seed : 0,
                                                  std::min(h->n_cus, h->n_panels), s));
    if (!rc) rc = mark(1);
    float ms[1] = {0.f};
    if (!rc) rc = mark.read(1, ms);
    if (!rc && mark.timed) {
        if (gemm_ms) *gemm_ms = 0.f;
        if (spmm_ms) *spmm_ms = ms[0];
    }
    return rc;
}

// The two root forwards: the stages of either order, the last of them the root kernel or, with `act`, its ReLU-and-dropout form.
int run_root(flex_axw *h, int order, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const float *dBias, flex_bf16 *dOut,
             const RootAct *act, flex_stream_t stream, float *gemm_ms, float *spmm_ms) {
    if (!h || !h->d_wf || !dX || !dW || !dR || !dOut || order < FLEX_AXW_AUTO || order > (h->d_panel_rows ? FLEX_AXW_AX_W_FUSED : FLEX_AXW_AX_W))
        return FLEX_ERR_INVALID;
    if (misaligned16({dX, dOut})) return FLEX_ERR_UNSUPPORTED;
    if (order == FLEX_AXW_AX_W_FUSED) return run_fused(h, dX, dW, dR, dBias, dOut, act, stream, gemm_ms, spmm_ms);
    if (order == FLEX_AXW_AUTO) order = h->cp <= h->dim ? FLEX_AXW_A_XW : FLEX_AXW_AX_W;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    flex_bf16 *xw = reinterpret_cast<flex_bf16 *>(h->d_xw), *ax = reinterpret_cast<flex_bf16 *>(h->d_ax);
    flex_bf16 *sum = reinterpret_cast<flex_bf16 *>(h->d_s), *wf = reinterpret_cast<flex_bf16 *>(h->d_wf);
    const flex::DeviceScope on(h->device);
    int rc = hip_fail(on.error());
    const Marks mark{h, s, gemm_ms || spmm_ms};
    auto last = [&](const flex_bf16 *L1, const flex_bf16 *W1, const flex_bf16 *L2, const flex_bf16 *W2, int d2, const flex_bf16 *Cin) {
        return hip_fail(act ? flex_axw_gemm_bf16_root_act_launch(L1, W1, h->dim, L2, W2, d2, Cin, dBias, wf, dOut, h->n, h->c, h->cp, h->n_cus,
                                                                  act->drop_p, act->seed, s)
                            : flex_axw_gemm_bf16_root_launch(L1, W1, h->dim, L2, W2, d2, Cin, dBias, wf, dOut, h->n, h->c, h->cp, h->n_cus, s));
    };
    if (!rc) rc = mark(0);
    if (order == FLEX_AXW_A_XW) {
        if (!rc && !h->wide) rc = pad_w(h, dW, sizeof(flex_bf16), s);
        if (!rc) rc = dense_bf16(h, dX, dW, xw, s);
        if (!rc) rc = mark(1);
        if (!rc) rc = flex_spmm_bf16(h->plan_c, xw, sum, stream);
        if (!rc && h->a_nonfinite) rc = hip_fail(flex_axw_bf16_clear_padding_launch(sum, h->n, h->c, h->cp, s));  // inf x 0 = NaN there
        if (!rc) rc = mark(2);
        if (!rc) rc = last(dX, dR, nullptr, nullptr, 0, sum);
    } else {
        if (!rc) rc = mark(1);  // no dense stage before the SpMM
        if (!rc) rc = flex_spmm_bf16(h->plan_dim, dX, ax, stream);
        if (!rc) rc = mark(2);
        if (!rc) rc = last(ax, dW, dX, dR, h->dim, nullptr);
    }
    if (!rc) rc = mark(3);
    float ms[3] = {0.f, 0.f, 0.f};
    if (!rc) rc = mark.read(3, ms);
    if (!rc && mark.timed) {  // the dense stages either side of the SpMM count as gemm
        if (gemm_ms) *gemm_ms = ms[0] + ms[2];
        if (spmm_ms) *spmm_ms = ms[1];
    }
    return rc;
}

// What the two root backwards refuse, before anything is enqueued; FLEX_OK: the call goes on.
int backward_root_refused(flex_axw *h, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const flex_bf16 *dOut, flex_bf16 *dGradX,
                          flex_bf16 *dGradW, flex_bf16 *dGradR, float *dGradBias) {
    if (!h || !h->bf16 || !h->plan_t || !h->d_wf || !dOut || (dGradW != nullptr) != (dGradR != nullptr) || (dGradX && (!dW || !dR)) ||
        (dGradW && !dX))
        return FLEX_ERR_INVALID;
    if (misaligned16({dOut, dGradX, dGradW, dGradR, dGradX ? dW : nullptr, dGradX ? dR : nullptr, dGradW ? dX : nullptr}))
        return FLEX_ERR_UNSUPPORTED;
    return reinterpret_cast<uintptr_t>(dGradBias) & 3 ? FLEX_ERR_UNSUPPORTED : FLEX_OK;
}

// The launches of the two root backwards, on a dOut (the activation's: its dZ) that backward_root_refused passed.
int backward_root(flex_axw *h, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const flex_bf16 *dOut, flex_bf16 *dGradX,
                  flex_bf16 *dGradW, flex_bf16 *dGradR, float *dGradBias, flex_stream_t stream) {
    if (!dGradX && !dGradW && !dGradBias) return FLEX_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    flex_bf16 *g = reinterpret_cast<flex_bf16 *>(h->d_g), *wf = reinterpret_cast<flex_bf16 *>(h->d_wf);
    const flex::DeviceScope on(h->device);
    int rc = hip_fail(on.error());
    if (!rc && (dGradX || dGradW)) rc = grad_aggregate_bf16(h, dOut, stream);  // dGradBias alone needs no G
    if (!rc && dGradX) rc = hip_fail(flex_axw_dx_bf16_root_launch(g, dW, dOut, dR, wf, dGradX, h->n, h->c, h->cp, h->dim, h->n_cus, s));
    if (!rc && (dGradW || dGradBias))
        rc = hip_fail(flex_axw_dw_bf16_root_launch(dGradW ? dX : nullptr, g, dOut, dGradW, dGradR, dGradBias, h->d_part, h->n, h->dim, h->c, h->cp,
                                                   h->n_cus, s));
    return rc;
}

}  // namespace

extern "C" {

// Whole 128-byte lines per row: a B row that starts mid-line costs every gather one extra line
// (measured, reddit shape: k=100 999 us, k=104 973 us, k=96 646 us, k=128 669 us -- DESIGN.md 3.3).
int flex_axw_ld(int c) { return c <= 0 ? 0 : (c + 31) / 32 * 32; }
int flex_axw_ld_bf16(int c) { return c <= 0 ? 0 : (c + 63) / 64 * 64; }  // the same 128 bytes, in 2-byte elements
int flex_axw_last_blas_status(void) { return g_blas_status; }

int flex_axw_destroy(flex_axw *h) {
    if (!h) return FLEX_OK;
    const flex::DeviceScope on(h->device);
    flex_plan_destroy(h->plan_c);
    flex_plan_destroy(h->plan_dim);
    flex_plan_destroy(h->plan_t);
    (void)hipFree(h->d_g);
    (void)hipFree(h->d_wt);
    (void)hipFree(h->d_part);
    (void)hipFree(h->d_row_ptr);
    (void)hipFree(h->d_col);
    (void)hipFree(h->d_vals);
    (void)hipFree(h->d_panel_rows);
    (void)hipFree(h->d_cost_prefix);
    (void)hipFree(h->d_s);
    (void)hipFree(h->d_wf);
    (void)hipFree(h->d_xw);
    (void)hipFree(h->d_ax);
    (void)hipFree(h->d_wp);
    if (h->blas) rocblas_destroy_handle(h->blas);
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
    return FLEX_OK;
}

int flex_axw_create(flex_axw **out, const flex_csr *A, int dim, int c, int device, unsigned flags) {
    if (!out) return FLEX_ERR_INVALID;
    *out = nullptr;
    if (!A || dim <= 0 || c <= 0 || device < 0 || A->m != A->n) return FLEX_ERR_INVALID;
    if (flags & FLEX_PLAN_BF16) return FLEX_ERR_INVALID;  // the bf16 layer is asked for by FLEX_AXW_BF16, which sets the plans' bit itself
    const bool bf16 = (flags & FLEX_AXW_BF16) != 0;
    // the bf16 layer has no rocBLAS path and runs the shapes of flex_axw_gemm_bf16_launch (dim <= 256) and flex_axw_gemm_bf16_wide_launch;
    // its backward writes dX in whole 32-column tiles
    if (bf16 && ((flags & FLEX_AXW_USE_BLAS) || dim % 16 != 0 || dim > 4096 || c > 256 || A->n < 32)) return FLEX_ERR_UNSUPPORTED;
    if (bf16 && (flags & FLEX_AXW_BACKWARD) && dim % 32 != 0) return FLEX_ERR_UNSUPPORTED;
    const bool root = (flags & FLEX_AXW_ROOT) != 0;
    if (root && !bf16) return FLEX_ERR_UNSUPPORTED;  // the root term is the bf16 layer's
    const bool fused = (flags & FLEX_AXW_FUSED) != 0;
    if (fused && (!bf16 || dim > 256)) return FLEX_ERR_UNSUPPORTED;  // the fused order keeps the whole W in LDS
    flex_axw *h = new (std::nothrow) flex_axw();
    if (!h) return FLEX_ERR_NOMEM;
    h->n = A->n;
    h->dim = dim;
    h->c = c;
    h->bf16 = bf16;
    h->wide = bf16 && dim > 256;
    h->cp = bf16 ? flex_axw_ld_bf16(c) : flex_axw_ld(c);
    h->device = device;
    const flex::DeviceScope on(device);
    int rc = hip_fail(on.error());
    const bool want_blas = (flags & FLEX_AXW_USE_BLAS) != 0;
    const bool backward = (flags & FLEX_AXW_BACKWARD) != 0;
    flags &= ~(FLEX_AXW_USE_BLAS | FLEX_AXW_BACKWARD | FLEX_AXW_BF16 | FLEX_AXW_ROOT | FLEX_AXW_FUSED);
    if (bf16) flags |= FLEX_PLAN_BF16;
    const size_t es = bf16 ? sizeof(flex_bf16) : sizeof(float);  // element size of the intermediates and of Wp
    if (!rc) rc = flex_plan_create(&h->plan_c, A, h->cp, device, flags);
    if (!rc) rc = flex_plan_create(&h->plan_dim, A, dim, device, flags);
    const size_t n1 = static_cast<size_t>(h->n > 0 ? h->n : 1);
    if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_xw), n1 * h->cp * es));
    if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_ax), n1 * dim * es));
    if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_wp), static_cast<size_t>(dim) * h->cp * es));
    if (!rc) rc = hip_fail(hipMemset(h->d_wp, 0, static_cast<size_t>(dim) * h->cp * es));
    if (!rc) rc = hip_fail(hipMemset(h->d_xw, 0, n1 * h->cp * es));  // its padding columns stay +0 for good
    for (int64_t e = 0; e < A->nnz && !h->a_nonfinite; ++e) h->a_nonfinite = !std::isfinite(A->vals[e]);
    for (int i = 0; i < 3 && !rc; ++i) rc = hip_fail(hipEventCreate(&h->ev[i]));
    if (root) {
        if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_s), n1 * h->cp * es));
        if (!rc) rc = hip_fail(hipMemset(h->d_s, 0, n1 * h->cp * es));
        if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_wf), static_cast<size_t>(2) * dim * h->cp * es));
        if (!rc) rc = hip_fail(hipEventCreate(&h->ev[3]));
    }
    if (!rc && !bf16 && rocblas_create_handle(&h->blas) != rocblas_status_success) rc = FLEX_ERR_UNSUPPORTED;
    if (!rc) {
        hipDeviceProp_t prop;
        rc = hip_fail(hipGetDeviceProperties(&prop, device));
        h->n_cus = prop.multiProcessorCount;
        h->use_blas = want_blas || dim % 4 != 0 || dim > 256 || h->n < 32;
    }
    if (!rc && backward && bf16) {
        // a bf16 plan takes k % 8 == 0: columns c .. k8-1 of dOut are read and of G written, the columns from k8 on stay +0 for good
        const int k8 = (c + 7) / 8 * 8;
        const size_t wt = static_cast<size_t>(h->cp) * dim;
        const int slices = h->wide ? flex_axw_dw_bf16_wide_slices(h->n, dim, c, h->n_cus) : flex_axw_dw_bf16_slices(h->n, h->n_cus);
        size_t part = static_cast<size_t>(std::max(1, slices)) * dim * c;
        if (root)  // flex_axw_backward_root_bf16's partials: [dW | dR | db] a slice, under a slice rule of their own
            part = std::max(part, static_cast<size_t>(std::max(1, flex_axw_dw_bf16_root_slices(h->n, dim, c, h->n_cus))) * (2 * static_cast<size_t>(dim) * c + c));
        rc = flex_plan_create_ld(&h->plan_t, A, k8, h->cp, h->cp, device, flags | FLEX_PLAN_TRANSPOSE);
        if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_g), n1 * h->cp * es));
        if (!rc) rc = hip_fail(hipMemset(h->d_g, 0, n1 * h->cp * es));
        if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_wt), wt * es));
        if (!rc) rc = hip_fail(hipMemset(h->d_wt, 0, wt * es));  // rows c .. cp-1 stay zero
        if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_part), part * sizeof(float)));
    } else if (!rc && backward) {
        const size_t wt = static_cast<size_t>(h->cp) * flex_axw_ld(dim);
        const size_t part = static_cast<size_t>(std::max(1, flex_axw_dw_slices(h->n, h->n_cus))) * dim * c;
        rc = flex_plan_create_ld(&h->plan_t, A, c, h->cp, h->cp, device, flags | FLEX_PLAN_TRANSPOSE);
        if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_g), n1 * h->cp * sizeof(float)));
        if (!rc) rc = hip_fail(hipMemset(h->d_g, 0, n1 * h->cp * sizeof(float)));  // its padding columns are never written
        if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_wt), wt * sizeof(float)));
        if (!rc) rc = hip_fail(hipMemset(h->d_wt, 0, wt * sizeof(float)));
        if (!rc) rc = hip_fail(hipMalloc(reinterpret_cast<void **>(&h->d_part), part * sizeof(float)));
    }
    if (!rc && fused) rc = build_fused(h, A, flags & FLEX_ORDER_MASK);
    if (rc) {
        flex_axw_destroy(h);
        return rc;
    }
    *out = h;
    return FLEX_OK;
}

int flex_axw_run(flex_axw *h, int order, const float *dX, const float *dW, float *dOut, flex_stream_t stream,
                 float *gemm_ms, float *spmm_ms) {
    if (!h || h->bf16 || !dX || !dW || !dOut || order < FLEX_AXW_AUTO || order > FLEX_AXW_AX_W) return FLEX_ERR_INVALID;
    if (h->n == 0) return FLEX_OK;
    if (order == FLEX_AXW_AUTO) order = h->cp <= h->dim ? FLEX_AXW_A_XW : FLEX_AXW_AX_W;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const flex::DeviceScope on(h->device);
    int rc = hip_fail(on.error());
    const Marks mark{h, s, gemm_ms || spmm_ms};
    if (!rc && rocblas_set_stream(h->blas, s) != rocblas_status_success) rc = FLEX_ERR_UNSUPPORTED;
    if (!rc) rc = pad_w(h, dW, sizeof(float), s);
    if (!rc) rc = mark(0);
    if (order == FLEX_AXW_A_XW) {  // run1: cusp.cu:18-75
        if (!rc) rc = gemm_rm(h, dX, h->d_xw, s);
        if (!rc) rc = mark(1);
        if (!rc) rc = flex_spmm(h->plan_c, h->d_xw, dOut, stream);
        if (!rc && h->a_nonfinite) rc = zero_padding(h, dOut, s);  // inf x 0 = NaN in the padding columns; finite A leaves them +0
        if (!rc) rc = mark(2);
    } else {  // run2: cusp.cu:121-178
        if (!rc) rc = flex_spmm(h->plan_dim, dX, h->d_ax, stream);
        if (!rc) rc = mark(1);
        if (!rc) rc = gemm_rm(h, h->d_ax, dOut, s);
        if (!rc) rc = mark(2);
    }
    float ms[2] = {0.f, 0.f};
    if (!rc) rc = mark.read(2, ms);
    if (!rc && mark.timed) {
        const bool gemm_first = order == FLEX_AXW_A_XW;
        if (gemm_ms) *gemm_ms = ms[gemm_first ? 0 : 1];
        if (spmm_ms) *spmm_ms = ms[gemm_first ? 1 : 0];
    }
    return rc;
}

// flex_axw_run on a FLEX_AXW_BF16 handle: the same two stages on flex_bf16, the dense one always axw_bf16_kernels.hip or, at dim > 256,
// axw_bf16_wide_kernels.hip (create refused every shape they do not take), the intermediate rounded to bf16 by the stage that writes it.
int flex_axw_run_bf16(flex_axw *h, int order, const flex_bf16 *dX, const flex_bf16 *dW, flex_bf16 *dOut, flex_stream_t stream,
                      float *gemm_ms, float *spmm_ms) {
    if (!h || !h->bf16 || !dX || !dW || !dOut || order < FLEX_AXW_AUTO || order > (h->d_panel_rows ? FLEX_AXW_AX_W_FUSED : FLEX_AXW_AX_W))
        return FLEX_ERR_INVALID;
    if (misaligned16({dX, dOut})) return FLEX_ERR_UNSUPPORTED;
    if (order == FLEX_AXW_AX_W_FUSED) return run_fused(h, dX, dW, nullptr, nullptr, dOut, nullptr, stream, gemm_ms, spmm_ms);
    if (order == FLEX_AXW_AUTO) order = h->cp <= h->dim ? FLEX_AXW_A_XW : FLEX_AXW_AX_W;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    flex_bf16 *xw = reinterpret_cast<flex_bf16 *>(h->d_xw), *ax = reinterpret_cast<flex_bf16 *>(h->d_ax);
    const flex::DeviceScope on(h->device);
    int rc = hip_fail(on.error());
    const Marks mark{h, s, gemm_ms || spmm_ms};
    if (!rc && !h->wide) rc = pad_w(h, dW, sizeof(flex_bf16), s);  // before the first mark and, in (A X) W, before the SpMM
    if (!rc) rc = mark(0);
    if (order == FLEX_AXW_A_XW) {
        if (!rc) rc = dense_bf16(h, dX, dW, xw, s);  // writes its padding columns as +0
        if (!rc) rc = mark(1);
        if (!rc) rc = flex_spmm_bf16(h->plan_c, xw, dOut, stream);
        if (!rc && h->a_nonfinite) rc = hip_fail(flex_axw_bf16_clear_padding_launch(dOut, h->n, h->c, h->cp, s));  // inf x 0 = NaN there
        if (!rc) rc = mark(2);
    } else {
        if (!rc) rc = flex_spmm_bf16(h->plan_dim, dX, ax, stream);
        if (!rc) rc = mark(1);
        if (!rc) rc = dense_bf16(h, ax, dW, dOut, s);
        if (!rc) rc = mark(2);
    }
    float ms[2] = {0.f, 0.f};
    if (!rc) rc = mark.read(2, ms);
    if (!rc && mark.timed) {
        const bool gemm_first = order == FLEX_AXW_A_XW;
        if (gemm_ms) *gemm_ms = ms[gemm_first ? 0 : 1];
        if (spmm_ms) *spmm_ms = ms[gemm_first ? 1 : 0];
    }
    return rc;
}

// flex_axw_run_bf16 with a root-weight term, on a handle made with FLEX_AXW_ROOT: Out = rn_bf16(A X W + X R + b).  The last stage of either
// order is one launch of axw_bf16_root_kernels.hip: in AX_W both products in one accumulator chain (L1 = A X, L2 = X), in A_XW the root
// product with A (X W) as its addend; the stages before it are flex_axw_run_bf16's own.
int flex_axw_run_root_bf16(flex_axw *h, int order, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const float *dBias,
                           flex_bf16 *dOut, flex_stream_t stream, float *gemm_ms, float *spmm_ms) {
    return run_root(h, order, dX, dW, dR, dBias, dOut, nullptr, stream, gemm_ms, spmm_ms);
}

// flex_axw_run_root_bf16 with ReLU and dropout applied to the last dense launch's accumulators before their one rounding
// (axw_bf16_act_kernels.hip); every launch before it, and the order of the graph's nodes, are that call's.
int flex_axw_run_root_act_bf16(flex_axw *h, int order, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const float *dBias,
                               flex_bf16 *dOut, float drop_p, uint64_t seed, flex_stream_t stream, float *gemm_ms, float *spmm_ms) {
    if (!drop_p_ok(drop_p)) return FLEX_ERR_INVALID;
    const RootAct act{drop_p, seed};
    return run_root(h, order, dX, dW, dR, dBias, dOut, &act, stream, gemm_ms, spmm_ms);
}

// G = A^T dOut (the transposed plan), then dGradX = G W^T and dGradW = X^T G (axw_kernels.hip; rocBLAS where the kernels do not take
// the shape or FLEX_AXW_USE_BLAS asked for it).  Everything is queued on `stream`: no allocation, no host sync.
int flex_axw_backward(flex_axw *h, const float *dX, const float *dW, const float *dOut, float *dGradX, float *dGradW, flex_stream_t stream) {
    if (!h || h->bf16 || !h->plan_t || !dOut || (dGradX && !dW) || (dGradW && !dX)) return FLEX_ERR_INVALID;
    if (h->n == 0 || (!dGradX && !dGradW)) return FLEX_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const flex::DeviceScope on(h->device);
    int rc = hip_fail(on.error());
    if (!rc && rocblas_set_stream(h->blas, s) != rocblas_status_success) rc = FLEX_ERR_UNSUPPORTED;
    if (!rc) rc = flex_spmm(h->plan_t, dOut, h->d_g, stream);  // reads columns 0 .. c-1 of dOut, writes columns 0 .. c-1 of G
    const float one = 1.0f, zero = 0.0f;
    auto blas = [&](rocblas_status st) -> int {
        if (st == rocblas_status_success) return FLEX_OK;
        g_blas_status = static_cast<int>(st);
        return FLEX_ERR_UNSUPPORTED;
    };
    if (!rc && dGradX) {
        // dGradX[n x dim] = G[n x cp] Wt[cp x dim]: the forward's MFMA kernel when dim is a whole number of 32-column tiles
        if (!h->use_blas && h->dim % 32 == 0 && h->cp <= 256 && h->n >= 32) {
            rc = hip_fail(flex_axw_transpose_launch(dW, h->d_wt, h->dim, h->c, h->dim, s));
            if (!rc) rc = hip_fail(flex_axw_gemm_launch(h->d_g, h->d_wt, dGradX, h->n, h->cp, h->dim, h->dim, h->n_cus, s));
        } else {  // column-major: dGradX^T[dim x n] = W[dim x c] G^T[c x n]
            rc = blas(rocblas_sgemm(h->blas, rocblas_operation_transpose, rocblas_operation_none, h->dim, h->n, h->c, &one, dW, h->c, h->d_g,
                                    h->cp, &zero, dGradX, h->dim));
        }
    }
    if (!rc && dGradW) {
        if (!h->use_blas && h->dim % 4 == 0 && h->dim <= 256 && h->cp <= 256 && h->n >= 32) {
            rc = hip_fail(flex_axw_dw_launch(dX, h->d_g, dGradW, h->d_part, h->n, h->dim, h->c, h->cp, h->n_cus, s));
        } else {  // column-major: dGradW^T[c x dim] = G^T[c x n] X[n x dim]
            rc = blas(rocblas_sgemm(h->blas, rocblas_operation_none, rocblas_operation_transpose, h->c, h->dim, h->n, &one, h->d_g, h->cp, dX,
                                    h->dim, &zero, dGradW, h->c));
        }
    }
    return rc;
}

// flex_axw_backward on a FLEX_AXW_BF16 handle: G = A^T dOut rounded once to bf16 (flex_spmm_bf16 on the transposed plan), then
// dGradX = G Wt on the forward's bf16 MFMA kernel and dGradW = X^T G on axw_bf16_backward_kernels.hip (at dim > 256 the launchers of
// axw_bf16_wide_kernels.hip: dX in 256-column passes, dW under its own slice rule).  Create refused every shape the kernels do not take, so there is no other path.  Everything is queued on `stream`: no allocation, no host sync.
int flex_axw_backward_bf16(flex_axw *h, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dOut, flex_bf16 *dGradX, flex_bf16 *dGradW,
                           flex_stream_t stream) {
    if (!h || !h->bf16 || !h->plan_t || !dOut || (dGradX && !dW) || (dGradW && !dX)) return FLEX_ERR_INVALID;
    if (misaligned16({dOut, dGradX, dGradW, dGradX ? dW : nullptr, dGradW ? dX : nullptr})) return FLEX_ERR_UNSUPPORTED;
    if (!dGradX && !dGradW) return FLEX_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    flex_bf16 *g = reinterpret_cast<flex_bf16 *>(h->d_g), *wt = reinterpret_cast<flex_bf16 *>(h->d_wt);
    const flex::DeviceScope on(h->device);
    int rc = hip_fail(on.error());
    if (!rc) rc = grad_aggregate_bf16(h, dOut, stream);
    if (!rc && dGradX) {
        rc = hip_fail(flex_axw_bf16_transpose_launch(dW, wt, h->dim, h->c, s));
        if (!rc) rc = hip_fail((h->wide ? flex_axw_dx_bf16_wide_launch : flex_axw_dx_bf16_launch)(g, wt, dGradX, h->n, h->cp, h->dim, h->n_cus, s));
    }
    if (!rc && dGradW)
        rc = hip_fail((h->wide ? flex_axw_dw_bf16_wide_launch : flex_axw_dw_bf16_launch)(dX, g, dGradW, h->d_part, h->n, h->dim, h->c, h->cp,
                                                                                         h->n_cus, s));
    return rc;
}

// The backward of flex_axw_run_root_bf16: G = A^T dOut as flex_axw_backward_bf16, then dGradX = rn_bf16(G W^T + dOut R^T) in one chain (the
// window form of axw_bf16_root_kernels.hip, [W^T; R^T] packed into the handle's d_wf: no d_wt and no transpose launch), and dGradW, dGradR
// and dGradBias from one pass over X (axw_bf16_root_backward_kernels.hip).  Everything is queued on `stream`: no allocation, no host sync.
int flex_axw_backward_root_bf16(flex_axw *h, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const flex_bf16 *dOut,
                                flex_bf16 *dGradX, flex_bf16 *dGradW, flex_bf16 *dGradR, float *dGradBias, flex_stream_t stream) {
    const int rc = backward_root_refused(h, dX, dW, dR, dOut, dGradX, dGradW, dGradR, dGradBias);
    return rc ? rc : backward_root(h, dX, dW, dR, dOut, dGradX, dGradW, dGradR, dGradBias, stream);
}

// The backward of flex_axw_run_root_act_bf16: one pass writes dZ = Out > 0 ? rn_bf16(dOut / (1 - drop_p)) : +0 into dWork
// (axw_bf16_act_kernels.hip: the stored Out is the mask), then flex_axw_backward_root_bf16's launches read dWork where they read dOut.
int flex_axw_backward_root_act_bf16(flex_axw *h, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const flex_bf16 *dFwdOut,
                                    const flex_bf16 *dOut, flex_bf16 *dWork, flex_bf16 *dGradX, flex_bf16 *dGradW, flex_bf16 *dGradR,
                                    float *dGradBias, float drop_p, flex_stream_t stream) {
    if (!dFwdOut || !dWork || dWork == dOut || dWork == dFwdOut || !drop_p_ok(drop_p)) return FLEX_ERR_INVALID;
    int rc = backward_root_refused(h, dX, dW, dR, dOut, dGradX, dGradW, dGradR, dGradBias);
    if (rc) return rc;
    if (misaligned16({dFwdOut, dWork})) return FLEX_ERR_UNSUPPORTED;
    if (!dGradX && !dGradW && !dGradBias) return FLEX_OK;
    const flex::DeviceScope on(h->device);
    rc = hip_fail(on.error());
    if (!rc)
        rc = hip_fail(flex_axw_act_grad_bf16_launch(dFwdOut, dOut, dWork, h->n, h->c, h->cp, 1.0f / (1.0f - drop_p),
                                                    reinterpret_cast<hipStream_t>(stream)));
    return rc ? rc : backward_root(h, dX, dW, dR, dWork, dGradX, dGradW, dGradR, dGradBias, stream);
}

// The launcher of order FLEX_AXW_AX_W_FUSED with the grid size as an argument (the run calls pass min(CUs, panels)); for tests, not part of
// flex_axw.h.  R == NULL: the plain layer (bias, relu and drop_p must then be NULL, 0 and 0); else the root forms.  hipErrorInvalidValue
// for n_workgroups <= 0, a misaligned X or Out, a handle made without FLEX_AXW_FUSED and a shape whose fragments do not fit in LDS.
hipError_t flex_axw_fused_bf16_launch(flex_axw *h, const flex_bf16 *X, const flex_bf16 *W, const flex_bf16 *R, const float *bias, flex_bf16 *Out,
                                      int relu, float drop_p, uint64_t seed, int n_workgroups, hipStream_t stream) {
    if (!h || !h->d_panel_rows) return hipErrorInvalidValue;
    const flex::DeviceScope on(h->device);
    if (on.error() != hipSuccess) return on.error();
    return flex_axw_bf16::fused_launch(h->d_row_ptr, h->d_col, h->d_vals, h->d_panel_rows, h->d_cost_prefix, h->n_panels, X, W, R, bias, Out, h->dim,
                                       h->c, h->cp, relu, drop_p, seed, n_workgroups, stream);
}

}  // extern "C"
