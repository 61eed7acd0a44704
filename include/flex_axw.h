/*
 * flex_axw.h -- C ABI of libflex_axw.so: the GCN layer product  Out = A * X * W  either side of the
 * SpMM.
 *
 * ≙ run1 / run2 of cusp.cu (3-104, 106-208), the AXW block of main.cu:22-77 (compiled out in the
 * reference: `//#define AXW 1`):  run1 = A*(X*W): SGEMM then SpMM at k = c;  run2 = (A*X)*W: SpMM at
 * k = dim then SGEMM.  Here the SpMM is the engine's (flex_spmm, a plan per width) instead of
 * cusparseSpMM, the dense product is a hand-written fp32 MFMA kernel for dim <= 256, dim % 4 == 0 and n >= 32
 * (axw_kernels.hip; rocBLAS SGEMM for other shapes), and all dense operands are ROW-major (the reference's are
 * column-major, cusp.cu:31-32, 55-60) so that they chain with flex_spmm without a transpose.
 * Kept in its own library: the engine (libflex_spmm.so) never depends on rocBLAS.
 */
#ifndef FLEX_AXW_H
#define FLEX_AXW_H
#include "flex_spmm.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct flex_axw flex_axw;

#define FLEX_AXW_A_XW 1 /* run1: B = X*W (n x c), Out = A*B : cheapest when c < dim */
#define FLEX_AXW_AX_W 2 /* run2: B = A*X (n x dim), Out = B*W */
#define FLEX_AXW_AUTO 0 /* the order with fewer SpMM columns (SpMM dominates both) */
#define FLEX_AXW_USE_BLAS 0x10000u /* flex_axw_create flag: rocBLAS SGEMM for the dense half instead of the hand-written MFMA kernel (tools/probe_axw.py) */
#define FLEX_AXW_BACKWARD 0x20000u /* flex_axw_create flag: also plan A^T and allocate what flex_axw_backward needs */

/* Leading dimension of Out and of the X*W intermediate: c rounded up to a multiple of 32 floats, so
 * that every row is a whole number of 128-byte cache lines (a row that starts mid-line costs each
 * gather one extra line: k=100 runs 50 % slower than k=128 on the reddit shape); the extra columns
 * come out as +0.0f, whatever the inputs hold (inf and NaN included). */
int flex_axw_ld(int c);

/* Plans A once per SpMM width (k = flex_axw_ld(c) and k = dim) and allocates the intermediates
 * (n x flex_axw_ld(c) and n x dim floats) and the padded copy of W on `device`.  `flags` as for
 * flex_plan_create (row schedule).  A must be square (a graph). */
int flex_axw_create(flex_axw **out, const flex_csr *hostA, int dim, int c, int device, unsigned flags);

/* Out[n x flex_axw_ld(c)] = A * dX[n x dim] * dW[dim x c], all device, row-major, fp32, on `stream`.
 * order: FLEX_AXW_*.  gemm_ms / spmm_ms (or NULL): device time of the two stages of THIS call; asking
 * for them makes the call synchronise.  ≙ Metrics.gemm_t / spmm_t (common.h:14-36).
 * dX may have any 4-byte alignment: in order FLEX_AXW_A_XW an X that is not 16-byte aligned is multiplied
 * by rocBLAS (the MFMA kernel loads 16 bytes at a time), correct and slower.
 * Accuracy (tests/f64ref.py): let u = 2^-24, gamma(m) = m u / (1 - m u), n_r = nnz(row r) + 32 (flex_spmm's
 * bound) and S = |A| (|X| |W|).  Every entry whose float64 reference (the product of the fp32 inputs in the
 * association order of the call: A (X W) for FLEX_AXW_A_XW, (A X) W for FLEX_AXW_AX_W) is finite is finite and
 *     |Out - ref| <= gamma(n_r + dim) S + 2^-149 (n_r + dim) (1 + sum_s |A_rs| + sum_k |W_kj|);
 * the SpMM's gamma(n_r) and the dense product's gamma(dim) compose as gamma(a) + gamma(b) + gamma(a) gamma(b)
 * <= gamma(a + b).  Every other entry is NaN / +inf / -inf exactly as that reference is (the two orders can
 * differ: X[s,k] = 0 against W[k,j] = inf is NaN in A (X W) and may be inf in (A X) W).  Both hold while no
 * stage's fp32 sum can overflow (its sum of finite |terms| < 2^120) and no finite intermediate that fp32 may
 * round to zero or to the other sign meets an inf or NaN in the next stage.  The MFMA GEMM is one fp32 fmaf
 * chain per entry in a fixed k order (axw_kernels.hip), bit for bit, signed zeros included; Out's padding
 * columns are +0.0f in every case.  Subnormal inputs and results are kept on both GEMM paths (rocBLAS included,
 * at the shapes tests/test_gpu_axw.py runs).  No residual is known. */
int flex_axw_run(flex_axw *h, int order, const float *dX, const float *dW, float *dOut, flex_stream_t stream,
                 float *gemm_ms, float *spmm_ms);

/* The layer's gradients, for a handle made with FLEX_AXW_BACKWARD (FLEX_ERR_INVALID otherwise):
 *     G = A^T dOut (one flex_spmm of the transposed plan, k = c),  dGradX[n x dim] = G W^T,  dGradW[dim x c] = X^T G,
 * all device, row-major, fp32, on `stream`.  dOut is n x flex_axw_ld(c); its padding columns are never read (NaN there has no effect).
 * dX [n x dim] and dW [dim x c] are the forward's inputs.  A NULL dGradX or dGradW skips that product, and its input (dW, resp. dX) may
 * then be NULL.  Like flex_spmm: no allocation, no host sync (safe to capture in a hipGraph); ONE call of a handle in flight at a time
 * (G and the partial sums are the handle's); the same inputs give the same bits on every call (no atomics).
 * G W^T runs on the forward's MFMA kernel (a zero-padded W^T staged by the call) when dim % 32 == 0, X^T G on its own MFMA kernel
 * (axw_kernels.hip) when dim % 4 == 0, dim <= 256; both need c <= 256 and n >= 32, and FLEX_AXW_USE_BLAS sends both to rocBLAS, as does
 * every other shape.  X is read 4 bytes at a time: any 4-byte alignment runs on the kernel.
 * X^T G: S = min(CUs, ceil(n / 256)) n-slices, each one fp32 fmaf chain per entry over its rows in ascending order, then the S partial
 * sums added in slice order: the longest chain is L_dW(n) = ceil(n / S) + S roundings.
 * Accuracy (tests/test_gpu_backward.py), in the association order A^T dOut first: with u, gamma as for flex_axw_run and
 * n_r = nnz(column r of A) + 32 (flex_spmm's bound for the rows of A^T), M = max_r n_r + L_dW,
 *     |dGradW - ref| <= gamma(M) |X|^T (|A|^T |dOut|) + 2^-149 M (1 + sum_r |X_ri|),
 *     |dGradX - ref| <= gamma(n_r + c) (|A|^T |dOut|) |W|^T + 2^-149 (n_r + c) (1 + sum_s |A_sr| + sum_j |W_ij|)   (row r),
 * the second being flex_axw_run's bound of order FLEX_AXW_AX_W for (A^T, dOut, W^T).  NaN / +inf / -inf classes are those of the
 * float64 reference, under flex_axw_run's conditions (no stage sum reaches 2^120; no finite G entry that fp32 may round to zero or to
 * the other sign meets an inf or NaN of X or W). */
int flex_axw_backward(flex_axw *h, const float *dX, const float *dW, const float *dOut, float *dGradX, float *dGradW, flex_stream_t stream);
int flex_axw_destroy(flex_axw *h);
/* last rocBLAS status seen (rocblas_status), for FLEX_ERR_UNSUPPORTED returns caused by rocBLAS */
int flex_axw_last_blas_status(void);

#ifdef __cplusplus
}
#endif
#endif
