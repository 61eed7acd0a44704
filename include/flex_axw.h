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

#define FLEX_AXW_BF16 0x200000u /* flex_axw_create flag: the bf16 layer -- X, W, Out and both intermediates are flex_bf16, the plans are
                                   FLEX_PLAN_BF16 plans and the handle runs flex_axw_run_bf16 and, made with FLEX_AXW_BACKWARD as well,
                                   flex_axw_backward_bf16 (both below) and nothing else.  Without a rocBLAS path: FLEX_ERR_UNSUPPORTED
                                   together with FLEX_AXW_USE_BLAS, for a shape its kernels do not take (dim % 16 != 0, dim > 4096,
                                   c > 256, n < 32) and, together with FLEX_AXW_BACKWARD, for dim % 32 != 0 (dGradX is written in whole
                                   32-column tiles).  dim <= 256 runs axw_bf16_kernels.hip and axw_bf16_backward_kernels.hip, 256 < dim <=
                                   4096 (the input layer of a GCN) axw_bf16_wide_kernels.hip.  A width that is no multiple of 16 (602, 1433)
                                   is served by zero columns appended to X and zero rows to W: exact, a zero product adds nothing.  The raw FLEX_PLAN_BF16 bit in `flags` stays FLEX_ERR_INVALID */

#define FLEX_AXW_ROOT 0x400000u /* flex_axw_create flag, with FLEX_AXW_BF16 only (FLEX_ERR_UNSUPPORTED without it): the handle also runs
                                   flex_axw_run_root_bf16 (below).  It only adds buffers -- a second n x flex_axw_ld_bf16(c) intermediate and
                                   2 dim x flex_axw_ld_bf16(c) elements for [W; R] as MFMA fragments; every other call behaves as on a handle
                                   made without it */

#define FLEX_AXW_FUSED 0x800000u /* flex_axw_create flag, with FLEX_AXW_BF16 only (FLEX_ERR_UNSUPPORTED without it, and for dim > 256): the handle
                                    also runs order FLEX_AXW_AX_W_FUSED of flex_axw_run_bf16, flex_axw_run_root_bf16 and
                                    flex_axw_run_root_act_bf16.  It only adds arrays -- A's CSR (rowPtr, col, vals) on the device, the 32-row
                                    panels of the handle's row order and the prefix sum of their cost; every other call and order behaves as
                                    on a handle made without it */
#define FLEX_AXW_AX_W_FUSED 3 /* an `order` of the three bf16 run calls, on a handle made with FLEX_AXW_FUSED (FLEX_ERR_INVALID on any other,
                                 like every out-of-range order): order FLEX_AXW_AX_W in ONE launch with no intermediate in memory
                                 (axw_bf16_fused_kernels.hip).  FLEX_AXW_AUTO never selects it.
                                     Out = rn_bf16( rn_bf16(A X) W )                     flex_axw_run_bf16
                                     Out = rn_bf16( act( b + rn_bf16(A X) W + X R ) )    the root calls; act: identity, or ReLU and dropout as
                                                                                         flex_axw_run_root_act_bf16 defines them (same mask)
                                 The roundings are FLEX_AXW_AX_W's: A X is summed in fp32 -- every entry ONE fmaf chain from +0 over its row's
                                 nonzeros in CSR order; a row of more than 512 nonzeros is cut into 8 ascending slices, one chain each, added in
                                 slice order -- and rounded once to bf16; the dense chain is fp32 from b (or +0), ascending k-steps of 16
                                 (v_mfma_f32_32x32x16_bf16), all of T W before all of X R, rounded once.  No atomics: the same inputs give the
                                 same bits on every call and replay.  Bit equality with FLEX_AXW_AX_W is NOT promised (flex_spmm_bf16 sums a
                                 row in another order); the accuracy statements of FLEX_AXW_AX_W hold unchanged, since their n_r = nnz(row) +
                                 32 covers any order of the row sum with one rounding per addition, the 8 slice additions included.  NaN /
                                 +inf / -inf and the +0 padding as for FLEX_AXW_AX_W, for a non-finite A too (the store masks the padding).
                                 Shapes: dim <= 256, c <= 256.  W (and R) live in LDS as dim (2 dim) x flex_axw_ld_bf16(c) elements beside
                                 tiles x 32 x (2 dim + 16) bytes of A X, 32 dim bytes of long-row partial sums and, in the root calls,
                                 4 flex_axw_ld_bf16(c) bytes of bias: two tiles (the gather of one panel overlaps the product of the one
                                 before) where that is within 160 KiB, else one; a root call that does not fit with one tile (dim = 256,
                                 c > 128) returns FLEX_ERR_UNSUPPORTED, nothing written or enqueued.  A timed call reports the launch as
                                 *spmm_ms and *gemm_ms = 0.  The call is one kernel launch: no allocation, no upload, capturable. */

/* Leading dimension of Out and of the X*W intermediate: c rounded up to a multiple of 32 floats, so
 * that every row is a whole number of 128-byte cache lines (a row that starts mid-line costs each
 * gather one extra line: k=100 runs 50 % slower than k=128 on the reddit shape); the extra columns
 * come out as +0.0f, whatever the inputs hold (inf and NaN included). */
int flex_axw_ld(int c);
/* The same for a FLEX_AXW_BF16 handle: c rounded up to a multiple of 64 elements of 2 bytes -- whole 128-byte lines again. */
int flex_axw_ld_bf16(int c);

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

/* flex_axw_run of a FLEX_AXW_BF16 handle: Out[n x flex_axw_ld_bf16(c)] = A * dX[n x dim] * dW[dim x c], all device, row-major flex_bf16
 * (the upper 16 bits of an IEEE float), on `stream`; orders, the AUTO rule (on flex_axw_ld_bf16(c) against dim) and gemm_ms / spmm_ms as
 * for flex_axw_run.  FLEX_ERR_INVALID on a handle made without FLEX_AXW_BF16, as flex_axw_run (and flex_axw_backward) are on one made with
 * it; dX and dOut must be 16-byte aligned (FLEX_ERR_UNSUPPORTED otherwise).  Nothing is enqueued in either case.
 * Definition, every bf16 operand read as the fp32 number it is, rn_bf16 = one rounding to nearest even (a NaN stays a quiet NaN, what
 * rounds past the largest finite bf16 becomes +-inf):
 *     FLEX_AXW_A_XW:  T = rn_bf16(X W in fp32),     Out = flex_spmm_bf16(A, T);
 *     FLEX_AXW_AX_W:  T = flex_spmm_bf16(A, X),     Out = rn_bf16(T W in fp32);
 * two bf16 roundings in each order.  The dense stage is the bf16 MFMA kernel of axw_bf16_kernels.hip (v_mfma_f32_32x32x16_bf16, fp32
 * accumulators, k in steps of 16 in ascending order) and, at 256 < dim <= 4096, its wide twin of axw_bf16_wide_kernels.hip (W streamed
 * through LDS in slabs of 128 k values, the same single ascending k chain per entry); there is no other path.  The accuracy statements
 * below hold unchanged over the whole range of dim (tests/test_gpu_axw_bf16_wide.py; DESIGN.md 3.28 holds the measured figures: the wide
 * GEMM alone at most 0.98 of its bound, 0.29 in the cancellation case).
 * Accuracy (tests/axw_bf16_ref.py), with u = 2^-24, gamma and n_r as for flex_axw_run and
 * bound_bf16(x, b) = b + 2^-8 (|x| + b) + 2^-134 (flex_attention_bf16's):
 *   dense stage alone:   |x32 - L W| <= g := gamma(dim) |L||W| + dim 2^-149,   |Out - L W| <= bound_bf16(L W, g);
 *   the layer: T64 the float64 first stage of the bf16 inputs, e1 its stage bound (bound_bf16(T64, g), or flex_spmm_bf16's bound), R the
 *   float64 second stage of T64, E1 = |A| e1 (A_XW) or e1 |W| (AX_W), b2 the second stage's fp32 bound at |T64| + e1
 *   (gamma(n_r) |A| (|T64| + e1) + n_r 2^-149, or gamma(dim) (|T64| + e1) |W| + dim 2^-149):
 *       |Out - R| <= bound_bf16(R, E1 + b2),
 *   NaN / +inf / -inf exactly where R has them, except that a rounding may overflow as flex_spmm_bf16 states; padding columns +0 bits
 *   in every case.  Stated for normal inputs and sums (magnitudes well above 2^-126): what the bf16 MFMA does with subnormals is
 *   recorded in DESIGN.md 3.26, not promised.
 *   gamma(dim) assumes the matrix unit's sum of the 16 products of a step rounds no more than once per addition; the cancellation case
 *   of tests/test_gpu_axw_bf16.py measures it (DESIGN.md 3.26 holds the figure). */
int flex_axw_run_bf16(flex_axw *h, int order, const flex_bf16 *dX, const flex_bf16 *dW, flex_bf16 *dOut, flex_stream_t stream,
                      float *gemm_ms, float *spmm_ms);

/* The bf16 layer with a root-weight (self) term and a bias, the layer of GraphSAGE, GraphConv, GIN and residual GCNs, on a handle made
 * with FLEX_AXW_BF16 | FLEX_AXW_ROOT (FLEX_ERR_INVALID on any other):
 *     Out[n x flex_axw_ld_bf16(c)] = A dX dW + dX dR + dBias
 * dX [n x dim], dW and dR [dim x c] flex_bf16, dBias c floats (fp32, like the other per-column operands of this library) or NULL, all
 * device, row-major, on `stream`; orders, the AUTO rule and the alignment of dX and dOut as for flex_axw_run_bf16; gemm_ms is the sum of
 * the dense stages, spmm_ms the SpMM's.  No allocation, no host sync unless timed, no atomics: the same inputs give the same bits on
 * every call, and on every replay of a hipGraph it was captured into; ONE call of a handle in flight at a time.  Its backward is
 * flex_axw_backward_root_bf16 (below).
 * Definition, every bf16 operand read as the fp32 number it is:
 *     FLEX_AXW_AX_W:  T = flex_spmm_bf16(A, X),  Out = rn_bf16(T W + X R + b)   one launch of axw_bf16_root_kernels.hip, L1 = T, L2 = X
 *     FLEX_AXW_A_XW:  U = rn_bf16(X W)           flex_axw_run_bf16's dense stage
 *                     S = flex_spmm_bf16(A, U)   into the handle's second intermediate
 *                     Out = rn_bf16(X R + S + b) the same kernel, L1 = X, W1 = R, no second source, addend S
 * two bf16 roundings in AX_W, three in A_XW.  The dense stage Out = rn_bf16(L1 W1 + L2 W2 + Cin + b) is one fp32 chain per entry: the
 * accumulator STARTS as fp32(Cin) + b (one addition; +0 where both are absent), then takes the k-steps of 16 in ascending order, all of
 * L1 W1 before all of L2 W2 (v_mfma_f32_32x32x16_bf16), and is rounded once at the store.  Cin's padding columns are ignored.
 * Accuracy (tests/axw_bf16_root_ref.py), u, gamma, n_r, bound_bf16 as for flex_axw_run_bf16, M = 1, TINY = 2^-149, eSpmm(T64) =
 * bound_bf16(T64, gamma(n_r) |A||B| + n_r TINY), flex_spmm_bf16's bound of T64 = A B:
 *   dense stage alone:  g = gamma(d1 + d2 + 2) (|L1||W1| + |L2||W2| + |Cin| + |b|) + (d1 + d2) TINY,   |Out - ref64| <= bound_bf16(ref64, g);
 *   FLEX_AXW_AX_W:  T64 = A X, e1 = eSpmm(T64), ref = T64 W + X R + b:
 *       |Out - ref| <= bound_bf16(ref, e1 |W| + gamma(2 dim + 2) ((|T64| + e1) |W| + |X||R| + |b|) + 2 dim TINY);
 *   FLEX_AXW_A_XW:  U64 = X W, eU = bound_bf16(U64, gamma(dim) |X||W| + dim TINY), S64 = A U64,
 *                   eS = bound_bf16(S64, |A| eU + gamma(n_r) |A| (|U64| + eU) + n_r TINY), ref = S64 + X R + b:
 *       |Out - ref| <= bound_bf16(ref, eS + gamma(dim + 2) (|X||R| + |S64| + eS + |b|) + dim TINY);
 *   NaN / +inf / -inf exactly where ref has them, except that a rounding may overflow as flex_spmm_bf16 states; padding columns +0 bits in
 *   every case.  Normal inputs and sums, and the matrix unit's one rounding per addition, as for flex_axw_run_bf16.  The bounds are
 *   derived; DESIGN.md 3.29 holds what tests/test_gpu_axw_bf16_root.py measured against them. */
int flex_axw_run_root_bf16(flex_axw *h, int order, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR,
                           const float *dBias /* c floats or NULL */, flex_bf16 *dOut, flex_stream_t stream, float *gemm_ms, float *spmm_ms);

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

/* flex_axw_backward of a handle made with FLEX_AXW_BF16 | FLEX_AXW_BACKWARD (FLEX_ERR_INVALID on any other, as flex_axw_backward is on a
 * bf16 handle), in the same association order, all device, row-major flex_bf16, on `stream`:
 *     G      = flex_spmm_bf16(A^T, dOut)      n x flex_axw_ld_bf16(c), one rounding to bf16
 *     dGradX = rn_bf16(G W^T in fp32)         n x dim     (the forward's bf16 MFMA kernel on a W^T staged by the call)
 *     dGradW = rn_bf16(X^T G in fp32)         dim x c     (axw_bf16_backward_kernels.hip: fp32 partial sums per n-slice, added in slice
 *                                                          order, rounded once)
 * A NULL dGradX or dGradW skips that product, and its input (dW, resp. dX) may then be NULL; no allocation, no host sync (safe to capture
 * in a hipGraph); ONE call of a handle in flight at a time; the same inputs give the same bits on every call (no atomics).  Every pointer
 * passed must be 16-byte aligned (FLEX_ERR_UNSUPPORTED otherwise); nothing is enqueued in any refusal.
 * At 256 < dim <= 4096 (axw_bf16_wide_kernels.hip) dGradX is computed in passes of 256 output columns and dGradW under the slice rule
 * rows = ceil(n / S0) rounded up to a multiple of 64, S0 = max(1, min(ceil(n / 256), ceil(2 CUs / (ceil(dim / 128) ceil(c / 128))),
 * floor(n / (2 c)))), slices = ceil(n / rows): the partial sums stay below the bytes of X.  The accuracy statements below carry over
 * unchanged, with L taken from that rule (DESIGN.md 3.28 holds the measured figures).
 * dOut is n x flex_axw_ld_bf16(c), and -- unlike flex_axw_backward -- its padding columns ARE read (the bf16 transposed plan gathers whole
 * groups of 8 columns): they must be finite (+0 is what flex_axw_run_bf16 writes).  Finite values there change no output bit: they meet
 * only the zero rows of the staged W^T, and dGradW drops those columns.
 * Accuracy (tests/axw_bf16_backward_ref.py), u, gamma, n_r and bound_bf16 as for flex_axw_run_bf16, cp = flex_axw_ld_bf16(c): G64 the
 * float64 A^T dOut of the bf16 inputs, eG flex_spmm_bf16's bound for it (n_r of the rows of A^T);
 *   dGradX: R = G64 W^T,  E1 = eG |W|^T,  b2 = gamma(cp) (|G64| + eG) |W|^T + cp 2^-149:            |dGradX - R| <= bound_bf16(R, E1 + b2);
 *   dGradW: R = X^T G64,  E1 = |X|^T eG,  b2 = gamma(L) |X|^T (|G64| + eG) + L 2^-149 (1 + sum_r |X_ri|),
 *           L = rows per slice + slices (flex_axw_backward's L_dW for this kernel's slices: rows = ceil(n / min(CUs, ceil(n / 256)))
 *           rounded up to a multiple of 64, slices = ceil(n / rows)):                               |dGradW - R| <= bound_bf16(R, E1 + b2);
 *   NaN / +inf / -inf exactly where R has them, under flex_axw_run_bf16's conditions.  Both gammas assume the matrix unit's sum of the 16
 *   products of a step rounds no more than once per addition; DESIGN.md 3.27 holds what the cancellation cases measured. */
int flex_axw_backward_bf16(flex_axw *h, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dOut, flex_bf16 *dGradX, flex_bf16 *dGradW,
                           flex_stream_t stream);

/* The backward of flex_axw_run_root_bf16, on a handle made with FLEX_AXW_BF16 | FLEX_AXW_ROOT | FLEX_AXW_BACKWARD (FLEX_ERR_INVALID on a
 * handle that lacks any of the three), all device, row-major, on `stream`; dX [n x dim], dW and dR [dim x c] are the forward's inputs:
 *     G         = flex_spmm_bf16(A^T, dOut)       n x flex_axw_ld_bf16(c), one rounding to bf16, as flex_axw_backward_bf16
 *     dGradX    = rn_bf16(G W^T + dOut R^T)       n x dim     ONE fp32 chain per entry: +0, all of G W^T in ascending k, then all of
 *                                                             dOut R^T, one rounding (axw_bf16_root_kernels.hip, 256-column passes)
 *     dGradW    = rn_bf16(X^T G)                  dim x c     } one pass over X (axw_bf16_root_backward_kernels.hip): fp32 partial sums per
 *     dGradR    = rn_bf16(X^T dOut)               dim x c     } n-slice, added in slice order, dGradW and dGradR rounded once,
 *     dGradBias = 1^T dOut                        c floats    } dGradBias kept in fp32
 * dGradW and dGradR come from one kernel and are asked for together: exactly one of them NULL is FLEX_ERR_INVALID.  dGradX and dGradBias
 * are each optional, and an input is needed only for the outputs that use it: dW and dR for dGradX, dX for dGradW and dGradR, dOut always.
 * Every flex_bf16 pointer passed must be 16-byte aligned (FLEX_ERR_UNSUPPORTED otherwise); nothing is enqueued in any refusal.  No
 * allocation, no host sync (safe to capture in a hipGraph), no atomics: the same inputs give the same bits on every call; ONE call of a
 * handle in flight at a time.  All of dOut's padding columns c .. flex_axw_ld_bf16(c)-1 are read and must be finite; they meet zero rows
 * of R^T (and, through G, of W^T) and change no output bit.  With dR = 0, dGradX has the bits of flex_axw_backward_bf16's.
 * Slices of the second kernel: rows = ceil(n / S0) rounded up to a multiple of 64, S0 = max(1, min(ceil(n / 256), floor(wgs CUs /
 * (ceil(dim / 128) ceil(c / 128))), floor(n / (4 c)))), wgs = 2 while c <= 64, else 1; slices = ceil(n / rows): the partial sums of dGradW
 * and dGradR stay below the bytes of X.
 * Accuracy (tests/axw_bf16_root_backward_ref.py), cp, G64, eG, u, gamma, bound_bf16, M = 1 and TINY = 2^-149 as for flex_axw_backward_bf16:
 *   the dX kernel alone:  g = gamma(2 cp + 2) (|G||W|^T + |dOut||R|^T) + 2 cp TINY,   |dX - ref64| <= bound_bf16(ref64, g);
 *   dGradX:    ref = G64 W^T + dOut R^T,  |dGradX - ref| <= bound_bf16(ref, eG |W|^T + gamma(2 cp + 2) ((|G64| + eG) |W|^T + |dOut||R|^T)
 *              + 2 cp TINY);
 *   dGradW:    flex_axw_backward_bf16's statement with L = rows per slice + slices of the rule above;
 *   dGradR:    the same with dOut in place of G64 and eG = 0;
 *   dGradBias: |dGradBias - 1^T dOut| <= gamma(L) 1^T |dOut| + L TINY, the same L; no bf16 rounding.
 *   NaN / +inf / -inf exactly where the reference has them, under flex_axw_run_bf16's conditions.  The bounds are derived; DESIGN.md 3.30
 *   holds what tests/test_gpu_axw_bf16_root_backward.py measured against them. */
int flex_axw_backward_root_bf16(flex_axw *h, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const flex_bf16 *dOut,
                                flex_bf16 *dGradX, flex_bf16 *dGradW, flex_bf16 *dGradR, float *dGradBias /* fp32 */, flex_stream_t stream);

/* flex_axw_run_root_bf16 with ReLU and dropout fused into its last dense launch (axw_bf16_act_kernels.hip), on the same handles, with the
 * same operands, orders, checks and order of launches; the hidden layer of a GNN in one call.  With z the fp32 value that
 * flex_axw_run_root_bf16 rounds (same chain, same order, same Cin + bias start), cs = 1.0f / (1.0f - drop_p) computed in fp32 on the host
 * and idx = row * c + col (64-bit; c the true width, not flex_axw_ld_bf16(c)):
 *     a   = z > 0 ? z : (z != z ? z : +0)            NaN stays NaN; -0 and negatives give +0 bits
 *     Out = keep(seed, idx) ? rn_bf16(a * cs) : +0   ONE bf16 rounding; drop_p == 0: Out = rn_bf16(a), no hash evaluated
 * Padding columns c .. flex_axw_ld_bf16(c)-1 are +0 bits.  Dropped entries are selected out, not multiplied by zero (the attention
 * kernels' rule): a dropped inf or NaN gives +0.  keep is the function behind flex_dropout_mask (flex_spmm.h), its threshold rule
 * included, bit for bit: flex_dropout_mask(seed, drop_p, 0, n * c, keep) is this call's mask, row-major [n x c].  With drop_p == 0, Out
 * has the bits of flex_axw_run_root_bf16's with every entry whose sign bit is set and that is no NaN replaced by +0 (rounding is monotone
 * and keeps the sign).  drop_p must be finite with 0 <= drop_p < 1, else FLEX_ERR_INVALID; nothing is enqueued by a refused call.  seed
 * and drop_p travel as kernel arguments: a captured hipGraph replays the same mask.  No allocation, no host sync unless timed, no
 * atomics: the same bits on every call.
 * Accuracy (tests/axw_bf16_act_ref.py): with ref, E of flex_axw_run_root_bf16's statement for the same order (|z - ref| <= E before the
 * last rounding), kept entries satisfy |Out - cs relu(ref)| <= bound_bf16(cs relu(ref), cs (1 + 2^-23) E + 2^-24 cs relu(|ref| + E)):
 * ReLU is 1-Lipschitz, the product a * cs is one fp32 rounding, and the final bf16 rounding is applied to cs relu(ref).  Dropped entries
 * and padding columns are +0 bits exactly.  DESIGN.md 3.32 holds what tests/test_gpu_axw_bf16_act.py measured. */
int flex_axw_run_root_act_bf16(flex_axw *h, int order, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR,
                               const float *dBias /* c floats or NULL */, flex_bf16 *dOut, float drop_p, uint64_t seed, flex_stream_t stream,
                               float *gemm_ms, float *spmm_ms);

/* The backward of flex_axw_run_root_act_bf16, on a handle that also has FLEX_AXW_BACKWARD.  It is defined on the STORED output dFwdOut of
 * that call, which the caller passes back -- no mask and no seed: Out > 0 exactly where the unit was active and kept --
 *     dZ = Out > 0 ? rn_bf16(fp32(dOut) * cs) : +0      a float compare: NaN, +0 and -0 in Out give +0; columns >= c: +0
 * with cs as above, written by one streaming pass into dWork, a caller-owned n x flex_axw_ld_bf16(c) flex_bf16 buffer, 16-byte aligned
 * and distinct from dOut and dFwdOut (equal pointers: FLEX_ERR_INVALID; NULL dFwdOut or dWork and a drop_p outside [0, 1) too).
 * Everything else is flex_axw_backward_root_bf16 evaluated on dZ in place of dOut, bit for bit: its outputs, NULL-output rules, checks
 * and accuracy statements.  dOut's padding columns are read by the pass and ignored: dZ's are +0 whatever they hold. */
int flex_axw_backward_root_act_bf16(flex_axw *h, const flex_bf16 *dX, const flex_bf16 *dW, const flex_bf16 *dR, const flex_bf16 *dFwdOut,
                                    const flex_bf16 *dOut, flex_bf16 *dWork, flex_bf16 *dGradX, flex_bf16 *dGradW, flex_bf16 *dGradR,
                                    float *dGradBias /* fp32 */, float drop_p, flex_stream_t stream);
int flex_axw_destroy(flex_axw *h);
/* last rocBLAS status seen (rocblas_status), for FLEX_ERR_UNSUPPORTED returns caused by rocBLAS */
int flex_axw_last_blas_status(void);

#ifdef __cplusplus
}
#endif
#endif
