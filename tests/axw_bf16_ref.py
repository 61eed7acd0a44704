"""float64 references and bounds of the bf16 A*X*W layer (include/flex_axw.h: FLEX_AXW_BF16) and of its bf16 MFMA GEMM, for
tests/test_gpu_axw_bf16.py.  Inputs are fp32 arrays of bf16 numbers.  GEMM: products of bf16 numbers are exact in fp32, so
|x32 - ref64| <= g = gamma(M dim) |L||W| + dim 2^-149 for any order of the sum with one rounding per addition (M = 1), and rn_bf16(x32) lies
within bound_bf16(ref64, g).  Layer: T64 the float64 first stage, e1 its stage bound, R the float64 second stage of T64, E1 = |A| e1 or
e1 |W|, b2 the second stage's fp32 bound at |T64| + e1: |Out - R| <= bound_bf16(R, E1 + b2).  Classes are R's, with spmm_bf16_ref.check's
overflow allowance; padding columns are +0 bits."""
import numpy as np

import f64ref
from attention_bf16_ref import bound_bf16, from_bf16, rounded
from f64ref import A_XW, TINY, gamma, gemm_f64, spmm64
from spmm_bf16_ref import BF16_MAX

M = 1  # the dense stage's gamma is gamma(M dim): 1 unless the cancellation case measures otherwise (flex_axw.h)


def gemm_bound(L, W):
    """g of Out = L W (its float64 reference is f64ref.gemm_f64)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return gamma(M * L.shape[1]) * gemm_f64(np.abs(L), np.abs(W)) + L.shape[1] * TINY


def layer_reference(a, X, W, order):
    """(R, E1 + b2) of the bf16 layer in `order`."""
    nr = (np.diff(a.rowPtr.astype(np.int64)) + f64ref.P)[:, None]
    absW = np.abs(W.astype(np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        if order == A_XW:
            T = gemm_f64(X, W)
            e1 = bound_bf16(T, gemm_bound(X, W))
            return spmm64(a, T), spmm64(a, e1, absolute=True) + gamma(nr) * spmm64(a, np.abs(T) + e1, absolute=True) + nr * TINY
        T = spmm64(a, X)
        e1 = bound_bf16(T, gamma(nr) * spmm64(a, X, absolute=True) + nr * TINY)
        return gemm_f64(T, W), gemm_f64(e1, absW) + gemm_bound(np.abs(T) + e1, W)


def check(ref, bound32, out_bits, what=""):
    """(message or None, worst err / bound) of bf16 bits Out [n x cp] against ref [n x c] and its fp32-stage bound."""
    c = ref.shape[1]
    assert out_bits.dtype == np.uint16 and out_bits.shape[0] == ref.shape[0] and out_bits.shape[1] >= c, (out_bits.dtype, out_bits.shape)
    if out_bits[:, c:].any():
        r, j = np.argwhere(out_bits[:, c:] != 0)[0]
        return f"[{what}] padding entry ({r}, {c + j}) is {out_bits[r, c + j]:#06x}, not +0 bits", np.inf
    got = from_bf16(out_bits[:, :c]).astype(np.float64)
    fin = np.isfinite(ref)
    with np.errstate(invalid="ignore"):
        overflow = fin & np.isinf(got) & (np.sign(got) == np.sign(ref)) & (np.abs(ref) + bound32 >= BF16_MAX)
    bad = f64ref._class_mismatch(ref, got) & ~overflow
    if bad.any():
        r, j = np.argwhere(bad)[0]
        return f"[{what}] {int(bad.sum())} entries of the wrong class; first at ({r}, {j}): got {got[r, j]!r}, reference {ref[r, j]!r}", np.inf
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.where(fin & ~overflow, np.abs(got - ref) / bound_bf16(np.where(fin, ref, 0.0), np.where(fin, bound32, 0.0)), 0.0)
    r, j = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    msg = (f"[{what}] {int((ratio > 1).sum())} entries beyond the bound; worst err/bound {ratio[r, j]:.3g} at ({r}, {j}): got {got[r, j]!r}, "
           f"reference {ref[r, j]!r}, bound32 {bound32[r, j]:.3g}")
    return (msg if ratio[r, j] > 1.0 else None), float(ratio[r, j])


def operands(rng, n, dim, c, cancel=False):
    """(L [n x dim], W [dim x c]) of bf16 numbers, magnitudes 2^U(-4, 4).  cancel: L's rows in pairs (x, -x (1 + 2^-7)) against constant
    columns of W, so that |L||W| >> |L W|."""
    L = rounded(f64ref._logu(rng, -4, 4, (n, dim)))
    W = f64ref._logu(rng, -4, 4, (dim, c))
    if cancel:
        L[:, 1::2] = -(L[:, 0::2] * np.float32(1 + 2.0 ** -7))
        W[:] = W[:1]
    return rounded(L), rounded(W)
